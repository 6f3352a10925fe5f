"""The split Winograd reductions through the C ABI -- ONE launch per case -- against the fp64 statement of
tests/wino_split_cases.py, slab by slab: dc_wino3x3_fwd, dc_wino3x3_dgrad, dc_wino3x3_dgrad_add, dc_wino3x3_fwd_bn with the loader
fold alone, and the fused 3x3 block (dc_conv3x3_fwd / dc_conv3x3_bwd_add) where its forward and its full-correlation data gradient
split.  The fitness of the cases and the agreement of the transcribed plan and layout with the library are the subject of
tests/test_wino_split_cases_cpu.py; the tables with their reasons, the gates and the measured figures are in DESIGN.md, "The split
reductions at their slab edges".  Every test prints its figures (`wino_split_parity <case> <tensor> e_hip e32 share-of-bound`)
before it asserts.

Gates (wino_split_cases.gate; the fused block: conv_block_cases.gate, unchanged)
    tensor    max|hip - fp64| <= 2e-5 max|fp64|; every element finite
    slabs     read back from the workspace: slab s against the fp64 convolution over its own channels, the same 2e-5 of that
              partial result's largest entry; an empty slab is bitwise +0.0 everywhere; everything behind slab ksplit - 1 is
              still NaN (the device ran the transcribed number of slabs)
    sum       the output is, bit for bit, the host's fp32 sum of the read-back slabs in slab order, the addend added last
The output and the whole workspace -- exactly dc_wino3x3_workspace bytes -- sit between sentinel guards that must come back
intact, and start as NaN."""
import os
import subprocess
import sys

import pytest
import torch

import conv_block_cases as CC
import wino_split_cases as WS

pytestmark = pytest.mark.gpu


def _check(case):
    inp = WS.reference(case)[0]
    out, ws = WS.launch(case, inp)
    WS.gate(case, inp, out, ws)
    return out, ws


@pytest.mark.parametrize("case", WS.params(WS.FWD))
def test_forward(case):
    _check(case)


@pytest.mark.parametrize("case", WS.params(WS.DGRAD))
def test_data_gradient(case):
    _check(case)


@pytest.mark.parametrize("case", WS.params(WS.LOADER))
def test_loader_fold(case):
    _check(case)


@pytest.mark.parametrize("case", CC.params(WS.fused_cases()))
def test_fused_block(case):
    """The fused launches split: the slab sum adds the bias and applies the activation; where the data gradient's plan splits too,
    the full correlation runs split and the fold pass follows.  The route is the library's own (dc_conv3x3_plan_query)."""
    assert CC.plan_mismatches(case) == []
    bm, r = WS.block_mech(case), CC.route(case)
    assert r["fwd"] == "wino_conv_fused_fwd" and bm["fwd"]["ksplit"] > 1
    assert (r["dx"] == "wino_conv_full_dgrad") == (bm["dgrad_same"]["ksplit"] > 1)
    inp, r64, r32 = CC.reference(case)
    print("wino_split_parity %s splits: forward %d x %s, data gradient %s" % (
        CC.case_id(case), bm["fwd"]["ksplit"], bm["fwd"]["slab_chunks"],
        "%d x %s (P = 2)" % (bm["dgrad_full"]["ksplit"], bm["dgrad_full"]["slab_chunks"]) if r["fold"] else "unsplit"))
    CC.gate(case, CC.launch(case, inp), r64, r32, tag="wino_split_parity")


@pytest.mark.parametrize("kind", sorted(WS.DETERMINISM))
def test_two_launches_are_bitwise_equal(kind):
    """Into fresh buffers: the output and every slab."""
    case = WS.DETERMINISM[kind]
    inp = WS.reference(case)[0]
    (a, wa), (b, wb) = WS.launch(case, inp), WS.launch(case, inp)
    assert torch.equal(CC.bits(a), CC.bits(b))
    m = WS.mech(case)
    lo, hi = WS.slab_offset_floats(case.Ci, case.Co, 0, m["nout"]), WS.slab_offset_floats(case.Ci, case.Co, m["ksplit"], m["nout"])
    assert torch.equal(CC.bits(wa[lo:hi]), CC.bits(wb[lo:hi]))


@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
@pytest.mark.parametrize("shape", WS.LOCKSTEP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_lockstep_batch_is_three_single_launches(shape, kind):
    """dc_set_wino_plan_streams(3): the batch of three is planned as one stream's launch, so image b of it is bitwise the B = 1
    launch on image b alone -- output and slabs.  That the plans differ without the setting (on the 12 x 40 shape) is a statement of
    the transcription: tests/test_wino_split_cases_cpu.py::test_plan_streams_in_the_transcription."""
    B, Ci, Co, H, W = shape
    case = WS.Case(kind, B, Ci, Co, H, W, 1, 0, None)
    one = case._replace(B=1)
    m, m1 = WS.mech(case, streams=WS.LOCKSTEP), WS.mech(one)
    assert (m["MT"], m["G"], m["ksplit"]) == (m1["MT"], m1["G"], m1["ksplit"]) and m["ksplit"] > 1
    inp = WS.build(case)
    full, ws = WS.launch(case, inp, streams=WS.LOCKSTEP)
    assert bool(torch.isfinite(full).all())
    off, off1 = WS.slab_offset_floats(Ci, Co, 0, m["nout"]), WS.slab_offset_floats(Ci, Co, 0, m1["nout"])
    slabs = ws[off:off + m["ksplit"] * m["nout"]].view(m["ksplit"], B, -1)
    assert bool(torch.isnan(ws[off + m["ksplit"] * m["nout"]:]).all())
    for b in range(B):
        sub = {k: (v if k == "w" else v[b:b + 1]) for k, v in inp.items()}
        y, w1 = WS.launch(one, sub)
        assert torch.equal(CC.bits(y[0]), CC.bits(full[b])), b
        s1 = w1[off1:off1 + m1["ksplit"] * m1["nout"]].view(m1["ksplit"], -1)
        assert torch.equal(CC.bits(s1), CC.bits(slabs[:, b].contiguous())), b
    print("wino_split_parity lockstep %s %s: %d x B = 1 bitwise equal, split %d x %s" % (kind, "x".join(map(str, shape)), B, m["ksplit"], m["slab_chunks"]))


def test_forced_plans():
    """The splits the cost model picks for no shape, in a fresh process under DC_WINO_FORCE (tests/wino_split_forced_child.py):
    9 chunks over 4 slabs (the empty slab begins exactly at nchunks) and the 32 x 64 tile variant."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wino_split_forced_child.py")
    p = subprocess.run([sys.executable, child], env={**os.environ, "DC_WINO_FORCE": WS.FORCED[0].force}, timeout=300, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("wino_split_forced ")]
    assert {ln.split()[1] for ln in lines} == {WS.case_id(c) for c in WS.FORCED} and len(lines) == 2 * len(WS.FORCED)
    assert p.stdout.rstrip().endswith("wino_split_forced_done %d" % len(WS.FORCED))
