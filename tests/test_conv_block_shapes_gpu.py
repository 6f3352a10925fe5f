"""The fused 3x3 block through the C ABI -- ONE dc_conv3x3_fwd and ONE dc_conv3x3_bwd_add per case (fp32 policy) -- against the
fp64 statement of tests/conv_block_cases.py, branch by branch of the host dispatch: head kernels, fused Winograd launches, direct
implicit GEMMs, both folds, the reflection ring, the split reductions, every way g' comes about and every null pattern of the
gradient pointers.  The fitness of the cases, route()'s agreement with the library and the refusals are the subject of
tests/test_conv_block_cases_cpu.py; the table with its reasons, the predicates, the gates and the measured shares are in DESIGN.md,
"The fused 3x3 block at its dispatch edges".  Every test prints its figures (`conv_block_parity ...`) before it asserts.

Gates (conv_block_cases.gate)
    y, dx0, dx1, dw   max|hip - fp64| <= 2e-5 max|fp64| where route() names a Winograd kernel for that output (the bound of
                      tests/test_wino_gpu.py), <= 1e-5 max|fp64| where it names a direct or plain-FMA kernel (tests/test_convs2_gpu.py)
    db                |hip - fp64| <= (n + 2) 2^-24 sum|g'| per channel, n = B H W: the worst case of an fp32 sum in any order
Every output and both workspaces -- exactly the bytes the queries return -- sit between sentinel guards that must come back
intact, and start as NaN: every output element must be finite afterwards.  A separate addend must come back bitwise unchanged."""
import os
import subprocess
import sys

import pytest
import torch

import conv_block_cases as CC

pytestmark = pytest.mark.gpu


def _run(case):
    inp, r64, r32 = CC.reference(case)
    res = CC.launch(case, inp)
    CC.gate(case, res, r64, r32)
    return res


@pytest.mark.parametrize("case", CC.params(CC.CASES))
def test_block(case):
    _run(case)


@pytest.mark.parametrize("family", sorted(CC.NULL_FAMILIES))
def test_null_patterns_leave_the_other_outputs_alone(family):
    """Each output of a partial-gradient launch against the same output of the all-gradients launch: bitwise equal where route()
    names the same kernels for that output in both launches, within the gate (which _run has applied) otherwise."""
    base, nulls = CC.NULL_FAMILIES[family]
    full, kb = _run(base), CC.output_kernels(base)
    for c in nulls:
        part, kc = _run(c), CC.output_kernels(c)
        assert torch.equal(CC.bits(part["y"]), CC.bits(full["y"]))
        for g, k in CC.OUTPUTS.items():
            assert (part[k] is not None) == (g in c.grads), (k, c.grads)
            if part[k] is None:
                continue
            same = kc[k] == kb[k]
            equal = torch.equal(CC.bits(part[k]), CC.bits(full[k]))
            print("conv_block_nulls %s grads=%s %s: %s, %s" % (family, "".join(c.grads), k, "same kernels" if same else "%s instead of %s" % (kc[k], kb[k]),
                                                              "bitwise equal" if equal else "differs"))
            assert equal or not same, (family, c.grads, k)


@pytest.mark.parametrize("case", CC.params(CC.DSPLIT_PAIRS))
def test_dgrad_split_modes_take_different_kernels(case):
    """dc_set_dgrad_split 2 (split store + ring) against 0 (full correlation + fold): both pass the gate, and the data gradients
    differ bitwise somewhere -- the evidence that the mode chose the route."""
    a, b = _run(case), _run(case._replace(dsplit=0))
    assert not torch.equal(CC.bits(a["dx0"]), CC.bits(b["dx0"]))
    for k in ("y", "dw", "db"):
        assert torch.equal(CC.bits(a[k]), CC.bits(b[k])), k


@pytest.mark.parametrize("kind", sorted(CC.DETERMINISM))
def test_two_launches_are_bitwise_equal(kind):
    case = CC.DETERMINISM[kind]
    inp = CC.reference(case)[0]
    a, b = CC.launch(case, inp), CC.launch(case, inp)
    for k, v in a.items():
        assert v is None or torch.equal(CC.bits(v), CC.bits(b[k])), k


def test_dgrad_split_mode_is_restored():
    from depthcore import _lib
    L = _lib.lib()
    before = L.dc_set_dgrad_split(1)
    try:
        _run(CC.DSPLIT_PAIRS[0])
        assert L.dc_set_dgrad_split(1) == 1
    finally:
        L.dc_set_dgrad_split(before)


def test_direct_kernels_with_winograd_disabled():
    """DC_CONV_WINO is read once per process: tests/conv_block_direct_child.py runs every table case whose route changes with
    DC_CONV_WINO=0 (forward and all-gradients backward, the 1e-5 gates) in a fresh process.  It must report all three
    conv_gemm_v2_kernel<MR, false>, each with up0 + concat + reflect and with a ragged Co."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_block_direct_child.py")
    p = subprocess.run([sys.executable, child], env={**os.environ, "DC_CONV_WINO": "0"}, timeout=600, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("conv_block_direct ")]
    by_id = {CC.case_id(c): c for c in CC.CASES}
    want = {CC.case_id(c) for c in CC.direct_child_cases()}
    assert {ln.split()[1] for ln in lines} == want and len(lines) == len(want)
    for mr in (1, 2, 4):
        hit = [by_id[ln.split()[1]] for ln in lines if "fwd conv_gemm_v2_kernel<%d, false>" % mr in ln]
        assert any(c.up0 and c.C1 and c.pad == CC.REFLECT for c in hit), mr
        assert any(c.Co % (16 * mr) for c in hit), mr
    assert p.stdout.rstrip().endswith("conv_block_direct_done %d" % len(want))
