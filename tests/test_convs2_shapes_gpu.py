"""The strided trunk convolutions through the C ABI -- dc_convs2_fwd / _wgrad / _dgrad and dc_stem_fwd / _wgrad -- against the fp64
statement of tests/convs2_cases.py, branch by branch of the host dispatch and at the edges of the kernels' tiles: the patch-staged
stem in both forward variants and on raw frames, the triple-gather kernels with every slab split, the general gather kernels in
every tile pick (the triple-gather and stem rows too, in a child process with the fast paths switched off), the parity data
gradient.  The fitness of the rows, route()'s agreement with the library and the refusals are the subject of
tests/test_convs2_cases_cpu.py; the table with its reasons, the predicates, the gate and the measured figures are in DESIGN.md, "The
strided convolutions at their dispatch edges".  Every test prints its figures (`convs2_parity <row> <output> err/max ...`) before
it asserts.

Gate (convs2_cases.gate): max|hip - fp64| <= 1e-5 max|fp64| for y, dx and dw (the bound of tests/test_convs2_gpu.py).  Every output
and every workspace -- exactly the bytes its query returns -- sits between sentinel guards that must come back intact, and starts
as NaN: every output element must be finite afterwards."""
import os
import subprocess
import sys

import pytest
import torch

import convs2_cases as S

pytestmark = pytest.mark.gpu


def _norm_err(got, ref):
    return float((got.double() - ref).norm() / ref.norm())


@pytest.mark.parametrize("case", S.params(S.CASES))
def test_row(case):
    """Forward, weight gradient and (where the plan has one) data gradient of one row under the default split mode."""
    r = S.route(case)
    assert S.plan_mismatches(case) == []
    inp, r64, r32 = S.reference(case)
    with S.split_mode(1):
        res = S.launch(case, inp, S.outputs(case))
    S.gate(case, res, r64, r32, note="| " + S.describe(r))


@pytest.mark.parametrize("case", S.params([c for c in S.CASES if S.route(c)["dx"] is None and c.only is None]))
def test_backward_raises_where_the_plan_has_no_data_gradient(case):
    from depthcore import ops, _lib
    inp = S.reference(case)[0]
    x, w = inp["x"].to(S.DEV).requires_grad_(True), inp["w"].to(S.DEV).requires_grad_(True)
    assert ops.conv_s2_supported(x, w)
    y = ops.conv_s2(x, w)
    with pytest.raises(_lib.DepthcoreError):
        y.backward(inp["gy"].to(S.DEV))
    # ... and the weight gradient alone is served
    x2 = inp["x"].to(S.DEV)
    (gw,) = torch.autograd.grad(ops.conv_s2(x2, w), w, inp["gy"].to(S.DEV))
    assert bool(torch.isfinite(gw).all())


@pytest.mark.parametrize("case", S.params(S.stem_rows()))
def test_stem_modes_and_raw_frames(case):
    """Every stem row's forward under dc_set_gemm_split(0) (stem_fwd_kernel) and (1) (stem_fwd_x3_kernel), through dc_convs2_* and
    through dc_stem_* on the raw frames (nf = 1; nf = 2 and 3 for six channels): the raw-frame results are bit for bit those of
    dc_convs2_* on the materialised (x - 0.45) / 0.225 -- weight gradient included -- and pass the gate; the split-operand forward's
    normwise error against fp64 is at most 1.25 x the fp32 kernel's + 2e-8 (the bound of tests/test_convs2_gpu.py)."""
    inp, r64, r32 = S.reference(case)
    y, e = {}, {}
    for mode in (0, 1):
        with S.split_mode(mode):
            want = "stem_x3" if mode else "stem_f32"
            assert S.plan_query(case)[1]["fwd"] == S.PLAN_FWD[want] == S.plan_query(case, raw=1)[1]["fwd"]
            y[mode] = S.launch(case, inp, ("y",))["y"]
            S.gate(case, {"y": y[mode]}, r64, r32, note="| split mode %d, dc_convs2_fwd, %s" % (mode, want))
            for nf in S.raw_modes(case):
                raw = S.launch(case, inp, ("y",), raw=nf)["y"]
                S.gate(case, {"y": raw}, r64, r32, note="| split mode %d, dc_stem_fwd nf = %d, %s" % (mode, nf, want))
                assert torch.equal(S.bits(raw), S.bits(y[mode])), (mode, nf)
        e[mode] = _norm_err(y[mode], r64["y"])
    print("convs2_stem_modes %s |x3 - f64| / |f64| = %.2e, |f32-MFMA - f64| / |f64| = %.2e" % (S.case_id(case), e[1], e[0]))
    assert e[1] <= 1.25 * e[0] + 2e-8, e
    assert not torch.equal(S.bits(y[0]), S.bits(y[1]))          # (the two kernels really are different arithmetic orders)
    with S.split_mode(1):
        dw = S.launch(case, inp, ("dw",))["dw"]
        for nf in S.raw_modes(case):
            raw = S.launch(case, inp, ("dw",), raw=nf)["dw"]
            S.gate(case, {"dw": raw}, r64, r32, note="| dc_stem_wgrad nf = %d" % nf)
            assert torch.equal(S.bits(raw), S.bits(dw)), nf


def test_split_mode_3_takes_the_eligible_row_only():
    """dc_set_gemm_split(3): (1,64,64,16,32,3) (Ho Wo = 128, N % 32 == 0) goes to the split-operand kernels of gemm1x1_x3.hip -- forward
    and weight gradient differ bitwise from mode 0's and pass the gate -- and (1,64,128,6,8,3) (Ho Wo = 12) stays on the fp32-MFMA
    kernels, bit for bit.  The data gradient is the same kernel in both modes.  The plan says which."""
    from depthcore import _lib
    before = _lib.lib().dc_get_gemm_split()
    for kind, case in sorted(S.SPLIT3.items()):
        inp, r64, r32 = S.reference(case)
        out = {}
        for mode in (0, 3):
            with S.split_mode(mode):
                assert S.plan_mismatches(case, mode) == []
                plan = S.plan_query(case)[1]
                assert (plan["fwd"] == S.PLAN_FWD["g1x3"]) == (plan["dw"] == S.PLAN_DW["g1x3"]) == (mode == 3 and kind == "eligible")
                out[mode] = S.launch(case, inp)
                S.gate(case, out[mode], r64, r32, note="| split mode %d, %s" % (mode, S.describe(S.route(case, mode))))
        for name in ("y", "dw"):
            assert torch.equal(S.bits(out[0][name]), S.bits(out[3][name])) == (kind == "ineligible"), (kind, name)
        assert torch.equal(S.bits(out[0]["dx"]), S.bits(out[3]["dx"]))
    assert _lib.lib().dc_get_gemm_split() == before


def test_split_mode_is_restored_after_a_failure():
    from depthcore import _lib
    L = _lib.lib()
    before = L.dc_get_gemm_split()
    with pytest.raises(ZeroDivisionError):
        with S.split_mode(0 if before else 1):
            assert L.dc_get_gemm_split() != before
            1 / 0
    assert L.dc_get_gemm_split() == before


@pytest.mark.parametrize("family", sorted(S.DETERMINISM))
def test_two_launches_are_bitwise_equal(family):
    case = S.DETERMINISM[family]
    assert {"stem": S.route(case)["stem"], "trip": S.route(case)["trip"], "gather": S.route(case)["fwd"] == "gather"}[family]
    inp = S.reference(case)[0]
    with S.split_mode(1):
        a, b = S.launch(case, inp, S.outputs(case)), S.launch(case, inp, S.outputs(case))
    for k, v in a.items():
        assert v is None or torch.equal(S.bits(v), S.bits(b[k])), k


def test_gather_kernels_with_the_fast_paths_disabled():
    """DC_STEM_PATCH and DC_CONV_TRIP are read once per process: tests/convs2_gather_child.py runs the triple-gather and stem rows
    through the general gather kernels in a fresh process, at the same gate.  It must report every such row."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "convs2_gather_child.py")
    p = subprocess.run([sys.executable, child], env={**os.environ, **S.GATHER_ENV}, timeout=600, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("convs2_gather ")]
    want = {S.case_id(c) for c in S.gather_child_cases()}
    assert {ln.split()[1] for ln in lines} == want and len(lines) == len(want)
    by_id = {S.case_id(c): c for c in S.CASES}
    hit = [by_id[ln.split()[1]] for ln in lines]
    assert any(c.k == 3 and c.Ci % 32 == 0 for c in hit) and any(c.k == 7 and c.Co == 64 for c in hit)
    assert p.stdout.rstrip().endswith("convs2_gather_done %d" % len(want))
