"""dc_set_wino_phase moves the staging phase of the two-group Winograd weight-gradient kernels inside a barrier interval and
nothing else: for every case the outputs under each forced phase and under auto are BITWISE those of the classic order (phase
PHASES - 1), and the classic order stays inside the 2e-5 max|fp64| gate of tests/test_wino_gpu.py.  Every launch goes through the
C ABI with sentinel bands around its outputs and workspaces (exactly the bytes the queries return); the modes are set and restored
in try / finally.

A two-group block (wino_wgrad_kernel<.., NG = 2>) runs its groups for (chunks of group 0, chunks of group 1); the rotated order
of phase 0 has a prologue stage, a loop and a tail whose conditions differ for 1, 2 and 3+ chunks, so the cases reach (1,0),
(1,1), (2,1), (2,2), (3,2) and (3,3) -- asserted on the CPU from the transcribed plan (tests/wino_bn_cases.py: wg_plan).  The
plan gives a two-group block at least two chunks per group, so the first three need DC_WGRAD_NG=2, which wg_plan reads at every
call; (2,2) and (3,2) also come from the plan alone (128 -> 128 at 32 x 64).  Beside them: a ragged map, the BatchNorm-folded
loader with two groups, the fused block (up0 + concat + reflect), and one-group launches (MR = 2 and MR = 4), which keep the
classic order in every mode."""
import contextlib
import os
import zlib

import pytest
import torch
import torch.nn.functional as F

import conv_block_cases as CC
import test_wino_bn_shapes_gpu as TB
import wino_bn_cases as WC

pytestmark = pytest.mark.gpu
DEV = CC.DEV
AUTO, PHASES = -1, 2          # include/depthcore.h, csrc/wino.h
CLASSIC = PHASES - 1
TOL = WC.TENSOR_TOL


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _under_every_mode(run):
    """{mode: run()} for the classic order, every other forced phase and auto; the mode the process had comes back."""
    L = WC.host_lib()
    before = L.dc_set_wino_phase(CLASSIC)
    try:
        out = {}
        for m in [CLASSIC] + [p for p in range(PHASES) if p != CLASSIC] + [AUTO]:
            L.dc_set_wino_phase(m)
            out[m] = run()
        return out
    finally:
        L.dc_set_wino_phase(before)


def _same_bits(outs, tag):
    for m, res in outs.items():
        for k, v in res.items():
            if v is not None:
                assert torch.equal(CC.bits(v), CC.bits(outs[CLASSIC][k])), "%s: %s under mode %d differs from the classic order" % (tag, k, m)


def _gate(tag, got, ref64):
    err = WC.rel_err(got, ref64)
    print("wino_phase_parity %-44s %.2e (%.0f%% of %.0e)" % (tag, err, 100 * err / TOL, TOL))
    assert err <= TOL, (tag, err)


def _seeded(tag):
    return torch.Generator().manual_seed(zlib.crc32(repr(("wino_phase", tag)).encode()))


# ---- weight gradient ---------------------------------------------------------------------------------------------------------------
def _wg_plan(B, Ci, Co, H, W, force_ng2):
    p = WC.wg_plan(B, Ci, Co, H, W)
    if force_ng2 and p.ng == 1:                     # wg_plan with DC_WGRAD_NG=2: 256 two-group blocks as the target
        assert p.mr == 4
        nmk = p.mblocks * p.kblocks
        splits = max(1, min(max(1, p.nsub // 4), WC.ceil_div(256, nmk)))
        p = p._replace(ng=2, splits=splits, ws_bytes=splits * nmk * WC.WG_SLAB_MR4 * 4)
    return p


def _wg_iters(p):
    """{(chunks of group 0, chunks of group 1)} over the blocks of the launch."""
    stride = p.ng * p.splits
    return {(len(range(s, p.nsub, stride)), len(range(s + p.splits, p.nsub, stride)) if p.ng == 2 else 0) for s in range(p.splits)}


# (B, Ci, Co, H, W, DC_WGRAD_NG=2?, mr, ng, chunks per group over the blocks)
WGRAD = [
    (1, 64, 128, 4, 16, True, 4, 2, {(1, 0)}),
    (2, 64, 128, 4, 16, True, 4, 2, {(1, 1)}),
    (3, 64, 128, 4, 16, True, 4, 2, {(2, 1)}),
    (4, 64, 128, 4, 16, True, 4, 2, {(2, 2)}),
    (5, 64, 128, 4, 16, True, 4, 2, {(3, 2)}),
    (6, 64, 128, 4, 16, True, 4, 2, {(3, 3)}),
    (4, 128, 128, 32, 64, False, 4, 2, {(2, 2)}),                 # the plan's own two-group launch: 32 splits, stride 64
    (5, 128, 128, 32, 64, False, 4, 2, {(3, 2)}),
    (5, 64, 64, 9, 22, True, 4, 2, {(3, 2), (2, 2)}),             # ragged map (H odd, W = 2 x odd), two groups, a ragged last round
    (3, 40, 32, 7, 10, False, 2, 1, {(2, 0)}),                    # MR = 2 (Co = 32), one group, ragged map
    (2, 64, 64, 16, 24, False, 4, 1, {(2, 0)}),                   # MR = 4, one group
    (5, 24, 64, 4, 8, False, 4, 1, {(3, 0), (2, 0)}),             # ... blocks with 3 chunks beside blocks with 2
]


def _wg_id(c):
    return "%dx%dto%dx%dx%d%s" % (c[0], c[1], c[2], c[3], c[4], "-ng2" if c[5] else "")


@pytest.mark.parametrize("case", [pytest.param(c, id=_wg_id(c)) for c in WGRAD])
def test_weight_gradient(case):
    from depthcore import _lib
    from depthcore._lib import ptr
    B, Ci, Co, H, W, force, mr, ng, iters = case
    p = _wg_plan(B, Ci, Co, H, W, force)
    assert (p.mr, p.ng) == (mr, ng) and _wg_iters(p) == iters, (p, _wg_iters(p))
    L = WC.host_lib()
    g = _seeded(case[:6])
    x, gy = torch.randn(B, Ci, H, W, generator=g).to(DEV), torch.randn(B, Co, H, W, generator=g).to(DEV)
    st = _lib.stream(x)

    def run():
        with _env(**({"DC_WGRAD_NG": "2"} if force else {})):
            nbytes = L.dc_wino3x3_wgrad_workspace(B, Ci, Co, H, W)
            assert nbytes >= p.ws_bytes and nbytes % 4 == 0
            out, ws = CC.Guarded(Co * Ci * 9), CC.Guarded(nbytes // 4)
            rc = L.dc_wino3x3_wgrad(ptr(x), ptr(gy), out.ptr(), ws.ptr(), B, Ci, Co, H, W, st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert out.intact() and ws.intact(), "the weight gradient wrote outside a buffer"
        res = out.body.cpu().view(Co, Ci, 3, 3)
        assert bool(torch.isfinite(res).all())
        return {"dW": res}

    outs = _under_every_mode(run)
    _same_bits(outs, "wgrad " + _wg_id(case))
    # fp64 statement on the device: dW[co, ci, ky, kx] = sum_{b, y, x} gy[b, co, y, x] xpad[b, ci, y + ky, x + kx]
    cols = F.unfold(x.double(), 3, padding=1)                     # (B, Ci 9, H W)
    ref = torch.einsum("bop,bkp->ok", gy.double().view(B, Co, H * W), cols).view(Co, Ci, 3, 3).cpu()
    _gate("wgrad " + _wg_id(case), outs[CLASSIC]["dW"], ref)


def test_weight_gradient_with_the_batchnorm_fold_and_two_groups():
    case = WC._wgrad(8, 128, 256, 12, 40, 2)
    m = WC.mech(case)
    assert m["plan"].ng == 2 and m["bnin"] == 2
    inp, r64, _ = WC.reference(case)
    outs = _under_every_mode(lambda: {"dW": TB._launch(case, inp)["out"]})
    _same_bits(outs, WC.case_id(case))
    _gate(WC.case_id(case), outs[CLASSIC]["dW"], r64["dW"])


# ---- the fused block's weight gradient ------------------------------------------------------------------------------------------
# (case, DC_WGRAD_NG=2?, mr, ng, chunks per group): up0 + concat + reflect with Cin, Co >= 32.  The step's decoder blocks that take
# two groups are megabytes; DC_WGRAD_NG=2 brings wino_wgrad_kernel<true, 4, 2> to a map of 8 x 12.
FUSED = [(CC.K(3, 32, 1, 32, 64, 8, 12, 1, CC.REFLECT, dsplit=2), True, 4, 2, {(3, 3)}),
         (CC.K(3, 24, 1, 40, 64, 10, 22, 4, CC.ZERO, bias=0), True, 4, 2, {(3, 2), (2, 2)}),       # ragged map, zero padding, no bias
         (CC.K(2, 16, 1, 16, 32, 8, 12, 1, CC.REFLECT, dsplit=2), False, 2, 1, {(2, 0)})]          # one group: the classic order in every mode


@pytest.mark.parametrize("case, force, mr, ng, iters", [pytest.param(*f, id=CC.case_id(f[0]) + ("-ng2" if f[1] else "")) for f in FUSED])
def test_fused_blocks(case, force, mr, ng, iters):
    r = CC.route(case)
    assert r["fwd"] == "wino_conv_fused_fwd" and r["dw"] == "wino_wgrad_fused", r
    assert case.C0 + case.C1 >= 32 and case.Co >= 32 and case.up0 and case.C1
    p = _wg_plan(case.B, case.C0 + case.C1, case.Co, case.H, case.W, force)
    assert (p.mr, p.ng) == (mr, ng) and _wg_iters(p) == iters, (p, _wg_iters(p))
    inp, r64, r32 = CC.reference(case)

    def run():
        with _env(**({"DC_WGRAD_NG": "2"} if force else {})):
            return CC.launch(case, inp)

    outs = _under_every_mode(run)
    _same_bits(outs, CC.case_id(case))
    CC.gate(case, outs[CLASSIC], r64, r32, tag="wino_phase_parity")
