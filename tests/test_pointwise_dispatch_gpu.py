"""The 1x1 dispatcher (csrc/pointwise.hip: dc_pointwise_fwd / _dgrad / _wgrad) against the family-pinned entry that the routing
table of include/depthcore.h predicts, on the same inputs, bitwise, under both split modes; and the folded BatchNorm passes
through depthcore.bnfold under mode 1 against mode 0, with the partial buffers sized by dc_pointwise_*_parts fully written."""
import ctypes

import pytest
import torch

from helpers import close, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
X3, G1, PW = "split bf16", "fp32-MFMA", "general"
# the shapes and families of tests/test_pointwise_dispatch_cpu.py (mode 1; mode 0: split -> fp32-MFMA)
SHAPES = {
    (2, 64, 96, 4, 8, 1): X3,
    (2, 64, 128, 8, 16, 2): X3,         # the data gradient through the split kernels' scatter epilogue
    (8, 64, 32, 2, 6, 1): G1,           # P = 12
    (3, 7, 5, 6, 10, 2): PW,
    (3, 2048, 512, 10, 32, 1): X3,      # tiles span images
}


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _bytes(n):
    return torch.empty(n, dtype=torch.uint8, device=DEV)


@pytest.fixture
def L():
    from depthcore import _lib
    lib = _lib.lib()
    prev = lib.dc_get_gemm_split()
    try:
        yield lib
    finally:
        lib.dc_set_gemm_split(prev)


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_dispatcher_runs_the_predicted_family_bitwise(L, shape, mode):
    B, Ci, Co, H, W, s = shape
    fam = SHAPES[shape] if mode else (G1 if SHAPES[shape] == X3 else SHAPES[shape])
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, Ci, H, W, generator=g).to(DEV)
    w = (torch.randn(Co, Ci, generator=g) / Ci ** 0.5).to(DEV)
    gy = torch.randn(B, Co, H // s, W // s, generator=g).to(DEV)
    add = torch.randn(B, Ci, H, W, generator=g).to(DEV)
    p = lambda t: t.data_ptr()
    L.dc_set_gemm_split(mode)
    # the dispatcher: one workspace query and one launch per pass
    y, dx, dw = _nan(*gy.shape), _nan(*x.shape), _nan(Co, Ci)
    ws = [_bytes(L.dc_pointwise_workspace(k, None, *shape)) for k in range(3)]
    assert L.dc_pointwise_fwd(p(x), p(w), None, p(y), p(ws[0]), *shape, 0, None, None) == 0
    assert L.dc_pointwise_dgrad(p(gy), p(w), p(dx), p(ws[1]), p(add), None, *shape, None, None) == 0
    assert L.dc_pointwise_wgrad(p(x), p(gy), p(dw), p(ws[2]), *shape, None, None) == 0
    # the pinned family
    yp, dxp, dwp = _nan(*gy.shape), _nan(*x.shape), _nan(Co, Ci)
    if fam == X3:
        wsp = _bytes(L.dc_gemm1x1x3_workspace(Ci, Co))
        wsw = _bytes(L.dc_gemm1x1x3_wgrad_workspace(*shape))
        assert L.dc_gemm1x1x3_fwd(p(x), p(w), None, p(yp), p(wsp), *shape, 0, None) == 0
        assert L.dc_gemm1x1x3_dgrad(p(gy), p(w), p(dxp), p(wsp), p(add), None, *shape, None) == 0
        assert L.dc_gemm1x1x3_wgrad(p(x), p(gy), p(dwp), p(wsw), *shape, None) == 0
    else:
        wsw = _bytes(L.dc_conv1x1_wgrad_workspace(*shape))
        assert L.dc_conv1x1_bias_act_fwd(p(x), p(w), None, p(yp), *shape, 0, None) == 0
        assert L.dc_conv1x1_dgrad_add2(p(gy), p(w), p(dxp), p(add), None, *shape, None) == 0
        assert L.dc_conv1x1_wgrad(p(x), p(gy), p(dwp), p(wsw), *shape, None) == 0
    torch.cuda.synchronize()
    for name, a, b in (("y", y, yp), ("dx", dx, dxp), ("dw", dw, dwp)):
        assert torch.isfinite(b).all(), name
        assert torch.equal(a, b), (name, shape, mode, fam)


@pytest.mark.parametrize("groups", [1, 2])
def test_folded_passes_fill_their_partials_and_agree_across_modes(L, groups):
    """relu(bn(x)) in the loader + statistics epilogue (forward), BatchNorm-backward epilogue (data gradient), the loader again (weight
    gradient), through bnfold._K1 with NaN-filled outputs and partial buffers of dc_pointwise_*_parts size.  Mode 1 against mode 0
    to the bounds tests/test_bnfold_gpu.py holds the folded chain to: outputs rtol 2e-4 / atol 2e-5 and gradients 3e-4 in norm
    (test_conv_bn_relu_conv_chain_vs_torch), summed statistics partials rtol 1e-4 / atol 1e-3 (test_stats_epilogue_...).  The two
    families lay their partials out differently (other counts per group), so the partials are compared summed per channel."""
    from depthcore import _lib, bnfold
    K = bnfold._K1
    shape = B, Ci, Co, H, W, s = 2, 64, 96, 4, 8, 1
    g = torch.Generator().manual_seed(11 + groups)
    x = torch.randn(B, Ci, H, W, generator=g).to(DEV)
    w = (torch.randn(Co, Ci, generator=g) / Ci ** 0.5).to(DEV)
    gy = torch.randn(B, Co, H, W, generator=g).to(DEV)
    gamma, beta = (torch.rand(Ci, generator=g) + 0.5).to(DEV), (torch.randn(Ci, generator=g) * 0.3).to(DEV)
    xg = x.view(groups, B // groups, Ci, H * W)
    mean = xg.mean((1, 3)).contiguous()                                                    # (groups, Ci)
    scale = (gamma / (xg.var((1, 3), unbiased=False) + 1e-5).sqrt()).contiguous()
    shift = (beta - mean * scale).contiguous()
    res = {}
    for mode in (1, 0):
        L.dc_set_gemm_split(mode)
        f, fb, fw = _lib.BnFold(), _lib.BnFold(), _lib.BnFold()
        f.groups = fb.groups = fw.groups = groups
        f.in_scale = fb.in_scale = fw.in_scale = scale.data_ptr()
        f.in_shift = fb.in_shift = fw.in_shift = shift.data_ptr()
        ppg = ctypes.c_int(0)
        n = K.stat_parts(L, *shape, groups, ctypes.byref(ppg))
        assert n > 0 and ppg.value > 0
        part, y = _nan(Co * n * 2), _nan(B, Co, H, W)
        f.stat_part = part.data_ptr()
        K.fwd(L, x, w, y, *shape, f)
        nb = K.bwd_parts(L, *shape, groups, ctypes.byref(ppg))
        assert nb > 0 and ppg.value > 0
        bpart, dx = _nan(Ci * nb * 2), _nan(B, Ci, H, W)
        fb.bwd_part, fb.bn_x, fb.bn_mean = bpart.data_ptr(), x.data_ptr(), mean.data_ptr()
        K.dgrad(L, gy, w, dx, None, *shape, fb)
        dw = _nan(Co, Ci)
        K.wgrad(L, x, gy, dw, *shape, fw)
        torch.cuda.synchronize()
        for name, t in (("stat_part", part), ("bwd_part", bpart), ("y", y), ("dx", dx), ("dw", dw)):
            assert not torch.isnan(t).any(), "%s not fully written (mode %d, %d of %d NaN)" % (name, mode, int(torch.isnan(t).sum()), t.numel())
        res[mode] = (y, part.view(Co, n, 2).double().sum(1).float(), dx, bpart.view(Ci, nb, 2).double().sum(1).float(), dw)
    y1, st1, dx1, bw1, dw1 = res[1]
    y0, st0, dx0, bw0, dw0 = res[0]
    close(y1, y0, rtol=2e-4, atol=2e-5)
    close(st1, st0, rtol=1e-4, atol=1e-3)
    for name, a, b in (("dx", dx1, dx0), ("bwd partial sums", bw1, bw0), ("dw", dw1, dw0)):
        assert rel_l2(a, b) < 3e-4, (name, rel_l2(a, b))
