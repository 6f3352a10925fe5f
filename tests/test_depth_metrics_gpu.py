"""ops.depth_errors (dc_depth_errors) against the restatements of tests/depth_metrics_ref.py: medians / ratios bitwise,
threshold counts exact, continuous metrics within 1e-5 of fp64 and no further from it than the fp32 torch formula."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import depth_metrics_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gt(B, Hg, Wg, seed, density=0.3, ties=True):
    g = torch.Generator().manual_seed(seed)
    gt = 0.5 + 85 * torch.rand(B, 1, Hg, Wg, generator=g)
    if ties:
        gt = torch.round(gt * 4) / 4                       # heavy ties
    keep = torch.rand(B, 1, Hg, Wg, generator=g) < density
    low = torch.rand(B, 1, Hg, Wg, generator=g) < 0.02
    gt = torch.where(low, torch.full((), 5e-4), gt)
    return torch.where(keep, gt, torch.zeros(())).contiguous()


def _check_row(got, want, counts, n, torch32=None):
    got = np.asarray(got, np.float64)
    np.testing.assert_allclose(got[:4], want[:4], rtol=1e-5)
    for k in range(3):                                     # counts exact: the kernel's a_k is fp32(count / n)
        assert np.float32(got[4 + k]) == np.float32(counts[k] / n), (k, got[4 + k], counts[k], n)
    if torch32 is not None:
        for k in range(4):
            assert abs(got[k] - want[k]) <= max(abs(torch32[k] - want[k]), 2.0 ** -23 * abs(want[k])), (k, got[k], want[k], torch32[k])


def _torch32(g, p):
    from layers import compute_depth_errors
    return np.array([float(v) for v in compute_depth_errors(g, p)])


@pytest.mark.parametrize("B,Hg,Wg,seed,ties", [(2, 375, 1242, 0, True), (3, 120, 200, 1, True), (1, 64, 97, 2, False),
                                               (2, 64, 96, 5, False)])
def test_trainer_same_size_bitwise(B, Hg, Wg, seed, ties):
    from depthcore import ops
    gt = _gt(B, Hg, Wg, seed, ties=ties)
    g = torch.Generator().manual_seed(100 + seed)
    pred = 0.5 + 90 * torch.rand(B, 1, Hg, Wg, generator=g)
    if ties:
        pred = torch.round(pred * 8) / 8
    crop = M.TRAINER_CROP if Hg == 375 else (3, Hg - 5, 4, Wg - 3)
    gv, pv, ratio, want, counts, n = M.trainer_protocol(pred, gt, crop)
    out, ratios, _ = ops._depth_errors(pred.to(DEV), gt.to(DEV), "trainer", crop, True, 1.0)
    assert ratios.cpu().numpy().tobytes() == ratio.numpy().reshape(1).tobytes()
    _check_row(out[0].cpu().numpy(), want, counts, n, _torch32(gv, pv))
    got = ops.depth_errors(pred.to(DEV), gt.to(DEV), "trainer", crop)
    assert got.shape == (7,) and got.is_cuda


def test_trainer_odd_and_even_n():
    from depthcore import ops
    for extra in (0, 1):
        gt = torch.zeros(1, 1, 16, 16)
        vals = torch.tensor([3.0, 3.0, 5.0, 7.0, 7.0, 7.0, 9.0, 11.0, 2.0][:8 + extra])
        gt.view(-1)[torch.arange(vals.numel()) * 3] = vals
        pred = torch.full((1, 1, 16, 16), 4.0)
        pred.view(-1)[::5] = 6.0
        _, _, ratio, want, counts, n = M.trainer_protocol(pred, gt, (0, 16, 0, 16))
        assert n == 8 + extra
        out, ratios, _ = ops._depth_errors(pred.to(DEV), gt.to(DEV), "trainer", (0, 16, 0, 16), True, 1.0)
        assert ratios.cpu().numpy().tobytes() == ratio.numpy().reshape(1).tobytes()
        _check_row(out[0].cpu().numpy(), want, counts, n)


@pytest.mark.parametrize("B,Hg,Wg,seed,scaling,sf", [(3, 375, 1242, 3, True, 1.0), (2, 100, 150, 4, True, 5.4),
                                                     (2, 100, 150, 6, False, 1.0), (2, 31, 45, 7, True, 1.0)])
def test_eigen_same_size_per_image(B, Hg, Wg, seed, scaling, sf):
    from depthcore import ops
    gt = _gt(B, Hg, Wg, seed)
    g = torch.Generator().manual_seed(200 + seed)
    disp = torch.round((0.01 + torch.rand(B, 1, Hg, Wg, generator=g)) * 64) / 64          # ties in the prediction too
    rows, ratios = M.eigen_protocol(disp, gt, None, scaling, sf)
    out, r = ops.depth_errors(disp.to(DEV), gt.to(DEV), "eigen", median_scaling=scaling, scale_factor=sf)
    assert out.shape == (B, 7) and r.shape == (B,)
    assert r.cpu().numpy().tobytes() == ratios.tobytes()
    for i in range(B):
        want, counts, n = rows[i]
        _check_row(out[i].cpu().numpy(), want, counts, n)


def test_eigen_even_n_upper_middle():
    """numpy's even-n median: the upper middle is a tie with the lower one, or the minimum of the values above it."""
    from depthcore import ops
    gt = torch.zeros(2, 1, 40, 40)
    gt[0, 0, 20, 5:9] = torch.tensor([2.0, 4.0, 6.0, 8.0])            # n = 4, no tie: (4 + 6) / 2
    gt[1, 0, 20, 5:9] = torch.tensor([2.0, 4.0, 4.0, 8.0])            # n = 4, tie: 4
    disp = torch.full((2, 1, 40, 40), 0.25)
    disp[:, 0, 20, 5:9] = torch.tensor([0.3, 0.7, 0.1, 0.9])
    crop = (0, 40, 0, 40)
    rows, ratios = M.eigen_protocol(disp, gt, crop)
    _, r = ops.depth_errors(disp.to(DEV), gt.to(DEV), "eigen", crop=crop)
    assert r.cpu().numpy().tobytes() == ratios.tobytes()


def test_upsampled_bitwise_vs_dc_upsample_and_close_to_interpolate():
    from depthcore import ops
    B, h, w, Hg, Wg = 2, 48, 160, 375, 1242
    gt = _gt(B, Hg, Wg, 9, density=0.1)
    g = torch.Generator().manual_seed(9)
    depth = 1.0 + 60 * torch.rand(B, 1, h, w, generator=g)
    up = ops.upsample_bilinear(depth.to(DEV), Hg, Wg).cpu()
    _, _, ratio, want, counts, n = M.trainer_protocol(up, gt)
    out, ratios, _ = ops._depth_errors(depth.to(DEV), gt.to(DEV), "trainer", None, True, 1.0)
    assert ratios.cpu().numpy().tobytes() == ratio.numpy().reshape(1).tobytes()
    _check_row(out[0].cpu().numpy(), want, counts, n)
    # against the framework's CPU interpolation: a tolerance
    _, _, _, want2, _, _ = M.trainer_protocol(F.interpolate(depth, [Hg, Wg], mode="bilinear", align_corners=False), gt)
    got = out[0].cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(got[:4], want2[:4], rtol=1e-5)
    np.testing.assert_allclose(got[4:], want2[4:], atol=1e-4)
    # eigen on upsampled disparity
    disp = 0.02 + torch.rand(B, 1, h, w, generator=g)
    upd = ops.upsample_bilinear(disp.to(DEV), Hg, Wg).cpu()
    rows, rat = M.eigen_protocol(upd, gt)
    out_e, r = ops.depth_errors(disp.to(DEV), gt.to(DEV), "eigen")
    assert r.cpu().numpy().tobytes() == rat.tobytes()
    for i in range(B):
        _check_row(out_e[i].cpu().numpy(), *rows[i])


def test_two_calls_bitwise_identical():
    from depthcore import ops
    from depthcore.synthetic import synthetic_depth_gt
    gt = synthetic_depth_gt(4, DEV, seed=1)
    pred = 1.0 + 50 * torch.rand(4, 1, 192, 640, device=DEV)
    a = ops.depth_errors(pred, gt)
    b = ops.depth_errors(pred, gt)
    assert torch.equal(a, b)
    e1, r1 = ops.depth_errors(1 / pred, gt, "eigen")
    e2, r2 = ops.depth_errors(1 / pred, gt, "eigen")
    assert torch.equal(e1, e2) and torch.equal(r1, r2)


def test_empty_mask_and_cpu_refusal():
    from depthcore import ops
    from depthcore._lib import DepthcoreError
    gt = _gt(3, 60, 80, 11)
    gt[1] = 0.0
    pred = 1.0 + torch.rand(3, 1, 60, 80)
    with pytest.raises(DepthcoreError, match="image 1"):
        ops.depth_errors(pred.to(DEV), gt.to(DEV), "eigen", crop=(0, 60, 0, 80))
    with pytest.raises(DepthcoreError, match="no pixel"):
        ops.depth_errors(pred.to(DEV), torch.zeros_like(gt).to(DEV), "trainer", crop=(0, 60, 0, 80))
    with pytest.raises(DepthcoreError):
        ops.depth_errors(pred, gt)
