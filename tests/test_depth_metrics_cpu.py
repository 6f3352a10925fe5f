"""synthetic_depth_gt's schema, and the depth-metrics restatements of tests/depth_metrics_ref.py against the reference's own
results (tests/golden/depth_metrics.npz, written by tests/golden/make_golden_metrics.py)."""
import os

import numpy as np
import torch

import depth_metrics_ref as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_metrics.npz")


def test_synthetic_depth_gt_schema():
    from depthcore.synthetic import synthetic_depth_gt
    gt = synthetic_depth_gt(2, "cpu", seed=3)
    assert gt.shape == (2, 1, 375, 1242) and gt.dtype == torch.float32 and gt.is_contiguous()
    ret = gt > 0
    assert 0.03 < ret.float().mean().item() < 0.07                        # density 0.05
    assert ((gt > 0) & (gt < 1e-3)).any() and (gt > 80).any()               # both masks have something to drop
    assert (gt[ret] <= 120).all()
    inside = gt[(gt > 1e-3) & (gt < 80)]
    assert inside.unique().numel() < inside.numel() // 2                    # quantised to 1/256 m: heavy ties
    assert torch.equal(gt, synthetic_depth_gt(2, "cpu", seed=3))
    assert not torch.equal(gt, synthetic_depth_gt(2, "cpu", seed=4))
    small = synthetic_depth_gt(1, "cpu", seed=0, height=40, width=64, density=0.5)
    assert small.shape == (1, 1, 40, 64) and 0.4 < (small > 0).float().mean().item() < 0.6


def _fixture():
    z = np.load(GOLDEN)
    shape = tuple(int(v) for v in z["shape"])
    gt = np.zeros(int(np.prod(shape)), np.float32)
    gt[z["gt_idx"]] = z["gt_val"]
    return z, torch.from_numpy(gt.reshape(shape)), torch.from_numpy(z["pred"]), torch.from_numpy(z["disp"])


def test_trainer_restatement_matches_reference_results():
    z, gt, pred, _ = _fixture()
    crop = tuple(int(v) for v in z["crop"])
    _, _, ratio, m, counts, n = M.trainer_protocol(pred, gt, crop)
    assert ratio.numpy().tobytes() == z["trainer_ratio"].tobytes()
    ref = z["trainer_errors"].astype(np.float64)
    np.testing.assert_allclose(m[:4], ref[:4], rtol=2e-6)
    assert [round(float(a) * n) for a in ref[4:]] == counts


def test_eigen_restatement_ratios_match_numpy_median():
    z, gt, _, disp = _fixture()
    crop = tuple(int(v) for v in z["crop"])
    _, ratios = M.eigen_protocol(disp, gt, crop)
    assert ratios.tobytes() == z["eigen_ratios"].tobytes()
