"""Writes tests/golden/depth_metrics.npz: a small sparse depth_gt and two predictions with the results of the reference's
own code -- layers.compute_depth_errors (layers.py:251-269) after the steps of trainer.py:624-652, and numpy's median for the
Eigen protocol's ratio (evaluate_depth.py:221-222).  The reference tree is only read when this script runs:

    python tests/golden/make_golden_metrics.py /path/to/reference
"""
import os
import sys

import numpy as np
import torch


def main(ref):
    sys.path.insert(0, ref)
    from layers import compute_depth_errors          # the reference's
    g = torch.Generator().manual_seed(7)
    B, Hg, Wg = 2, 48, 80
    crop = (5, 43, 3, 77)
    gt = torch.round((2 + 60 * torch.rand(B, 1, Hg, Wg, generator=g)) * 256) / 256
    keep = torch.rand(B, 1, Hg, Wg, generator=g) < 0.2
    gt = torch.where(keep, gt, torch.zeros(()))
    pred = 1.0 + 50 * torch.rand(B, 1, Hg, Wg, generator=g)                 # depth, already at gt's size
    disp = 0.01 + torch.rand(B, 1, Hg, Wg, generator=g)                      # scaled disparity
    # trainer.py:624-652
    depth_pred = torch.clamp(pred, 1e-3, 80)
    mask = gt > 0
    crop_mask = torch.zeros_like(mask)
    crop_mask[:, :, crop[0]:crop[1], crop[2]:crop[3]] = 1
    mask = mask * crop_mask
    dg, dp = gt[mask], depth_pred[mask]
    ratio = torch.median(dg) / torch.median(dp)
    dp = torch.clamp(dp * ratio, min=1e-3, max=80)
    errs = np.array([float(e) for e in compute_depth_errors(dg, dp)], np.float32)
    # evaluate_depth.py:221-222, per image (mask 1e-3 < gt < 80 inside the same crop)
    eig = []
    for i in range(B):
        gd = gt[i, 0].numpy()
        m = np.logical_and(gd > 1e-3, gd < 80)
        cm = np.zeros(m.shape)
        cm[crop[0]:crop[1], crop[2]:crop[3]] = 1
        m = np.logical_and(m, cm)
        eig.append(np.median(gd[m]) / np.median((np.float32(1) / disp[i, 0].numpy())[m]))
    idx = np.flatnonzero(gt.numpy().ravel()).astype(np.int32)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "depth_metrics.npz")
    np.savez_compressed(out, shape=np.array([B, 1, Hg, Wg], np.int32), crop=np.array(crop, np.int32), gt_idx=idx,
                        gt_val=gt.numpy().ravel()[idx], pred=pred.numpy(), disp=disp.numpy(), trainer_errors=errs,
                        trainer_ratio=np.float32(ratio), eigen_ratios=np.array(eig, np.float32))
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
