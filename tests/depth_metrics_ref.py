"""Restatements of the two depth-evaluation protocols for the tests of ops.depth_errors / Trainer.compute_depth_losses, written
from the reference's lines in plain torch / numpy fp32 (the selection and ratio steps) and fp64 (the metrics):
  trainer  -- trainer.py:624-652: clamp [1e-3, 80], gt > 0 inside crop, torch.median (lower middle) over the whole batch;
  eigen    -- evaluate_depth.py:198-232: depth = 1 / disp * scale_factor, 1e-3 < gt < 80 inside the fractional crop,
              np.median (fp32 mean of the two middles) per image.
Inputs are CPU tensors; `pred_up` is the prediction ALREADY at gt's resolution."""
import numpy as np
import torch

TRAINER_CROP = (153, 371, 44, 1197)


def eigen_crop(Hg, Wg):
    c = np.array([0.40810811 * Hg, 0.99189189 * Hg, 0.03594771 * Wg, 0.96405229 * Wg]).astype(np.int32)
    return tuple(int(v) for v in c)


def metrics64(gt, pred):
    """The seven metrics of layers.py:251-269 in fp64 from fp32 vectors; the thresholds on the fp32 ratio (as the reference);
    also returns the three threshold counts."""
    g32, p32 = np.asarray(gt, np.float32), np.asarray(pred, np.float32)
    th = np.maximum(g32 / p32, p32 / g32)
    counts = [int((th < t).sum()) for t in (np.float32(1.25), np.float32(1.5625), np.float32(1.953125))]
    g, p = g32.astype(np.float64), p32.astype(np.float64)
    n = g.size
    vals = [np.mean(np.abs(g - p) / g), np.mean((g - p) ** 2 / g), np.sqrt(np.mean((g - p) ** 2)),
            np.sqrt(np.mean((np.log(g) - np.log(p)) ** 2))] + [c / n for c in counts]
    return np.array(vals), counts, n


def trainer_protocol(pred_up, gt, crop=TRAINER_CROP):
    """-> (gt vector, scaled pred vector (fp32), ratio (fp32), metrics64, counts, n)."""
    depth_pred = torch.clamp(pred_up.float(), 1e-3, 80)
    mask = gt > 0
    crop_mask = torch.zeros_like(mask)
    crop_mask[:, :, crop[0]:crop[1], crop[2]:crop[3]] = 1
    mask = mask * crop_mask
    g = gt[mask]
    p = depth_pred[mask]
    ratio = torch.median(g) / torch.median(p)
    p = p * ratio
    p = torch.clamp(p, min=1e-3, max=80)
    m, counts, n = metrics64(g.numpy(), p.numpy())
    return g, p, ratio, m, counts, n


def eigen_protocol(disp_up, gt, crop=None, median_scaling=True, scale_factor=1.0):
    """Per image -> list of (metrics64, counts, n), ratios (fp32 numpy)."""
    rows, ratios = [], []
    for i in range(gt.shape[0]):
        gt_depth = gt[i, 0].numpy()
        Hg, Wg = gt_depth.shape
        pred_depth = np.float32(1) / disp_up[i, 0].numpy()
        mask = np.logical_and(gt_depth > 1e-3, gt_depth < 80)
        c = crop if crop is not None else eigen_crop(Hg, Wg)
        crop_mask = np.zeros(mask.shape)
        crop_mask[c[0]:c[1], c[2]:c[3]] = 1
        mask = np.logical_and(mask, crop_mask)
        pred_depth = pred_depth[mask]
        gt_depth = gt_depth[mask]
        pred_depth *= np.float32(scale_factor)
        ratio = np.float32(1.0)
        if median_scaling:
            ratio = np.median(gt_depth) / np.median(pred_depth)
            pred_depth *= ratio
        pred_depth[pred_depth < 1e-3] = 1e-3
        pred_depth[pred_depth > 80] = 80
        rows.append(metrics64(gt_depth, pred_depth))
        ratios.append(np.float32(ratio))
    return rows, np.array(ratios, np.float32)
