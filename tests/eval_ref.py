"""Restatement of the reference's evaluate_depth.py for the tests of depthcore.evaluate / ops.post_process_disparity /
ops.depth_png16, in numpy, in the reference's own types:
  post_process64   -- batch_post_process_disparity (lines 48-56): fp32 mean, fp64 masks and products, fp64 result;
  resize           -- the resize to the gt's size (line 198), stated as F.interpolate(bilinear, align_corners=False): the
                      half-pixel sampling of cv2.resize(INTER_LINEAR) (cv2 is not a dependency of this project);
  compute_errors   -- lines 27-45 (numpy, on the fp32 vectors: fp32 means as there);
  evaluate_loop    -- lines 189-232: per image mask / median scaling / clamp / errors, then the means and ratio statistics;
  png16            -- lines 165-169 on an already resized disparity.
Inputs are host arrays."""
import numpy as np
import torch
import torch.nn.functional as F

MIN_DEPTH, MAX_DEPTH = 1e-3, 80
STEREO_SCALE_FACTOR = 5.4


def post_process64(l_disp, r_disp):
    """l_disp, r_disp: (N,h,w) fp32, r_disp already mirrored back (pred_disp[N:, :, ::-1]) -> (N,h,w) fp64."""
    _, h, w = l_disp.shape
    m_disp = 0.5 * (l_disp + r_disp)
    l, _ = np.meshgrid(np.linspace(0, 1, w), np.linspace(0, 1, h))
    l_mask = (1.0 - np.clip(20 * (l - 0.05), 0, 1))[None, ...]
    r_mask = l_mask[:, :, ::-1]
    return r_mask * l_disp + l_mask * r_disp + (1.0 - l_mask - r_mask) * m_disp


def resize(disp, Hg, Wg):
    """(h,w) fp32 -> (Hg,Wg) fp32, half-pixel bilinear."""
    t = torch.from_numpy(np.ascontiguousarray(disp, np.float32))[None, None]
    return F.interpolate(t, size=(Hg, Wg), mode="bilinear", align_corners=False)[0, 0].numpy()


def compute_errors(gt, pred):
    thresh = np.maximum((gt / pred), (pred / gt))
    a1 = (thresh < 1.25).mean()
    a2 = (thresh < 1.25 ** 2).mean()
    a3 = (thresh < 1.25 ** 3).mean()
    rmse = np.sqrt(((gt - pred) ** 2).mean())
    rmse_log = np.sqrt(((np.log(gt) - np.log(pred)) ** 2).mean())
    abs_rel = np.mean(np.abs(gt - pred) / gt)
    sq_rel = np.mean(((gt - pred) ** 2) / gt)
    return abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3


def eigen_crop(Hg, Wg):
    return np.array([0.40810811 * Hg, 0.99189189 * Hg, 0.03594771 * Wg, 0.96405229 * Wg]).astype(np.int32)


def masked(gt_depth, pred_depth, split):
    """The mask of lines 201-211 applied to both -> (gt vector, pred vector)."""
    if split == "eigen":
        Hg, Wg = gt_depth.shape
        mask = np.logical_and(gt_depth > MIN_DEPTH, gt_depth < MAX_DEPTH)
        crop = eigen_crop(Hg, Wg)
        crop_mask = np.zeros(mask.shape)
        crop_mask[crop[0]:crop[1], crop[2]:crop[3]] = 1
        mask = np.logical_and(mask, crop_mask)
    else:
        mask = gt_depth > 0
    return gt_depth[mask], pred_depth[mask]


def scored(gt_depth, pred_disp, split, median_scaling=True, scale_factor=1.0):
    """Lines 194-223 for one image whose disparity is already at gt's size -> (gt vector, final pred vector, ratio or None)."""
    gt, pred = masked(gt_depth, 1 / pred_disp, split)
    pred *= scale_factor
    ratio = None
    if median_scaling:
        ratio = np.median(gt) / np.median(pred)
        pred *= ratio
    pred[pred < MIN_DEPTH] = MIN_DEPTH
    pred[pred > MAX_DEPTH] = MAX_DEPTH
    return gt, pred, ratio


def evaluate_loop(pred_disps, gt_depths, split, median_scaling=True, scale_factor=1.0, resized=None):
    """Lines 189-232.  pred_disps (N,h,w), gt_depths N (Hg,Wg) fp32 maps; `resized` (optional) the disparities already at the
    gt sizes.  -> dict(errors (N,7) fp64, ratios fp32 or None, mean_errors, ratio_median, ratio_std, counts, n)."""
    errors, ratios, counts, ns = [], [], [], []
    for i in range(len(gt_depths)):
        gt_depth = np.asarray(gt_depths[i])
        Hg, Wg = gt_depth.shape[:2]
        disp = resized[i] if resized is not None else resize(pred_disps[i], Hg, Wg)
        gt, pred, ratio = scored(gt_depth, disp, split, median_scaling, scale_factor)
        if ratio is not None:
            ratios.append(ratio)
        errors.append(compute_errors(gt, pred))
        th = np.maximum(gt / pred, pred / gt)
        counts.append([int((th < t).sum()) for t in (1.25, 1.25 ** 2, 1.25 ** 3)])
        ns.append(gt.size)
    out = {"errors": np.array(errors, np.float64), "mean_errors": np.array(errors).mean(0), "ratios": None,
           "ratio_median": None, "ratio_std": None, "counts": np.array(counts), "n": np.array(ns)}
    if median_scaling:
        ratios = np.array(ratios)
        med = np.median(ratios)
        out.update(ratios=ratios, ratio_median=med, ratio_std=np.std(ratios / med))
    return out


def png16(disp_resized, scale=STEREO_SCALE_FACTOR):
    depth = scale / disp_resized
    depth = np.clip(depth, 0, 80)
    return np.uint16(depth * 256)
