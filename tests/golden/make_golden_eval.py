"""Writes tests/golden/depth_eval.npz: small scaled disparities and ground truths of two shapes with the results of the
reference's own evaluate_depth.py functions -- batch_post_process_disparity (lines 48-56) on a left / right pair, and the
per-image loop of lines 189-232 with its compute_errors (lines 27-45) for mono-eigen, stereo-eigen and eigen_benchmark.

The two functions are taken from the reference file's source (ast) and run in a namespace holding numpy only: importing
evaluate_depth as a module would pull in cv2, skimage and torchvision.  The loop below is lines 192-232 as written there,
with cv2.resize(x, (w, h)) stated as the half-pixel bilinear of F.interpolate(bilinear, align_corners=False) -- the
sampling INTER_LINEAR uses when upsampling (this project does not depend on cv2).  The reference tree is only read when this
script runs:

    python tests/golden/make_golden_eval.py /path/to/reference
"""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

N, h, w = 5, 12, 40
GT_SHAPES = [(50, 160), (48, 150), (50, 160), (48, 150), (50, 160)]


def reference_functions(ref):
    src = open(os.path.join(ref, "evaluate_depth.py")).read()
    tree = ast.parse(src)
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("compute_errors", "batch_post_process_disparity")]
    ns = {"np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "evaluate_depth.py", "exec"), ns)
    return ns["compute_errors"], ns["batch_post_process_disparity"]


def cv2_resize(x, size):
    wo, ho = size
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32))[None, None]
    return F.interpolate(t, size=(ho, wo), mode="bilinear", align_corners=False)[0, 0].numpy()


def reference_loop(compute_errors, pred_disps, gt_depths, eval_split, disable_median_scaling, pred_depth_scale_factor):
    MIN_DEPTH, MAX_DEPTH = 1e-3, 80
    errors, ratios = [], []
    for i in range(pred_disps.shape[0]):
        gt_depth = gt_depths[i]
        gt_height, gt_width = gt_depth.shape[:2]
        pred_disp = pred_disps[i]
        pred_disp = cv2_resize(pred_disp, (gt_width, gt_height))
        pred_depth = 1 / pred_disp
        if eval_split == "eigen":
            mask = np.logical_and(gt_depth > MIN_DEPTH, gt_depth < MAX_DEPTH)
            crop = np.array([0.40810811 * gt_height, 0.99189189 * gt_height,
                             0.03594771 * gt_width, 0.96405229 * gt_width]).astype(np.int32)
            crop_mask = np.zeros(mask.shape)
            crop_mask[crop[0]:crop[1], crop[2]:crop[3]] = 1
            mask = np.logical_and(mask, crop_mask)
        else:
            mask = gt_depth > 0
        pred_depth = pred_depth[mask]
        gt_depth = gt_depth[mask]
        pred_depth *= pred_depth_scale_factor
        if not disable_median_scaling:
            ratio = np.median(gt_depth) / np.median(pred_depth)
            ratios.append(ratio)
            pred_depth *= ratio
        pred_depth[pred_depth < MIN_DEPTH] = MIN_DEPTH
        pred_depth[pred_depth > MAX_DEPTH] = MAX_DEPTH
        errors.append(compute_errors(gt_depth, pred_depth))
    out = {"errors": np.array(errors, np.float64), "mean": np.array(errors).mean(0)}
    if not disable_median_scaling:
        ratios = np.array(ratios)
        med = np.median(ratios)
        out.update(ratios=ratios.astype(np.float32), med=np.float64(med), std=np.float64(np.std(ratios / med)))
    return out


def main(ref):
    compute_errors, batch_post_process_disparity = reference_functions(ref)
    rng = np.random.RandomState(11)
    lo, rng_d = np.float32(1 / 100.0), np.float32(1 / 0.1 - 1 / 100.0)
    raw = rng.rand(2 * N, h, w).astype(np.float32)
    scaled = (lo + rng_d * raw).astype(np.float32)                      # disp_to_depth's scaled disparity
    left, right = scaled[:N], scaled[N:]                                 # right: the decoder output of the mirrored input
    post = batch_post_process_disparity(left, right[:, :, ::-1])         # fp64
    gts = []
    for Hg, Wg in GT_SHAPES:
        g = np.round((0.5 + 90 * rng.rand(Hg, Wg)) * 4).astype(np.float32) / np.float32(4)    # ties
        g[rng.rand(Hg, Wg) < 0.03] = 5e-4
        g[rng.rand(Hg, Wg) > 0.3] = 0
        gts.append(g.astype(np.float32))
    res = {}
    for name, split, disable, sf in (("mono_eigen", "eigen", False, 1), ("stereo_eigen", "eigen", True, 5.4),
                                     ("mono_benchmark", "eigen_benchmark", False, 1)):
        r = reference_loop(compute_errors, left, gts, split, disable, sf)
        for k, v in r.items():
            res["%s_%s" % (name, k)] = v
    flat = np.concatenate([g.ravel() for g in gts])
    idx = np.flatnonzero(flat).astype(np.int32)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "depth_eval.npz")
    np.savez_compressed(out, left=left, right=right, post=post, gt_shapes=np.array(GT_SHAPES, np.int32), gt_idx=idx,
                        gt_val=flat[idx], **res)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
