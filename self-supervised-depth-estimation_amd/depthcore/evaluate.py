"""Depth evaluation of a trained model: the reference's evaluate_depth.py (lines 59-235) as two library calls.

  predict_disparities  -- lines 95-135: the networks in eval mode under no_grad, disp_to_depth's scaled disparity of every
                          image, optionally flip post-processed (ops.flip_concat, ops.post_process_disparity);
  evaluate_depth       -- lines 189-235: per image, the disparity upsampled to the ground truth's size, depth = 1 / disp,
                          the split's mask, median scaling or a fixed scale factor, the clamp and the seven errors
                          (ops.depth_errors), then the mean over the images and the statistics of the median ratios.

Everything that touches a pixel runs on depthcore's kernels; the host sees the (N, 7) errors and (N,) ratios only.
The drop-in script `evaluate_depth.py` next to `trainer.py` wraps both with the reference's options."""
import collections

import numpy as np
import torch

from . import _lib, ops
from ._lib import check, ptr, stream

METRIC_NAMES = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")
MIN_DEPTH, MAX_DEPTH = 1e-3, 80.0                 # evaluate_depth.py:62-63


def _batches(images, batch_size):
    if torch.is_tensor(images):
        for i0 in range(0, images.shape[0], batch_size):
            yield images[i0:i0 + batch_size]
    else:
        yield from images


def _scaled_disparity(disp, dst, post_process, min_depth, max_depth):
    """disp_to_depth's scaled disparity of the decoder output `disp`, or its post-processed blend, written into `dst`."""
    L = _lib.lib()
    d = disp if disp.is_contiguous() else disp.contiguous()
    if post_process:
        B, _, h, w = dst.shape
        check(L.dc_disp_post_process(ptr(d), ptr(dst), B, h, w, float(min_depth), float(max_depth), stream(d)), "dc_disp_post_process")
    else:
        check(L.dc_disp_to_depth_fwd(ptr(d), ptr(dst), None, d.numel(), float(min_depth), float(max_depth), stream(d)),
              "dc_disp_to_depth_fwd")


def predict_disparities(encoder, decoder, images, min_depth=0.1, max_depth=100.0, post_process=False, batch_size=16):
    """evaluate_depth.py:116-136 -> (N,1,h,w) scaled disparities on the device.

    `images`: (N,3,h,w) float32 device tensor at the networks' resolution (already resized), or an iterable of such batches
    (batch_size is then the iterable's).  The modules run in eval mode under no_grad; every submodule's `training` flag is
    restored on exit, and parameters and BatchNorm running statistics are not touched (eval-mode BatchNorm reads them).
    post_process: each batch is run as [x; flip_w(x)] and the two halves blended (batch_post_process_disparity)."""
    if batch_size <= 0:
        raise ValueError("batch_size must be positive")
    flags = [(m, m.training) for net in (encoder, decoder) for m in net.modules()]
    outs = []
    out = None
    try:
        encoder.eval()
        decoder.eval()
        with torch.no_grad():
            if torch.is_tensor(images):
                if images.dim() != 4 or images.shape[1] != 3 or images.dtype != torch.float32 or not images.is_cuda:
                    raise _lib.DepthcoreError("predict_disparities: images must be a (N,3,h,w) float32 device tensor, got %s %s on %s"
                                              % (tuple(images.shape), images.dtype, images.device))
                out = torch.empty((images.shape[0], 1) + tuple(images.shape[2:]), dtype=torch.float32, device=images.device)
            row = 0
            for x in _batches(images, batch_size):
                x = x if x.is_contiguous() else x.contiguous()
                B = x.shape[0]
                disp = decoder(encoder(ops.flip_concat(x) if post_process else x))[("disp", 0)]
                if out is not None:
                    dst = out[row:row + B]
                else:
                    dst = torch.empty((B, 1) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
                    outs.append(dst)
                _scaled_disparity(disp, dst, post_process, min_depth, max_depth)
                row += B
    finally:
        for m, t in flags:
            m.training = t
    if out is not None:
        return out
    if not outs:
        raise ValueError("predict_disparities: no images")
    if any(o.shape[1:] != outs[0].shape[1:] for o in outs):
        raise _lib.DepthcoreError("predict_disparities: the batches differ in their image size")
    return ops.stack_frames([outs])[0]


def evaluate_depth(pred_disps, gt_depths, split="eigen", median_scaling=True, scale_factor=1.0, chunk=32):
    """evaluate_depth.py:189-235 on the device.

    pred_disps: (N,1,h,w) (or (N,h,w)) scaled disparities -- a device tensor, or host data that is copied over.
    gt_depths:  N ground-truth depth maps (Hg,Wg), any mix of shapes (KITTI's frame size varies by drive), compared in fp32.
    split:      "eigen" -> 1e-3 < gt < 80 inside the fractional Eigen crop; any other split -> gt > 0 on the whole frame
                (eigen_benchmark); "odom_*" raises ValueError (pose evaluation, evaluate_pose.py).
    median_scaling=False, scale_factor: --disable_median_scaling, --pred_depth_scale_factor (stereo: False and 5.4).
    Images are grouped by gt shape and scored `chunk` at a time, one dc_depth_errors launch chain per chunk.
    -> dict(errors (N,7) float32 per image, ratios (N,) float32 or None, mean_errors (7,) float64 -- the mean over the images,
    ratio_median = np.median(ratios), ratio_std = np.std(ratios / ratio_median) (None without median scaling), names)."""
    if split.startswith("odom"):
        raise ValueError("split %r: the odometry splits are pose evaluation (evaluate_pose.py), not depth" % split)
    protocol = "eigen" if split == "eigen" else "gt_positive"
    if not torch.is_tensor(pred_disps):
        pred_disps = torch.from_numpy(np.ascontiguousarray(pred_disps, np.float32))
    if pred_disps.dim() == 3:
        pred_disps = pred_disps.unsqueeze(1)
    if not pred_disps.is_cuda:
        pred_disps = pred_disps.to(torch.device("cuda", torch.cuda.current_device()))
    if pred_disps.dtype != torch.float32 or pred_disps.dim() != 4 or pred_disps.shape[1] != 1:
        raise _lib.DepthcoreError("evaluate_depth: pred_disps must be (N,1,h,w) float32, got %s %s"
                                  % (tuple(pred_disps.shape), pred_disps.dtype))
    pred = pred_disps if pred_disps.is_contiguous() else pred_disps.contiguous()
    N = pred.shape[0]
    if len(gt_depths) != N:
        raise ValueError("evaluate_depth: %d predictions for %d ground-truth maps" % (N, len(gt_depths)))
    groups = collections.OrderedDict()
    for i in range(N):
        shape = tuple(np.shape(gt_depths[i]))[:2]
        groups.setdefault(shape, []).append(i)
    errors = np.empty((N, 7), np.float32)
    ratios = np.empty(N, np.float32)
    for shape, idx in groups.items():
        for c0 in range(0, len(idx), chunk):
            ids = idx[c0:c0 + chunk]
            gt = np.stack([np.asarray(gt_depths[i], np.float32).reshape(shape) for i in ids])[:, None]
            gt = torch.from_numpy(gt).to(pred.device)
            if ids[-1] - ids[0] == len(ids) - 1:
                p = pred[ids[0]:ids[-1] + 1]
            else:
                p = ops.stack_frames([[pred[i:i + 1] for i in ids]])[0]
            _, _, host = ops._depth_errors(p, gt, protocol, None, median_scaling, scale_factor, image_ids=ids)
            G = len(ids)
            errors[ids] = host[:G * 7].view(G, 7).numpy()
            ratios[ids] = host[G * 7:G * 8].numpy()
    res = {"names": METRIC_NAMES, "errors": errors, "mean_errors": errors.astype(np.float64).mean(0),
           "ratios": None, "ratio_median": None, "ratio_std": None}
    if median_scaling:
        med = np.median(ratios)                                   # evaluate_depth.py:228-230, fp32 as there
        res.update(ratios=ratios, ratio_median=float(med), ratio_std=float(np.std(ratios / med)))
    return res
