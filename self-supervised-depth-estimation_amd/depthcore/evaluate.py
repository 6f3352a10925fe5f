"""Evaluation of trained models: the reference's evaluate_depth.py (lines 59-235) and evaluate_pose.py (lines 49-129), each as two
library calls.

  predict_disparities  -- lines 95-135: the networks in eval mode under no_grad, disp_to_depth's scaled disparity of every
                          image, optionally flip post-processed (ops.flip_concat, ops.post_process_disparity);
  evaluate_depth       -- lines 189-235: per image, the disparity upsampled to the ground truth's size, depth = 1 / disp,
                          the split's mask, median scaling or a fixed scale factor, the clamp and the seven errors
                          (ops.depth_errors), then the mean over the images and the statistics of the median ratios.

  predict_poses        -- evaluate_pose.py:89-102: every consecutive frame pair of a sequence through the pose network in eval
                          mode, the pair formed by the stem kernel's loader (ResnetEncoder.forward_pair);
  evaluate_pose        -- evaluate_pose.py:104-125: the absolute trajectory error of every snippet (ops.pose_ate).

  render_disparities   -- test_simple.py:126-145: the colour image of every disparity map at its photo's size (ops.render_disparity).

Everything that touches a pixel runs on depthcore's kernels; the host sees the (N, 7) errors and (N,) ratios, or the (N,) ATEs
with their mean and std, or the RGB bytes and two floats per image, only.  The drop-in scripts `evaluate_depth.py` /
`evaluate_pose.py` / `test_simple.py` next to `trainer.py` wrap them with the reference's options."""
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
        raise ValueError("split %r: the odometry splits are pose evaluation (evaluate_pose / evaluate_pose.py), not depth" % split)
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


def _pair_groups(frames, batch_size):
    """(f_a, f_b) views of up to batch_size consecutive pairs: f_a[b], f_b[b] are frames i+b, i+b+1 of the sequence.  A tensor is
    sliced in place.  Chunks of an iterable are gathered in a staging buffer of batch_size + 1 frames whose last frame is
    carried over to slot 0 -- the same groups as for the tensor, whatever the chunk sizes; no pair tensor either way."""
    if torch.is_tensor(frames):
        for i0 in range(0, frames.shape[0] - 1, batch_size):
            b = min(batch_size, frames.shape[0] - 1 - i0)
            yield frames[i0:i0 + b], frames[i0 + 1:i0 + b + 1]
        return
    buf, k = None, 0
    for chunk in frames:
        if chunk.dim() != 4 or chunk.shape[1] != 3 or chunk.dtype != torch.float32:
            raise _lib.DepthcoreError("predict_poses: a chunk must be (n,3,h,w) float32, got %s %s" % (tuple(chunk.shape), chunk.dtype))
        if buf is None:
            if not chunk.is_cuda:
                raise _lib.DepthcoreError("predict_poses: frames must live on the device (got %s)" % chunk.device)
            buf = torch.empty((batch_size + 1, 3) + tuple(chunk.shape[2:]), dtype=torch.float32, device=chunk.device)
        if chunk.shape[2:] != buf.shape[2:]:
            raise _lib.DepthcoreError("predict_poses: the chunks differ in their image size")
        c0 = 0
        while c0 < chunk.shape[0]:
            n = min(batch_size + 1 - k, chunk.shape[0] - c0)
            buf[k:k + n].copy_(chunk[c0:c0 + n])                     # staging copy
            k, c0 = k + n, c0 + n
            if k == batch_size + 1:
                yield buf[:batch_size], buf[1:]
                buf[0:1].copy_(buf[batch_size:])                     # staging copy: the carried frame
                k = 1
    if k >= 2:
        yield buf[:k - 1], buf[1:k]


def predict_poses(pose_encoder, pose_decoder, frames, batch_size=16):
    """evaluate_pose.py:89-102 -> (N,4,4) float32 source-to-target transforms on the device, one per consecutive frame pair.

    `frames`: the N+1 consecutive frames of a sequence at the network's resolution -- a (N+1,3,h,w) float32 device tensor, or an
    iterable of chunks (n,3,h,w) of consecutive frames.  Pair i goes in as (frame i, frame i+1) and its matrix is
    transformation_from_parameters(axisangle[:, 0], translation[:, 0]), not inverted (lines 94-100).  The networks are the ones
    the reference evaluates: ResnetEncoder(num_layers, False, 2) and PoseDecoder(num_ch_enc, 1, 2).  They run in eval mode
    under no_grad; every submodule's `training` flag is restored on exit, and parameters and BatchNorm running statistics are
    not touched (the contract of predict_disparities)."""
    if batch_size <= 0:
        raise ValueError("batch_size must be positive")
    if not hasattr(pose_encoder, "forward_pair") or not hasattr(pose_decoder, "forward_poses"):
        raise NotImplementedError("predict_poses evaluates ResnetEncoder(num_layers, False, 2) + PoseDecoder(num_ch_enc, 1, 2) "
                                  "(--pose_model_type separate_resnet), as the reference's evaluate_pose.py does")
    if torch.is_tensor(frames) and (frames.dim() != 4 or frames.shape[1] != 3 or frames.dtype != torch.float32 or not frames.is_cuda):
        raise _lib.DepthcoreError("predict_poses: frames must be a (N+1,3,h,w) float32 device tensor, got %s %s on %s"
                                  % (tuple(frames.shape), frames.dtype, frames.device))
    flags = [(m, m.training) for net in (pose_encoder, pose_decoder) for m in net.modules()]
    outs = []
    try:
        pose_encoder.eval()
        pose_decoder.eval()
        with torch.no_grad():
            for f_a, f_b in _pair_groups(frames, batch_size):
                features = [pose_encoder.forward_pair(f_a, f_b)]
                outs.append(pose_decoder.forward_poses(features, [(0, f_a.shape[0], 0, 0)])[2][0])
    finally:
        for m, t in flags:
            m.training = t
    if not outs:
        raise ValueError("predict_poses: a sequence needs at least two frames")
    return outs[0] if len(outs) == 1 else ops.stack_frames([outs])[0]


def evaluate_pose(pred_poses, gt_global_poses, track_length=5):
    """evaluate_pose.py:104-125 on the device.

    pred_poses:      (N,4,4) float32 transforms of predict_poses -- a device tensor, or host data that is copied over.
    gt_global_poses: the N+1 global poses of KITTI's poses/XX.txt, (N+1,3,4) or (N+1,12), host or device data; compared in fp64.
    -> dict(ates (N,) float64 -- the absolute trajectory error of the snippet starting at each frame, mean = np.mean(ates),
    std = np.std(ates), track_length).  A snippet whose predicted points all coincide is NaN, as in numpy."""
    if not torch.is_tensor(pred_poses):
        pred_poses = torch.from_numpy(np.ascontiguousarray(pred_poses, np.float32))
    if not torch.is_tensor(gt_global_poses):
        gt_global_poses = torch.from_numpy(np.ascontiguousarray(gt_global_poses, np.float64))
    if pred_poses.dim() != 3 or tuple(pred_poses.shape[1:]) != (4, 4):
        raise ValueError("evaluate_pose: pred_poses must be (N,4,4), got %s" % (tuple(pred_poses.shape),))
    if gt_global_poses.dim() not in (2, 3) or gt_global_poses[0].numel() != 12:
        raise ValueError("evaluate_pose: gt_global_poses must be (M,3,4) or (M,12), got %s" % (tuple(gt_global_poses.shape),))
    N, M = pred_poses.shape[0], gt_global_poses.shape[0]
    if N < 1 or N != M - 1:
        raise ValueError("evaluate_pose: %d predicted transforms (frame pairs) need %d ground-truth poses, got %d" % (N, N + 1, M))
    dev = pred_poses.device if pred_poses.is_cuda else torch.device("cuda", torch.cuda.current_device())
    pred = pred_poses.to(device=dev, dtype=torch.float32)
    gt = gt_global_poses.to(device=dev, dtype=torch.float64).reshape(M, 3, 4)
    ates, mean, std = ops.pose_ate(pred, gt, track_length)
    return {"ates": ates.numpy(), "mean": float(mean), "std": float(std), "track_length": int(track_length)}


def render_disparities(disps, sizes, percentile=95.0, lut=None, chunk=64):
    """test_simple.py:126-145 for N maps -> (images, ranges): images[i] a host uint8 array (Ho_i, Wo_i, 3) -- what
    PIL.Image.fromarray takes -- and ranges (N,2) float32 = (vmin, vmax) of every image, in input order.

    disps: (N,1,h,w) (or (N,h,w)) float32 disparities -- a device tensor, or host data that is copied over.
    sizes: N target sizes (Ho, Wo), any mix (the photos of a folder differ in size), or one (Ho, Wo) for all.
    Images are grouped by target size and rendered `chunk` at a time: one dc_disp_render launch chain and ONE device-to-host
    copy (bytes and ranges together) per chunk.  The upsampled fp32 maps never exist, on either side."""
    if not torch.is_tensor(disps):
        disps = torch.from_numpy(np.ascontiguousarray(disps, np.float32))
    if disps.dim() == 3:
        disps = disps.unsqueeze(1)
    if not disps.is_cuda:
        disps = disps.to(torch.device("cuda", torch.cuda.current_device()))
    if disps.dtype != torch.float32 or disps.dim() != 4 or disps.shape[1] != 1:
        raise _lib.DepthcoreError("render_disparities: disps must be (N,1,h,w) float32, got %s %s" % (tuple(disps.shape), disps.dtype))
    if chunk <= 0:
        raise ValueError("chunk must be positive")
    d = disps if disps.is_contiguous() else disps.contiguous()
    N = d.shape[0]
    if len(sizes) == 2 and all(isinstance(v, (int, np.integer)) for v in sizes):
        sizes = [sizes] * N
    if len(sizes) != N:
        raise ValueError("render_disparities: %d maps for %d sizes" % (N, len(sizes)))
    if lut is not None and not torch.is_tensor(lut):
        lut = torch.from_numpy(np.ascontiguousarray(lut, np.uint8))
    if lut is not None:
        lut = lut.to(d.device)
    groups = collections.OrderedDict()
    for i in range(N):
        groups.setdefault((int(sizes[i][0]), int(sizes[i][1])), []).append(i)
    images = [None] * N
    ranges = np.empty((N, 2), np.float32)
    for (Ho, Wo), idx in groups.items():
        for c0 in range(0, len(idx), chunk):
            ids = idx[c0:c0 + chunk]
            if ids[-1] - ids[0] == len(ids) - 1:
                x = d[ids[0]:ids[-1] + 1]
            else:
                x = ops.stack_frames([[d[i:i + 1] for i in ids]])[0]
            _, _, buf = ops._render_disparity(x, (Ho, Wo), percentile, lut)
            host = buf.cpu().numpy()
            G, nb = len(ids), Ho * Wo * 3
            rgb = host[:G * nb].reshape(G, Ho, Wo, 3)
            ranges[ids] = host[(G * nb + 3) & ~3:].view(np.float32).reshape(G, 2)
            for k, i in enumerate(ids):
                images[i] = rgb[k]
    return images, ranges
