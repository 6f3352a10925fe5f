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


# ---- recurrent front-ends: ConvGRU v5 (evaluate_depth_gru_fusion.py:504-554) and Fusion_v3 (evaluate_depth_fusion_v3.py:131-165) ----
class _EvalMode:
    """predict_disparities' contract as a context: the networks in eval mode under no_grad, every submodule's `training` flag
    restored on exit (also when the body raises)."""

    def __init__(self, *nets):
        self.nets = nets

    def __enter__(self):
        self.flags = [(m, m.training) for net in self.nets for m in net.modules()]
        self.grad = torch.no_grad()
        for net in self.nets:
            net.eval()
        self.grad.__enter__()

    def __exit__(self, *exc):
        self.grad.__exit__(*exc)
        for m, t in self.flags:
            m.training = t
        return False


def _frames_ok(x, what, shape=None):
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32 or not x.is_cuda or \
            (shape is not None and tuple(x.shape[2:]) != tuple(shape)):
        raise _lib.DepthcoreError("%s: frames must be a (B,3,h,w) float32 device tensor%s, got %s" % (
            what, "" if shape is None else " with (h,w) = %s" % (tuple(shape),),
            "%s %s on %s" % (tuple(x.shape), x.dtype, x.device) if torch.is_tensor(x) else type(x).__name__))


def lockstep_groups(lengths, streams):
    """The schedule that advances independent sequences together: -> [(ids, widths)], one entry per group of up to `streams`
    sequences.  `ids` are indices into `lengths`, sorted by length (descending, stable) over ALL sequences and then cut into
    consecutive groups, so a group's members are of similar length; widths[t] is how many of them still have a frame t.  The
    sequences alive at a step are a PREFIX of ids, which is why a step's tensors are prefix slices: no gather, no mask."""
    if streams <= 0:
        raise ValueError("streams must be positive")
    if any(n <= 0 for n in lengths):
        raise ValueError("every sequence needs at least one frame")
    order = sorted(range(len(lengths)), key=lambda i: -lengths[i])
    groups = []
    for g0 in range(0, len(order), streams):
        ids = order[g0:g0 + streams]
        groups.append((ids, [sum(1 for i in ids if lengths[i] > t) for t in range(lengths[ids[0]])]))
    return groups


class SequencePredictor:
    """Streaming inference of the ConvGRU v5 front-end for up to `streams` independent sequences that advance together
    (evaluate_depth_gru_fusion.py:519-548 is one stream): `step(frames)` takes frame t of streams 0..B-1 and returns their
    scaled disparities; the hidden states live here, one (S, C_k, h_k, w_k) buffer per level, and are carried to the next call.

    One step at batch B: the encoder; the five gate convolutions (dc_conv3x3_fwd over cat(features, state[:B]), sigmoid); ONE
    dc_gru_infer_rh; the five candidate convolutions; ONE dc_gru_infer_tail, which rewrites state[:B] in place and leaves
    features + (h_cur + h_prev) / 2; the decoder; dc_disp_to_depth_fwd.  The state buffers are copies (dc_gru_infer_init) of
    the learned `h0_layer1`, which are never written; the gates / r*h / candidate / fused buffers are allocated once, here."""

    def __init__(self, encoder, gru, decoder, streams=16, min_depth=0.1, max_depth=100.0):
        if streams <= 0:
            raise ValueError("streams must be positive")
        self.encoder, self.gru, self.decoder = encoder, gru, decoder
        self.streams, self.min_depth, self.max_depth = int(streams), float(min_depth), float(max_depth)
        cells = gru.cells()
        dev = cells[0].h0_layer1.device
        if dev.type != "cuda":
            raise _lib.DepthcoreError("SequencePredictor runs on depthcore kernels only (the ConvGRU is on %s); there is no CPU path" % dev)

        def buf(mult=1):
            return [torch.empty((self.streams, mult * c.h0_layer1.shape[1]) + tuple(c.h0_layer1.shape[2:]), dtype=torch.float32, device=dev)
                    for c in cells]
        self.state, self.gates, self.rh, self.cnm, self.out = buf(), buf(2), buf(), buf(), buf()
        self._ws = None
        self.reset()

    def reset(self):
        """Every stream back to the learned initial states (as they are now: a later optimiser step is seen by the next reset)."""
        ops.gru_infer_init([c.h0_layer1 for c in self.gru.cells()], self.state)

    def _workspace(self, B):
        L = _lib.lib()
        need = 1
        for s in self.state:
            C, H, W = s.shape[1:]
            need = max(need, L.dc_conv3x3_fwd_workspace(C, C, B, 2 * C, H, W), L.dc_conv3x3_fwd_workspace(C, C, B, C, H, W))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.state[0].device)
        return self._ws.data_ptr()

    def _fuse(self, features):
        L = _lib.lib()
        feats = [f if f.is_contiguous() else f.contiguous() for f in features]
        B = feats[0].shape[0]
        if len(feats) != len(self.state) or any(tuple(f.shape) != (B,) + tuple(s.shape[1:]) for f, s in zip(feats, self.state)):
            raise _lib.DepthcoreError("encoder features %s do not match the ConvGRU's states %s" % (
                [tuple(f.shape) for f in feats], [tuple(s.shape[1:]) for s in self.state]))
        if not 1 <= B <= self.streams:
            raise _lib.DepthcoreError("a step of %d frames on a predictor of %d streams" % (B, self.streams))
        ops._use_precision(ops._precision[0])                    # the caller's ops.matrix_precision, as ops.conv3x3_block
        ws = self._workspace(B)
        st = stream(feats[0])
        for kind, dst, x1, act in (("conv_gates", self.gates, self.state, ops.ACT_SIGMOID), ("conv_can", self.cnm, self.rh, ops.ACT_TANH)):
            for cell, f, s1, y in zip(self.gru.cells(), feats, x1, dst):
                conv = getattr(cell.cgru_1, kind)
                C, H, W = f.shape[1:]
                w, b = conv.weight.detach(), conv.bias.detach()
                # rnn.py:125-134: act(conv(cat(x, h))) / act(conv(cat(x, r*h))), the call ops._GruLevel.forward makes at batch 1
                check(L.dc_conv3x3_fwd(ptr(f), C, 0, ptr(s1), C, ptr(w), ptr(b), ptr(y), ws, B, w.shape[0], H, W, act, ops.PAD_ZERO, st),
                      "dc_conv3x3_fwd")
            if kind == "conv_gates":
                ops.gru_infer_rh(self.gates, self.state, self.rh, B)
        ops.gru_infer_tail(self.gates, self.cnm, feats, self.state, self.out, B)
        return [o[:B] for o in self.out]

    def fuse(self, features):
        """The recurrent part of a step on its own: the encoder features of frame t of streams 0..B-1 -> features + (h_cur +
        h_prev) / 2 per level, as VIEWS of this predictor's buffers (the next call overwrites them); the states advance."""
        with torch.no_grad():
            return self._fuse(features)

    def _step(self, frames):
        _frames_ok(frames, "SequencePredictor.step")
        x = frames if frames.is_contiguous() else frames.contiguous()
        disp = self.decoder(self._fuse(self.encoder(x)))[("disp", 0)]
        dst = torch.empty((x.shape[0], 1) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        _scaled_disparity(disp, dst, False, self.min_depth, self.max_depth)
        return dst

    def step(self, frames):
        """frames (B,3,h,w), B <= streams: frame t of streams 0..B-1 -> (B,1,h,w) scaled disparities; their states advance, the
        states of the streams behind B stay.  predict_disparities' contract holds for every call."""
        with _EvalMode(self.encoder, self.gru, self.decoder):
            return self._step(frames)


def predict_disparities_lockstep(encoder, gru, decoder, lengths, batch_fn, min_depth=0.1, max_depth=100.0, streams=16):
    """The ConvGRU v5 evaluation of several independent scenes that advance in lockstep.  lengths[c]: the frames of scene c;
    batch_fn(t, ids) -> the (len(ids),3,h,w) float32 device tensor that holds frame t of the scenes `ids`, in that order (called
    once per step, so a caller that decodes images holds one step's frames at a time).  -> a list with one (n_c,1,h,w) tensor of
    scaled disparities per scene, in the order of `lengths`.  Schedule: lockstep_groups; contract: predict_disparities'."""
    groups = lockstep_groups(list(lengths), streams)
    outs = [None] * len(lengths)
    with _EvalMode(encoder, gru, decoder):
        sp = SequencePredictor(encoder, gru, decoder, min(streams, max(len(lengths), 1)), min_depth, max_depth)
        for g, (ids, widths) in enumerate(groups):
            if g:
                sp.reset()
            steps = [sp._step(batch_fn(t, ids[:B])) for t, B in enumerate(widths)]
            for c in ids:
                outs[c] = torch.empty((lengths[c],) + tuple(steps[0].shape[1:]), dtype=torch.float32, device=steps[0].device)
            pairs = [(steps[t][b], outs[c][t]) for t, B in enumerate(widths) for b, c in enumerate(ids[:B])]
            ops.copy_segments([p[0] for p in pairs], [p[1] for p in pairs])
    return outs


def predict_disparities_sequences(encoder, gru, decoder, scenes, min_depth=0.1, max_depth=100.0, streams=16):
    """evaluate_v5_seq (evaluate_depth_gru_fusion.py:504-554) for a list of scenes -> a list of (n_c,1,h,w) scaled disparities
    in input order.  scenes[c]: the frames of one scene in order, a (n_c,3,h,w) float32 device tensor at the networks'
    resolution, or a sized iterable that yields them as (1,3,h,w) tensors.  Every scene starts from the learned initial states
    and its state is carried from frame to frame; the scenes are independent of each other, so up to `streams` of them run as
    one batch (predict_disparities_lockstep).  Memory beyond the inputs and the result is O(streams)."""
    scenes = list(scenes)
    if not scenes:
        raise ValueError("predict_disparities_sequences: no scenes")
    lengths = [s.shape[0] if torch.is_tensor(s) else len(s) for s in scenes]
    for s in scenes:
        if torch.is_tensor(s):
            _frames_ok(s, "predict_disparities_sequences")
    its = [None if torch.is_tensor(s) else iter(s) for s in scenes]

    def batch(t, ids):
        rows = [scenes[c][t:t + 1] if its[c] is None else next(its[c]) for c in ids]
        for r in rows:
            _frames_ok(r, "predict_disparities_sequences", rows[0].shape[2:])
        return rows[0] if len(rows) == 1 else ops.stack_frames([rows])[0]
    return predict_disparities_lockstep(encoder, gru, decoder, lengths, batch, min_depth, max_depth, streams)


# ---- ConvLSTM v8 (evaluate_depth_gru_fusion.py:557-618 `evaluate_v8_seq`): every test file is a window of its own -------------
def window_groups(lengths, streams):
    """The right-aligned counterpart of lockstep_groups, for windows that END at the frame that is scored: -> [(ids, widths)].
    `ids` as there (sorted by length, descending and stable, over ALL windows, then cut into consecutive groups of up to
    `streams`).  A group whose longest window has L frames takes L steps; the windows alive at step j are those with
    length >= L - j -- a GROWING prefix of ids, widths[j] of them -- and window c shows its frame j - (L - lengths[c]).  All
    windows of a group reach their last frame together at step L - 1, so the head runs once per group, at full width."""
    if streams <= 0:
        raise ValueError("streams must be positive")
    if any(n <= 0 for n in lengths):
        raise ValueError("every window needs at least one frame")
    order = sorted(range(len(lengths)), key=lambda i: -lengths[i])
    groups = []
    for g0 in range(0, len(order), streams):
        ids = order[g0:g0 + streams]
        L = lengths[ids[0]]
        groups.append((ids, [sum(1 for i in ids if lengths[i] >= L - j) for j in range(L)]))
    return groups


class WindowPredictor:
    """Streaming inference of the ConvLSTM v8 front-end for up to `streams` independent windows that advance together
    (evaluate_depth_gru_fusion.py:595-607 is one stream).  The recurrence reads, per frame and scale, only the LSTM convolution,
    resConfUnit1 and the hand-over; resConfUnit2, the conv3x3 head and the sigmoid feed nothing but the disparity, which is
    wanted at scale 0 of a window's last frame.  So `advance(frames)` runs no head at all (and at scale 0 just the state
    update), and `step(frames)` adds scale 0's resConfUnit1, resConfUnit2 and head and returns the scaled disparities.

    Per scale 3, 2, 1 of a frame at batch B: the decoder map copied into the lower channel half of the scale's cat(dec, up)
    buffer and the buffer's ReLU (stock tensor ops); the LSTM convolution over (x_s, h[:B]) and resConfUnit1's two convolutions
    (dc_conv3x3_fwd); ONE dc_lstm_infer_step, which rewrites (h, c)[:B] in place and writes up_s into the upper channel half of
    scale s - 1's buffer.  Scale 0 of `advance`: the copy, the convolution and the state-only dc_lstm_infer_step.
    Allocated once, here: the (h, c) buffers of `streams` rows per scale -- copies (dc_gru_infer_init) of the learned
    h0_layer1 / c0_layer1, which are never written --, the cat(dec, up) and ReLU-ed input buffers per scale, one cc / conv1 /
    conv2 / pre buffer sized for the largest scale, and the convolutions' workspace.

    What belongs to the cell type is five methods -- `_input_dim`, `_alloc_cell`, `reset`, `_cell_workspace`, `_cell` -- which
    GruWindowPredictor restates for the ConvGRU cells of v10; the rest (the buffers of the fusion blocks, the walk over the
    scales, the units, the head, the public methods) is stated here once."""

    def __init__(self, encoder, decoder, lstm, streams=16, min_depth=0.1, max_depth=100.0):
        if streams <= 0:
            raise ValueError("streams must be positive")
        self.encoder, self.decoder, self.lstm = encoder, decoder, lstm
        self.streams, self.min_depth, self.max_depth = int(streams), float(min_depth), float(max_depth)
        cells = lstm.cells()
        dev = cells[0].h0_layer1.device
        if dev.type != "cuda":
            raise _lib.DepthcoreError("WindowPredictor runs on depthcore kernels only (the ConvLSTM is on %s); there is no CPU path" % dev)
        S, self._dev = self.streams, dev
        self.hid = [int(c.h0_layer1.shape[1]) for c in cells]                       # 2 * num_ch_dec[s]
        self.size = [tuple(c.h0_layer1.shape[2:]) for c in cells]
        if any(self.hid[s] % 4 or self._input_dim(cells[s]) != (self.hid[s] if s < 3 else self.hid[s] // 2) or
               (s and (self.hid[s] != 2 * self.hid[s - 1] or self.size[s - 1] != (2 * self.size[s][0], 2 * self.size[s][1])))
               for s in range(4)):
            raise _lib.DepthcoreError("%s: not %s's cells (hidden %s at %s)" % (type(self).__name__, self.BLOCKS, self.hid, self.size))
        self.h = [self._buf(s) for s in range(4)]
        self.x = [self._buf(s) for s in range(3)]            # cat(dec_s, up_{s+1}); scale 3's input is dec_3 itself
        self.r = [self._buf(s) for s in range(4)]            # relu(input_1): input_1 = x_s, or cat(dec_3, dec_3)
        n = max(S * self.hid[s] * self.size[s][0] * self.size[s][1] for s in range(4))
        self._t, self._y, self._pre = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))
        self._alloc_cell(n, dev)
        self._ws = None
        self.reset()

    def _buf(self, s):
        return torch.empty((self.streams, self.hid[s]) + self.size[s], dtype=torch.float32, device=self._dev)

    # ---- the cell type: ConvLSTMCell_v1 here -------------------------------------------------------------------------------
    BLOCKS = "ConvGRUBlocks_v8"

    @staticmethod
    def _input_dim(cell):
        lstm = getattr(cell, "clstm_1", None)                    # None: another cell type, refused by the caller
        return None if lstm is None else lstm.input_dim

    def _alloc_cell(self, n, dev):
        """The cell's own buffers: the cell state per scale and one buffer of gate pre-activations for the largest scale."""
        self.c = [self._buf(s) for s in range(4)]
        self._cc = torch.empty(4 * n, dtype=torch.float32, device=dev)

    def reset(self):
        """Every stream back to the learned initial states (as they are now: a later optimiser step is seen by the next reset)."""
        cells = self.lstm.cells()
        ops.gru_infer_init([c.h0_layer1 for c in cells] + [c.c0_layer1 for c in cells], self.h + self.c)

    def _cell_workspace(self, L, s, B):
        C, (H, W) = self.hid[s], self.size[s]
        return L.dc_conv3x3_fwd_workspace(C if s < 3 else C // 2, C, B, 4 * C, H, W)

    def _cell(self, conv, s, x, B, y=None, r=None, pre=None, up=None):
        """The cell's convolution over (x_s, h[:B]) and the one launch that steps the state and, with y, hands over."""
        cc = self._view(self._cc, s, 4)
        # [i | f | o | g] = conv(cat(x_s, h))                                                              rnn.py:67-70
        conv(x, x.shape[1], self.h[s], self.hid[s], self.lstm.cells()[s].clstm_1.conv, cc, s, ops.ACT_NONE)
        ops.lstm_infer_step(cc, self.h[s], self.c[s], y, r, pre, up, B)

    def _view(self, flat, s, mult=1):
        shape = (self.streams, mult * self.hid[s]) + self.size[s]
        return flat[:shape[0] * shape[1] * shape[2] * shape[3]].view(shape)

    def _workspace(self, B):
        L = _lib.lib()
        need = 1
        for s in range(4):
            C, (H, W) = self.hid[s], self.size[s]
            need = max(need, self._cell_workspace(L, s, B), L.dc_conv3x3_fwd_workspace(C, 0, B, C, H, W))
        need = max(need, L.dc_conv3x3_fwd_workspace(self.hid[0], 0, B, 1, self.size[0][0], self.size[0][1]))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.h[0].device)
        return self._ws.data_ptr()

    def _recur(self, dec, head):
        """The recurrent part of a frame on the decoder's pre_disp maps [dec_0..dec_3] of streams 0..B-1; head: also scale 0's
        unit, hand-over and disparity head -> the (B,1,h,w) sigmoid output (None without)."""
        L = _lib.lib()
        dec = [d if d.is_contiguous() else d.contiguous() for d in dec]
        B = dec[0].shape[0]
        if len(dec) != 4 or any(d.dtype != torch.float32 or tuple(d.shape) != (B, self.hid[s] // 2) + self.size[s] for s, d in enumerate(dec)):
            raise _lib.DepthcoreError("decoder maps %s do not match the ConvLSTM's states %s at %s" % (
                [tuple(d.shape) for d in dec], [c // 2 for c in self.hid], self.size))
        if not 1 <= B <= self.streams:
            raise _lib.DepthcoreError("a step of %d frames on a predictor of %d streams" % (B, self.streams))
        ops._use_precision(ops._precision[0])                    # the caller's ops.matrix_precision, as ops.conv3x3_block
        ws = self._workspace(B)
        st = stream(dec[0])

        def conv(x0, C0, x1, C1, m, y, s, act, pad=ops.PAD_ZERO):
            w, b = m.weight.detach(), m.bias.detach()
            check(L.dc_conv3x3_fwd(ptr(x0), C0, 0, ptr(x1), C1, ptr(w), ptr(b), ptr(y), ws, B, w.shape[0], self.size[s][0], self.size[s][1],
                                   act, pad, st), "dc_conv3x3_fwd")

        def unit(u, r, s):                                       # conv2(relu(conv1(r))) -> y; the caller adds r
            t, y = self._view(self._t, s), self._view(self._y, s)
            conv(r, self.hid[s], None, 0, u.conv1, t, s, ops.ACT_RELU)
            conv(t, self.hid[s], None, 0, u.conv2, y, s, ops.ACT_NONE)
            return y
        for s in (3, 2, 1, 0):
            C, d = self.hid[s], dec[s]
            fusion = getattr(self.lstm, "fusion_%d" % s)
            if s == 3:
                x = d
            else:
                x = self.x[s]
                x[:B, :C // 2].copy_(d)                          # the upper half is scale s + 1's up, written by its launch
            if s == 0 and not head:
                self._cell(conv, s, x, B)
                return None
            r = self.r[s]
            if s == 3:
                r[:B].view(B, 2, C // 2, *self.size[s]).copy_(torch.relu(d).unsqueeze(1))       # relu(cat(dec_3, dec_3))
            else:
                torch.clamp_min(x[:B], 0.0, out=r[:B])           # relu(x_s) (torch.relu takes no `out`)
            y = unit(fusion.resConfUnit1, r, s)
            pre = self._view(self._pre, 0) if s == 0 else None
            self._cell(conv, s, x, B, y, r, pre, None if s == 0 else self.x[s - 1][:, C // 4:])
        # scale 0's head: sigmoid(conv3x3(reflect_pad(unit2(pre))))                                       rnn.py:774-777
        y = unit(fusion.resConfUnit2, pre, 0)                    # (unit2's leading ReLU finds pre non-negative already)
        t = self._view(self._t, 0)
        torch.add(y[:B], pre[:B], out=t[:B])
        disp = torch.empty((B, 1) + self.size[0], dtype=torch.float32, device=t.device)
        conv(t, C, None, 0, fusion.conv3x3.conv, disp, 0, ops.ACT_SIGMOID, ops.PAD_REFLECT)
        return disp

    def _maps(self, frames, what):
        _frames_ok(frames, what)
        x = frames if frames.is_contiguous() else frames.contiguous()
        out = self.decoder(self.encoder(x), True)
        return [out[("disp", s)] for s in range(4)]

    def _advance(self, frames):
        self._recur(self._maps(frames, "WindowPredictor.advance"), False)

    def _step(self, frames):
        disp = self._recur(self._maps(frames, "WindowPredictor.step"), True)
        dst = torch.empty_like(disp)
        _scaled_disparity(disp, dst, False, self.min_depth, self.max_depth)
        return dst

    def _nets(self):
        return [net for net in (self.encoder, self.decoder, self.lstm) if net is not None]

    def advance(self, frames):
        """frames (B,3,h,w), B <= streams: the next frame of streams 0..B-1; their states advance, the states of the streams
        behind B stay.  Returns nothing: no head is run at any scale.  predict_disparities' contract holds for every call."""
        with _EvalMode(*self._nets()):
            self._advance(frames)

    def step(self, frames):
        """As advance, for a frame whose disparity is wanted: -> (B,1,h,w) scaled disparities of scale 0."""
        with _EvalMode(*self._nets()):
            return self._step(frames)

    def advance_maps(self, dec):
        """The recurrent part of `advance` on its own: dec = [dec_0..dec_3], the decoder's pre_disp maps of streams 0..B-1."""
        with _EvalMode(*self._nets()):
            self._recur(dec, False)

    def step_maps(self, dec):
        """The recurrent part of `step` on its own -> the UNSCALED (B,1,h,w) scale-0 disparity."""
        with _EvalMode(*self._nets()):
            return self._recur(dec, True)


class GruWindowPredictor(WindowPredictor):
    """WindowPredictor for the coarse-to-fine ConvGRU front-end, v10 (evaluate_depth_gru_fusion_my_v.py:673-690 is one stream):
    `lstm` is a ConvGRUBlocks_v9(attention=False).  Per frame and scale the cell is the gate convolution over (x_s, h[:B]),
    dc_gru_infer_rh with one level, the candidate convolution over (x_s, r * h), and ONE dc_gru_c2f_infer_step, which rewrites
    h[:B] in place and hands over; there is no cell state.  Its own buffers: gates, r * h and the candidate for the largest
    scale."""
    BLOCKS = "ConvGRUBlocks_v9"

    @staticmethod
    def _input_dim(cell):
        gru = getattr(cell, "cgru_1", None)
        return None if gru is None else gru.conv_gates.in_channels - gru.hidden_dim

    def _alloc_cell(self, n, dev):
        self._gates, self._rh, self._cnm = (torch.empty(k * n, dtype=torch.float32, device=dev) for k in (2, 1, 1))

    def reset(self):
        ops.gru_infer_init([c.h0_layer1 for c in self.lstm.cells()], self.h)

    def _cell_workspace(self, L, s, B):
        C, (H, W) = self.hid[s], self.size[s]
        return max(L.dc_conv3x3_fwd_workspace(C if s < 3 else C // 2, C, B, co, H, W) for co in (2 * C, C))

    def _cell(self, conv, s, x, B, y=None, r=None, pre=None, up=None):
        cell, C = self.lstm.cells()[s].cgru_1, self.hid[s]
        gates, rh, cnm = self._view(self._gates, s, 2), self._view(self._rh, s), self._view(self._cnm, s)
        conv(x, x.shape[1], self.h[s], C, cell.conv_gates, gates, s, ops.ACT_SIGMOID)                    # rnn.py:125-130
        ops.gru_infer_rh([gates], [self.h[s]], [rh], B)
        conv(x, x.shape[1], rh, C, cell.conv_can, cnm, s, ops.ACT_TANH)                                  # rnn.py:132-134
        ops.gru_c2f_infer_step(gates, cnm, self.h[s], y, r, pre, up, B)


def window_predictor_class(blocks):
    """WindowPredictor for ConvGRUBlocks_v8 (ConvLSTM cells), GruWindowPredictor for ConvGRUBlocks_v9 (ConvGRU cells)."""
    return WindowPredictor if hasattr(blocks.cells()[0], "clstm_1") else GruWindowPredictor


def predict_disparities_windows(encoder, decoder, lstm, lengths, batch_fn, min_depth=0.1, max_depth=100.0, streams=16):
    """The ConvLSTM v8 / ConvGRU v10 evaluation of N independent windows that advance in lockstep (window_groups' schedule):
    window c has lengths[c] frames, starts from the learned initial states and is scored at its last frame.  batch_fn(j, ids, frame_of) -> the
    (len(ids),3,h,w) float32 device tensor of step j of a group: frame frame_of[b] (counted inside the window) of window
    ids[b]; called once per step.  -> (N,1,h,w) scaled disparities in the order of `lengths`.  One reset and one head per group;
    contract: predict_disparities'."""
    lengths = list(lengths)
    if not lengths:
        raise ValueError("predict_disparities_windows: no windows")
    groups = window_groups(lengths, streams)
    out = None
    with _EvalMode(encoder, decoder, lstm):
        wp = window_predictor_class(lstm)(encoder, decoder, lstm, min(streams, len(lengths)), min_depth, max_depth)
        for g, (ids, widths) in enumerate(groups):
            if g:
                wp.reset()
            L = len(widths)
            for j, B in enumerate(widths):
                frames = batch_fn(j, ids[:B], [j - (L - lengths[c]) for c in ids[:B]])
                if j < L - 1:
                    wp._advance(frames)
                else:
                    disp = wp._step(frames)
            if out is None:
                out = torch.empty((len(lengths),) + tuple(disp.shape[1:]), dtype=torch.float32, device=disp.device)
            ops.copy_segments([disp[b] for b in range(len(ids))], [out[c] for c in ids])
    return out


def predict_disparities_fusion(encoder, decoder, fusion, triplets, min_depth=0.1, max_depth=100.0, post_process=False, batch_size=16):
    """evaluate_depth_fusion_v3.py:131-165 -> (N,1,h,w) scaled disparities on the device.

    `triplets`: (3,N,3,h,w) float32 device tensor, frames [-2, -1, 0] of N test files frame-major (triplets[j, i] is frame j - 2
    of file i), or an iterable of such (3,B,3,h,w) batches (batch_size is then the iterable's).  A batch goes through
    encoder -> decoder -> Fusion_v3 stacked along the batch as Trainer._depth_branch stacks it.  post_process: the mirrored
    triplets are a fusion call of their own and the two results are blended by ops.post_process_disparity (the reference
    concatenates [x; flip(x)] BEFORE the networks, so that Fusion_v3's three chunks mix frames and mirrored frames).
    Contract: predict_disparities'."""
    if batch_size <= 0:
        raise ValueError("batch_size must be positive")
    if torch.is_tensor(triplets):
        if triplets.dim() != 5 or triplets.shape[0] != 3:
            raise _lib.DepthcoreError("predict_disparities_fusion: triplets must be (3,N,3,h,w), got %s" % (tuple(triplets.shape),))
        triplets = [triplets[:, i0:i0 + batch_size] for i0 in range(0, triplets.shape[1], batch_size)]
    outs = []
    with _EvalMode(encoder, decoder, fusion):
        for t in triplets:
            if t.dim() != 5 or t.shape[0] != 3:
                raise _lib.DepthcoreError("predict_disparities_fusion: a batch must be (3,B,3,h,w), got %s" % (tuple(t.shape),))
            B = t.shape[1]
            x = t.reshape((3 * B,) + tuple(t.shape[2:])) if t.is_contiguous() else ops.stack_frames([[t[0], t[1], t[2]]])[0]
            _frames_ok(x, "predict_disparities_fusion")
            if post_process:
                both = ops.flip_concat(x)                                   # [x; flip_w(x)]: rows 3B.. are the mirrored stack
                disps = [fusion(decoder(encoder(half)))[("disp", 0)] for half in (both[:3 * B], both[3 * B:])]
                outs.append(ops.post_process_disparity(ops.stack_frames([disps])[0], min_depth, max_depth))
            else:
                disp = fusion(decoder(encoder(x)))[("disp", 0)]
                dst = torch.empty_like(disp)
                _scaled_disparity(disp, dst, False, min_depth, max_depth)
                outs.append(dst)
    if not outs:
        raise ValueError("predict_disparities_fusion: no triplets")
    return outs[0] if len(outs) == 1 else ops.stack_frames([outs])[0]


# ---- whole drives: every frame of a video scored, the work shared between overlapping windows (test_sequence.py) ---------------
def drive_window_plan(n_frames, n_prev, streams):
    """The lockstep schedule of a drive's windows, as pure arithmetic: frame t of a drive of `n_frames` is predicted from the
    window of frames max(0, t - n_prev) .. t (evaluate_depth_gru.window_paths' protocol).  -> [(t0, t1, ids, steps)], one entry
    per group of up to `streams` windows, in frame order:
      t0, t1    the group's targets are frames t0 .. t1 - 1;
      ids       the target of every stream, in window_groups' order (by window length, descending and stable), so the streams
                alive at a step are a prefix;
      steps     steps[j][b]: the frame that stream b reads at step j, for the streams alive then.  The windows are right
                aligned: all of them read their own target at the last step, where the head runs once at full width.
    The ragged windows (t < n_prev) are grouped apart from the full ones.  In a group of full windows ids is t0 .. t1 - 1 and
    step j reads frames t0 - n_prev + j .. t1 - 1 - n_prev + j: consecutive, ascending -- a slice of a frame-ordered cache."""
    if n_frames < 1 or n_prev < 0 or streams < 1:
        raise ValueError("drive_window_plan: n_frames >= 1, n_prev >= 0 and streams >= 1, got %r, %r, %r" % (n_frames, n_prev, streams))
    head = min(n_prev, n_frames)
    cuts = [(t0, min(t0 + streams, head)) for t0 in range(0, head, streams)]
    cuts += [(t0, min(t0 + streams, n_frames)) for t0 in range(head, n_frames, streams)]
    plan = []
    for t0, t1 in cuts:
        lengths = [min(t, n_prev) + 1 for t in range(t0, t1)]
        (local, widths), = window_groups(lengths, len(lengths))
        ids = [t0 + i for i in local]
        L = len(widths)
        plan.append((t0, t1, ids, [[t - (L - 1) + j for t in ids[:B]] for j, B in enumerate(widths)]))
    return plan


class _MapRing:
    """The decoder maps of the last `size` frames of a drive on the device, frame f in slot f % size, and a mirror of the first
    `mirror` slots behind the last one: any run of up to mirror + 1 consecutive frames is ONE slice of the arrays, also where
    it runs over the ring's end.  A frame is copied in once (twice when its slot is mirrored); reading copies nothing."""

    def __init__(self, like, size, mirror):
        self.size, self.mirror = int(size), int(mirror)
        self.maps = [torch.empty((self.size + self.mirror,) + tuple(m.shape[1:]), dtype=torch.float32, device=m.device) for m in like]

    def store(self, first, maps):
        """maps[s][i] is frame first + i."""
        maps = [m if m.is_contiguous() else m.contiguous() for m in maps]
        n, done, src, dst = maps[0].shape[0], 0, [], []
        while done < n:
            p = (first + done) % self.size
            k = min(n - done, self.size - p)
            spans = [(p, k)] + ([(self.size + p, min(p + k, self.mirror) - p)] if p < self.mirror else [])
            for at, m in spans:
                src += [x[done:done + m] for x in maps]
                dst += [r[at:at + m] for r in self.maps]
            done += k
        ops.copy_segments(src, dst)

    def run(self, first, B):
        """Frames first .. first + B - 1 (B <= mirror + 1) as views."""
        p = first % self.size
        return [r[p:p + B] for r in self.maps]

    def rows(self, frames):
        """Any frames, gathered (stock indexing): the ragged groups at the head of a drive."""
        idx = torch.tensor([f % self.size for f in frames], dtype=torch.long, device=self.maps[0].device)
        return [r.index_select(0, idx) for r in self.maps]


def _drive_chunk(batch_fn, lo, hi, shape):
    x = batch_fn(lo, hi)
    _frames_ok(x, "predict_disparities_drive", shape)
    if x.shape[0] != hi - lo:
        raise _lib.DepthcoreError("predict_disparities_drive: batch_fn(%d, %d) returned %d frames" % (lo, hi, x.shape[0]))
    return x if x.is_contiguous() else x.contiguous()


def _drive_windows(encoder, decoder, front, n_frames, batch_fn, n_prev, streams, chunk, min_depth, max_depth):
    plan = drive_window_plan(n_frames, n_prev, streams)
    S = min(streams, n_frames)
    out = ring = shape = None
    hi = 0
    with _EvalMode(encoder, decoder, front):
        wp = window_predictor_class(front)(encoder, decoder, front, S, min_depth, max_depth)
        for g, (t0, t1, ids, steps) in enumerate(plan):
            while hi < t1:                                       # every frame passes the encoder and the decoder once, here
                nxt = min(hi + chunk, n_frames)
                x = _drive_chunk(batch_fn, hi, nxt, shape)
                shape = tuple(x.shape[2:])
                maps = wp._maps(x, "predict_disparities_drive")
                if ring is None:
                    ring = _MapRing(maps, min(n_prev + S + chunk, n_frames), S - 1)
                ring.store(hi, maps)
                hi = nxt
            if g:
                wp.reset()
            for j, frames in enumerate(steps):
                B = len(frames)
                dec = ring.run(frames[0], B) if frames == list(range(frames[0], frames[0] + B)) else ring.rows(frames)
                disp = wp._recur(dec, j == len(steps) - 1)
            if out is None:
                out = torch.empty((n_frames,) + tuple(disp.shape[1:]), dtype=torch.float32, device=disp.device)
            if ids == list(range(t0, t1)):
                _scaled_disparity(disp, out[t0:t1], False, min_depth, max_depth)
            else:
                dst = torch.empty_like(disp)
                _scaled_disparity(disp, dst, False, min_depth, max_depth)
                ops.copy_segments([dst[b] for b in range(len(ids))], [out[t] for t in ids])
    return out


def _drive_v5(encoder, decoder, gru, n_frames, batch_fn, chunk, min_depth, max_depth):
    out = fused = shape = None
    with _EvalMode(encoder, gru, decoder):
        sp = SequencePredictor(encoder, gru, decoder, 1, min_depth, max_depth)        # one stream: the states live there
        for lo in range(0, n_frames, chunk):
            hi = min(lo + chunk, n_frames)
            x = _drive_chunk(batch_fn, lo, hi, shape)
            shape = tuple(x.shape[2:])
            feats = [f if f.is_contiguous() else f.contiguous() for f in encoder(x)]
            if fused is None:
                fused = [torch.empty((min(chunk, n_frames),) + tuple(f.shape[1:]), dtype=torch.float32, device=f.device) for f in feats]
                out = torch.empty((n_frames, 1) + shape, dtype=torch.float32, device=x.device)
            for i in range(hi - lo):                             # the recurrence, in order; the states carry over to the next chunk
                ops.copy_segments(sp._fuse([f[i:i + 1] for f in feats]), [u[i:i + 1] for u in fused])
            disp = decoder([u[:hi - lo] for u in fused])[("disp", 0)]
            _scaled_disparity(disp, out[lo:hi], False, min_depth, max_depth)
    return out


def predict_disparities_drive(encoder, decoder, front, n_frames, batch_fn, n_prev=6, streams=16, chunk=16, min_depth=0.1, max_depth=100.0):
    """A recurrent model on the `n_frames` consecutive frames of one drive -> (n_frames,1,h,w) scaled disparities in frame
    order, on the device.  `front`: a ConvGRUBlocks_v5, ConvGRUBlocks_v8 or ConvGRUBlocks_v9(attention=False).
    batch_fn(lo, hi) -> frames lo .. hi - 1 as a (hi - lo,3,h,w) float32 device tensor; called once per chunk of `chunk`
    consecutive frames, in order.  Contract: predict_disparities'.

    v8 / v10: frame t is predicted from the window of frames max(0, t - n_prev) .. t, started from the learned initial states
    -- what predict_disparities_windows computes for those windows, without sending a frame through the encoder and the
    decoder once per window it belongs to.  Every frame passes encoder -> decoder(pre_disp) exactly ONCE, `chunk` frames a
    batch; its four decoder maps stay on the device in a ring of n_prev + streams + chunk frames (about 15 MB per frame at
    192 x 640; plus streams - 1 mirrored slots, so that a step's frames are always one slice) until no later window reads
    them.  The windows of `streams` consecutive targets advance in lockstep through WindowPredictor / GruWindowPredictor on
    drive_window_plan's schedule: in a group of full windows a step's decoder maps are a slice of the ring -- no gather, no
    copy --; the ragged groups of the first n_prev frames gather their rows.  One reset and one head per group.

    v5: one stream whose hidden states are carried along the whole drive from the learned h0 (n_prev and streams are not
    used).  Per chunk the encoder runs once on all its frames, the recurrence walks them in order (SequencePredictor's fused
    step at width 1, the states carried across chunks), and the decoder runs once on the chunk."""
    if n_frames < 1 or n_prev < 0 or streams < 1 or chunk < 1:
        raise ValueError("predict_disparities_drive: n_frames, streams, chunk >= 1 and n_prev >= 0, got %r, %r, %r, %r"
                         % (n_frames, streams, chunk, n_prev))
    n_frames, n_prev, streams, chunk = int(n_frames), int(n_prev), int(streams), int(chunk)
    if hasattr(front, "cgru_4"):                                 # ConvGRUBlocks_v5: a cell per encoder level
        return _drive_v5(encoder, decoder, front, n_frames, batch_fn, chunk, min_depth, max_depth)
    return _drive_windows(encoder, decoder, front, n_frames, batch_fn, n_prev, streams, chunk, min_depth, max_depth)


def render_drive(pred, size, percentile=95.0, chunk=64, lut=None):
    """The colour images of a drive under ONE range, so that a surface keeps its colour from frame to frame: -> (images, (vmin,
    vmax)), images a host uint8 array (N, Ho, Wo, 3) and the pair two np.float32.

    pred: (N,1,h,w) float32 disparities at network resolution -- a device tensor (491 KB per frame at 192 x 640), or host data
    that is copied over.  The range is ops.disparity_range_pooled's, computed once over all frames at size = (Ho, Wo); the
    pictures are rendered `chunk` at a time (ops.render_disparity_fixed, one launch) and leave through one pinned buffer."""
    if not torch.is_tensor(pred):
        pred = torch.from_numpy(np.ascontiguousarray(pred, np.float32))
    if not pred.is_cuda:
        pred = pred.to(torch.device("cuda", torch.cuda.current_device()))
    if pred.dtype != torch.float32 or pred.dim() != 4 or pred.shape[1] != 1 or pred.shape[0] < 1:
        raise _lib.DepthcoreError("render_drive: pred must be (N,1,h,w) float32 with N >= 1, got %s %s" % (tuple(pred.shape), pred.dtype))
    if chunk <= 0:
        raise ValueError("chunk must be positive")
    d = pred if pred.is_contiguous() else pred.contiguous()
    if lut is not None:
        lut = (lut if torch.is_tensor(lut) else torch.from_numpy(np.ascontiguousarray(lut, np.uint8))).to(d.device)
    N, (Ho, Wo) = d.shape[0], (int(size[0]), int(size[1]))
    rng = ops.disparity_range_pooled(d, (Ho, Wo), percentile)
    c, nb = min(int(chunk), N), Ho * Wo * 3
    dev = torch.empty(c * nb, dtype=torch.uint8, device=d.device)
    pinned = torch.empty(c * nb, dtype=torch.uint8, pin_memory=True)
    images = np.empty((N, Ho, Wo, 3), np.uint8)
    for c0 in range(0, N, c):
        k = min(c, N - c0)
        ops.render_disparity_fixed(d[c0:c0 + k], (Ho, Wo), rng, lut, out=dev)
        pinned[:k * nb].copy_(dev[:k * nb], non_blocking=True)
        torch.cuda.current_stream(d.device).synchronize()
        images[c0:c0 + k] = pinned[:k * nb].numpy().reshape(k, Ho, Wo, 3)
    vmin, vmax = rng.cpu().numpy()
    return images, (vmin, vmax)
