"""torch.autograd bindings of the C ABI in include/depthcore.h.

Every op enqueues hand-written gfx950 kernels on the current HIP stream; tensors
are allocated by PyTorch's caching allocator and passed down as raw pointers.
"""
import ctypes
import weakref

import torch

from . import _lib
from ._autograd import (PRECISIONS, GradFork, SkipSum, WgradLanes, _c, _decision_observers, _fork_addend, _grad_dst,  # noqa: F401
                        _lane_param, _parked_forks, _precision, _record_kink, _slot, _tls, _use_precision,
                        add_decision_observer, assert_no_dangling_sums, matrix_precision, remove_decision_observer, skip_of)
from ._lib import PhotoDesc, check, ptr, stream
from .convnode import _ConvF
from .data import seq_item_rows, seq_rows  # noqa: F401


DepthcoreError = _lib.DepthcoreError


# ----------------------------------------------------------------------------------------------
# fused photometric loss  (reference trainer.py:465-622)
# ----------------------------------------------------------------------------------------------
class PhotoConfig:
    """Non-differentiable inputs + options of one fused photometric step.

    target/src: inputs[("color", 0|-1|+1, 0)];  color_s[s]: inputs[("color", 0, s)];
    K / inv_K: inputs[("K"|"inv_K", 0)];  noise[s]: the tie-break randn of trainer.py:594-595
    (None -> on-device counter RNG).  `materialize` asks for the log tensors of
    generate_images_pred (depth / sample / color / identity_selection).
    packed: optional (target, src_m1, src_p1) as pixel-interleaved RGBx (B,H,W,4) tensors -- `pack_rgbx(x)` or the data step's
    ("color_packed", f, 0) -- the layout the kernels gather from; without it every forward repacks the three frames.
    """

    def __init__(self, target, src_m1, src_p1, color_s, K, inv_K, noise=None, min_depth=0.1, max_depth=100.0,
                 smoothness=1e-3, disable_automasking=False, avg_reprojection=False, no_ssim=False,
                 align_corners=False, materialize=False, rng_seed=0, packed=None):
        self.target, self.src = _c(target), (_c(src_m1), _c(src_p1))
        self.packed = None if packed is None else tuple(_c(t) for t in packed)
        self.color_s = [_c(c) for c in color_s]
        self.K, self.inv_K = _c(K), _c(inv_K)
        self.noise = None if noise is None else [_c(n) for n in noise]
        self.min_depth, self.max_depth, self.smoothness = float(min_depth), float(max_depth), float(smoothness)
        self.flags = ((_lib.OPT_NO_AUTOMASK if disable_automasking else 0)
                      | (_lib.OPT_AVG_REPROJ if avg_reprojection else 0)
                      | (_lib.OPT_NO_SSIM if no_ssim else 0)
                      | (_lib.OPT_ALIGN_CORNERS if align_corners else 0))
        self.materialize = materialize
        # an int, or a one-element int64 device tensor read by the kernel at run time (hipGraph replays)
        self.rng_seed_dev = rng_seed if torch.is_tensor(rng_seed) else None
        self.rng_seed = 0 if torch.is_tensor(rng_seed) else int(rng_seed)
        self.extras = {}          # filled by forward: argmin maps + optional log tensors
        self.n_masks = 0          # set by photometric_loss(pred_masks=...)
        self.n_Ts = 0             # set by photometric_loss(T_scales=...): 2 * num_scales per-scale poses, else 0


def _fill_desc(cfg, T0, T1, disps, no_grad=False, masks=(), Ts=(), mode=0):
    B, _, H, W = cfg.target.shape
    ns = len(disps)
    if ns < 1 or ns > _lib.MAX_SCALES:
        raise _lib.DepthcoreError("1..4 scales supported, got %d" % ns)
    if cfg.target.shape[1] != 3:
        raise _lib.DepthcoreError("images must be (B,3,H,W)")
    d = PhotoDesc()
    d.B, d.H, d.W, d.num_scales = B, H, W, ns
    d.flags = cfg.flags | (_lib.OPT_NO_GRAD if no_grad else 0) | (_lib.OPT_PRED_MASK if masks else 0) | mode
    if masks:
        if not (cfg.flags & _lib.OPT_NO_AUTOMASK):
            raise _lib.DepthcoreError("predictive masks need disable_automasking (reference trainer.py:116-117)")
        if len(masks) != ns or any(tuple(m.shape) != (B, 2, H, W) for m in masks):
            raise _lib.DepthcoreError("predictive masks: one (B,2,H,W) full-resolution tensor per scale")
        for s in range(ns):
            d.pred_mask[s] = ptr(masks[s])
    d.min_depth, d.max_depth, d.smoothness = cfg.min_depth, cfg.max_depth, cfg.smoothness
    d.target = ptr(cfg.target)
    for f in range(2):
        if cfg.src[f].shape != cfg.target.shape:
            raise _lib.DepthcoreError("source / target shape mismatch")
        d.source[f] = ptr(cfg.src[f])
    if Ts and len(Ts) != 2 * ns:
        raise _lib.DepthcoreError("per-scale poses: one (T_-1, T_+1) pair per scale")
    for t in (cfg.K, cfg.inv_K, *((T0, T1) if not Ts else Ts)):
        if tuple(t.shape) != (B, 4, 4):
            raise _lib.DepthcoreError("K / inv_K / T must be (B,4,4), got %s" % (tuple(t.shape),))
    d.K, d.inv_K = ptr(cfg.K), ptr(cfg.inv_K)
    if Ts:                                    # posecnn: one pose per (scale, frame), trainer.py:490-499
        for s in range(ns):
            d.T_scale[s][0], d.T_scale[s][1] = ptr(Ts[2 * s]), ptr(Ts[2 * s + 1])
    else:
        d.T[0], d.T[1] = ptr(T0), ptr(T1)
    if cfg.packed is not None:
        if len(cfg.packed) != 3 or any(tuple(t.shape) != (B, H, W, 4) for t in cfg.packed):
            raise _lib.DepthcoreError("packed must be three (B,H,W,4) RGBx tensors (target, source -1, source +1)")
        for k in range(3):
            d.packed[k] = ptr(cfg.packed[k])
    nch = 1 if (cfg.flags & _lib.OPT_AVG_REPROJ) else 2
    for s in range(ns):
        shp = (B, 1, H >> s, W >> s)
        if tuple(disps[s].shape) != shp:
            raise _lib.DepthcoreError("disp[%d] must be %s, got %s" % (s, shp, tuple(disps[s].shape)))
        if tuple(cfg.color_s[s].shape) != (B, 3, H >> s, W >> s):
            raise _lib.DepthcoreError("color_s[%d] has shape %s" % (s, tuple(cfg.color_s[s].shape)))
        d.disp[s] = ptr(disps[s])
        d.color_s[s] = ptr(cfg.color_s[s])
        if cfg.noise is not None and not (cfg.flags & _lib.OPT_NO_AUTOMASK):
            if tuple(cfg.noise[s].shape) != (B, nch, H, W):
                raise _lib.DepthcoreError("noise[%d] must be %s" % (s, (B, nch, H, W)))
            d.noise[s] = ptr(cfg.noise[s])
    d.rng_seed = cfg.rng_seed
    if cfg.rng_seed_dev is not None:
        d.rng_seed_dev = ptr(cfg.rng_seed_dev, torch.int64)
    return d


class _PhotoLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg, T0, T1, *tensors):
        L = _lib.lib()
        # tensors = disps..., [predictive masks (one per scale)], [per-scale poses (T_-1, T_+1 per scale)]
        nm, nT = cfg.n_masks, cfg.n_Ts
        Ts = [_c(x.detach()) for x in tensors[len(tensors) - nT:]] if nT else []
        tensors = tensors[:len(tensors) - nT]
        T0, T1 = (None, None) if nT else (_c(T0.detach()), _c(T1.detach()))
        disps = [_c(x.detach()) for x in tensors[:len(tensors) - nm]]
        masks = [_c(x.detach()) for x in tensors[len(tensors) - nm:]] if nm else []
        dev = cfg.target.device
        B, _, H, W = cfg.target.shape
        ns = len(disps)
        # evaluation (nothing requires a gradient): the forward skips the gradient emission and its 24 B/pixel/scale
        ctx.no_grad = not any(ctx.needs_input_grad)
        # the all-the-way / split choice (dc_set_photo_full) is read ONCE, here, and pinned in the desc of the forward and of its
        # backward: the workspace layout both derive cannot change between them whatever the setter does in the meantime
        ctx.mode = _lib.OPT_PHOTO_FULL if L.dc_get_photo_full() else _lib.OPT_PHOTO_SPLIT
        d = _fill_desc(cfg, T0, T1, disps, ctx.no_grad, masks, Ts, ctx.mode)
        wsz = L.dc_photo_workspace(ctypes.byref(d))
        ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
        d.workspace, d.workspace_bytes = ws.data_ptr(), wsz
        losses = torch.empty(ns + 1, dtype=torch.float32, device=dev)
        d.losses = ptr(losses)
        argmin = [torch.empty(B, H, W, dtype=torch.uint8, device=dev) for _ in range(ns)]
        ex = {"argmin": argmin}
        for s in range(ns):
            d.argmin[s] = argmin[s].data_ptr()
        if cfg.materialize:
            ex["depth"] = [torch.empty(B, 1, H, W, device=dev) for _ in range(ns)]
            ex["sample"] = [[torch.empty(B, H, W, 2, device=dev) for _ in range(2)] for _ in range(ns)]
            ex["color"] = [[torch.empty(B, 3, H, W, device=dev) for _ in range(2)] for _ in range(ns)]
            automask = not (cfg.flags & _lib.OPT_NO_AUTOMASK)
            ex["identity_selection"] = [torch.empty(B, H, W, device=dev) for _ in range(ns)] if automask else None
            for s in range(ns):
                d.depth[s] = ptr(ex["depth"][s])
                for f in range(2):
                    d.sample[s][f] = ptr(ex["sample"][s][f])
                    d.color[s][f] = ptr(ex["color"][s][f])
                if automask:
                    d.identity_selection[s] = ptr(ex["identity_selection"][s])
        check(L.dc_photo_fwd(ctypes.byref(d), stream(cfg.target)), "dc_photo_fwd")
        cfg.extras = ex
        ctx.cfg, ctx.ws, ctx.argmin, ctx.nm, ctx.nT = cfg, ws, argmin, nm, nT
        ctx.save_for_backward(*(() if nT else (T0, T1)), *disps, *masks, *Ts)
        return losses

    @staticmethod
    def backward(ctx, g_losses):
        L = _lib.lib()
        cfg = ctx.cfg
        rest = list(ctx.saved_tensors)
        T0, T1 = (None, None) if ctx.nT else (rest.pop(0), rest.pop(0))
        Ts = [rest.pop() for _ in range(ctx.nT)][::-1]
        disps, masks = (rest[:len(rest) - ctx.nm], rest[len(rest) - ctx.nm:]) if ctx.nm else (rest, [])
        d = _fill_desc(cfg, T0, T1, disps, ctx.no_grad, masks, Ts, ctx.mode)
        d.workspace, d.workspace_bytes = ctx.ws.data_ptr(), ctx.ws.numel()
        g = _c(g_losses.to(torch.float32))
        d.g_losses = ptr(g)
        d_disp = [torch.empty_like(x) for x in disps]
        dT = [None, None] if ctx.nT else [torch.empty_like(T0), torch.empty_like(T1)]
        dTs = [torch.empty_like(t) for t in Ts]
        for s in range(len(disps)):
            d.argmin[s] = ctx.argmin[s].data_ptr()
            d.d_disp[s] = ptr(d_disp[s])
            if ctx.nT:
                d.d_T_scale[s][0], d.d_T_scale[s][1] = ptr(dTs[2 * s]), ptr(dTs[2 * s + 1])
        if not ctx.nT:
            d.d_T[0], d.d_T[1] = ptr(dT[0]), ptr(dT[1])
        d_masks = [torch.empty_like(m) for m in masks]
        for s in range(len(d_masks)):
            d.d_pred_mask[s] = ptr(d_masks[s])
        check(L.dc_photo_bwd(ctypes.byref(d), stream(cfg.target)), "dc_photo_bwd")
        return (None, dT[0], dT[1], *d_disp, *d_masks, *dTs)


def pack_rgbx(x):
    """(B,3,H,W) float32 -> (B,H,W,4) pixel-interleaved RGBx: the layout the fused photometric kernels gather from (`PhotoConfig(
    packed=...)`).  The data step (depthcore.data.GpuPreprocessor) writes it directly as ("color_packed", f, 0)."""
    xx = _c(x.detach())
    B, C, H, W = xx.shape
    if C != 3:
        raise _lib.DepthcoreError("pack_rgbx takes (B,3,H,W) images")
    out = torch.empty(B, H, W, 4, dtype=torch.float32, device=xx.device)
    check(_lib.lib().dc_pack_rgbx(ptr(xx), ptr(out), B, H * W, stream(xx)), "dc_pack_rgbx")
    return out


def photometric_loss(cfg, T_m1, T_p1, disps, pred_masks=None, T_scales=None):
    """-> losses tensor (num_scales+1,): [loss/0, ..., loss]  (trainer.py:618-621).
    T_scales: `pose_model_type == "posecnn"` (trainer.py:490-499) -- a list of (T_-1, T_+1) pairs, one per scale, each built from
    the translation scaled by that scale's mean inverse depth; replaces T_m1 / T_p1 (pass None) and each gets its own gradient.
    pred_masks: opt.predictive_mask (trainer.py:571-584, needs disable_automasking) -- one FULL-resolution (B,2,H,W) mask per
    scale (the caller upsamples, trainer.py:574-577); the reprojection losses are multiplied by them inside the kernels and
    the masks get their gradient.  The BCE weighting term (trainer.py:579-581) is not part of this op."""
    cfg.n_masks = len(pred_masks) if pred_masks else 0
    flat_T = [t for pair in (T_scales or []) for t in pair]
    cfg.n_Ts = len(flat_T)
    return _PhotoLoss.apply(cfg, T_m1, T_p1, *disps, *(pred_masks or []), *flat_T)


def photo_algorithmic_bytes(cfg, T0, T1, disps, backward):
    d = _fill_desc(cfg, _c(T0.detach()), _c(T1.detach()), [_c(x.detach()) for x in disps])
    return _lib.lib().dc_photo_algorithmic_bytes(ctypes.byref(d), int(backward))


# ----------------------------------------------------------------------------------------------
# a5  transformation_from_parameters                                   (reference layers.py:28-103)
# ----------------------------------------------------------------------------------------------
class _PoseMatrix(torch.autograd.Function):
    @staticmethod
    def forward(ctx, axisangle, translation, invert):
        L = _lib.lib()
        aa = _c(axisangle.detach().reshape(-1, 3))
        tr = _c(translation.detach().reshape(-1, 3))
        B = aa.shape[0]
        M = torch.empty(B, 4, 4, dtype=torch.float32, device=aa.device)
        check(L.dc_pose_matrix_fwd(ptr(aa), ptr(tr), int(bool(invert)), ptr(M), B, stream(aa)), "dc_pose_matrix_fwd")
        ctx.save_for_backward(aa, tr)
        ctx.invert = int(bool(invert))
        ctx.shapes = (axisangle.shape, translation.shape)
        return M

    @staticmethod
    def backward(ctx, gM):
        L = _lib.lib()
        aa, tr = ctx.saved_tensors
        B = aa.shape[0]
        daa, dtr = torch.empty_like(aa), torch.empty_like(tr)
        g_c = _c(gM)      # named: stays alive until the launch is enqueued
        check(L.dc_pose_matrix_bwd(ptr(aa), ptr(tr), ctx.invert, ptr(g_c), ptr(daa), ptr(dtr), B, stream(aa)),
              "dc_pose_matrix_bwd")
        return daa.reshape(ctx.shapes[0]), dtr.reshape(ctx.shapes[1]), None


def pose_matrix(axisangle, translation, invert=False):
    return _PoseMatrix.apply(axisangle, translation, invert)


class _PoseHead(torch.autograd.Function):
    """The tail of PoseDecoder / PoseCNN and the cam_T_cam of their callers as one launch each way (dc_pose_head_fwd / _bwd).
    Outputs: vec (N, nf, 1, 6) -- NOT differentiable (the axisangle / translation entries of `outputs` are records; the loss
    reaches the pose networks through the matrices) -- and one (rows,4,4) matrix tensor per group."""

    @staticmethod
    def forward(ctx, y, nf, groups):
        L = _lib.lib()
        yy = _c(y.detach())
        N, C = yy.shape[0], yy.shape[1]
        P = yy.shape[2] * yy.shape[3]
        if C != 6 * nf:
            raise _lib.DepthcoreError("pose head: %d channels for %d predicted frames" % (C, nf))
        gs = (_lib.PoseGroup * len(groups))(*[_lib.PoseGroup(int(r0), int(rows), int(slot), int(bool(inv))) for r0, rows, slot, inv in groups])
        vec = torch.empty(N, nf, 1, 6, dtype=torch.float32, device=yy.device)
        Ms = [torch.empty(int(g[1]), 4, 4, dtype=torch.float32, device=yy.device) for g in groups]
        mp = (ctypes.c_void_p * len(groups))(*[m.data_ptr() for m in Ms])
        check(L.dc_pose_head_fwd(ptr(yy), N, nf, P, 0.01, gs, len(groups), ptr(vec), mp, stream(yy)), "dc_pose_head_fwd")
        ctx.save_for_backward(vec)
        ctx.cfg = (N, nf, P, yy.shape, tuple(groups))
        ctx.mark_non_differentiable(vec)
        return (vec,) + tuple(Ms)

    @staticmethod
    def backward(ctx, _gvec, *gMs):
        L = _lib.lib()
        vec, = ctx.saved_tensors
        N, nf, P, yshape, groups = ctx.cfg
        gs = (_lib.PoseGroup * len(groups))(*[_lib.PoseGroup(int(r0), int(rows), int(slot), int(bool(inv))) for r0, rows, slot, inv in groups])
        keep = [None if g is None else _c(g) for g in gMs]       # named: alive until the launch is enqueued
        dp = (ctypes.c_void_p * len(groups))(*[None if g is None else g.data_ptr() for g in keep])
        dy = torch.empty(yshape, dtype=torch.float32, device=vec.device)
        check(L.dc_pose_head_bwd(ptr(vec), N, nf, P, 0.01, gs, len(groups), dp, ptr(dy), stream(vec)), "dc_pose_head_bwd")
        return dy, None, None


def pose_head(y, nf, groups):
    """y (N, 6 nf, h, w), the pose network's last convolution -> (axisangle (N,nf,1,3), translation (N,nf,1,3), [cam_T_cam per
    group]); groups: (row0, rows, slot, invert) -- rows [row0, row0+rows) of predicted frame `slot`.  pose_decoder.py:50-54 +
    trainer.py:416-419 / 436-440 in one launch each way."""
    out = _PoseHead.apply(y, int(nf), tuple(tuple(int(v) for v in g) for g in groups))
    vec = out[0]
    return vec[..., :3], vec[..., 3:], list(out[1:])


# ----------------------------------------------------------------------------------------------
# a6  disp_to_depth                                                      (reference layers.py:16-25)
# ----------------------------------------------------------------------------------------------
class _DispToDepth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp, min_depth, max_depth):
        L = _lib.lib()
        d = _c(disp.detach())
        scaled, depth = torch.empty_like(d), torch.empty_like(d)
        check(L.dc_disp_to_depth_fwd(ptr(d), ptr(scaled), ptr(depth), d.numel(), float(min_depth), float(max_depth),
                                     stream(d)), "dc_disp_to_depth_fwd")
        ctx.save_for_backward(d)
        ctx.lim = (float(min_depth), float(max_depth))
        return scaled, depth

    @staticmethod
    def backward(ctx, gs, gd):
        L = _lib.lib()
        (d,) = ctx.saved_tensors
        out = torch.empty_like(d)
        # keep both contiguous temporaries alive across the call: two unnamed temporaries would be freed and
        # could be handed the SAME block by the caching allocator before the launch
        gs_c = _c(gs) if gs is not None else None
        gd_c = _c(gd) if gd is not None else None
        check(L.dc_disp_to_depth_bwd(ptr(d), ptr(gs_c), ptr(gd_c), ptr(out), d.numel(), ctx.lim[0], ctx.lim[1],
                                     stream(d)), "dc_disp_to_depth_bwd")
        return out, None, None


def disp_to_depth(disp, min_depth, max_depth):
    return _DispToDepth.apply(disp, min_depth, max_depth)


# ----------------------------------------------------------------------------------------------
# a7  BackprojectDepth                                                  (reference layers.py:139-168)
# ----------------------------------------------------------------------------------------------
def pix_coords(B, H, W, device):
    L = _lib.lib()
    pc = torch.empty(B, 3, H * W, dtype=torch.float32, device=device)
    check(L.dc_pix_coords(ptr(pc), B, H, W, stream(pc)), "dc_pix_coords")
    return pc


class _Backproject(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, inv_K):
        L = _lib.lib()
        d, ik = _c(depth.detach()), _c(inv_K.detach())
        B, _, H, W = d.shape
        cam = torch.empty(B, 4, H * W, dtype=torch.float32, device=d.device)
        check(L.dc_backproject_fwd(ptr(d), ptr(ik), ptr(cam), B, H, W, stream(d)), "dc_backproject_fwd")
        ctx.save_for_backward(ik)
        ctx.shape = d.shape
        return cam

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        (ik,) = ctx.saved_tensors
        B, _, H, W = ctx.shape
        dd = torch.empty(ctx.shape, dtype=torch.float32, device=g.device)
        g_c = _c(g)      # named: stays alive until the launch is enqueued
        check(L.dc_backproject_bwd(ptr(g_c), ptr(ik), ptr(dd), B, H, W, stream(g_c)), "dc_backproject_bwd")
        return dd, None


def backproject(depth, inv_K):
    return _Backproject.apply(depth, inv_K)


# ----------------------------------------------------------------------------------------------
# a8  Project3D                                                         (reference layers.py:171-193)
# ----------------------------------------------------------------------------------------------
class _Project3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, K, T, H, W, eps):
        L = _lib.lib()
        p, k, t = _c(points.detach()), _c(K.detach()), _c(T.detach())
        B = p.shape[0]
        grid = torch.empty(B, H, W, 2, dtype=torch.float32, device=p.device)
        check(L.dc_project3d_fwd(ptr(p), ptr(k), ptr(t), ptr(grid), B, H, W, float(eps), stream(p)), "dc_project3d_fwd")
        ctx.save_for_backward(p, k, t)
        ctx.dims = (B, H, W, float(eps))
        return grid

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        p, k, t = ctx.saved_tensors
        B, H, W, eps = ctx.dims
        dp, dT = torch.empty_like(p), torch.empty_like(t)
        ws = torch.empty(L.dc_project3d_bwd_workspace(B, H, W), dtype=torch.uint8, device=p.device)
        g_c = _c(g)      # named: stays alive until the launch is enqueued
        check(L.dc_project3d_bwd(ptr(p), ptr(k), ptr(t), ptr(g_c), ptr(dp), ptr(dT), ws.data_ptr(), B, H, W, eps,
                                 stream(p)), "dc_project3d_bwd")
        return dp, None, dT, None, None, None


def project3d(points, K, T, H, W, eps=1e-7):
    return _Project3D.apply(points, K, T, H, W, eps)


# ----------------------------------------------------------------------------------------------
# a9  F.grid_sample(bilinear, border)                                      (reference trainer.py:508)
# ----------------------------------------------------------------------------------------------
class _GridSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, grid, align_corners):
        L = _lib.lib()
        im, g = _c(img.detach()), _c(grid.detach())
        B, C, H, W = im.shape
        Ho, Wo = g.shape[1], g.shape[2]
        out = torch.empty(B, C, Ho, Wo, dtype=torch.float32, device=im.device)
        check(L.dc_grid_sample_fwd(ptr(im), ptr(g), ptr(out), B, C, H, W, Ho, Wo, int(bool(align_corners)), stream(im)),
              "dc_grid_sample_fwd")
        ctx.save_for_backward(im, g)
        ctx.ac = int(bool(align_corners))
        return out

    @staticmethod
    def backward(ctx, go):
        L = _lib.lib()
        im, g = ctx.saved_tensors
        B, C, H, W = im.shape
        Ho, Wo = g.shape[1], g.shape[2]
        dg = torch.empty_like(g)
        g_c = _c(go)      # named: stays alive until the launch is enqueued
        check(L.dc_grid_sample_bwd(ptr(im), ptr(g), ptr(g_c), ptr(dg), B, C, H, W, Ho, Wo, ctx.ac, stream(im)),
              "dc_grid_sample_bwd")
        return None, dg, None       # images are leaves without grad on this path


def grid_sample_border(img, grid, align_corners=False):
    return _GridSample.apply(img, grid, align_corners)


# ----------------------------------------------------------------------------------------------
# a10 F.interpolate(bilinear, align_corners=False)                         (reference trainer.py:474)
# ----------------------------------------------------------------------------------------------
class _UpsampleBilinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, Ho, Wo):
        L = _lib.lib()
        xx = _c(x.detach())
        B, C, h, w = xx.shape
        out = torch.empty(B, C, Ho, Wo, dtype=torch.float32, device=xx.device)
        check(L.dc_upsample_bilinear_fwd(ptr(xx), ptr(out), B * C, h, w, Ho, Wo, stream(xx)), "dc_upsample_bilinear_fwd")
        ctx.dims = (B, C, h, w, Ho, Wo)
        return out

    @staticmethod
    def backward(ctx, go):
        L = _lib.lib()
        B, C, h, w, Ho, Wo = ctx.dims
        dx = torch.empty(B, C, h, w, dtype=torch.float32, device=go.device)
        g_c = _c(go)      # named: stays alive until the launch is enqueued
        check(L.dc_upsample_bilinear_bwd(ptr(g_c), ptr(dx), B * C, h, w, Ho, Wo, stream(g_c)), "dc_upsample_bilinear_bwd")
        return dx, None, None


def upsample_bilinear(x, Ho, Wo):
    return _UpsampleBilinear.apply(x, Ho, Wo)


# ----------------------------------------------------------------------------------------------
# a3  upsample(x): nearest x2                                          (reference layers.py:196-199)
# ----------------------------------------------------------------------------------------------
def _aligned8(t):
    """The nearest x2 kernels move the doubled rows as float2 (the input of the forward is read float by float): an upstream
    gradient that is a contiguous view at an odd float offset of its storage (a slice of a flat buffer, say) is copied to a
    buffer of its own."""
    return t.clone() if t.data_ptr() & 7 else t


class _UpsampleNearest2x(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        xx = _c(x.detach())
        B, C, h, w = xx.shape
        out = torch.empty(B, C, 2 * h, 2 * w, dtype=torch.float32, device=xx.device)   # the allocator's own alignment
        check(_lib.lib().dc_upsample_nearest2x_fwd(ptr(xx), ptr(out), B * C, h, w, stream(xx)), "dc_upsample_nearest2x_fwd")
        return out

    @staticmethod
    def backward(ctx, go):
        g = _aligned8(_c(go))
        B, C, H2, W2 = g.shape
        dx = torch.empty(B, C, H2 // 2, W2 // 2, dtype=torch.float32, device=g.device)
        check(_lib.lib().dc_upsample_nearest2x_bwd(ptr(g), ptr(dx), B * C, H2 // 2, W2 // 2, stream(g)), "dc_upsample_nearest2x_bwd")
        return dx


def upsample_nearest2x(x):
    return _UpsampleNearest2x.apply(x)


# ----------------------------------------------------------------------------------------------
# a11 SSIM                                                              (reference layers.py:218-248)
# ----------------------------------------------------------------------------------------------
class _SSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        L = _lib.lib()
        xx, yy = _c(x.detach()), _c(y.detach())
        B, C, H, W = xx.shape
        out = torch.empty_like(xx)
        check(L.dc_ssim_fwd(ptr(xx), ptr(yy), ptr(out), B * C, H, W, stream(xx)), "dc_ssim_fwd")
        ctx.save_for_backward(xx, yy)
        return out

    @staticmethod
    def backward(ctx, go):
        L = _lib.lib()
        xx, yy = ctx.saved_tensors
        B, C, H, W = xx.shape
        dx = torch.empty_like(xx) if ctx.needs_input_grad[0] else None
        dy = torch.empty_like(yy) if ctx.needs_input_grad[1] else None
        g_c = _c(go)      # named: stays alive until the launch is enqueued
        check(L.dc_ssim_bwd(ptr(xx), ptr(yy), ptr(g_c), ptr(dx), ptr(dy), B * C, H, W, stream(xx)), "dc_ssim_bwd")
        return dx, dy


def ssim(x, y):
    return _SSIM.apply(x, y)


# ----------------------------------------------------------------------------------------------
# a13 get_smooth_loss                                                   (reference layers.py:202-215)
# ----------------------------------------------------------------------------------------------
class _Smooth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp, img):
        L = _lib.lib()
        d, im = _c(disp.detach()), _c(img.detach())
        B, _, h, w = d.shape
        C = im.shape[1]
        out = torch.empty(1, dtype=torch.float32, device=d.device)
        ws = torch.empty(L.dc_smooth_workspace(B, h, w), dtype=torch.uint8, device=d.device)
        check(L.dc_smooth_fwd(ptr(d), ptr(im), ptr(out), ws.data_ptr(), B, C, h, w, stream(d)), "dc_smooth_fwd")
        ctx.save_for_backward(d, im)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        d, im = ctx.saved_tensors
        B, _, h, w = d.shape
        dd = torch.empty_like(d)
        g_c = _c(g.reshape(1))      # named: stays alive until the launch is enqueued
        check(L.dc_smooth_bwd(ptr(d), ptr(im), ptr(g_c), ptr(dd), B, im.shape[1], h, w, stream(d)),
              "dc_smooth_bwd")
        return dd, None


def smooth_loss(disp, img):
    return _Smooth.apply(disp, img)


# ----------------------------------------------------------------------------------------------
# measurement hook (bench.py): hipEvent timing of the dominant photometric kernels
# ----------------------------------------------------------------------------------------------
def profile_enable(max_launches):
    check(_lib.lib().dc_profile_enable(int(max_launches)), "dc_profile_enable")


def profile_collect():
    """-> dict(fwd_ms, fwd_launches, bwd_ms, bwd_launches, fwd_chain_ms, bwd_chain_ms): the dominant kernel of each
    direction and the whole launch chain of each direction; synchronises on the recorded events."""
    fm, bm, fc, bc = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
    fn, bn = ctypes.c_int(0), ctypes.c_int(0)
    check(_lib.lib().dc_profile_collect(ctypes.byref(fm), ctypes.byref(fn), ctypes.byref(bm), ctypes.byref(bn),
                                        ctypes.byref(fc), ctypes.byref(bc)), "dc_profile_collect")
    return {"fwd_ms": fm.value, "fwd_launches": fn.value, "bwd_ms": bm.value, "bwd_launches": bn.value,
            "fwd_chain_ms": fc.value, "bwd_chain_ms": bc.value}


def conv_profile_enable(max_launches, every=1):
    """hipEvent pairs around every `every`-th Winograd conv launch of each kind (0 launches: disable and free)."""
    check(_lib.lib().dc_conv_profile_enable(int(max_launches), int(every)), "dc_conv_profile_enable")


def conv_profile_collect(kind):
    """kind 0: wino_ps_kernel (conv forward / data gradient), 1: wino_wgrad_kernel.
    -> dict(ms, flops (SURVEY 8d algorithmic), executed_flops (issued to the matrix cores), bytes (algorithmic), launches)."""
    ms, fl, ex, by = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
    n = ctypes.c_int(0)
    check(_lib.lib().dc_conv_profile_collect(int(kind), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(ex), ctypes.byref(by),
                                             ctypes.byref(n)), "dc_conv_profile_collect")
    return {"ms": ms.value, "flops": fl.value, "executed_flops": ex.value, "bytes": by.value, "launches": n.value}


# ----------------------------------------------------------------------------------------------
# a2/a3 fused decoder block: act(conv3x3(pad1(cat(up2?(x0), x1))) + bias)
#                                   (reference layers.py:106-136,196-199; networks/depth_decoder.py:50-66)
# ----------------------------------------------------------------------------------------------
ACT_NONE, ACT_ELU, ACT_SIGMOID, ACT_RELU, ACT_TANH = 0, 1, 2, 3, 4
PAD_REFLECT, PAD_ZERO = 0, 1


class _Conv3x3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, x1, weight, bias, up0, act, pad, fork0=None):
        L = _lib.lib()
        a0 = _c(x0.detach())
        a1 = _c(x1.detach()) if x1 is not None else None
        w = _c(weight.detach())
        bs = _c(bias.detach()) if bias is not None else None
        B, C0, h0, w0 = a0.shape
        H, W = (h0 * 2, w0 * 2) if up0 else (h0, w0)
        C1 = 0 if a1 is None else a1.shape[1]
        Co = w.shape[0]
        if tuple(w.shape) != (Co, C0 + C1, 3, 3):
            raise _lib.DepthcoreError("weight %s does not match inputs (%d+%d channels)" % (tuple(w.shape), C0, C1))
        if a1 is not None and tuple(a1.shape) != (B, C1, H, W):
            raise _lib.DepthcoreError("skip tensor %s must be %s" % (tuple(a1.shape), (B, C1, H, W)))
        y = torch.empty(B, Co, H, W, dtype=torch.float32, device=a0.device)
        ctx.prec = _use_precision(_precision[0])
        ws = torch.empty(L.dc_conv3x3_fwd_workspace(C0, C1, B, Co, H, W), dtype=torch.uint8, device=a0.device)
        check(L.dc_conv3x3_fwd(ptr(a0), C0, int(up0), ptr(a1), C1, ptr(w), ptr(bs), ptr(y), ws.data_ptr(), B, Co, H, W,
                               int(act), int(pad), stream(a0)), "dc_conv3x3_fwd")
        ctx.save_for_backward(a0, a1, w, y)
        if act == ACT_RELU:
            _record_kink("relu", y)
        ctx.cfg = (int(up0), int(act), int(pad), bias is not None)
        ctx.slots = (_slot(weight), _slot(bias) if bias is not None else None)
        if ctx.needs_input_grad[2]:
            WgradLanes.count_use(weight)     # (no lane of its own; a weight shared with a laned op must not look single-use)
        # x0 shared with another fused block (the decoder's x feeds dispconv AND the next upconv): a pair GradFork -- whichever
        # backward runs first parks its dx0, the second adds it in the pass that writes its own.  x1 an encoder feature map
        # with a SkipSum: dx1 is offered to the feature's primary consumer (SkipSum)
        ctx.fork0 = fork0 if (fork0 is not None and x0.requires_grad) else None
        ctx.skip1 = skip_of(x1) if (x1 is not None and x1.requires_grad) else None
        return y

    @staticmethod
    def backward(ctx, gy):
        L = _lib.lib()
        a0, a1, w, y = ctx.saved_tensors
        up0, act, pad, has_bias = ctx.cfg
        B, C0 = a0.shape[0], a0.shape[1]
        C1 = 0 if a1 is None else a1.shape[1]
        Co, H, W = y.shape[1], y.shape[2], y.shape[3]
        need = ctx.needs_input_grad
        dx0 = torch.empty_like(a0) if need[0] else None
        dx1 = torch.empty_like(a1) if (a1 is not None and need[1]) else None
        dw = _grad_dst(ctx.slots[0], w) if need[2] else None
        db = None
        if has_bias and need[3]:
            db = _grad_dst(ctx.slots[1], None)
            if db is None:
                db = torch.empty(Co, dtype=torch.float32, device=y.device)
        _use_precision(ctx.prec)
        ws = torch.empty(L.dc_conv3x3_bwd_workspace(C0, C1, B, Co, H, W), dtype=torch.uint8, device=y.device)
        g_c = _c(gy)      # named: stays alive until the launch is enqueued
        fork0 = ctx.fork0 if dx0 is not None else None
        first = fork0 is not None and fork0.arrive() == 0
        add0 = fork0.take() if (fork0 is not None and not first) else None
        if add0 is not None and (add0.shape != a0.shape or not add0.is_contiguous()):
            raise _lib.DepthcoreError("GradFork: parked gradient %s does not match the shared input %s" % (tuple(add0.shape), tuple(a0.shape)))
        check(L.dc_conv3x3_bwd_add(ptr(a0), C0, up0, ptr(a1), C1, ptr(w), ptr(y), ptr(g_c), ptr(dx0), ptr(dx1), ptr(add0), None, ptr(dw),
                                   ptr(db), ws.data_ptr(), B, Co, H, W, act, pad, stream(a0)), "dc_conv3x3_bwd_add")
        if first:
            fork0.park(dx0)            # the other block adds it and returns the sum
            dx0 = None
        if ctx.skip1 is not None:
            dx1 = ctx.skip1.offer(dx1)
        return dx0, dx1, dw, db, None, None, None, None


def conv3x3_block(x0, x1, weight, bias, up0=False, act=ACT_NONE, pad=PAD_REFLECT, fork0=None):
    return _Conv3x3.apply(x0, x1, weight, bias, up0, act, pad, fork0)


# ----------------------------------------------------------------------------------------------
# a1 training-mode BatchNorm2d (+ residual add) (+ ReLU), fused  (ResNet BasicBlock / Bottleneck / stem)
# ----------------------------------------------------------------------------------------------
class _BNReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, gamma, beta, running_mean, running_var, eps, momentum, relu, groups, fork=None):
        L = _lib.lib()
        xx = _c(x.detach())
        rr = _c(res.detach()) if res is not None else None
        g, b = _c(gamma.detach()), _c(beta.detach())
        N, C, H, W = xx.shape
        y = torch.empty_like(xx)
        mean = torch.empty(groups * C, dtype=torch.float32, device=xx.device)
        invstd = torch.empty(groups * C, dtype=torch.float32, device=xx.device)
        ws = torch.empty(L.dc_bn_workspace(N, C, H * W), dtype=torch.uint8, device=xx.device)
        nmask = L.dc_bn_mask_bytes(N, C, H * W) if relu else 0
        mask = torch.empty(nmask, dtype=torch.uint8, device=xx.device) if nmask else None      # [y > 0] as bits
        check(L.dc_bn_relu_fwd(ptr(xx), ptr(rr), ptr(g), ptr(b), ptr(y), ptr(mean), ptr(invstd),
                               ptr(running_mean), ptr(running_var), ws.data_ptr(), mask.data_ptr() if nmask else None,
                               N, C, H * W, float(eps), float(momentum), int(relu), int(groups), stream(xx)), "dc_bn_relu_fwd")
        ctx.save_for_backward(xx, y, g, mean, invstd, mask)
        if relu:
            _record_kink("relu", y)
        ctx.cfg = (int(relu), res is not None, int(groups))
        ctx.slots = (_slot(gamma), _slot(beta))
        ctx.fork = fork if (fork is not None and res is not None and res.requires_grad) else None
        return y

    @staticmethod
    def backward(ctx, gy):
        L = _lib.lib()
        xx, y, g, mean, invstd, mask = ctx.saved_tensors
        relu, has_res, groups = ctx.cfg
        N, C, H, W = xx.shape
        g_c = _c(gy)
        dx = torch.empty_like(xx)
        dres = torch.empty_like(xx) if (has_res and ctx.needs_input_grad[1]) else None
        dgamma = _grad_dst(ctx.slots[0], g)
        dbeta = _grad_dst(ctx.slots[1], g)
        ws = torch.empty(L.dc_bn_workspace(N, C, H * W), dtype=torch.uint8, device=xx.device)
        check(L.dc_bn_relu_bwd(ptr(xx), ptr(y), ptr(g_c), ptr(g), ptr(mean), ptr(invstd), ptr(dx), ptr(dres), ptr(dgamma),
                               ptr(dbeta), ws.data_ptr(), mask.data_ptr() if mask is not None else None, N, C, H * W, relu,
                               groups, stream(xx)), "dc_bn_relu_bwd")
        if ctx.fork is not None and dres is not None:
            ctx.fork.park(dres)             # conv1's data-gradient kernel adds it (GradFork)
            dres = None
        return dx, dres, dgamma, dbeta, None, None, None, None, None, None, None


def bn_relu(x, bn, res=None, relu=True, groups=1, fork=None):
    """y = relu?(bn(x) [+ res]) with `bn` an nn.BatchNorm2d in training mode (batch statistics; updates its
    running_mean / running_var in place; `num_batches_tracked` is advanced by the caller).  `groups` > 1:
    the batch is that many independent sub-batches (statistics and running-stat updates per sub-batch)."""
    mom = 0.1 if bn.momentum is None else bn.momentum
    return _BNReLU.apply(x, res, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, mom, relu, groups, fork)


# ----------------------------------------------------------------------------------------------
# a1 eval-mode BatchNorm2d (+ residual add) (+ ReLU): running statistics, read only  (trainer.py:222-226 set_eval)
# ----------------------------------------------------------------------------------------------
class _BNEval(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, gamma, beta, running_mean, running_var, eps, relu):
        L = _lib.lib()
        xx = _c(x.detach())
        rr = _c(res.detach()) if res is not None else None
        g, b = _c(gamma.detach()), _c(beta.detach())
        rm, rv = running_mean.detach(), running_var.detach()
        N, C, H, W = xx.shape
        coef = torch.empty(3, C, dtype=torch.float32, device=xx.device)        # scale, shift, invstd
        check(L.dc_bn_eval_coef(ptr(g), ptr(b), ptr(rm), ptr(rv), ptr(coef[0]), ptr(coef[1]), ptr(coef[2]), C, float(eps),
                                stream(xx)), "dc_bn_eval_coef")
        y = torch.empty_like(xx)
        check(L.dc_bn_apply(ptr(xx), ptr(rr), ptr(coef[0]), ptr(coef[1]), ptr(y), None, N, C, H * W, int(relu), 1, stream(xx)),
              "dc_bn_apply")
        ctx.save_for_backward(xx, y if relu else None, coef, rm)
        if relu:
            _record_kink("relu", y)
        ctx.cfg = (int(relu), res is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        L = _lib.lib()
        xx, y, coef, rm = ctx.saved_tensors
        relu, has_res = ctx.cfg
        N, C, H, W = xx.shape
        g_c = _c(gy)
        dx = torch.empty_like(xx)
        dres = torch.empty_like(xx) if (has_res and ctx.needs_input_grad[1]) else None
        dgamma = torch.empty(C, dtype=torch.float32, device=xx.device) if ctx.needs_input_grad[2] else None
        dbeta = torch.empty(C, dtype=torch.float32, device=xx.device) if ctx.needs_input_grad[3] else None
        ws = torch.empty(L.dc_bn_eval_bwd_workspace(N, C, H * W), dtype=torch.uint8, device=xx.device)
        check(L.dc_bn_eval_bwd(ptr(xx), ptr(y), ptr(g_c), ptr(coef[0]), ptr(rm), ptr(coef[2]), ptr(dx), ptr(dres), ptr(dgamma),
                               ptr(dbeta), ws.data_ptr(), N, C, H * W, relu, stream(xx)), "dc_bn_eval_bwd")
        return dx, dres, dgamma, dbeta, None, None, None, None


def bn_eval(x, bn, res=None, relu=True):
    """y = relu?(bn(x) [+ res]) with `bn` an nn.BatchNorm2d in eval mode: its running statistics (never modified; nor is
    `num_batches_tracked`).  Differentiable -- frozen-statistics fine-tuning: dx = scale g', dres = g', dbeta = sum g',
    dgamma = sum g' (x - running_mean) invstd, with g' the gradient masked by the ReLU decision.  `bn_groups` play no role in
    eval mode.  A BatchNorm without running statistics (track_running_stats=False normalises with batch statistics even in
    eval mode) or without affine parameters is refused."""
    if not bn.track_running_stats or bn.running_mean is None or bn.running_var is None:
        raise DepthcoreError("eval-mode BatchNorm2d without running statistics (track_running_stats=False) is not supported")
    if bn.weight is None or bn.bias is None:
        raise DepthcoreError("eval-mode BatchNorm2d without affine parameters is not supported")
    return _BNEval.apply(x, res, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, relu)


# ----------------------------------------------------------------------------------------------
# depth metrics of validation  (trainer.py:624-652, evaluate_depth.py:190-235, layers.py:251-269)
# ----------------------------------------------------------------------------------------------
TRAINER_CROP = (153, 371, 44, 1197)      # trainer.py:638 (garg / eigen crop of a 375 x 1242 frame)
_PROTOCOLS = {"trainer": _lib.EVAL_TRAINER, "eigen": _lib.EVAL_EIGEN, "gt_positive": _lib.EVAL_GT_POSITIVE}


def eigen_crop(Hg, Wg):
    """evaluate_depth.py:207-208: the crop rows / columns as numpy computes them (fp64 products, truncated to int32)."""
    import numpy as np
    c = np.array([0.40810811 * Hg, 0.99189189 * Hg, 0.03594771 * Wg, 0.96405229 * Wg]).astype(np.int32)
    return tuple(int(v) for v in c)


def _depth_errors(pred, gt, protocol, crop, median_scaling, scale_factor, image_ids=None):
    """-> (metrics (G, 7), ratios (G,), host copy of [metrics | ratios | status]) after ONE device-to-host copy.
    image_ids: the caller's numbers of the B images, for the error message of an empty mask."""
    if protocol not in _PROTOCOLS:
        raise ValueError("protocol: 'trainer' (trainer.py:624-652), 'eigen' (evaluate_depth.py:190-235) or 'gt_positive' "
                         "(evaluate_depth.py:210-211)")
    L = _lib.lib()
    p, g = _c(pred.detach()), _c(gt.detach())
    if p.dim() != 4 or g.dim() != 4 or p.shape[1] != 1 or g.shape[1] != 1 or p.shape[0] != g.shape[0]:
        raise DepthcoreError("depth_errors: pred (B,1,h,w) and gt (B,1,Hg,Wg), got %s and %s" % (tuple(p.shape), tuple(g.shape)))
    B, _, h, w = p.shape
    Hg, Wg = g.shape[-2:]
    eigen = protocol != "trainer"                  # per-image groups (either mask of evaluate_depth.py)
    if protocol == "gt_positive":
        crop = (0, Hg, 0, Wg)                       # the whole frame (the kernel ignores crop for this protocol)
    elif crop is None:
        crop = eigen_crop(Hg, Wg) if eigen else TRAINER_CROP
    G = B if eigen else 1
    buf = torch.empty(G * 9, dtype=torch.float32, device=p.device)       # metrics | ratios | status (int32)
    d = _lib.DepthEvalDesc()
    d.B, d.h, d.w, d.Hg, d.Wg = B, h, w, Hg, Wg
    d.protocol = _PROTOCOLS[protocol]
    for i in range(4):
        d.crop[i] = int(crop[i])
    d.median_scaling = int(bool(median_scaling))
    d.scale_factor = float(scale_factor)
    d.ratios = buf[G * 7:].data_ptr()
    status = buf[G * 8:].view(torch.int32)
    d.status = ptr(status, torch.int32)
    ws = torch.empty(L.dc_depth_errors_workspace(ctypes.byref(d)), dtype=torch.uint8, device=p.device)
    check(L.dc_depth_errors(ctypes.byref(d), ptr(p), ptr(g), ptr(buf), ws.data_ptr(), stream(p)), "dc_depth_errors")
    host = buf.cpu()
    bad = [i for i, v in enumerate(host[G * 8:].view(torch.int32).tolist()) if v != 0]
    if bad:
        what = ("image %d" % image_ids[bad[0]] if image_ids is not None else "image %d of the batch" % bad[0]) if eigen else "the batch"
        raise DepthcoreError("depth_errors (%s protocol): the mask of %s selects no pixel (%s)" % (protocol, what, _lib._ERR.get(
            host[G * 8:].view(torch.int32)[bad[0]].item(), "status %d")))
    return buf[:G * 7].view(G, 7), buf[G * 7:G * 8], host


def depth_errors(pred, gt, protocol="trainer", crop=None, median_scaling=True, scale_factor=1.0):
    """Depth metrics abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3 of `pred` (B,1,h,w) against `gt` (B,1,Hg,Wg), pred
    bilinearly upsampled to gt's size on the way (dc_depth_errors: one launch chain, medians by radix selection, fp64 sums,
    bitwise reproducible).
      protocol="trainer": Trainer.compute_depth_losses (trainer.py:624-652) -- pred is depth; gt > 0 inside `crop` (default
        rows 153:371, cols 44:1197); torch.median; one ratio for the whole batch.  Returns a (7,) device tensor.
      protocol="eigen": evaluate_depth.py:198-232 -- pred is scaled disparity (depth = 1 / disp * scale_factor);
        1e-3 < gt < 80 inside the fractional Eigen crop; np.median; per image.  Returns ((B, 7), ratios (B,)).
      protocol="gt_positive": as "eigen" but the mask is gt > 0 over the whole frame (`crop` is not used) -- every split
        but "eigen" in evaluate_depth.py:210-211 (eigen_benchmark).  Returns ((B, 7), ratios (B,)).
    median_scaling=False: --disable_median_scaling (ratios are then 1).  A group whose mask selects no pixel raises
    DepthcoreError naming it (this waits for the result: one small device-to-host copy per call)."""
    out, ratios, _ = _depth_errors(pred, gt, protocol, crop, median_scaling, scale_factor)
    if protocol == "trainer":
        return out[0]
    return out, ratios


# ----------------------------------------------------------------------------------------------
# pose evaluation: the trajectory scoring of evaluate_pose.py:23-46, 104-125
# ----------------------------------------------------------------------------------------------
def pose_ate(pred, gt_global, track_length=5):
    """Absolute trajectory error of every `track_length`-frame snippet (dc_pose_ate: fp64, two launches, bitwise reproducible).
    pred (N,4,4) float32 source-to-target transforms on the device; gt_global (N+1,3,4) float64 rows of KITTI's poses/XX.txt
    on the device.  -> (ates (N,), mean, std) as views of ONE host float64 tensor: the call ends with the only device-to-host
    copy.  A snippet whose predicted points all coincide is NaN (0 / 0 as in numpy), and so are mean and std then."""
    L = _lib.lib()
    p, g = _c(pred.detach()), _c(gt_global.detach())
    if p.dim() != 3 or tuple(p.shape[1:]) != (4, 4) or g.dim() != 3 or tuple(g.shape[1:]) != (3, 4):
        raise DepthcoreError("pose_ate: pred (N,4,4) and gt_global (M,3,4), got %s and %s" % (tuple(p.shape), tuple(g.shape)))
    N, M = p.shape[0], g.shape[0]
    if M < 2 or N != M - 1:
        raise DepthcoreError("pose_ate: %d predicted transforms need %d ground-truth poses, got %d" % (N, N + 1, M))
    if int(track_length) < 1:
        raise DepthcoreError("pose_ate: track_length must be at least 1")
    out = torch.empty(N + 2, dtype=torch.float64, device=p.device)
    check(L.dc_pose_ate(ptr(p), ptr(g, torch.float64), ptr(out, torch.float64), N, M, int(track_length), stream(p)), "dc_pose_ate")
    host = out.cpu()
    return host[:N], host[N], host[N + 1]


# ----------------------------------------------------------------------------------------------
# velodyne depth maps: kitti_utils.generate_depth_map + KITTIRAWDataset.get_depth's resize and flip, a batch per call
# ----------------------------------------------------------------------------------------------
def lidar_depth_maps(points, counts, P, sizes, out_size=None, vel_depth=False, flips=None):
    """Sparse depth maps of B velodyne scans (dc_lidar_depth_maps: three launches on the current stream, bitwise reproducible).
      points: (N, 4) float32 device tensor, the scans back to back in file layout (column 3 is ignored), 16-byte aligned;
      counts: B ints, the points of every scan (0 gives an all-zero map), sum <= N;
      P: (B, 3, 4) float64 on the host (numpy or CPU tensor), lidar.velo_to_image's matrix of every scan;
      sizes: B native (W, H);  out_size: (Ho, Wo) of the result, resized from the native size by Pillow's NEAREST rule
        (lidar.nearest_tables) -- None: the native size, which all scans must then share;
      vel_depth: one bool or B of them (True: the depth is x_velo, the export's convention);  flips: B bools (np.fliplr).
    -> (B, 1, Ho, Wo) float32.  The descriptors and index tables are small host arrays (lidar.descriptors): one host-to-device
    copy per call; a caller whose upload already carries them uses `lidar_depth_maps_staged`."""
    from .lidar import descriptors
    d = descriptors(counts, P, sizes, out_size, vel_depth, flips)
    return lidar_depth_maps_staged(points, d, torch.from_numpy(d.host).to(points.device))


def lidar_depth_maps_staged(points, d, block):
    """`lidar_depth_maps` with the descriptors already on the device: d is lidar.descriptors(...), block a uint8 device tensor
    holding the bytes of d.host at an 8-byte aligned address (the loader's one upload carries them behind the scans)."""
    L = _lib.lib()
    pts = points.detach()
    if pts.dim() != 2 or pts.shape[1] != 4:
        raise DepthcoreError("lidar_depth_maps: points (N, 4), got %s" % (tuple(pts.shape),))
    if block.dtype != torch.uint8 or block.numel() != d.host.size or block.data_ptr() % 8 or block.device != pts.device:
        raise DepthcoreError("lidar_depth_maps: the device block must be the %d descriptor bytes, 8-byte aligned, on %s"
                             % (d.host.size, pts.device))
    dev, n_points = pts.device, pts.shape[0]
    if n_points == 0:                 # every scan is empty: the entry point still wants a valid pointer
        pts = torch.zeros((1, 4), dtype=torch.float32, device=dev)
    ws_bytes = L.dc_lidar_workspace_bytes(d.B, int(d.desc["W"].max()), int(d.desc["H"].max()))
    if ws_bytes == 0:
        raise DepthcoreError("lidar_depth_maps: native sizes up to %d x %d are out of range" % (d.desc["W"].max(), d.desc["H"].max()))
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    out = torch.empty((d.B, 1, d.Ho, d.Wo), dtype=torch.float32, device=dev)
    base = ptr(block, torch.uint8)
    check(L.dc_lidar_depth_maps(ptr(pts), n_points, d.desc.ctypes.data, base, d.B, d.rows.ctypes.data, base + d.rows_off,
                                d.cols.ctypes.data, base + d.cols_off, d.Ho, d.Wo, ptr(out), ws.data_ptr(), ws_bytes, stream(pts)),
          "dc_lidar_depth_maps")
    return out


# ----------------------------------------------------------------------------------------------
# depth evaluation: the prediction side of evaluate_depth.py:95-135 and its benchmark export (:159-171)
# ----------------------------------------------------------------------------------------------
def flip_concat(x):
    """torch.cat((x, torch.flip(x, [3])), 0) of evaluate_depth.py:123 in one launch (dc_flip_concat): (B,C,H,W) -> (2B,C,H,W).
    No gradient (an evaluation input)."""
    L = _lib.lib()
    xx = _c(x.detach())
    if xx.dim() != 4:
        raise DepthcoreError("flip_concat: (B,C,H,W), got %s" % (tuple(xx.shape),))
    B, C, H, W = xx.shape
    out = torch.empty((2 * B, C, H, W), dtype=torch.float32, device=xx.device)
    check(L.dc_flip_concat(ptr(xx), ptr(out), B, C, H, W, stream(xx)), "dc_flip_concat")
    return out


def post_process_disparity(disp, min_depth, max_depth):
    """The decoder's sigmoid disparity (2B,1,h,w) of the batch [x; flip_w(x)] -> (B,1,h,w) post-processed scaled disparity
    (dc_disp_post_process): disp_to_depth's scaled disparity of both halves (bit for bit ops.disp_to_depth's), the second
    mirrored back, blended as batch_post_process_disparity (evaluate_depth.py:48-56) in its own types -- fp32 mean, fp64 masks
    and products -- and rounded to fp32 once.  No gradient."""
    L = _lib.lib()
    d = _c(disp.detach())
    if d.dim() != 4 or d.shape[1] != 1 or d.shape[0] % 2:
        raise DepthcoreError("post_process_disparity: (2B,1,h,w), got %s" % (tuple(d.shape),))
    B, _, h, w = d.shape
    out = torch.empty((B // 2, 1, h, w), dtype=torch.float32, device=d.device)
    check(L.dc_disp_post_process(ptr(d), ptr(out), B // 2, h, w, float(min_depth), float(max_depth), stream(d)),
          "dc_disp_post_process")
    return out


STEREO_SCALE_FACTOR = 5.4       # evaluate_depth.py:24
BENCHMARK_SIZE = (352, 1216)    # evaluate_depth.py:166 (cv2's (width, height) = (1216, 352))


def depth_png16(disp, size=BENCHMARK_SIZE, scale=STEREO_SCALE_FACTOR):
    """KITTI benchmark depth maps of evaluate_depth.py:165-169 (dc_depth_png16): scaled disparity (N,1,h,w) ->
    (N, Ho, Wo) uint16 = uint16(clip(scale / bilinear(disp), 0, 80) * 256), the upsample F.interpolate(bilinear,
    align_corners=False)'s (bit for bit ops.upsample_bilinear's).  The PNG encoding is the caller's."""
    L = _lib.lib()
    d = _c(disp.detach())
    if d.dim() != 4 or d.shape[1] != 1:
        raise DepthcoreError("depth_png16: (N,1,h,w), got %s" % (tuple(d.shape),))
    N, _, h, w = d.shape
    Ho, Wo = int(size[0]), int(size[1])
    out = torch.empty((N, Ho, Wo), dtype=torch.uint16, device=d.device)
    check(L.dc_depth_png16(ptr(d), out.data_ptr(), N, h, w, Ho, Wo, float(scale), stream(d)), "dc_depth_png16")
    return out


# ----------------------------------------------------------------------------------------------
# single-image inference: the colour image of test_simple.py:126-145
# ----------------------------------------------------------------------------------------------
_MAGMA = {}


def magma_lut(device=None):
    """matplotlib's 256-entry magma quantised as test_simple.py:141 does, (lut[:256, :3] * 255).astype(uint8): a (256,3) uint8
    tensor from the literal in depthcore/_magma.py (matplotlib is not a dependency).  device=None: on the host."""
    if "host" not in _MAGMA:
        from ._magma import MAGMA_LUT8_HEX
        raw = bytes.fromhex(MAGMA_LUT8_HEX)
        if len(raw) != 768:
            raise DepthcoreError("depthcore/_magma.py: expected 768 bytes, got %d" % len(raw))
        _MAGMA["host"] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).view(256, 3)
    if device is None:
        return _MAGMA["host"]
    device = torch.device(device)
    if device not in _MAGMA:
        _MAGMA[device] = _MAGMA["host"].to(device)
    return _MAGMA[device]


def _render_disparity(disp, size, percentile, lut, buf=None):
    """dc_disp_render into `buf`, a uint8 device tensor laid out [rgb (N*Ho*Wo*3) | pad to 4 | range (N*2 fp32)] (allocated when
    None) -> (rgb, range, buf): views of it, so that a caller brings both to the host with one copy."""
    L = _lib.lib()
    d = _c(disp.detach())
    if d.dim() != 4 or d.shape[1] != 1:
        raise DepthcoreError("render_disparity: (N,1,h,w), got %s" % (tuple(d.shape),))
    N, _, h, w = d.shape
    Ho, Wo = int(size[0]), int(size[1])
    q = float(percentile)
    if N < 1 or h < 1 or w < 1 or Ho < 1 or Wo < 1:
        raise DepthcoreError("render_disparity: empty input %s or target size %s" % (tuple(d.shape), (Ho, Wo)))
    if not 0.0 <= q <= 100.0:
        raise DepthcoreError("render_disparity: percentile must be in [0, 100], got %r" % (percentile,))
    if lut is None:
        lut = magma_lut(d.device)
    if tuple(lut.shape) != (256, 3) or lut.dtype != torch.uint8 or lut.device != d.device:
        raise DepthcoreError("render_disparity: lut must be a (256,3) uint8 tensor on %s, got %s %s on %s"
                             % (d.device, tuple(lut.shape), lut.dtype, lut.device))
    nrgb = N * Ho * Wo * 3
    roff = (nrgb + 3) & ~3
    if buf is None:
        buf = torch.empty(roff + N * 8, dtype=torch.uint8, device=d.device)
    rgb = buf[:nrgb].view(N, Ho, Wo, 3)
    rng = buf[roff:roff + N * 8].view(torch.float32).view(N, 2)
    nws = L.dc_disp_render_ws_bytes(N, h, w, Ho, Wo)
    if nws == 0:
        raise DepthcoreError("render_disparity: unsupported shape %s -> %s" % (tuple(d.shape), (Ho, Wo)))
    ws = torch.empty(nws, dtype=torch.uint8, device=d.device)
    check(L.dc_disp_render(ptr(d), ptr(_c(lut), torch.uint8), ptr(rgb, torch.uint8), ptr(rng), N, h, w, Ho, Wo, q, ws.data_ptr(),
                           nws, stream(d)), "dc_disp_render")
    return rgb, rng, buf


def render_disparity(disp, size, percentile=95.0, lut=None):
    """The colour image of test_simple.py:126-145 (dc_disp_render): disp (N,1,h,w) -> (rgb (N,Ho,Wo,3) uint8 -- interleaved, what
    PIL.Image.fromarray takes -- and range (N,2) float32 = (vmin, vmax) of every image), device tensors on the current stream.
    Each image is upsampled to size = (Ho, Wo) by F.interpolate(bilinear, align_corners=False)'s expression (bit for bit
    ops.upsample_bilinear's, never stored), normalised between its own minimum and its own `percentile` (numpy's linear
    interpolation between two exact order statistics, found by radix selection) as matplotlib's Normalize does, and looked up
    in `lut`, a (256,3) uint8 device tensor (default: magma).  Values above the percentile take the last colour; a constant
    image takes the first.  Non-finite input is outside the contract.  Bitwise reproducible.  No gradient."""
    rgb, rng, _ = _render_disparity(disp, size, percentile, lut)
    return rgb, rng


# ----------------------------------------------------------------------------------------------
# training-log image panels: the pictures of trainer.py:666-698, composed on the device
# ----------------------------------------------------------------------------------------------
TILE_KINDS = {"rgb": _lib.TILE_RGB, "norm": _lib.TILE_NORM, "unit": _lib.TILE_UNIT, "mask": _lib.TILE_MASK}


def log_panels(tiles, n_panels, size, lut=None, background=0, buf=None):
    """`n_panels` interleaved uint8 images (n_panels, PH, PW, 3), size = (PH, PW), composed from `tiles` (dc_log_panel: at most
    three launches on the current stream, bitwise reproducible).  A tile is (src, kind, panel, up, x0, y0[, thr]):
      src: a device tensor -- "rgb" (3,h,w) float32, "norm" / "unit" (h,w) float32, "mask" (h,w) uint8;
      kind: "rgb" | "norm" | "unit" | "mask" (or the DC_TILE_* number): [0, 1] -> bytes by round-half-up per channel; the
        reference's normalize_image and the colour table `lut` ((256,3) uint8 on the device, default magma); [0, 1] -> grey;
        src >= thr ? 255 : 0;
      panel, (x0, y0): the destination image and the tile's top-left corner in it; up: integer nearest-neighbour factor, the
        tile covers (h*up) x (w*up) pixels.
    Tiles of one panel must not overlap and must lie inside it; a pixel no tile covers holds `background`.  `buf`: a uint8
    device tensor of at least n_panels*PH*PW*3 bytes to compose into (the result is a view of it); None allocates.  The tile
    descriptors are a small host array: one host-to-device copy per call.  No gradient."""
    L = _lib.lib()
    PH, PW = int(size[0]), int(size[1])
    n = len(tiles)
    if n < 1:
        raise DepthcoreError("log_panels: no tiles")
    desc = (_lib.PanelTile * n)()
    keep, dev = [], None
    for i, t in enumerate(tiles):
        src, kind, panel, up, x0, y0 = t[:6]
        thr = t[6] if len(t) > 6 else 0
        kind = TILE_KINDS.get(kind, kind)
        if kind not in TILE_KINDS.values():
            raise DepthcoreError("log_panels: tile %d: unknown kind %r" % (i, t[1]))
        s = _c(src.detach())
        p = ptr(s, torch.uint8 if kind == _lib.TILE_MASK else torch.float32)
        if s.dim() != (3 if kind == _lib.TILE_RGB else 2) or (kind == _lib.TILE_RGB and s.shape[0] != 3):
            raise DepthcoreError("log_panels: tile %d: a %s tile reads %s, got %s"
                                 % (i, t[1], "(3,h,w)" if kind == _lib.TILE_RGB else "(h,w)", tuple(s.shape)))
        dev = s.device if dev is None else dev
        if s.device != dev:
            raise DepthcoreError("log_panels: tile %d lives on %s, the others on %s" % (i, s.device, dev))
        keep.append(s)
        d = desc[i]
        d.src, d.src_elems, d.kind, d.panel = p, s.numel(), kind, int(panel)
        d.h, d.w, d.up, d.x0, d.y0, d.thr = int(s.shape[-2]), int(s.shape[-1]), int(up), int(x0), int(y0), int(thr)
    if lut is None:
        lut = magma_lut(dev)
    if tuple(lut.shape) != (256, 3) or lut.dtype != torch.uint8 or lut.device != dev:
        raise DepthcoreError("log_panels: lut must be a (256,3) uint8 tensor on %s, got %s %s on %s"
                             % (dev, tuple(lut.shape), lut.dtype, lut.device))
    nbytes = max(int(n_panels), 0) * max(PH, 0) * max(PW, 0) * 3
    if buf is None:
        buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    if buf.dtype != torch.uint8 or buf.device != dev or buf.numel() < nbytes or not buf.is_contiguous():
        raise DepthcoreError("log_panels: buf must be a contiguous uint8 tensor of at least %d bytes on %s" % (nbytes, dev))
    # one upload: [descriptors | the range keys' workspace] (sizeof(dc_panel_tile) = 48 keeps the keys 8-byte aligned)
    nd, nws = ctypes.sizeof(desc), L.dc_log_panel_ws_bytes(n)
    host = torch.zeros(nd + nws, dtype=torch.uint8)
    ctypes.memmove(host.data_ptr(), ctypes.addressof(desc), nd)
    block = host.to(dev)
    base = block.data_ptr()
    check(L.dc_log_panel(ctypes.addressof(desc), base, n, ptr(_c(lut), torch.uint8), buf.data_ptr(), int(n_panels), PH, PW,
                         int(background), base + nd, nws, stream(buf)), "dc_log_panel")
    return buf[:nbytes].view(int(n_panels), PH, PW, 3)


# ----------------------------------------------------------------------------------------------
# a1 nn.MaxPool2d(3, 2, 1) of the ResNet stem
# ----------------------------------------------------------------------------------------------
class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, skip=None):
        L = _lib.lib()
        xx = _c(x.detach())
        N, C, H, W = xx.shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = torch.empty(N, C, Ho, Wo, dtype=torch.float32, device=xx.device)
        code = torch.empty(N, C, Ho, Wo, dtype=torch.uint8, device=xx.device)
        check(L.dc_maxpool3x3s2_fwd(ptr(xx), ptr(y), code.data_ptr(), N * C, H, W, stream(xx)), "dc_maxpool3x3s2_fwd")
        ctx.save_for_backward(code)
        _record_kink("maxpool", code)
        ctx.dims = (N, C, H, W)
        ctx.skip = skip if (skip is not None and x.requires_grad) else None
        if ctx.skip is not None:
            ctx.skip.arm()
        return y

    @staticmethod
    def backward(ctx, gy):
        L = _lib.lib()
        (code,) = ctx.saved_tensors
        N, C, H, W = ctx.dims
        g_c = _c(gy)
        dx = torch.empty(N, C, H, W, dtype=torch.float32, device=gy.device)
        add = ctx.skip.take() if ctx.skip is not None else None
        if add is not None and (tuple(add.shape) != (N, C, H, W) or not add.is_contiguous()):
            raise _lib.DepthcoreError("SkipSum: gradient %s does not match the pooled tensor %s" % (tuple(add.shape), (N, C, H, W)))
        check(L.dc_maxpool3x3s2_bwd_add(ptr(g_c), code.data_ptr(), ptr(dx), ptr(add), N * C, H, W, stream(g_c)), "dc_maxpool3x3s2_bwd_add")
        return dx, None


def maxpool3x3s2(x, skip=None):
    """nn.MaxPool2d(3, 2, 1).  `skip`: the SkipSum of x (its other consumers' gradients are added in the backward kernel)."""
    return _MaxPool.apply(x, skip)


# ----------------------------------------------------------------------------------------------
# a1 trunk conv3x3 (stride 1, zero pad 1, no bias): fused Winograd F(2x2,3x3) forward and data gradient
# ----------------------------------------------------------------------------------------------
def wino_conv3x3(x, weight, fork=None):
    """F.conv2d(x, weight, None, 1, 1) for 3x3 kernels on even-width maps (fused Winograd on the matrix cores).
    The Winograd kernels use 32-bit buffer offsets: a tensor of 2 GiB or more takes the direct implicit-GEMM kernels of
    the fused conv block (same arithmetic contract, size_t indexing) instead."""
    if max(x.numel(), x.numel() // x.shape[1] * weight.shape[0]) * 4 >= 0x7fffffff:
        if fork is not None:
            fork.armed = False          # (the direct kernels have no addend: the caller falls back to autograd's sum)
            raise _lib.DepthcoreError("GradFork is not available on the >= 2 GiB path; call without a fork")
        return conv3x3_block(x, None, weight, None, False, ACT_NONE, PAD_ZERO)
    return _ConvF.apply(x, weight, "wino", 1, fork, None, None, None, None, None)


# ---- transformed-weight cache of the Winograd kernels (include/depthcore.h: dc_wino_cache_*) ----------------------
def _wino_release(owner):
    """weakref.finalize target: runs when a WinoWeightCache is closed or collected (never touches the dead object)."""
    try:
        _lib.lib().dc_wino_cache_release_owner(owner)
    except Exception:
        pass


class WinoWeightCache:
    """A model's registrations in libdepthcore's Winograd weight cache (one owner per Trainer).

    `refresh()` at the start of a training step transforms every registered 3x3 weight in one launch; the step's
    convolutions (forward, data gradient, and every frame of the sequence models) then skip their per-launch transform;
    `invalidate()` once the backward is done, before the optimiser rewrites the weights.

    Every cache object is its own OWNER in the library: its refresh launch (and a hipGraph that captured it) reads this
    object's weights only, which `_keep` holds alive for as long as the owner exists.  Constructing, closing or garbage-
    collecting another cache can therefore neither free nor rewrite anything a captured graph of this one reads; `close()`
    (also run when the object is collected) releases this owner only, and its device buffers are parked until `clear_all()`."""

    def __init__(self, params):
        L = _lib.lib()
        self._keep = []
        self._owner = int(L.dc_wino_cache_new_owner())
        for p_ in params:
            # (3x3: Winograd U / prepared bf16 weights; 1x1: the split-operand GEMMs' three bf16 pieces, csrc/gemm1x1_x3.hip)
            if p_.dim() == 4 and tuple(p_.shape[2:]) in ((3, 3), (1, 1)) and p_.is_cuda and p_.dtype == torch.float32 and p_.is_contiguous():
                check(L.dc_wino_cache_register(self._owner, p_.data_ptr(), int(p_.shape[1]), int(p_.shape[0])),
                      "dc_wino_cache_register")
                self._keep.append(p_)           # the registry holds raw addresses: keep the tensors alive with it
        self._fin = weakref.finalize(self, _wino_release, self._owner)

    def refresh(self):
        if self._fin.alive and self._keep:
            check(_lib.lib().dc_wino_cache_refresh(self._owner, stream(self._keep[0])), "dc_wino_cache_refresh")

    def invalidate(self):
        if self._fin.alive:
            _lib.lib().dc_wino_cache_invalidate(self._owner)

    def variants(self):
        """cached (weight, pass, tile layout) variants in the whole registry (0 once every owner is closed)."""
        return int(_lib.lib().dc_wino_cache_variants()) if self._fin.alive else 0

    def close(self):
        self._fin()                             # unregister once (idempotent)
        self._keep = []

    @staticmethod
    def clear_all():
        """Drop every registration and free every parked buffer (device-synchronising).  Only when no captured graph that
        used the cache will be replayed again."""
        check(_lib.lib().dc_wino_cache_clear(), "dc_wino_cache_clear")


# ----------------------------------------------------------------------------------------------
# a1 / a4  1x1 convolutions (stride 1 / 2; optional bias + activation): MFMA GEMMs on the NCHW tensors
# ----------------------------------------------------------------------------------------------
class _Conv1x1(torch.autograd.Function):
    """with a bias and / or an activation (the pose decoder, PoseCNN); the plain convolution is convnode._ConvF"""
    @staticmethod
    def forward(ctx, x, weight, bias, stride, act):
        L = _lib.lib()
        xx, ww = _c(x.detach()), _c(weight.detach())
        bs = _c(bias.detach()) if bias is not None else None
        B, Ci, Hi, Wi = xx.shape
        Co = ww.shape[0]
        if ww.numel() != Co * Ci or (bs is not None and bs.numel() != Co):
            raise _lib.DepthcoreError("1x1 weight %s / bias do not match %d input channels" % (tuple(ww.shape), Ci))
        y = torch.empty(B, Co, Hi // stride, Wi // stride, dtype=torch.float32, device=xx.device)
        # dc_pointwise_*: the library picks the kernel family per pass (csrc/pointwise.hip: split bf16 / fp32-MFMA / general)
        ws = torch.empty(L.dc_pointwise_workspace(_lib.PASS_FWD, None, B, Ci, Co, Hi, Wi, int(stride)), dtype=torch.uint8, device=xx.device)
        check(L.dc_pointwise_fwd(ptr(xx), ptr(ww), ptr(bs), ptr(y), ws.data_ptr(), B, Ci, Co, Hi, Wi, int(stride), int(act), None, stream(xx)),
              "dc_pointwise_fwd")
        if act == ACT_RELU:
            _record_kink("relu", y)
        ctx.save_for_backward(xx, ww, y)
        ctx.cfg = (int(stride), int(act), bias is not None)
        ctx.slots = (_slot(weight), _slot(bias) if bias is not None else None)
        ctx.param = _lane_param(ctx, 1, weight)
        return y

    @staticmethod
    def backward(ctx, gy):
        L = _lib.lib()
        xx, ww, y = ctx.saved_tensors
        B, Ci, Hi, Wi = xx.shape
        s_, act, has_bias = ctx.cfg
        Co = ww.shape[0]
        g_c = _c(gy)
        gx = gw = gb = None
        # gradient of the pre-activation (+ bias gradient), one pass
        P = (Hi // s_) * (Wi // s_)
        gpre = torch.empty_like(g_c) if act != ACT_NONE else None
        if has_bias and ctx.needs_input_grad[2]:
            gb = _grad_dst(ctx.slots[1], None)
            if gb is None:
                gb = torch.empty(Co, dtype=torch.float32, device=xx.device)
        check(L.dc_bias_act_bwd(ptr(y), ptr(g_c), ptr(gpre), ptr(gb), B, Co, P, act, stream(xx)), "dc_bias_act_bwd")
        if gpre is not None:
            g_c = gpre
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(xx)
            ws = torch.empty(L.dc_pointwise_workspace(_lib.PASS_DGRAD, None, B, Ci, Co, Hi, Wi, s_), dtype=torch.uint8, device=xx.device)
            check(L.dc_pointwise_dgrad(ptr(g_c), ptr(ww), ptr(gx), ws.data_ptr(), None, None, B, Ci, Co, Hi, Wi, s_, None, stream(xx)),
                  "dc_pointwise_dgrad")
        if ctx.needs_input_grad[1]:
            with WgradLanes.lane(ctx.param, xx, g_c):
                gw = _grad_dst(ctx.slots[0], ww)
                ws = torch.empty(L.dc_pointwise_workspace(_lib.PASS_WGRAD, None, B, Ci, Co, Hi, Wi, s_), dtype=torch.uint8, device=xx.device)
                check(L.dc_pointwise_wgrad(ptr(xx), ptr(g_c), ptr(gw), ws.data_ptr(), B, Ci, Co, Hi, Wi, s_, None, stream(xx)),
                      "dc_pointwise_wgrad")
        return gx, gw, gb, None, None


def conv1x1(x, weight, stride=1, bias=None, act=ACT_NONE, fork=None, skip=None):
    """act(F.conv2d(x, weight, bias, stride)) for (Co,Ci,1,1) weights; stride 2 needs even H, W.  `fork`: GradFork; `skip`:
    the SkipSum of x (used when `fork` is a pair fork)."""
    if bias is None and act == ACT_NONE:
        return _ConvF.apply(x, weight, "g1", int(stride), fork, skip, None, None, None, None)
    if fork is not None:
        raise _lib.DepthcoreError("GradFork handed to a 1x1 convolution with a bias or an activation: only the plain "
                                  "convolution's data gradient takes addends")
    return _Conv1x1.apply(x, weight, bias, stride, act)


# ----------------------------------------------------------------------------------------------
# a1 strided trunk convolutions: 7x7 / 2 stem and 3x3 / 2 (no bias), implicit GEMMs on the matrix cores
# ----------------------------------------------------------------------------------------------
def conv_s2_supported(x, weight):
    B, Ci, Hi, Wi = x.shape
    return bool(_lib.lib().dc_convs2_supported(B, Ci, weight.shape[0], Hi, Wi, weight.shape[-1]))


def conv_s2(x, weight, fork=None):
    """F.conv2d(x, weight, None, stride=2, padding=k // 2) for k = 3 or 7.  `fork`: pair GradFork shared with the block's
    1x1 `downsample` (the other consumer of x)."""
    return _ConvF.apply(x, weight, "s2", 2, fork, None, None, None, None, None)


# ----------------------------------------------------------------------------------------------
# a1 every other nn.Conv2d shape of the trunk (odd / tiny maps, a stem whose input needs a gradient): plain direct kernels
# ----------------------------------------------------------------------------------------------
class _ConvDirect(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad):
        L = _lib.lib()
        xx, ww = _c(x.detach()), _c(weight.detach())
        bs = _c(bias.detach()) if bias is not None else None
        B, Ci, Hi, Wi = xx.shape
        Co, k = ww.shape[0], ww.shape[-1]
        if tuple(ww.shape) != (Co, Ci, k, k) or (bs is not None and bs.numel() != Co):
            raise _lib.DepthcoreError("weight %s / bias do not match an input of %d channels" % (tuple(ww.shape), Ci))
        Ho, Wo = (Hi + 2 * pad - k) // stride + 1, (Wi + 2 * pad - k) // stride + 1
        y = torch.empty(B, Co, max(Ho, 0), max(Wo, 0), dtype=torch.float32, device=xx.device)
        check(L.dc_conv2d_direct_fwd(ptr(xx), ptr(ww), ptr(bs), ptr(y), B, Ci, Co, Hi, Wi, k, int(stride), int(pad), stream(xx)),
              "dc_conv2d_direct_fwd")
        ctx.save_for_backward(xx, ww)
        ctx.cfg = (int(stride), int(pad), bias is not None)
        ctx.slots = (_slot(weight), _slot(bias) if bias is not None else None)
        if ctx.needs_input_grad[1]:
            WgradLanes.count_use(weight)     # (see _Conv3x3)
        return y

    @staticmethod
    def backward(ctx, gy):
        L = _lib.lib()
        xx, ww = ctx.saved_tensors
        s_, p_, has_bias = ctx.cfg
        B, Ci, Hi, Wi = xx.shape
        Co, k = ww.shape[0], ww.shape[-1]
        g_c = _c(gy)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(xx)
            check(L.dc_conv2d_direct_dgrad(ptr(g_c), ptr(ww), ptr(gx), B, Ci, Co, Hi, Wi, k, s_, p_, stream(xx)), "dc_conv2d_direct_dgrad")
        if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
            gw = _grad_dst(ctx.slots[0], ww)
            if has_bias and ctx.needs_input_grad[2]:
                gb = _grad_dst(ctx.slots[1], None)
                if gb is None:
                    gb = torch.empty(Co, dtype=torch.float32, device=xx.device)
            check(L.dc_conv2d_direct_wgrad(ptr(xx), ptr(g_c), ptr(gw), ptr(gb), B, Ci, Co, Hi, Wi, k, s_, p_, stream(xx)),
                  "dc_conv2d_direct_wgrad")
        return gx, gw, gb, None, None


def conv2d_direct(x, weight, bias=None, stride=1, padding=0):
    """F.conv2d(x, weight, bias, stride, padding) for square kernels (k <= 11), stride <= 4, padding < k, no groups / dilation:
    the shapes outside the tiled kernels (slow, correct, deterministic)."""
    return _ConvDirect.apply(x, weight, bias, stride, padding)


# ----------------------------------------------------------------------------------------------
# a1 the stem on the raw frames: (image - mean) / std and the pose pairs' concat inside the kernels' patch loader
#                                   (reference networks/resnet_encoder.py:89-90, trainer.py:398-412)
# ----------------------------------------------------------------------------------------------
def stem_supported(frames, weight):
    f0 = frames[0]
    return (f0.is_cuda and f0.dtype == torch.float32 and len(frames) in (1, 2, 3) and f0.shape[1] == 3
            and tuple(weight.shape[1:]) == (3 * (1 if len(frames) == 1 else 2), 7, 7)
            and all(t.shape == f0.shape and not t.requires_grad for t in frames)
            and bool(_lib.lib().dc_stem_supported(len(frames), f0.shape[0], weight.shape[0], f0.shape[2], f0.shape[3])))


class _StemConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, mean, std, *frames):
        L = _lib.lib()
        fr = [_c(t.detach()) for t in frames]
        ww = _c(weight.detach())
        nf = len(fr)
        Bf, _, Hi, Wi = fr[0].shape
        Co = ww.shape[0]
        B, Ci = (2 * Bf if nf == 3 else Bf), (3 if nf == 1 else 6)
        ptrs = (ctypes.c_void_p * nf)(*[ptr(t) for t in fr])
        y = torch.empty(B, Co, Hi // 2, Wi // 2, dtype=torch.float32, device=ww.device)
        _use_precision(_lib.PREC_F32)                      # (the stem has no reduced-precision kernel: 3 / 6 input channels)
        ws = torch.empty(L.dc_convs2_fwd_workspace(B, Ci, Co, Hi, Wi, 7), dtype=torch.uint8, device=ww.device)
        check(L.dc_stem_fwd(ptrs, nf, float(mean), float(std), ptr(ww), ptr(y), ws.data_ptr(), Bf, Hi, Wi, Co, stream(ww)),
              "dc_stem_fwd")
        ctx.save_for_backward(ww, *fr)
        ctx.cfg = (float(mean), float(std))
        ctx.slot = _slot(weight)
        ctx.param = _lane_param(ctx, 0, weight)
        return y

    @staticmethod
    def backward(ctx, gy):
        L = _lib.lib()
        ww, *fr = ctx.saved_tensors
        nf = len(fr)
        Bf, _, Hi, Wi = fr[0].shape
        Co = ww.shape[0]
        B, Ci = (2 * Bf if nf == 3 else Bf), (3 if nf == 1 else 6)
        g_c = _c(gy)
        gw = None
        if ctx.needs_input_grad[0]:
            with WgradLanes.lane(ctx.param, g_c):
                gw = _grad_dst(ctx.slot, ww)
                ptrs = (ctypes.c_void_p * nf)(*[ptr(t) for t in fr])
                ws = torch.empty(L.dc_convs2_wgrad_workspace(B, Ci, Co, Hi, Wi, 7), dtype=torch.uint8, device=ww.device)
                check(L.dc_stem_wgrad(ptrs, nf, ctx.cfg[0], ctx.cfg[1], ptr(g_c), ptr(gw), ws.data_ptr(), Bf, Hi, Wi, Co, stream(ww)),
                      "dc_stem_wgrad")
        return (gw, None, None) + (None,) * nf


def stem_conv(frames, weight, mean=0.45, std=0.225):
    """conv2d((x - mean) / std, weight, stride 2, padding 3) with x = frames[0] (one frame), the pairs cat(f_a, f_b) of two
    frame tensors (which may be overlapping views X[i:i+B], X[i+1:i+B+1] of one sequence: the evaluation layout) or, for three
    frames (f-1, f0, f+1), the two temporal pairs cat(f-1, f0), cat(f0, f+1) stacked along the batch -- neither the normalised
    image nor the pair tensor is materialised.  Frames are inputs (no gradient)."""
    return _StemConv.apply(weight, mean, std, *frames)


# ----------------------------------------------------------------------------------------------
# f1 ResidualAttentionUnit of the Fusion_v3 front-end (reference networks/fusion_v2.py:46-137)
# ----------------------------------------------------------------------------------------------
PLAIN, PIXEL_SHUFFLE2 = "plain", "ps2"


def _attn_map(tensors, kinds, H, W):
    """dc_attn_map over a list of contiguous source tensors: `plain` (B,c,H,W) contributes c channels, `ps2`
    (B,4,H/2,W/2) one channel read through PixelShuffle(2)."""
    m = _lib.AttnMap()
    c = 0
    for t, k in zip(tensors, kinds):
        if k == PLAIN:
            if t.shape[2] != H or t.shape[3] != W:
                raise _lib.DepthcoreError("attention source %s does not match %dx%d" % (tuple(t.shape), H, W))
            for ch in range(t.shape[1]):
                m.ptr[c] = ptr(t) + ch * H * W * 4
                m.batch_stride[c] = t.shape[1] * H * W
                m.mode[c] = _lib.ATTN_PLAIN
                c += 1
        else:
            if tuple(t.shape[1:]) != (4, H // 2, W // 2) or (H & 1) or (W & 1):
                raise _lib.DepthcoreError("pixel-shuffle source %s does not match %dx%d" % (tuple(t.shape), H, W))
            m.ptr[c] = ptr(t)
            m.batch_stride[c] = 4 * (H // 2) * (W // 2)
            m.mode[c] = _lib.ATTN_PIXEL_SHUFFLE2
            c += 1
    return m, c


def _attn_params(ps):
    """ps: (rel_h, rel_w, wk, bk, wq, bq, wv, bv) in the reference's registration order -> dc_attn_params."""
    a = _lib.AttnParams()
    a.rel_h, a.rel_w, a.wk, a.bk, a.wq, a.bq, a.wv, a.bv = (ptr(t) for t in ps)
    return a


def _attn_param_grads(dp, C, like):
    """dparams vector [dWq, dbq, dWk, dbk, dWv, dbv, drel_h, drel_w] -> gradients in the order/shape of `like`
    (rel_h, rel_w, wk, bk, wq, bq, wv, bv)."""
    cc = C * C
    o = [0, cc, cc + C, 2 * cc + C, 2 * cc + 2 * C, 3 * cc + 2 * C, 3 * cc + 3 * C, 3 * cc + 3 * C + 3, 3 * cc + 3 * C + 6]
    dwq, dbq, dwk, dbk, dwv, dbv, drh, drw = (dp[o[i]:o[i + 1]] for i in range(8))
    out = (drh, drw, dwk, dbk, dwq, dbq, dwv, dbv)
    return tuple(g.reshape(t.shape) for g, t in zip(out, like))


class _ResidualAttentionUnit(torch.autograd.Function):
    """atten2(relu(atten1(relu(u)))) + relu(u) with u gathered from `srcs` (no cat / pixel-shuffle tensors): two fused
    launches forward, two backward (the unit's in-place ReLUs make the skip connection add relu(u), fusion_v2.py:130-136)."""

    @staticmethod
    def forward(ctx, kinds, nsrc, *args):
        L = _lib.lib()
        srcs = [_c(t.detach()) for t in args[:nsrc]]
        p1 = [_c(t.detach()) for t in args[nsrc:nsrc + 8]]
        p2 = [_c(t.detach()) for t in args[nsrc + 8:nsrc + 16]]
        B = srcs[0].shape[0]
        H, W = (srcs[0].shape[2], srcs[0].shape[3]) if kinds[0] == PLAIN else (srcs[0].shape[2] * 2, srcs[0].shape[3] * 2)
        xm, C = _attn_map(srcs, kinds, H, W)
        if C not in (2, 4) or p1[2].shape[0] != C:
            raise _lib.DepthcoreError("AttentionConv kernels cover 2 and 4 channels (got %d sources channels, weights %s)"
                                      % (C, tuple(p1[2].shape)))
        dev = srcs[0].device
        y1 = torch.empty(B, C, H, W, dtype=torch.float32, device=dev)
        y = torch.empty_like(y1)
        a1, a2 = _attn_params(p1), _attn_params(p2)
        st = stream(srcs[0])
        check(L.dc_attnconv_fwd(ctypes.byref(xm), ctypes.byref(a1), None, ptr(y1), B, C, H, W, 1, 0, st), "dc_attnconv_fwd")
        y1m, _ = _attn_map([y1], [PLAIN], H, W)
        check(L.dc_attnconv_fwd(ctypes.byref(y1m), ctypes.byref(a2), ctypes.byref(xm), ptr(y), B, C, H, W, 1, 1, st),
              "dc_attnconv_fwd")
        ctx.save_for_backward(y1, *srcs, *p1, *p2)
        ctx.cfg = (tuple(kinds), nsrc, B, C, H, W)
        return y

    @staticmethod
    def backward(ctx, gy):
        L = _lib.lib()
        kinds, nsrc, B, C, H, W = ctx.cfg
        saved = ctx.saved_tensors
        y1, srcs, p1, p2 = saved[0], list(saved[1:1 + nsrc]), list(saved[1 + nsrc:9 + nsrc]), list(saved[9 + nsrc:17 + nsrc])
        dev = y1.device
        g_c = _c(gy)
        npar = L.dc_attnconv_param_count(C)
        dp1 = torch.empty(npar, dtype=torch.float32, device=dev)
        dp2 = torch.empty(npar, dtype=torch.float32, device=dev)
        ws = torch.empty(L.dc_attnconv_bwd_workspace(B, C, H, W), dtype=torch.uint8, device=dev)
        dy1 = torch.empty_like(y1)
        dskip = torch.empty_like(y1)
        xm, _ = _attn_map(srcs, kinds, H, W)
        y1m, _ = _attn_map([y1], [PLAIN], H, W)
        dy1m, _ = _attn_map([dy1], [PLAIN], H, W)
        dskm, _ = _attn_map([dskip], [PLAIN], H, W)
        a1, a2 = _attn_params(p1), _attn_params(p2)
        st = stream(y1)
        # second AttentionConv: input relu(y1), skip relu(u)
        check(L.dc_attnconv_bwd(ctypes.byref(y1m), ctypes.byref(a2), ctypes.byref(xm), ptr(g_c), ctypes.byref(dy1m), None,
                                ctypes.byref(dskm), ptr(dp2), ws.data_ptr(), B, C, H, W, 1, 1, st), "dc_attnconv_bwd")
        # first AttentionConv: input relu(u); its input gradient + the skip gradient go straight to the sources' gradients
        dsrcs = [torch.empty_like(t) for t in srcs]
        dm, _ = _attn_map(dsrcs, kinds, H, W)
        check(L.dc_attnconv_bwd(ctypes.byref(xm), ctypes.byref(a1), None, ptr(dy1), ctypes.byref(dm), ptr(dskip), None,
                                ptr(dp1), ws.data_ptr(), B, C, H, W, 1, 0, st), "dc_attnconv_bwd")
        return (None, None, *dsrcs, *_attn_param_grads(dp1, C, p1), *_attn_param_grads(dp2, C, p2))


def residual_attention_unit(srcs, kinds, params1, params2):
    """srcs / kinds: the unit's input channels as a list of tensors (`PLAIN` (B,c,H,W) or `PIXEL_SHUFFLE2` (B,4,H/2,W/2));
    params1 / params2: (rel_h, rel_w, key w, key b, query w, query b, value w, value b) of atten1 / atten2."""
    return _ResidualAttentionUnit.apply(tuple(kinds), len(srcs), *srcs, *params1, *params2)


# ----------------------------------------------------------------------------------------------
# f3 7x7 local self-attention of the attention encoder    (reference networks/attention.py:29-52, behind the 1x1 convolutions)
# ----------------------------------------------------------------------------------------------
def _plane_strided(t):
    """(tensor, batch stride in elements) for dc_sasa_*: `t` itself when it is a fp32 device tensor whose images are dense
    (C,H,W) blocks -- a channel slice of a wider tensor included -- and a contiguous copy otherwise."""
    if not t.is_cuda:
        raise _lib.DepthcoreError("depthcore ops need device tensors (got %s); there is no CPU path" % t.device)
    if t.dtype != torch.float32:
        raise _lib.DepthcoreError("expected %s, got %s" % (torch.float32, t.dtype))
    B, C, H, W = t.shape
    if t.stride()[1:] != (H * W, W, 1) or (B > 1 and t.stride(0) < C * H * W):
        t = t.contiguous()
    return t, (t.stride(0) if B > 1 else C * H * W)


class _LocalAttention7(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, rel_h, rel_w):
        L = _lib.lib()
        (qq, qs), (kk, ks), (vv, vs) = (_plane_strided(t.detach()) for t in (q, k, v))
        B, C, H, W = qq.shape
        rh, rw = _c(rel_h.detach()), _c(rel_w.detach())
        if kk.shape != qq.shape or vv.shape != qq.shape or C % 2 or rh.numel() != (C // 2) * 7 or rw.numel() != (C // 2) * 7:
            raise _lib.DepthcoreError("local_attention7: q %s, k %s, v %s must agree, C even, rel_h / rel_w (C/2, 7) (got %s, %s)"
                                      % (tuple(qq.shape), tuple(kk.shape), tuple(vv.shape), tuple(rh.shape), tuple(rw.shape)))
        need = any(ctx.needs_input_grad)
        y = torch.empty(B, C, H, W, dtype=torch.float32, device=qq.device)
        lse = torch.empty_like(y) if need else None           # (no_grad: the inference path saves nothing)
        check(L.dc_sasa_fwd(qq.data_ptr(), kk.data_ptr(), vv.data_ptr(), qs, ks, vs, ptr(rh), ptr(rw), ptr(y), ptr(lse), B, C, H, W,
                            stream(qq)), "dc_sasa_fwd")
        if need:
            ctx.save_for_backward(qq, kk, vv, rh, rw, y, lse)
            ctx.strides = (qs, ks, vs)
            ctx.slots = (_slot(rel_h), _slot(rel_w))
        return y

    @staticmethod
    def backward(ctx, gy):
        L = _lib.lib()
        qq, kk, vv, rh, rw, y, lse = ctx.saved_tensors
        qs, ks, vs = ctx.strides
        B, C, H, W = y.shape
        g_c = _c(gy)
        dq, dk, dv = torch.empty_like(y), torch.empty_like(y), torch.empty_like(y)
        drh, drw = _grad_dst(ctx.slots[0], rh), _grad_dst(ctx.slots[1], rw)      # (C/2 * 7 contiguous values in the parameters' shapes)
        ws = torch.empty(L.dc_sasa_bwd_workspace(B, C, H, W), dtype=torch.uint8, device=y.device)
        check(L.dc_sasa_bwd(qq.data_ptr(), kk.data_ptr(), vv.data_ptr(), qs, ks, vs, ptr(rh), ptr(rw), ptr(y), ptr(lse), ptr(g_c),
                            ptr(dq), ptr(dk), ptr(dv), ptr(drh), ptr(drw), ws.data_ptr(), B, C, H, W, stream(y)), "dc_sasa_bwd")
        return dq, dk, dv, drh, drw


def local_attention7(q, k, v, rel_h, rel_w):
    """y[c] = sum_t softmax_t(q[c] (k_t[c] + rel_t[c])) v_t[c] over the 7x7 window (zero padding 3, stride 1) of (B,C,H,W) fp32
    maps; rel_t = rel_h[c, dy] for c < C/2 and rel_w[c - C/2, dx] otherwise (rel_h, rel_w: C/2 * 7 values in any shape).  One fused
    kernel forward (it saves y and the log-sum-exp; under no_grad nothing), one plus a small reduction backward.  q, k, v may be
    channel slices of one wider tensor: they are read in place."""
    return _LocalAttention7.apply(q, k, v, rel_h, rel_w)


# ----------------------------------------------------------------------------------------------
# f2 ConvGRU cell gate arithmetic + sequence residual        (reference networks/rnn.py:101-143, trainer_gru.py:637-639)
# ----------------------------------------------------------------------------------------------
class _GruRH(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gates, h):
        L = _lib.lib()
        gt, hh = _c(gates.detach()), _c(h.detach())
        B, C = hh.shape[0], hh.shape[1]
        P = hh.shape[2] * hh.shape[3]
        if tuple(gt.shape) != (B, 2 * C) + tuple(hh.shape[2:]):
            raise _lib.DepthcoreError("gates %s do not match state %s" % (tuple(gt.shape), tuple(hh.shape)))
        rh = torch.empty_like(hh)
        check(L.dc_gru_rh_fwd(ptr(gt), ptr(hh), ptr(rh), B, C, P, stream(hh)), "dc_gru_rh_fwd")
        ctx.save_for_backward(gt, hh)
        return rh

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        gt, hh = ctx.saved_tensors
        B, C = hh.shape[0], hh.shape[1]
        P = hh.shape[2] * hh.shape[3]
        g_c = _c(g)
        dg, dh = torch.empty_like(gt), torch.empty_like(hh)
        check(L.dc_gru_rh_bwd(ptr(gt), ptr(hh), ptr(g_c), ptr(dg), ptr(dh), B, C, P, stream(hh)), "dc_gru_rh_bwd")
        return dg, dh


class _GruBlend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gates, h, cnm):
        L = _lib.lib()
        gt, hh, cc = _c(gates.detach()), _c(h.detach()), _c(cnm.detach())
        B, C = hh.shape[0], hh.shape[1]
        P = hh.shape[2] * hh.shape[3]
        if tuple(gt.shape) != (B, 2 * C) + tuple(hh.shape[2:]) or cc.shape != hh.shape:
            raise _lib.DepthcoreError("gates %s / candidate %s do not match state %s" % (tuple(gt.shape), tuple(cc.shape), tuple(hh.shape)))
        out = torch.empty_like(hh)
        check(L.dc_gru_blend_fwd(ptr(gt), ptr(hh), ptr(cc), ptr(out), B, C, P, stream(hh)), "dc_gru_blend_fwd")
        ctx.save_for_backward(gt, hh, cc)
        return out

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        gt, hh, cc = ctx.saved_tensors
        B, C = hh.shape[0], hh.shape[1]
        P = hh.shape[2] * hh.shape[3]
        g_c = _c(g)
        dg, dh, dc = torch.empty_like(gt), torch.empty_like(hh), torch.empty_like(cc)
        check(L.dc_gru_blend_bwd(ptr(gt), ptr(hh), ptr(cc), ptr(g_c), ptr(dg), ptr(dh), ptr(dc), B, C, P, stream(hh)), "dc_gru_blend_bwd")
        return dg, dh, dc


class _GruResidual(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, H):
        L = _lib.lib()
        ff, HH = _c(f.detach()), _c(H.detach())
        n = ff.shape[0]
        M = ff[0].numel()
        if tuple(HH.shape) != (n + 1,) + tuple(ff.shape[1:]):
            raise _lib.DepthcoreError("hidden states %s must be (n+1, ...) for features %s" % (tuple(HH.shape), tuple(ff.shape)))
        out = torch.empty_like(ff)
        check(L.dc_gru_residual_fwd(ptr(ff), ptr(HH), ptr(out), n, M, stream(ff)), "dc_gru_residual_fwd")
        ctx.dims = (n, M, HH.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        n, M, hshape = ctx.dims
        g_c = _c(g)
        dH = torch.empty(hshape, dtype=torch.float32, device=g.device)
        check(L.dc_gru_residual_bwd(ptr(g_c), ptr(dH), n, M, stream(g_c)), "dc_gru_residual_bwd")
        return g_c, dH


def stack_frames(groups):
    """[[t_0, t_1, ...], ...] -> [torch.cat(group, 0) for group in groups] in ONE launch (dc_gather_copy): the sequence trainer's
    stacking of the frames of a sequence along the batch (trainer_gru.py:819-821, 886-896, 943-944).  float32 device tensors
    without a gradient (inputs of the step); a group's members share their trailing shape."""
    L = _lib.lib()
    outs, src, dst, n, keep = [], [], [], [], []
    for g in groups:
        ts = [_c(t.detach()) for t in g]
        if any(t.dtype != torch.float32 or not t.is_cuda or t.shape[1:] != ts[0].shape[1:] for t in ts):
            raise _lib.DepthcoreError("stack_frames takes float32 device tensors that agree in their trailing shape")
        out = torch.empty((sum(t.shape[0] for t in ts),) + tuple(ts[0].shape[1:]), dtype=torch.float32, device=ts[0].device)
        off = 0
        for t in ts:
            src.append(t.data_ptr()); dst.append(out.data_ptr() + 4 * off); n.append(t.numel())
            off += t.numel()
        keep.append(ts)
        outs.append(out)
    for i in range(0, len(src), 96):
        k = len(src[i:i + 96])
        check(L.dc_gather_copy((ctypes.c_void_p * k)(*src[i:i + 96]), (ctypes.c_void_p * k)(*dst[i:i + 96]),
                               (ctypes.c_size_t * k)(*n[i:i + 96]), k, stream(outs[0])), "dc_gather_copy")
    return outs


def gru_reset_times_state(gates, h):
    """r * h with r = gates[:, :C]."""
    return _GruRH.apply(gates, h)


def gru_blend(gates, h, cnm):
    """(1 - u) * h + u * cnm with u = gates[:, C:]."""
    return _GruBlend.apply(gates, h, cnm)


def gru_sequence_residual(features, hidden_states):
    """features (n,C,H,W) + (H[1:] + H[:-1]) / 2 with H (n+1,C,H,W)."""
    return _GruResidual.apply(features, hidden_states)


class _plan_streams:
    """`with _plan_streams(S)`: the calling thread's Winograd launches plan their reduction as ONE of S stacked streams would
    (dc_set_wino_plan_streams), so that a sequence's results in a lockstep step are those of its single-sequence call.  S == 1
    touches nothing."""

    def __init__(self, streams):
        self.streams, self.before = int(streams), None

    def __enter__(self):
        if self.streams > 1:
            self.before = _lib.lib().dc_set_wino_plan_streams(self.streams)
            if self.before < 1:
                raise _lib.DepthcoreError("dc_set_wino_plan_streams(%d) failed" % self.streams)
        return self

    def __exit__(self, *exc):
        if self.before is not None:
            _lib.lib().dc_set_wino_plan_streams(self.before)
        return False


class _GruLevel(torch.autograd.Function):
    """One feature level of `run_gru_v5` for a sequence of n frames (batch_size 1, trainer_gru.py:607-639) as ONE autograd node:
    the cell runs over the frames from the learned initial state, every tensor of every step lives in one buffer per kind
    (gates / r*h / candidate / the n+1 hidden states -- a step reads and writes its slot by pointer, so there is neither a
    per-frame slice node nor a torch.cat of the trace), and the backward walks the frames in reverse itself: each step's
    gradient of h_i is ACCUMULATED into the slot that already holds the residual's and the later step's share
    (dc_gru_blend_bwd_acc, dc_gru_rh_bwd_acc, the gate convolution's data-gradient store with the slot as its own addend), the
    feature gradient leaves the gate convolution's store with the candidate convolution's and the residual's share added on the
    way, and the shared parameters get their gradients from ONE weight-gradient pass per convolution over the n frames as a
    batch once the walk is done (per-frame passes + a sum over frames otherwise).  Against the per-op
    graph (ConvGRUCell.forward, kept for single calls) that is ~9 elementwise sums, 3 fills / copies and 1.7 concatenations
    fewer per cell step: 137 + 47 + 25 launches of a C4 step.
    S > 1 (beyond the reference): the rows hold S sequences time-major (`seq_rows`: frame j of stream s is row j * S + s), every
    launch of a time step takes the S streams as its batch, the weight-gradient pass takes the n * S rows, and the gradient of
    the initial state the streams share is the sum of their rows (dc_gru_state_bwd).  S == 1 issues exactly the calls above."""

    @staticmethod
    def forward(ctx, feats, h0, wg, bg, wc, bc, S=1):
        L = _lib.lib()
        ff = _c(feats.detach())
        rows, C, H, W = ff.shape
        P = H * W
        S = int(S)
        if S < 1 or rows % S or rows < S:
            raise _lib.DepthcoreError("ConvGRU level: %d rows are not the frames of %d lockstep streams" % (rows, S))
        n = rows // S
        if tuple(h0.shape) != (1, C, H, W) or tuple(wg.shape) != (2 * C, 2 * C, 3, 3) or tuple(wc.shape) != (C, 2 * C, 3, 3):
            raise _lib.DepthcoreError("ConvGRU level: state %s / gate weights %s / candidate weights %s do not match features %s" % (
                tuple(h0.shape), tuple(wg.shape), tuple(wc.shape), tuple(ff.shape)))
        w_g, b_g, w_c, b_c = _c(wg.detach()), _c(bg.detach()), _c(wc.detach()), _c(bc.detach())
        dev = ff.device
        Hs = torch.empty((n + 1) * S, C, H, W, dtype=torch.float32, device=dev)
        if S == 1:
            Hs[0].copy_(h0.detach()[0])
        else:
            gru_infer_init([_c(h0.detach())], [Hs[:S]])                                              # the shared h0, one row per stream
        gates = torch.empty(rows, 2 * C, H, W, dtype=torch.float32, device=dev)
        rh = torch.empty(rows, C, H, W, dtype=torch.float32, device=dev)
        cnm = torch.empty(rows, C, H, W, dtype=torch.float32, device=dev)
        ctx.prec = _use_precision(_precision[0])
        with _plan_streams(S):      # a stream's sums are ordered as in its single-sequence call, whatever S is
            ws = torch.empty(max(L.dc_conv3x3_fwd_workspace(C, C, S, 2 * C, H, W), L.dc_conv3x3_fwd_workspace(C, C, S, C, H, W)),
                             dtype=torch.uint8, device=dev)
            st = stream(ff)
            for i in range(n):
                t = seq_rows(i, S)                                # time step i of the S streams: one contiguous slab
                x, h = ff[t], Hs[t]
                # [reset | update] = sigmoid(conv_gates(cat(x, h)))                                       rnn.py:125-130
                check(L.dc_conv3x3_fwd(ptr(x), C, 0, ptr(h), C, ptr(w_g), ptr(b_g), ptr(gates[t]), ws.data_ptr(), S, 2 * C, H, W,
                                       ACT_SIGMOID, PAD_ZERO, st), "dc_conv3x3_fwd")
                check(L.dc_gru_rh_fwd(ptr(gates[t]), ptr(h), ptr(rh[t]), S, C, P, st), "dc_gru_rh_fwd")
                # cnm = tanh(conv_can(cat(x, reset * h)))                                                   rnn.py:132-134
                check(L.dc_conv3x3_fwd(ptr(x), C, 0, ptr(rh[t]), C, ptr(w_c), ptr(b_c), ptr(cnm[t]), ws.data_ptr(), S, C, H, W,
                                       ACT_TANH, PAD_ZERO, st), "dc_conv3x3_fwd")
                check(L.dc_gru_blend_fwd(ptr(gates[t]), ptr(h), ptr(cnm[t]), ptr(Hs[seq_rows(i + 1, S)]), S, C, P, st),
                      "dc_gru_blend_fwd")                                                                # rnn.py:136
        out = torch.empty_like(ff)
        check(L.dc_gru_residual_fwd(ptr(ff), ptr(Hs), ptr(out), n, S * C * P, st), "dc_gru_residual_fwd")   # trainer_gru.py:637-639
        ctx.save_for_backward(ff, Hs, gates, rh, cnm, w_g, w_c)
        ctx.streams = S
        ctx.slots = tuple(_slot(t) for t in (wg, bg, wc, bc))
        for t, k in ((wg, 2), (wc, 4)):
            if ctx.needs_input_grad[k]:
                WgradLanes.count_use(t)
        return out

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        ff, Hs, gates, rh, cnm, w_g, w_c = ctx.saved_tensors
        rows, C, H, W = ff.shape
        S = ctx.streams
        n = rows // S
        P = H * W
        dev = ff.device
        need = ctx.needs_input_grad
        g_c = _c(g)
        st = stream(ff)
        f32 = dict(dtype=torch.float32, device=dev)
        dHs = torch.empty_like(Hs)
        check(L.dc_gru_residual_bwd(ptr(g_c), ptr(dHs), n, S * C * P, st), "dc_gru_residual_bwd")
        dfe = torch.empty_like(ff)
        dgates, dcn = torch.empty(rows, 2 * C, H, W, **f32), torch.empty(rows, C, H, W, **f32)     # g of the two convolutions' outputs, per frame
        dxc, drh = torch.empty(S, C, H, W, **f32), torch.empty(S, C, H, W, **f32)
        _use_precision(ctx.prec)
        with _plan_streams(S):      # the workspace is sized and the walk's data gradients are planned as one stream's
            ws = torch.empty(max(L.dc_conv3x3_bwd_workspace(C, C, b, co, H, W) for b in (S, rows) for co in (C, 2 * C)),
                             dtype=torch.uint8, device=dev)
            for i in range(n - 1, -1, -1):
                t = seq_rows(i, S)
                x, h, gt, dh = ff[t], Hs[t], gates[t], dHs[t]
                dg, dc = dgates[t], dcn[t]
                # h_{i+1} = (1-u) h_i + u cnm: dHs[i+1] is complete here (residual + step i+1)
                check(L.dc_gru_blend_bwd_acc(ptr(gt), ptr(h), ptr(cnm[t]), ptr(dHs[seq_rows(i + 1, S)]), ptr(dg), ptr(dh), ptr(dc),
                                             S, C, P, st), "dc_gru_blend_bwd_acc")
                # candidate convolution over cat(x, r*h), data gradients only: that of x takes the residual's share (g[i]) along
                check(L.dc_conv3x3_bwd_add(ptr(x), C, 0, ptr(rh[t]), C, ptr(w_c), ptr(cnm[t]), ptr(dc), ptr(dxc), ptr(drh),
                                           ptr(g_c[t]), None, None, None, ws.data_ptr(), S, C, H, W, ACT_TANH, PAD_ZERO, st),
                      "dc_conv3x3_bwd_add")
                check(L.dc_gru_rh_bwd_acc(ptr(gt), ptr(h), ptr(drh), ptr(dg), ptr(dh), S, C, P, st), "dc_gru_rh_bwd_acc")
                # gate convolution over cat(x, h): d x = own + (candidate's + residual's), d h_i = own + what the slot holds
                check(L.dc_conv3x3_bwd_add(ptr(x), C, 0, ptr(h), C, ptr(w_g), ptr(gt), ptr(dg), ptr(dfe[t]), ptr(dh),
                                           ptr(dxc), ptr(dh), None, None, ws.data_ptr(), S, 2 * C, H, W, ACT_SIGMOID, PAD_ZERO, st),
                      "dc_conv3x3_bwd_add")
        # the parameters are shared by the n steps and nothing downstream waits for their gradients: ONE weight-gradient pass
        # per convolution with the n * S frames as its batch (sum over frames and streams = sum over the batch), after the walk.
        # Hs / rh hold the state each frame READ in their first n * S rows (time-major: row j * S + s), as the frames do.
        outs = [None] * 4
        for k, (like, x1, y, gy, co, act) in enumerate(((w_g, Hs, gates, dgates, 2 * C, ACT_SIGMOID), (w_c, rh, cnm, dcn, C, ACT_TANH))):
            if not (need[2 + 2 * k] or need[3 + 2 * k]):
                continue
            dw = _grad_dst(ctx.slots[2 * k], like) if need[2 + 2 * k] else None
            db = None
            if need[3 + 2 * k]:
                db = _grad_dst(ctx.slots[2 * k + 1], None)
                if db is None:
                    db = torch.empty(co, **f32)
            check(L.dc_conv3x3_bwd_add(ptr(ff), C, 0, ptr(x1), C, ptr(like), ptr(y), ptr(gy), None, None, None, None, ptr(dw), ptr(db),
                                       ws.data_ptr(), rows, co, H, W, act, PAD_ZERO, st), "dc_conv3x3_bwd_add")
            outs[2 * k], outs[2 * k + 1] = dw, db
        dh0 = None
        if need[1]:
            if S == 1:
                dh0 = dHs[0:1]
            else:                                             # the streams share h0: its gradient is the sum of their rows
                dh0 = torch.empty(1, C, H, W, **f32)
                check(L.dc_gru_state_bwd(ptr(dHs), ptr(dh0), S, C * P, st), "dc_gru_state_bwd")
        return (dfe if need[0] else None, dh0) + tuple(outs) + (None,)


def gru_level_sequence(features, h0, conv_gates, conv_can, streams=1):
    """features (n,C,H,W) of one sequence, h0 (1,C,H,W) -> features + (H[1:] + H[:-1]) / 2, H the hidden states of the cell
    (conv_gates / conv_can: its two nn.Conv2d) run over the frames in order (trainer_gru.py:607-639 at one level).
    streams = S > 1: features (n * S, C, H, W) hold S sequences time-major (`seq_rows`); they advance in lockstep from the
    shared h0 -- the same four launches per time step with S as their batch -- and the parameters' and h0's gradients are the
    sums over the streams."""
    return _GruLevel.apply(features, h0, conv_gates.weight, conv_gates.bias, conv_can.weight, conv_can.bias, int(streams))


# ---- inference form of the cell step: B independent streams, every level in one launch (dc_gru_infer_*) ---------------------
def _infer_rows(name, B, *groups):
    """The tensors of an inference step, one list per kind and one entry per level: contiguous float32 device tensors whose
    leading dimension holds the streams.  No autograd here: a tensor that requires grad is detached.  -> (lists, B)."""
    nlev = len(groups[0])
    if not 1 <= nlev <= 8 or any(len(g) != nlev for g in groups):
        raise DepthcoreError("%s: 1..8 levels, one tensor per level and kind" % name)
    groups = [[t.detach() for t in g] for g in groups]
    rows = min(t.shape[0] for g in groups for t in g)
    B = rows if B is None else int(B)
    if not 1 <= B <= rows:
        raise DepthcoreError("%s: B = %d streams of buffers that hold %d" % (name, B, rows))
    return groups, B


def _infer_levels(gates, h, cnm=None, f=None, rh=None, out=None):
    """The dc_gru_infer_level array of a step's tensors (shapes checked: gates (S,2C,H,W), the others (S,C,H,W))."""
    lv = (_lib.GruInferLevel * len(h))()
    for k, hh in enumerate(h):
        if hh.dim() != 4 or tuple(gates[k].shape[1:]) != (2 * hh.shape[1],) + tuple(hh.shape[2:]):
            raise DepthcoreError("level %d: gates %s do not match state %s" % (k, tuple(gates[k].shape), tuple(hh.shape)))
        C, P = hh.shape[1], hh.shape[2] * hh.shape[3]
        lv[k].gates, lv[k].h, lv[k].C, lv[k].P = ptr(gates[k]), ptr(hh), C, P
        for field, ts in (("cnm", cnm), ("f", f), ("rh", rh), ("out", out)):
            if ts is not None:
                if ts[k].shape[1:] != hh.shape[1:]:
                    raise DepthcoreError("level %d: %s %s does not match state %s" % (k, field, tuple(ts[k].shape), tuple(hh.shape)))
                setattr(lv[k], field, ptr(ts[k]))
    return lv


def gru_infer_rh(gates, h, rh, B=None):
    """rh[k][:B] = gates[k][:B, :C] * h[k][:B] for every level k, one launch (dc_gru_infer_rh).  Lists with one tensor per
    level; B: the streams stepped, a prefix of the buffers' rows (default: all).  Writes into `rh`; no autograd."""
    (gates, h, rh), B = _infer_rows("gru_infer_rh", B, gates, h, rh)
    check(_lib.lib().dc_gru_infer_rh(_infer_levels(gates, h, rh=rh), len(h), B, stream(h[0])), "dc_gru_infer_rh")
    return rh


def gru_infer_tail(gates, cnm, f, h, out, B=None):
    """The rest of a cell step after the candidate convolution, every level in one launch (dc_gru_infer_tail): with
    u = gates[k][:B, C:], h_next = (1 - u) * h + u * cnm, out[k][:B] = f[k] + (h_next + h) / 2, and h[k][:B] IS OVERWRITTEN by
    h_next.  `f[k]` may hold just the B rows; no autograd."""
    (gates, cnm, f, h, out), B = _infer_rows("gru_infer_tail", B, gates, cnm, f, h, out)
    check(_lib.lib().dc_gru_infer_tail(_infer_levels(gates, h, cnm=cnm, f=f, out=out), len(h), B, stream(h[0])), "dc_gru_infer_tail")
    return out


def gru_infer_init(h0, state, B=None):
    """state[k][b] = h0[k][0] for b < B, every level in one launch (dc_gru_infer_init): the learned initial states (1,C,H,W)
    broadcast over the streams of the state buffers (S,C,H,W).  `h0` is only read."""
    (h0, state), _ = _infer_rows("gru_infer_init", 1, h0, state)
    rows = min(s.shape[0] for s in state)
    B = rows if B is None else int(B)
    if not 1 <= B <= rows or any(a.shape[0] != 1 or a.shape[1:] != s.shape[1:] for a, s in zip(h0, state)):
        raise DepthcoreError("gru_infer_init: h0 (1,C,H,W) into B <= S rows of state (S,C,H,W)")
    n = len(state)
    check(_lib.lib().dc_gru_infer_init((ctypes.c_void_p * n)(*[ptr(a) for a in h0]), (ctypes.c_void_p * n)(*[ptr(s) for s in state]),
                                       (ctypes.c_size_t * n)(*[a.numel() for a in h0]), n, B, stream(state[0])), "dc_gru_infer_init")
    return state


def copy_segments(srcs, dsts):
    """dsts[i].copy_(srcs[i]) for contiguous float32 device tensors of pairwise equal size, 96 pairs per launch
    (dc_gather_copy): the rows of a lockstep step go to their scenes' outputs this way."""
    L = _lib.lib()
    if len(srcs) != len(dsts) or any(s.numel() != d.numel() or s.numel() == 0 for s, d in zip(srcs, dsts)):
        raise DepthcoreError("copy_segments: pairs of tensors of equal, non-zero size")
    for i in range(0, len(srcs), 96):
        s, d = srcs[i:i + 96], dsts[i:i + 96]
        k = len(s)
        check(L.dc_gather_copy((ctypes.c_void_p * k)(*[ptr(t.detach()) for t in s]), (ctypes.c_void_p * k)(*[ptr(t) for t in d]),
                               (ctypes.c_size_t * k)(*[t.numel() for t in s]), k, stream(d[0])), "dc_gather_copy")


# ----------------------------------------------------------------------------------------------
# f3 ConvLSTM v8: state update and coarse-to-fine hand-over   (reference networks/rnn.py:70-79, 767-773, 783-791)
# ----------------------------------------------------------------------------------------------
def _rows(t, B, what):
    """A learned initial state (1, C, H, W) shared by B > 1 items, expanded: its gradient's sum over B is autograd's (a plain,
    ordered torch reduction)."""
    if t.shape[0] == 1 and B > 1:
        return t.expand((B,) + tuple(t.shape[1:]))
    if t.shape[0] != B:
        raise DepthcoreError("%s has %d rows for a batch of %d" % (what, t.shape[0], B))
    return t


class _LstmCell(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cc, c_cur):
        L = _lib.lib()
        g, c = _c(cc.detach()), _c(c_cur.detach())
        if c.dim() != 4 or tuple(g.shape) != (c.shape[0], 4 * c.shape[1]) + tuple(c.shape[2:]):
            raise DepthcoreError("gate pre-activations %s do not match the cell state %s" % (tuple(g.shape), tuple(c.shape)))
        B, C, P = c.shape[0], c.shape[1], c.shape[2] * c.shape[3]
        h_next, c_next = torch.empty_like(c), torch.empty_like(c)
        check(L.dc_lstm_cell_fwd(ptr(g), ptr(c), ptr(h_next), ptr(c_next), B, C, P, stream(c)), "dc_lstm_cell_fwd")
        ctx.save_for_backward(g, c)
        ctx.set_materialize_grads(False)        # a state nobody reads (the last frame's c) arrives as None -> NULL
        return h_next, c_next

    @staticmethod
    def backward(ctx, g_h, g_c):
        if g_h is None and g_c is None:
            return None, None
        L = _lib.lib()
        g, c = ctx.saved_tensors
        B, C, P = c.shape[0], c.shape[1], c.shape[2] * c.shape[3]
        gh = _c(g_h) if g_h is not None else None
        gc = _c(g_c) if g_c is not None else None
        d_cc, d_c = torch.empty_like(g), torch.empty_like(c)
        check(L.dc_lstm_cell_bwd(ptr(g), ptr(c), ptr(gh), ptr(gc), ptr(d_cc), ptr(d_c), B, C, P, stream(c)), "dc_lstm_cell_bwd")
        return d_cc, d_c


def lstm_cell(cc, c_cur):
    """(h_next, c_next) of a ConvLSTM step from the raw output cc (B, 4C, H, W) = [i | f | o | g] of the cell's convolution and
    the cell state c_cur (B, C, H, W), or (1, C, H, W): a learned initial state shared over the batch."""
    return _LstmCell.apply(cc, _rows(c_cur, cc.shape[0], "c_cur"))


class _LstmHandover(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, h_prev, h_new, need_up):
        L = _lib.lib()
        aa, hp, hn = _c(a.detach()), _c(h_prev.detach()), _c(h_new.detach())
        if aa.dim() != 4 or hp.shape != aa.shape or hn.shape != aa.shape or aa.shape[1] % 4:
            raise DepthcoreError("hand-over takes three (B, C, h, w) tensors with C a multiple of 4, got %s %s %s"
                                 % (tuple(aa.shape), tuple(hp.shape), tuple(hn.shape)))
        B, C, h, w = aa.shape
        pre = torch.empty_like(aa)
        up = torch.empty(B, C // 4, 2 * h, 2 * w, dtype=torch.float32, device=aa.device) if need_up else None
        check(L.dc_lstm_handover_fwd(ptr(aa), ptr(hp), ptr(hn), ptr(pre), ptr(up), B, C, h, w, stream(aa)), "dc_lstm_handover_fwd")
        ctx.save_for_backward(pre)
        ctx.set_materialize_grads(False)
        return pre, up

    @staticmethod
    def backward(ctx, g_pre, g_up):
        need = ctx.needs_input_grad
        if (g_pre is None and g_up is None) or not any(need[:3]):
            return None, None, None, None
        L = _lib.lib()
        pre, = ctx.saved_tensors
        B, C, h, w = pre.shape
        gp = _c(g_pre) if g_pre is not None else None
        gu = _c(g_up) if g_up is not None else None
        d = [torch.empty_like(pre) if need[k] else None for k in range(3)]
        check(L.dc_lstm_handover_bwd(ptr(pre), ptr(gp), ptr(gu), ptr(d[0]), ptr(d[1]), ptr(d[2]), B, C, h, w, stream(pre)),
              "dc_lstm_handover_bwd")
        return d[0], d[1], d[2], None


def lstm_handover(a, h_prev, h_new, need_up=True):
    """pre = relu(a + (h_prev + h_new) / 2) and up = pixel_shuffle(tanh(pre), 2) (None without need_up) in one launch:
    FeatureFusionBlock_v2's join of the residual unit's output with the mean hidden state, and its UpscalePS.  h_prev may be
    (1, C, h, w): the learned initial hidden state shared over the batch."""
    return _LstmHandover.apply(a, _rows(h_prev, a.shape[0], "h_prev"), h_new, bool(need_up))
