"""The fused photometric loss: one forward and one backward launch chain for warping, SSIM / L1, the minimum over the
source frames, automasking and the smoothness term of every scale, and the hipEvent profiler of its dominant kernels.

Imports `_lib` and `_autograd` only; `ops` re-exports every name.
"""
import ctypes

import torch

from . import _lib
from ._autograd import _c
from ._lib import PhotoDesc, check, ptr, stream


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
