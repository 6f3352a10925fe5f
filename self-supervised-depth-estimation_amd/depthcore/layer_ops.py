"""The unfused `layers.*` ops, one autograd node each: pose matrix and head, disp_to_depth, pixel coordinates, backprojection,
projection, border grid sampling, the bilinear and nearest x2 upsamples, SSIM and the smoothness loss.

Imports `_lib` and `_autograd` only; `ops` re-exports every name.
"""
import ctypes

import torch

from . import _lib
from ._autograd import _c
from ._lib import check, ptr, stream


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
