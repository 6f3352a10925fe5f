"""Convolutions and their neighbours: the fused 3x3 block, training- and eval-mode BatchNorm, the stem max-pool, the Winograd
trunk convolution with its weight cache, 1x1, strided, direct and stem convolutions, and the convolution profiler.

The plain trunk convolutions are thin wrappers of `convnode._ConvF`.  Imports `_lib`, `_autograd` and `convnode`; `ops`
re-exports every name.
"""
import ctypes
import weakref

import torch

from . import _lib
from ._autograd import (WgradLanes, _bias_grad_dst, _c, _grad_dst, _lane_param, _precision, _record_kink, _slot, _use_precision,
                        skip_of)
from ._lib import DepthcoreError, check, ptr, stream
from .convnode import _ConvF


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
        db = _bias_grad_dst(ctx.slots[1], Co, y.device) if has_bias and need[3] else None
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
            gb = _bias_grad_dst(ctx.slots[1], Co, xx.device)
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
                gb = _bias_grad_dst(ctx.slots[1], Co, xx.device)
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


# ---- measurement hook (bench.py): hipEvent timing of the Winograd convolution launches -----------------------------------
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
