"""The one autograd node of the trunk's tiled convolutions (`_ConvF`) and its kernel tables: "wino" stride-1 3x3
(dc_wino3x3_*), "g1" 1x1 (dc_pointwise_*), "s2" 3x3 / 2 and 7x7 / 2 (dc_convs2_*).

One backward protocol for a convolution whose input has other consumers -- GradFork arrive / take / park, SkipSum arm / take,
the addend checks, the weight gradient on a WgradLanes lane -- with or without a BatchNorm folded in (dc_bn_fold, see
bnfold.py).  `convs` holds the plain wrappers (wino_conv3x3, conv1x1, conv_s2; `ops` re-exports them), `bnfold` the folded ones.
"""
import ctypes

import torch

from . import _lib
from ._autograd import (WgradLanes, _c, _fork_addend, _grad_dst, _lane_param, _precision, _record_kink, _slot,
                        _use_precision)
from ._lib import BnFold, check, ptr, stream


class BNStats:
    """Partial {sum, sum of squares} of a raw convolution output, per channel (dc_bn_fold.stat_part)."""
    __slots__ = ("part", "nparts", "ppg", "groups")

    def __init__(self, part, nparts, ppg, groups):
        self.part, self.nparts, self.ppg, self.groups = part, nparts, ppg, groups


class BNLink:
    """Left on a block output y = relu(bn(x) + skip) by `bn_apply`: what the output's ONLY consumer (the next block: conv1 +
    skip, joined by a GradFork) needs to do the first pass of this BatchNorm's backward in its data-gradient epilogue."""
    __slots__ = ("x", "mean", "mask", "groups", "bwd", "armed")

    def __init__(self, x, mean, mask, groups):
        self.x, self.mean, self.mask, self.groups = x, mean, mask, groups
        self.bwd = None          # (part, nparts, ppg): set by the consumer's backward -- the gradient it returned is g', masked
        self.armed = False       # a consumer has taken the link in its forward


def _ival():
    return ctypes.c_int(0)


def _finalize(L, xx, stats, gamma, beta, rm, rv, eps, momentum, groups):
    """BNStats (or a stand-alone statistics pass when the producer had no epilogue) -> tab (4, groups*C): mean, invstd, scale, shift."""
    N, C, H, W = xx.shape
    if stats is None:
        ppg = _ival()
        nparts = L.dc_bn_stat_parts(N, C, H * W, groups, ctypes.byref(ppg))
        if not nparts:
            raise _lib.DepthcoreError("BatchNorm fold: no statistics layout for %s with %d groups" % (tuple(xx.shape), groups))
        part = torch.empty(C * nparts * 2, dtype=torch.float32, device=xx.device)
        check(L.dc_bn_stats(ptr(xx), ptr(part), N, C, H * W, groups, stream(xx)), "dc_bn_stats")
        stats = BNStats(part, nparts, ppg.value, groups)
    if stats.groups != groups:
        raise _lib.DepthcoreError("BatchNorm fold: statistics were taken for %d groups, the layer has %d" % (stats.groups, groups))
    tab = torch.empty(4, groups * C, dtype=torch.float32, device=xx.device)
    check(L.dc_bn_finalize(ptr(stats.part), stats.nparts, stats.ppg, float(N // groups) * H * W, ptr(gamma), ptr(beta), ptr(rm), ptr(rv),
                           tab[0].data_ptr(), tab[1].data_ptr(), tab[2].data_ptr(), tab[3].data_ptr(), C, groups, float(eps),
                           float(momentum), stream(xx)), "dc_bn_finalize")
    return tab


def _bwd_finish(L, xx, gp, bwd, gamma, tab, groups, slots):
    """backward partials -> coefficients, dgamma, dbeta; dx = a g' + b (x - mean) + c0 in one pass."""
    N, C, H, W = xx.shape
    part, nparts, ppg = bwd
    coef = torch.empty(groups * C * 4, dtype=torch.float32, device=xx.device)
    dgamma = _grad_dst(slots[0], gamma)
    dbeta = _grad_dst(slots[1], gamma)
    check(L.dc_bn_bwd_finalize(ptr(part), nparts, ppg, float(N // groups) * H * W, ptr(gamma), tab[0].data_ptr(), tab[1].data_ptr(),
                               ptr(coef), ptr(dgamma), ptr(dbeta), C, groups, stream(xx)), "dc_bn_bwd_finalize")
    dx = torch.empty_like(xx)
    check(L.dc_bn_bwd_apply(ptr(xx), ptr(gp), ptr(coef), ptr(dx), N, C, H * W, groups, stream(xx)), "dc_bn_bwd_apply")
    return dx, dgamma, dbeta


class _Cfg:
    """non-tensor arguments of the folded ops (one object, so that the autograd signatures stay short)"""
    __slots__ = ("groups", "in_stats", "bn", "prev", "want_stats", "relu", "res_fork", "leave_link",
                 "out_stats", "out_link")      # the last two are written by the forward (read by the wrapper right after apply)

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def _bn_buffers(bn):
    mom = 0.1 if bn.momentum is None else bn.momentum
    return bn.running_mean, bn.running_var, bn.eps, mom


def _fold(groups):
    """The dc_bn_fold of one launch, or None (NULL) for a caller without the fold: the library tells the two apart even when
    every pointer of the struct is null (csrc/pointwise.hip: pw_family gates the split kernels on `groups`' statistics layout)."""
    if groups is None:
        return None
    f = BnFold()
    f.groups = groups
    return f


def _ref(f):
    return ctypes.byref(f) if f is not None else None


# ----------------------------------------------------------------------------------------------
# kernel tables: the launches of one family with their workspace queries.  `f`: dc_bn_fold or None.  `policy`: the kernels
# follow the matrix-precision policy; `addend`: the data-gradient kernel adds the input's other gradients in its store epilogue;
# `ksizes`: the weights' trailing dimensions
# ----------------------------------------------------------------------------------------------
class _K1:
    """1x1 (stride 1 / 2) through dc_pointwise_* (csrc/pointwise.hip): the library picks the kernel family per pass -- split-operand
    bf16 (csrc/gemm1x1_x3.hip) under dc_set_gemm_split where it takes the shape, else fp32-MFMA (csrc/gemm1x1.hip), else, without a
    fold, the general kernels -- with ONE function behind the partial-count queries, the workspace queries and the launches (the
    epilogues' partial layouts follow each family's own tiles).  The split mode is read per call: set it around forward AND backward."""
    policy, addend, ksizes = False, True, ((), (1, 1))

    @staticmethod
    def out_hw(Hi, Wi, s_):
        return Hi // s_, Wi // s_

    @staticmethod
    def stat_parts(L, B, Ci, Co, Hi, Wi, s_, groups, ppg):
        return L.dc_pointwise_stat_parts(B, Ci, Co, Hi, Wi, s_, groups, ppg)

    @staticmethod
    def bwd_parts(L, B, Ci, Co, Hi, Wi, s_, groups, ppg):
        return L.dc_pointwise_bwd_parts(B, Ci, Co, Hi, Wi, s_, groups, ppg)

    @staticmethod
    def fwd(L, xx, ww, y, B, Ci, Co, Hi, Wi, s_, f):
        ws = torch.empty(L.dc_pointwise_workspace(_lib.PASS_FWD, _ref(f), B, Ci, Co, Hi, Wi, s_), dtype=torch.uint8, device=xx.device)
        check(L.dc_pointwise_fwd(ptr(xx), ptr(ww), None, ptr(y), ws.data_ptr(), B, Ci, Co, Hi, Wi, s_, 0, _ref(f), stream(xx)),
              "dc_pointwise_fwd")

    @staticmethod
    def dgrad(L, g_c, ww, gx, add, B, Ci, Co, Hi, Wi, s_, f, add2=None):
        # (with f.bwd_part: the BatchNorm-backward epilogue, stride 1, one addend; else the addends of the input's other consumers)
        ws = torch.empty(L.dc_pointwise_workspace(_lib.PASS_DGRAD, _ref(f), B, Ci, Co, Hi, Wi, s_), dtype=torch.uint8, device=gx.device)
        check(L.dc_pointwise_dgrad(ptr(g_c), ptr(ww), ptr(gx), ws.data_ptr(), ptr(add), ptr(add2), B, Ci, Co, Hi, Wi, s_, _ref(f),
                                   stream(gx)), "dc_pointwise_dgrad")

    @staticmethod
    def wgrad(L, xx, g_c, gw, B, Ci, Co, Hi, Wi, s_, f):
        ws = torch.empty(L.dc_pointwise_workspace(_lib.PASS_WGRAD, _ref(f), B, Ci, Co, Hi, Wi, s_), dtype=torch.uint8, device=xx.device)
        check(L.dc_pointwise_wgrad(ptr(xx), ptr(g_c), ptr(gw), ws.data_ptr(), B, Ci, Co, Hi, Wi, s_, _ref(f), stream(xx)),
              "dc_pointwise_wgrad")


class _KW:
    """stride-1 3x3, zero padding 1: fused Winograd F(2x2,3x3) on the matrix cores (the *_bn entries with a NULL fold are
    dc_wino3x3_fwd / dc_wino3x3_dgrad_add / dc_wino3x3_wgrad)"""
    policy, addend, ksizes = True, True, ((3, 3),)

    @staticmethod
    def out_hw(Hi, Wi, s_):
        return Hi, Wi

    @staticmethod
    def stat_parts(L, B, Ci, Co, Hi, Wi, s_, groups, ppg):
        return L.dc_wino3x3_stat_parts(B, Ci, Co, Hi, Wi, groups, ppg)

    @staticmethod
    def bwd_parts(L, B, Ci, Co, Hi, Wi, s_, groups, ppg):
        return L.dc_wino3x3_bwd_parts(B, Ci, Co, Hi, Wi, groups, ppg)

    @staticmethod
    def fwd(L, xx, ww, y, B, Ci, Co, Hi, Wi, s_, f):
        ws = torch.empty(L.dc_wino3x3_workspace(B, Ci, Co, Hi, Wi), dtype=torch.uint8, device=xx.device)
        check(L.dc_wino3x3_fwd_bn(ptr(xx), ptr(ww), ptr(y), ws.data_ptr(), B, Ci, Co, Hi, Wi, _ref(f), stream(xx)), "dc_wino3x3_fwd_bn")

    @staticmethod
    def dgrad(L, g_c, ww, gx, add, B, Ci, Co, Hi, Wi, s_, f, add2=None):
        if add2 is not None:
            raise _lib.DepthcoreError("SkipSum on a 3x3 convolution")
        ws = torch.empty(L.dc_wino3x3_workspace(B, Ci, Co, Hi, Wi), dtype=torch.uint8, device=gx.device)
        check(L.dc_wino3x3_dgrad_bn(ptr(g_c), ptr(ww), ptr(gx), ptr(add), ws.data_ptr(), B, Ci, Co, Hi, Wi, _ref(f), stream(gx)),
              "dc_wino3x3_dgrad_bn")

    @staticmethod
    def wgrad(L, xx, g_c, gw, B, Ci, Co, Hi, Wi, s_, f):
        ws = torch.empty(L.dc_wino3x3_wgrad_workspace(B, Ci, Co, Hi, Wi), dtype=torch.uint8, device=xx.device)
        check(L.dc_wino3x3_wgrad_bn(ptr(xx), ptr(g_c), ptr(gw), ws.data_ptr(), B, Ci, Co, Hi, Wi, _ref(f), stream(xx)),
              "dc_wino3x3_wgrad_bn")


class _KS:
    """3x3 / 2 and the 7x7 / 2 stem, zero padding k // 2: implicit GEMMs on the matrix cores.  No fold (no stat_parts /
    bwd_parts), and a data gradient without the addend epilogue: the second arrival at a pair fork adds in a pass of its own."""
    policy, addend, ksizes = True, False, ((3, 3), (7, 7))
    out_hw = staticmethod(_K1.out_hw)

    @staticmethod
    def fwd(L, xx, ww, y, B, Ci, Co, Hi, Wi, s_, f):
        ks = ww.shape[-1]
        if f is not None or not L.dc_convs2_supported(B, Ci, Co, Hi, Wi, ks):
            raise _lib.DepthcoreError("strided convolution %s on input %s is outside dc_convs2_* (3x3 / 7x7, stride 2, even sizes, "
                                      "output width %% 4 == 0, no BatchNorm fold)" % (tuple(ww.shape), tuple(xx.shape)))
        ws = torch.empty(L.dc_convs2_fwd_workspace(B, Ci, Co, Hi, Wi, ks), dtype=torch.uint8, device=xx.device)
        check(L.dc_convs2_fwd(ptr(xx), ptr(ww), ptr(y), ws.data_ptr(), B, Ci, Co, Hi, Wi, ks, stream(xx)), "dc_convs2_fwd")

    @staticmethod
    def dgrad(L, g_c, ww, gx, add, B, Ci, Co, Hi, Wi, s_, f, add2=None):
        ks = ww.shape[-1]
        n = L.dc_convs2_dgrad_workspace(B, Ci, Co, Hi, Wi, ks)
        if not n:
            raise _lib.DepthcoreError("no data gradient for this strided convolution (the 7x7 stem reads the image)")
        ws = torch.empty(n, dtype=torch.uint8, device=gx.device)
        check(L.dc_convs2_dgrad(ptr(g_c), ptr(ww), ptr(gx), ws.data_ptr(), B, Ci, Co, Hi, Wi, ks, stream(gx)), "dc_convs2_dgrad")

    @staticmethod
    def wgrad(L, xx, g_c, gw, B, Ci, Co, Hi, Wi, s_, f):
        ks = gw.shape[-1]
        ws = torch.empty(L.dc_convs2_wgrad_workspace(B, Ci, Co, Hi, Wi, ks), dtype=torch.uint8, device=xx.device)
        check(L.dc_convs2_wgrad(ptr(xx), ptr(g_c), ptr(gw), ws.data_ptr(), B, Ci, Co, Hi, Wi, ks, stream(xx)), "dc_convs2_wgrad")


_KINDS = {"g1": _K1, "wino": _KW, "s2": _KS}


# ----------------------------------------------------------------------------------------------
# [relu(bn(x)) in the loader] -> conv -> [statistics epilogue]; the data gradient adds the gradients of the input's other
# consumers and, with a fold, carries the BatchNorm-backward epilogue
# ----------------------------------------------------------------------------------------------
class _ConvF(torch.autograd.Function):
    """`groups` None: no dc_bn_fold reaches the library (the plain wrappers in convs.py); an int: every launch gets one with
    `groups` set (bnfold.py), `cfg` then carries in_stats / bn / prev / want_stats and receives out_stats."""
    @staticmethod
    def forward(ctx, x, weight, kind, stride, fork=None, skip=None, groups=None, cfg=None, gamma=None, beta=None):
        L = _lib.lib()
        K = _KINDS[kind]
        xx, ww = _c(x.detach()), _c(weight.detach())
        B, Ci, Hi, Wi = xx.shape
        Co, s_ = ww.shape[0], stride
        if ww.shape[1] != Ci or tuple(ww.shape[2:]) not in K.ksizes:
            raise _lib.DepthcoreError("weight %s does not match a %r convolution of %d input channels" % (tuple(ww.shape), kind, Ci))
        f = _fold(groups)
        # the plain paths follow the thread's policy; the fold is an fp32-policy path (its callers check the policy)
        ctx.prec = _use_precision(_precision[0] if f is None else _lib.PREC_F32) if K.policy else None
        fold_in = gamma is not None
        tab = g = None
        if fold_in:
            g = _c(gamma.detach())
            tab = _finalize(L, xx, cfg.in_stats, g, _c(beta.detach()), *_bn_buffers(cfg.bn), groups)
            f.in_scale, f.in_shift = tab[2].data_ptr(), tab[3].data_ptr()
            _record_kink("relu", lambda: _materialize(xx, tab, groups))
        Ho, Wo = K.out_hw(Hi, Wi, s_)
        y = torch.empty(B, Co, Ho, Wo, dtype=torch.float32, device=xx.device)
        if cfg is not None and cfg.want_stats:
            ppg = _ival()
            nparts = K.stat_parts(L, B, Ci, Co, Hi, Wi, s_, groups, ctypes.byref(ppg))
            if nparts:
                part = torch.empty(Co * nparts * 2, dtype=torch.float32, device=xx.device)
                f.stat_part = part.data_ptr()
                cfg.out_stats = BNStats(part, nparts, ppg.value, groups)
        K.fwd(L, xx, ww, y, B, Ci, Co, Hi, Wi, s_, f)
        prev = cfg.prev if (cfg is not None and cfg.prev is not None and x.requires_grad and fork is not None and not fork.pair) else None
        if prev is not None:
            prev.armed = True
        ctx.save_for_backward(xx, ww, g, tab, prev.x if prev is not None else None, prev.mean if prev is not None else None,
                              prev.mask if prev is not None else None)
        ctx.cfg = (s_, groups, fold_in, kind)
        ctx.prev = prev
        ctx.slots = (_slot(weight), _slot(gamma) if fold_in else None, _slot(beta) if fold_in else None)
        ctx.param = _lane_param(ctx, 1, weight)
        ctx.fork = fork if x.requires_grad else None
        # x's SkipSum (ops.SkipSum): the member of a pair fork that runs second collects the secondary consumers' gradients
        ctx.skip = skip if (skip is not None and kind == "g1" and ctx.fork is not None and ctx.fork.pair and not fold_in) else None
        if ctx.skip is not None:
            ctx.skip.arm()
        return y

    @staticmethod
    def backward(ctx, gy):
        L = _lib.lib()
        xx, ww, g, tab, px, pmean, pmask = ctx.saved_tensors
        B, Ci, Hi, Wi = xx.shape
        s_, groups, fold_in, kind = ctx.cfg
        K = _KINDS[kind]
        Co = ww.shape[0]
        g_c = _c(gy)
        if ctx.prec is not None:
            _use_precision(ctx.prec)
        gx = gw = dgamma = dbeta = None
        fork = ctx.fork
        # (a kernel without the addend epilogue shares its input through pair forks only: `arrive` refuses any other)
        first_of_pair = fork is not None and (fork.pair or not K.addend) and fork.arrive() == 0
        add = None if (first_of_pair or not K.addend) else _fork_addend(ctx, xx)
        if ctx.prev is not None and add is None:
            raise _lib.DepthcoreError("BNLink: the block's skip gradient did not arrive -- the convolution's result would not be "
                                      "the complete gradient of the linked output")
        f = _fold(groups)
        bwd = None
        # (the folded BatchNorm's dgamma / dbeta come out of the data-gradient epilogue's partials: that launch runs whenever
        # they are wanted, even if the raw input itself needs no gradient -- a frozen producer)
        bn_only = fold_in and not ctx.needs_input_grad[0] and (ctx.needs_input_grad[8] or ctx.needs_input_grad[9])
        if ctx.needs_input_grad[0] or bn_only:
            gx = torch.empty_like(xx)
            if fold_in or ctx.prev is not None:
                ppg = _ival()
                nparts = K.bwd_parts(L, B, Ci, Co, Hi, Wi, s_, groups, ctypes.byref(ppg))
                if not nparts:
                    raise _lib.DepthcoreError("BatchNorm fold: no backward epilogue for %s" % (tuple(xx.shape),))
                bpart = torch.empty(Ci * nparts * 2, dtype=torch.float32, device=xx.device)
                bwd = (bpart, nparts, ppg.value)
                f.bwd_part = bpart.data_ptr()
                if fold_in:
                    f.bn_x, f.bn_mean = xx.data_ptr(), tab[0].data_ptr()
                    f.in_scale, f.in_shift = tab[2].data_ptr(), tab[3].data_ptr()
                else:
                    f.bn_x, f.bn_mean, f.bn_mask = px.data_ptr(), pmean.data_ptr(), pmask.data_ptr()
            add2 = ctx.skip.take() if (ctx.skip is not None and not first_of_pair) else None
            if add2 is not None and (add2.shape != xx.shape or not add2.is_contiguous()):
                raise _lib.DepthcoreError("SkipSum: gradient %s does not match the input %s" % (tuple(add2.shape), tuple(xx.shape)))
            K.dgrad(L, g_c, ww, gx, add, B, Ci, Co, Hi, Wi, s_, f, add2)
            if first_of_pair:
                fork.park(gx)                   # the other convolution of the pair adds it and returns the sum
                gx = None
            elif fork is not None and not K.addend:
                gx = gx + fork.take()           # (no addend epilogue: arriving second, this kernel's gradient is added in a pass of its own)
            elif ctx.prev is not None:
                ctx.prev.bwd = bwd              # gx is g' of the producing block's last BatchNorm: its backward is one pass now
        elif first_of_pair or (fork is not None and not K.addend):
            raise _lib.DepthcoreError("GradFork: the shared input needs no gradient")
        if ctx.needs_input_grad[1]:
            fw = _fold(groups)
            reads = [xx, g_c]
            if fold_in:
                fw.in_scale, fw.in_shift = tab[2].data_ptr(), tab[3].data_ptr()
                reads.append(tab)
            with WgradLanes.lane(ctx.param, *reads):
                gw = _grad_dst(ctx.slots[0], ww)
                K.wgrad(L, xx, g_c, gw, B, Ci, Co, Hi, Wi, s_, fw)
        if fold_in and gx is not None:
            gx, dgamma, dbeta = _bwd_finish(L, xx, gx, bwd, g, tab, groups, ctx.slots[1:])
            if bn_only:
                gx = None
        return gx, gw, None, None, None, None, None, None, dgamma, dbeta


def _materialize(xx, tab, groups):
    """relu(scale x + shift) as a tensor -- decision observers (tests) only; the training path never forms it."""
    N, C = xx.shape[:2]
    sc = tab[2].view(groups, 1, C, 1, 1)
    sh = tab[3].view(groups, 1, C, 1, 1)
    return torch.relu(xx.view(groups, N // groups, C, *xx.shape[2:]) * sc + sh).view_as(xx)
