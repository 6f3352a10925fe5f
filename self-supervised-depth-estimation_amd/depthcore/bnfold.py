"""BatchNorm folded into the neighbouring convolutions of the ResNet trunks (include/depthcore.h: dc_bn_fold).

torchvision's BasicBlock / Bottleneck (reference networks/resnet_encoder.py:87-98) put a training-mode BatchNorm2d (+ReLU, and
on the block output + the skip) behind every convolution.  As stand-alone kernels that is four streaming passes over HBM per
layer (statistics, apply, backward statistics, backward apply).  Here:

  * the PRODUCING convolution emits the per-channel partial sums of its raw output in its store epilogue (`BNStats`), a
    finalize launch turns them into mean / invstd / scale / shift (and the running statistics);
  * a BatchNorm + ReLU with ONE consumer (bn1 -> conv2, bn2 -> conv3) is never materialised: the consuming convolution reads
    relu(scale * x + shift) in its loader (forward and weight gradient), its data-gradient epilogue applies the ReLU decision
    and emits the backward partials, and one pass forms dx (`FoldedConv*`);
  * a block output relu(bn(x) + skip) keeps its apply pass (`bn_apply`), and when the next block's conv1 is its only consumer
    (`BNLink`) that convolution's data-gradient epilogue -- which already adds the skip's gradient -- does the masking and the
    backward partials, so the backward is one pass as well.

Same arithmetic as depthcore.convs.bn_relu (`ops.bn_relu`) up to the order of the sums; deterministic.  No fallback: CPU tensors raise.
"""
import torch

from . import _lib
from . import ops as _ops
from ._autograd import _c
from ._lib import check, ptr, stream
from .convnode import BNLink, BNStats, _bn_buffers, _bwd_finish, _Cfg, _ConvF, _finalize, _K1, _KW  # noqa: F401


def conv1x1_ok(conv, xshape, groups):
    """All three passes of this stride-1 1x1 convolution on an fp32 device tensor of shape `xshape` take the fold with a
    BatchNorm on its input (tiled kernels, 16-byte staging, backward epilogue for this group layout)."""
    B, Ci, Hi, Wi = xshape
    L = _lib.lib()
    return (conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0) and conv.groups == 1 and conv.bias is None
            and conv.in_channels == Ci and B % groups == 0 and (Hi * Wi) % 4 == 0
            and bool(L.dc_conv1x1_bn_ok(B, Ci, conv.out_channels, Hi, Wi))
            and L.dc_conv1x1_bwd_parts(B, Ci, conv.out_channels, Hi, Wi, groups, None) > 0)


def wino_ok(conv, xshape, groups):
    """Forward and data gradient of this stride-1 3x3 convolution take the fold with a BatchNorm on its input."""
    B, Ci, Hi, Wi = xshape
    _ops._use_precision(_lib.PREC_F32)      # (the query below looks at the calling thread's policy; the callers run the fp32 one)
    return (conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1) and conv.dilation == (1, 1)
            and conv.groups == 1 and conv.bias is None and conv.in_channels == Ci and Wi % 2 == 0 and (Hi * Wi) % 4 == 0
            and max(B * Ci * Hi * Wi, B * conv.out_channels * Hi * Wi) * 4 < 0x7fffffff
            and bool(_lib.lib().dc_wino3x3_bn_ok(B, Ci, conv.out_channels, Hi, Wi, groups)))


def _conv(kind, x, weight, stride, groups, fork, in_bn, in_stats, prev, want_stats, skip=None):
    # (`groups` is an int here: every launch gets a dc_bn_fold, also with nothing to fold -- see convnode._fold)
    cfg = _Cfg(in_stats=in_stats, bn=in_bn, prev=prev, want_stats=want_stats)
    y = _ConvF.apply(x, weight, kind, int(stride), fork, skip, int(groups), cfg, in_bn.weight if in_bn is not None else None,
                     in_bn.bias if in_bn is not None else None)
    return y, cfg.out_stats


def conv1x1(x, weight, stride=1, groups=1, fork=None, in_bn=None, in_stats=None, prev=None, want_stats=True, skip=None):
    """y_raw, BNStats-or-None = conv1x1([relu(in_bn(x))]).  `in_bn`: the nn.BatchNorm2d (training mode) in front of this convolution
    whose ReLU-ed output has no other consumer -- x is then that BatchNorm's RAW input and `in_stats` its statistics partials
    (None: a stand-alone statistics pass).  `prev`: BNLink of the block output x.  `fork`: GradFork."""
    return _conv("g1", x, weight, stride, groups, fork, in_bn, in_stats, prev, want_stats, skip)


def conv3x3(x, weight, groups=1, fork=None, in_bn=None, in_stats=None, prev=None, want_stats=True):
    """The same for F.conv2d(x, weight, None, 1, 1) on the Winograd kernels (even width)."""
    return _conv("wino", x, weight, 1, groups, fork, in_bn, in_stats, prev, want_stats)


# ----------------------------------------------------------------------------------------------
# the apply pass that remains: block outputs y = relu?(bn(x) [+ skip]) with several consumers
# ----------------------------------------------------------------------------------------------
class _BNApply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, gamma, beta, cfg):
        L = _lib.lib()
        xx = _c(x.detach())
        rr = _c(res.detach()) if res is not None else None
        g = _c(gamma.detach())
        N, C, H, W = xx.shape
        groups, relu = cfg.groups, cfg.relu
        tab = _finalize(L, xx, cfg.in_stats, g, _c(beta.detach()), *_bn_buffers(cfg.bn), groups)
        y = torch.empty_like(xx)
        nmask = L.dc_bn_mask_bytes(N, C, H * W) if relu else 0
        mask = torch.empty(nmask, dtype=torch.uint8, device=xx.device) if nmask else None
        check(L.dc_bn_apply(ptr(xx), ptr(rr), tab[2].data_ptr(), tab[3].data_ptr(), ptr(y), mask.data_ptr() if nmask else None,
                            N, C, H * W, int(relu), groups, stream(xx)), "dc_bn_apply")
        if relu:
            _ops._record_kink("relu", y)
        ctx.save_for_backward(xx, y if (relu and mask is None) else None, g, tab, mask)
        ctx.cfg = (int(relu), res is not None, groups)
        ctx.slots = (_ops._slot(gamma), _ops._slot(beta))
        ctx.fork = cfg.res_fork if (cfg.res_fork is not None and res is not None and res.requires_grad) else None
        ctx.link = cfg.out_link = BNLink(xx, tab[0], mask, groups) if (cfg.leave_link and relu and mask is not None) else None
        return y

    @staticmethod
    def backward(ctx, gy):
        L = _lib.lib()
        xx, y, g, tab, mask = ctx.saved_tensors
        relu, has_res, groups = ctx.cfg
        N, C, H, W = xx.shape
        g_c = _c(gy)
        link = ctx.link
        want_res = has_res and ctx.needs_input_grad[1]
        if link is not None and link.bwd is not None:
            # the only consumer's data-gradient epilogue masked the gradient and took the partials: one pass left; the masked
            # gradient itself is the skip's gradient
            dx, dgamma, dbeta = _bwd_finish(L, xx, g_c, link.bwd, g, tab, groups, ctx.slots)
            dres = g_c if want_res else None
            link.bwd = None
        else:
            if link is not None and link.armed:
                raise _lib.DepthcoreError("BNLink: the consumer took the link but its backward has not run before this BatchNorm's")
            dx = torch.empty_like(xx)
            dres = torch.empty_like(xx) if want_res else None
            dgamma = _ops._grad_dst(ctx.slots[0], g)
            dbeta = _ops._grad_dst(ctx.slots[1], g)
            ws = torch.empty(L.dc_bn_workspace(N, C, H * W), dtype=torch.uint8, device=xx.device)
            check(L.dc_bn_relu_bwd(ptr(xx), ptr(y), ptr(g_c), ptr(g), tab[0].data_ptr(), tab[1].data_ptr(), ptr(dx), ptr(dres),
                                   ptr(dgamma), ptr(dbeta), ws.data_ptr(), mask.data_ptr() if mask is not None else None, N, C, H * W,
                                   relu, groups, stream(xx)), "dc_bn_relu_bwd")
        if ctx.fork is not None and dres is not None:
            ctx.fork.park(dres)
            dres = None
        return dx, dres, dgamma, dbeta, None


def bn_apply(x, bn, stats=None, res=None, relu=True, groups=1, fork=None, leave_link=False):
    """y = relu?(bn(x) [+ res]) from the producing convolution's statistics partials (`stats`; None: a stand-alone statistics
    pass).  `leave_link`: attach a BNLink to y for a consumer that is known to be the only one (ResNetTrunk sets it for block
    outputs inside a stage)."""
    cfg = _Cfg(groups=int(groups), in_stats=stats, bn=bn, relu=bool(relu), res_fork=fork, leave_link=bool(leave_link))
    y = _BNApply.apply(x, res, bn.weight, bn.bias, cfg)
    if cfg.out_link is not None and y.requires_grad:
        y._dc_bn_link = cfg.out_link
    return y


def take_link(x, conv, groups):
    """The BNLink of a block output for its only consumer `conv` (the caller vouches for "only"), or None when there is none
    or the convolution's data gradient has no BatchNorm epilogue on this shape."""
    link = getattr(x, "_dc_bn_link", None)
    if link is None or link.groups != groups:
        return None
    B, Ci, Hi, Wi = x.shape
    if (Hi * Wi) % 4:
        ok = False
    elif conv.kernel_size == (1, 1):
        ok = conv.stride == (1, 1) and _lib.lib().dc_conv1x1_bwd_parts(B, Ci, conv.out_channels, Hi, Wi, groups, None) > 0
    elif conv.kernel_size == (3, 3):
        ok = (conv.stride == (1, 1) and conv.padding == (1, 1) and Wi % 2 == 0
              and _lib.lib().dc_wino3x3_bwd_parts(B, Ci, conv.out_channels, Hi, Wi, groups, None) > 0)
    else:
        ok = False
    return link if ok else None
