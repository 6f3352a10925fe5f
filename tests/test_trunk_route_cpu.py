"""networks/resnet_encoder.py:_route -- the one place that picks a trunk convolution's kernel family -- against a table of
literal expectations, and the fork predicates (_fork_for, _pair_fork_for, _basic_pair_fork) against the routes they must agree
with: a fork handed to a kernel without the addend epilogue is a DepthcoreError in the middle of a step, a fork withheld from
one that has it costs an elementwise pass.  No GPU: the inputs are stand-ins that carry only what _route may read; the one
library call behind it (dc_convs2_supported) is host code.

The `want` column was recorded once from the previous revision's `_conv` (wino_conv3x3, conv1x1, conv_s2 and conv2d_direct
replaced by recorders, the same stand-ins fed in; a refusal counts as "direct")."""
import types

import pytest
import torch
import torch.nn as nn

from networks import resnet_encoder as RE

FLAGS = ("WINO_TRUNK", "GEMM_1X1", "CONV_S2")


class X:
    """what _route may read of its input, and nothing else"""
    __slots__ = ("shape", "dtype", "is_cuda", "requires_grad")

    def __init__(self, shape, dtype=torch.float32, is_cuda=True, requires_grad=True):
        self.shape, self.dtype, self.is_cuda, self.requires_grad = torch.Size(shape), dtype, is_cuda, requires_grad


class XT(X):
    """+ what the block-level conditions of the fork predicates read"""
    __slots__ = ()

    def numel(self):
        return self.shape.numel()


def conv(ci, co, k, s, p, d=1, bias=False):
    return nn.Conv2d(ci, co, k, s, p, d, bias=bias)


# name: (conv, input, flags switched off, want)
ROWS = {
    "3x3": (conv(64, 64, 3, 1, 1), X((2, 64, 8, 16)), (), "wino"),
    "3x3 odd width": (conv(64, 64, 3, 1, 1), X((2, 64, 8, 15)), (), "direct"),
    "3x3 odd height": (conv(64, 64, 3, 1, 1), X((2, 64, 7, 16)), (), "wino"),
    "3x3 bias": (conv(64, 64, 3, 1, 1, bias=True), X((2, 64, 8, 16)), (), "direct"),
    "3x3 dilated": (conv(64, 64, 3, 1, 2, 2), X((2, 64, 8, 16)), (), "direct"),
    "3x3 no padding": (conv(64, 64, 3, 1, 0), X((2, 64, 8, 16)), (), "direct"),
    "3x3 fp64": (conv(64, 64, 3, 1, 1), X((2, 64, 8, 16), torch.float64), (), "direct"),
    "3x3 on the CPU": (conv(64, 64, 3, 1, 1), X((2, 64, 8, 16), is_cuda=False), (), "direct"),
    "3x3 no WINO_TRUNK": (conv(64, 64, 3, 1, 1), X((2, 64, 8, 16)), ("WINO_TRUNK",), "direct"),
    "3x3 no grad": (conv(64, 64, 3, 1, 1), X((2, 64, 8, 16), requires_grad=False), (), "wino"),
    "1x1": (conv(256, 64, 1, 1, 0), X((2, 256, 8, 16)), (), "g1"),
    "1x1 odd map": (conv(256, 64, 1, 1, 0), X((2, 256, 7, 15)), (), "g1"),
    "1x1 / 2": (conv(256, 512, 1, 2, 0), X((2, 256, 8, 16)), (), "g1"),
    "1x1 / 2 height 7": (conv(256, 512, 1, 2, 0), X((2, 256, 7, 16)), (), "direct"),
    "1x1 / 2 width 15": (conv(256, 512, 1, 2, 0), X((2, 256, 8, 15)), (), "direct"),
    "1x1 bias": (conv(256, 64, 1, 1, 0, bias=True), X((2, 256, 8, 16)), (), "direct"),
    "1x1 fp64": (conv(256, 64, 1, 1, 0), X((2, 256, 8, 16), torch.float64), (), "direct"),
    "1x1 no GEMM_1X1": (conv(256, 64, 1, 1, 0), X((2, 256, 8, 16)), ("GEMM_1X1",), "direct"),
    "1x1 / 2 no GEMM_1X1": (conv(256, 512, 1, 2, 0), X((2, 256, 8, 16)), ("GEMM_1X1",), "direct"),
    "3x3 / 2": (conv(64, 128, 3, 2, 1), X((2, 64, 16, 32)), (), "s2"),
    "3x3 / 2 six channels in": (conv(6, 128, 3, 2, 1), X((2, 6, 16, 32)), (), "direct"),
    "3x3 / 2 48 channels out": (conv(64, 48, 3, 2, 1), X((2, 64, 16, 32)), (), "direct"),
    "3x3 / 2 dilated": (conv(64, 128, 3, 2, 2, 2), X((2, 64, 16, 32)), (), "direct"),
    "3x3 / 2 odd height": (conv(64, 128, 3, 2, 1), X((2, 64, 15, 32)), (), "direct"),
    "3x3 / 2 no CONV_S2": (conv(64, 128, 3, 2, 1), X((2, 64, 16, 32)), ("CONV_S2",), "direct"),
    "stem": (conv(3, 64, 7, 2, 3), X((2, 3, 32, 64), requires_grad=False), (), "s2"),
    "stem, input needs a gradient": (conv(3, 64, 7, 2, 3), X((2, 3, 32, 64)), (), "direct"),
    "stem no CONV_S2": (conv(3, 64, 7, 2, 3), X((2, 3, 32, 64), requires_grad=False), ("CONV_S2",), "direct"),
    "5x5 / 2": (conv(64, 128, 5, 2, 2), X((2, 64, 16, 32)), (), "direct"),
}


def _off(monkeypatch, flags):
    for f in FLAGS:
        monkeypatch.setattr(RE, f, f not in flags)


@pytest.mark.parametrize("name", list(ROWS))
def test_route(monkeypatch, name):
    c, x, off, want = ROWS[name]
    _off(monkeypatch, off)
    assert RE._route(c, x) == want


def _tensorlike(x):
    return XT(x.shape, x.dtype, x.is_cuda, x.requires_grad)


def _block(conv1, down=None):
    return types.SimpleNamespace(conv1=conv1, downsample=None if down is None else [down, None], training=True)


@pytest.mark.parametrize("name", list(ROWS))
def test_identity_block_gets_a_fork_exactly_on_the_addend_kernels(monkeypatch, name):
    """the property the fork predicate and `_conv` used to keep in step by hand"""
    c, x, off, want = ROWS[name]
    _off(monkeypatch, off)
    monkeypatch.setattr(RE, "GRAD_FORK", True)
    fork = RE._fork_for(_block(c), _tensorlike(x))
    assert (fork is not None) == (want in ("wino", "g1") and c.stride == (1, 1) and x.requires_grad), name
    assert fork is None or not fork.pair
    blk = _block(c)
    blk.training = False
    assert RE._fork_for(blk, _tensorlike(x)) is None
    monkeypatch.setattr(RE, "GRAD_FORK", False)
    assert RE._fork_for(_block(c), _tensorlike(x)) is None


@pytest.mark.parametrize("name", list(ROWS))
def test_pair_forks_agree_with_both_routes(monkeypatch, name):
    c, x, off, want = ROWS[name]
    _off(monkeypatch, off)
    monkeypatch.setattr(RE, "GRAD_FORK", True)
    xt = _tensorlike(x)
    ci = c.in_channels
    for d in (conv(ci, 128, 1, 1, 0), conv(ci, 128, 1, 2, 0), conv(ci, 128, 1, 2, 0, bias=True), conv(ci, 128, 3, 2, 1)):
        rd = RE._route(d, x)
        blk = _block(c, d)
        pair = RE._pair_fork_for(blk, xt)
        assert (pair is not None) == (want == "g1" and c.stride == (1, 1) and rd == "g1" and x.requires_grad), (name, d)
        basic = RE._basic_pair_fork(blk, xt)
        assert (basic is not None) == (want == "s2" and c.kernel_size == (3, 3) and rd == "g1" and d.stride == (2, 2)
                                       and x.requires_grad), (name, d)
        assert all(f is None or f.pair for f in (pair, basic))
