"""The ConvGRU recurrence for S sequences in lockstep (ops.gru_level_sequence(..., streams=S), ConvGRUBlocks_v5.run_sequence
(..., streams=S)) at the five level shapes of a resnet18 on 32 x 96 images: against S separate single-sequence calls on the
gathered rows, against the fp64 oracle called per item, and the kernel that sums the streams' gradients of the shared
initial state (dc_gru_state_bwd) against an fp64 sum."""
import functools

import numpy as np
import pytest
import torch

from helpers import rel_l2
from oracle import gru_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEVELS = ((64, 16, 48), (64, 8, 24), (128, 4, 12), (256, 2, 6), (512, 1, 3))      # resnet18, 32 x 96


# ---- dc_gru_state_bwd ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [105, 1536, 49152])          # odd; the smallest level (512 x 1 x 3); the largest (64 x 16 x 48)
@pytest.mark.parametrize("S", [1, 2, 5])
def test_state_gradient_is_the_sum_over_the_streams(S, M):
    """One fp32 rounding per addend: |got - sum| <= S * 2^-24 * sum of magnitudes, elementwise; two calls agree bit for bit.
    The buffer holds the rows of a later time step behind the S rows, as the hidden-state gradients do: they are not read."""
    from depthcore import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(100 * S + M % 97)
    d_H = (torch.randn(S + 2, M, generator=g) * torch.logspace(-3, 3, M)[None]).to(DEV)
    outs = []
    for _ in range(2):
        out = torch.full((M + 8,), 7.0, device=DEV)
        _lib.check(L.dc_gru_state_bwd(d_H.data_ptr(), out.data_ptr(), S, M, _lib.stream(out)), "dc_gru_state_bwd")
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    assert bool((outs[0][M:] == 7.0).all())                                     # nothing written past the M elements
    rows = d_H[:S].double().cpu()
    want, mag = rows.sum(0), rows.abs().sum(0)
    err = (outs[0][:M].double().cpu() - want).abs()
    bound = S * 2.0 ** -24 * mag
    print("S %d M %d: max err / bound %.3f" % (S, M, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all())
    if S == 1:
        assert torch.equal(outs[0][:M], d_H[0])


# ---- the 1 x 3 level: the fused block under zero padding on a map of one row ---------------------------------------------------
@pytest.mark.parametrize("B,C0,C1,Co,H,W,act", [(2, 512, 512, 1024, 1, 3, "sigmoid"), (3, 512, 512, 512, 1, 3, "tanh"),
                                               (2, 24, 8, 20, 1, 16, "sigmoid"), (1, 16, 16, 16, 5, 1, "tanh")])
def test_conv_block_on_one_row_maps_under_zero_padding(B, C0, C1, Co, H, W, act):
    """The last level of a resnet18 on 32 x 96 images is 1 x 3: the cells' two convolutions (cat of two sources, bias, sigmoid /
    tanh, ZeroPad2d) against torch's conv2d in fp64 -- output and the four gradients.  Bound: an fp32 dot product of
    K = 9 (C0 + C1) terms is off by about 2^-24 sqrt(K) relative (5.7e-6 at K = 9216), 1e-5 in rel_l2; reflection padding
    still refuses such a map."""
    import torch.nn.functional as F
    from depthcore import _lib, ops
    g = torch.Generator().manual_seed(B + Co + W)
    x0, x1 = torch.randn(B, C0, H, W, generator=g), torch.randn(B, C1, H, W, generator=g)
    w = torch.randn(Co, C0 + C1, 3, 3, generator=g) / (9 * (C0 + C1)) ** 0.5
    b, cot = torch.randn(Co, generator=g), torch.randn(B, Co, H, W, generator=g)
    fn = torch.sigmoid if act == "sigmoid" else torch.tanh
    ref = [t.double().requires_grad_() for t in (x0, x1, w, b)]
    want = fn(F.conv2d(torch.cat(ref[:2], 1), ref[2], ref[3], padding=1))
    want_g = torch.autograd.grad((want * cot.double()).sum(), ref)
    dev = [t.to(DEV).requires_grad_() for t in (x0, x1, w, b)]
    code = ops.ACT_SIGMOID if act == "sigmoid" else ops.ACT_TANH
    got = ops.conv3x3_block(dev[0], dev[1], dev[2], dev[3], False, code, ops.PAD_ZERO)
    got_g = torch.autograd.grad((got * cot.to(DEV)).sum(), dev)
    torch.cuda.synchronize()
    figures = [rel_l2(got, want.detach())] + [rel_l2(a, b_) for a, b_ in zip(got_g, want_g)]
    print("one-row block %s:" % ((B, C0, C1, Co, H, W),), " ".join("%.2e" % v for v in figures))
    assert all(v < 1e-5 for v in figures), figures
    with pytest.raises(_lib.DepthcoreError):
        ops.conv3x3_block(dev[0], dev[1], dev[2], dev[3], False, code, ops.PAD_REFLECT)


# ---- one level: streams = S against S single-sequence calls ----------------------------------------------------------------
def _level(k, seed=0):
    import torch.nn as nn
    C, h, w = LEVELS[k]
    g = torch.Generator().manual_seed(10 + k + 100 * seed)
    gates, can = nn.Conv2d(2 * C, 2 * C, 3, padding=1), nn.Conv2d(2 * C, C, 3, padding=1)
    for p in list(gates.parameters()) + list(can.parameters()):
        p.data = torch.randn(p.shape, generator=g) * 0.05
    h0 = torch.randn(1, C, h, w, generator=g) * 0.1
    return gates.to(DEV), can.to(DEV), h0.to(DEV).requires_grad_()


def _params(gates, can):
    return [gates.weight, gates.bias, can.weight, can.bias]


def _lockstep(feats, cot, h0, gates, can, S):
    from depthcore import ops
    f = feats.clone().requires_grad_()
    out = ops.gru_level_sequence(f, h0, gates, can, streams=S)
    gr = torch.autograd.grad((out * cot).sum(), [f, h0] + _params(gates, can))
    return out.detach(), gr


def _per_item(feats, cot, h0, gates, can, S, n):
    """S separate single-sequence calls on the gathered rows; outputs and feature gradients scattered back, the shared
    tensors' gradients summed over the items."""
    from depthcore import ops
    out, gf = torch.empty_like(feats), torch.empty_like(feats)
    shared = None
    for s in range(S):
        rows = ops.seq_item_rows(s, S, n)
        f = feats[rows].clone().requires_grad_()
        o = ops.gru_level_sequence(f, h0, gates, can)
        gr = torch.autograd.grad((o * cot[rows]).sum(), [f, h0] + _params(gates, can))
        out[rows], gf[rows] = o.detach(), gr[0]
        shared = list(gr[1:]) if shared is None else [a + b for a, b in zip(shared, gr[1:])]
    return out, [gf] + shared


NAMES = ("features", "h0", "gates.weight", "gates.bias", "can.weight", "can.bias")


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("k", range(5))
def test_lockstep_level_equals_the_items_run_one_by_one(k, S, n):
    C, h, w = LEVELS[k]
    gates, can, h0 = _level(k)
    g = torch.Generator().manual_seed(7 * k + S + 31 * n)
    feats = torch.randn(n * S, C, h, w, generator=g).to(DEV)
    cot = torch.randn(n * S, C, h, w, generator=g).to(DEV)
    out_l, gr_l = _lockstep(feats, cot, h0, gates, can, S)
    out_i, gr_i = _per_item(feats, cot, h0, gates, can, S, n)
    torch.cuda.synchronize()
    figures = {"out": rel_l2(out_l, out_i)}
    figures.update({name: rel_l2(a, b) for name, a, b in zip(NAMES, gr_l, gr_i)})
    print("level %d S %d n %d:" % (k, S, n), " ".join("%s %.2e" % kv for kv in figures.items()))
    assert gr_l[1].shape == h0.shape
    for name, v in figures.items():
        assert v < 1e-5, (name, v)


@pytest.mark.parametrize("shape", [(64, 32, 64), (64, 16, 32), (128, 8, 16), (64, 16, 48), (512, 1, 3)])
def test_a_stream_does_not_depend_on_its_companions(shape):
    """The lockstep launches plan their reductions as one stream's launch does (dc_set_wino_plan_streams), so a sequence's
    outputs and feature gradients in a step of S are, bit for bit, those of its single-sequence call -- also where the planner
    would split the reduction differently for the larger batch (the 64-channel levels of a 64 x 128 image)."""
    from depthcore import _lib, ops
    import torch.nn as nn
    C, h, w = shape
    g = torch.Generator().manual_seed(C + h)
    gates, can = nn.Conv2d(2 * C, 2 * C, 3, padding=1), nn.Conv2d(2 * C, C, 3, padding=1)
    for p in list(gates.parameters()) + list(can.parameters()):
        p.data = torch.randn(p.shape, generator=g) * 0.05
    gates, can = gates.to(DEV), can.to(DEV)
    h0 = (torch.randn(1, C, h, w, generator=g) * 0.1).to(DEV).requires_grad_()
    S, n = 2, 3
    feats = torch.randn(n * S, C, h, w, generator=g).to(DEV)
    cot = torch.randn(n * S, C, h, w, generator=g).to(DEV)
    out_l, gr_l = _lockstep(feats, cot, h0, gates, can, S)
    out_i, gr_i = _per_item(feats, cot, h0, gates, can, S, n)
    torch.cuda.synchronize()
    print("shape %s: %d outputs and %d feature gradients of %d differ" % (shape, int((out_l != out_i).sum()), int((gr_l[0] != gr_i[0]).sum()), out_l.numel()))
    assert torch.equal(out_l, out_i) and torch.equal(gr_l[0], gr_i[0])
    assert _lib.lib().dc_set_wino_plan_streams(1) == 1                          # the node restored the thread's setting


@pytest.mark.parametrize("k", range(5))
def test_one_stream_through_the_new_argument_is_today_s_result(k):
    from depthcore import ops
    C, h, w = LEVELS[k]
    gates, can, h0 = _level(k)
    g = torch.Generator().manual_seed(3 + k)
    feats = torch.randn(3, C, h, w, generator=g).to(DEV)
    cot = torch.randn(3, C, h, w, generator=g).to(DEV)
    res = []
    for kw in ({}, {"streams": 1}):
        f = feats.clone().requires_grad_()
        out = ops.gru_level_sequence(f, h0, gates, can, **kw)
        res.append([out.detach()] + list(torch.autograd.grad((out * cot).sum(), [f, h0] + _params(gates, can))))
    out_l, gr_l = _lockstep(feats, cot, h0, gates, can, 1)
    for a, b, c in zip(res[0], res[1], [out_l] + list(gr_l)):
        assert torch.equal(a, b) and torch.equal(a, c)
    with pytest.raises(Exception, match="streams"):
        ops.gru_level_sequence(feats, h0, gates, can, streams=2)                 # 3 rows are not the frames of 2 streams


def test_module_takes_the_streams_per_call():
    """ConvGRUBlocks_v5.run_sequence(features, streams=S): the level nodes with S streams, and the same module still runs one
    sequence -- the number of streams is a property of the call."""
    import networks
    from depthcore import ops
    torch.manual_seed(5)
    blk = networks.ConvGRUBlocks_v5(kernel_size=(3, 3), bias=True, device="cpu", height=32, width=96).to(DEV)
    for p_ in blk.parameters():
        p_.data.normal_(0, 0.05)
    n, S = 3, 2
    feats = [torch.randn(n * S, c, h, w, device=DEV) for c, h, w in LEVELS]
    outs = blk.run_sequence(feats, streams=S)
    for s in range(S):
        rows = ops.seq_item_rows(s, S, n)
        one = blk.run_sequence([f[rows].contiguous() for f in feats])
        for a, b in zip(outs, one):
            assert rel_l2(a[rows], b) < 1e-5
    with pytest.raises(Exception, match="streams"):
        blk.run_sequence(feats, streams=4)


# ---- against the fp64 oracle, called per item ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_case(S, n):
    """Inputs of all five levels, the oracle's outputs and gradients in fp64 (sums over the items for the shared tensors)."""
    g = torch.Generator().manual_seed(40 + S)
    st = {key: torch.randn(shape, generator=g) * (0.1 if key.endswith("h0_layer1") else 0.05)
          for key, shape in G.gru_v5_layout(32, 96)}
    feats = [torch.randn(n * S, c, h, w, generator=g) for c, h, w in LEVELS]
    cots = [torch.randn(n * S, c, h, w, generator=g) for c, h, w in LEVELS]
    st64 = {k: v.double().requires_grad_() for k, v in st.items()}
    f64 = [f.double().requires_grad_() for f in feats]
    total, outs = 0.0, [torch.empty_like(f, dtype=torch.float64) for f in feats]
    for s in range(S):
        rows = slice(s, s + (n - 1) * S + 1, S)
        o = G.run_gru_v5([f[rows] for f in f64], st64)
        for k in range(5):
            outs[k][rows] = o[k].detach()
            total = total + (o[k] * cots[k][rows].double()).sum()
    keys = list(st64)
    gr = torch.autograd.grad(total, f64 + [st64[k] for k in keys])
    return st, feats, cots, outs, gr[:5], dict(zip(keys, gr[5:]))


def test_lockstep_against_the_fp64_oracle_per_item():
    """Error of a level = the largest rel_l2 against the oracle among its output, feature gradient, h0 gradient and the four
    parameter gradients.  The lockstep path's error is reported next to the per-item path's and must be at most twice it
    (the weight gradient's reduction grows from n to n * S rows)."""
    import torch.nn as nn
    S, n = 3, 3
    st, feats, cots, want_out, want_gf, want_g = _oracle_case(S, n)
    for k, (C, h, w) in enumerate(LEVELS):
        p = "cgru_%d." % k
        gates, can = nn.Conv2d(2 * C, 2 * C, 3, padding=1), nn.Conv2d(2 * C, C, 3, padding=1)
        gates.weight.data, gates.bias.data = st[p + "cgru_1.conv_gates.weight"].clone(), st[p + "cgru_1.conv_gates.bias"].clone()
        can.weight.data, can.bias.data = st[p + "cgru_1.conv_can.weight"].clone(), st[p + "cgru_1.conv_can.bias"].clone()
        gates, can = gates.to(DEV), can.to(DEV)
        h0 = st[p + "h0_layer1"].to(DEV).requires_grad_()
        f, c = feats[k].to(DEV), cots[k].to(DEV)
        want = [want_out[k], want_gf[k]] + [want_g[p + name] for name in
                                            ("h0_layer1", "cgru_1.conv_gates.weight", "cgru_1.conv_gates.bias",
                                             "cgru_1.conv_can.weight", "cgru_1.conv_can.bias")]
        errs = {}
        for path, (out, gr) in (("lockstep", _lockstep(f, c, h0, gates, can, S)), ("per item", _per_item(f, c, h0, gates, can, S, n))):
            errs[path] = max(rel_l2(a, b) for a, b in zip([out] + list(gr), want))
        print("level %d %s: lockstep %.3e  per item %.3e" % (k, (C, h, w), errs["lockstep"], errs["per item"]))
        assert errs["lockstep"] <= 2 * errs["per item"], (k, errs)
