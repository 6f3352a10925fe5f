"""Case table, seeded input builder and fp64 reference statement for ONE AttentionConv call of the Fusion_v3 front-end
(csrc/attn.hip: dc_attnconv_fwd / dc_attnconv_bwd) at the tile, padding and reduction edges of its kernels.  Shared by
tests/test_attn_cases_cpu.py (no GPU: the table reaches its mechanisms, the cases are well conditioned, the exact claims hold
for the statement itself) and tests/test_attn_shapes_gpu.py (the kernels against the statement).  DESIGN.md, "AttentionConv
at its tile, padding and reduction edges", has the table with its reasons, the gate and the measured errors.

    Case                     (B, C, H, W, x_layout, res_layout, relu_in, relu_res, dx_add, dres, param_style)
    build(case)              seeded fp64 masters (every value fp32-representable, so the device sees the same numbers)
    evaluate(case, inp, dt)  y = attention_conv(relu?(x)) + relu?(res) by oracle/fusion_ref.py, gradients by CPU autograd
    reference(case)          cached (inputs, fp64 results, fp32 results, info); nobody may modify what it returns

A layout lists the sources that make up the C channels of a map, in channel order:
    "p1" "p2" "p4"   a plain (B,c,H,W) tensor of 1 / 2 / 4 channels
    "ps2"            a (B,4,H/2,W/2) tensor read through PixelShuffle(2): one channel
    "c1"             a plain 1-channel source that lives as a batch chunk of a (3B,1,H,W) tensor (chunk 1, then chunk 2)
    "w4"             channels 1..4 of a (B,6,H,W) tensor: the batch stride is larger than C*H*W
`res_layout` is None, a layout, or SAME: the residual is the x sources themselves (what the unit's second AttentionConv does).
Gradients are stated per source, in the source's own shape.

`param_style`: "normal"; "wide" (weights x 4, x x 3: logit spreads beyond fp32's exp range); "uniform" (wq = bq = 0: the softmax
is 1/9 everywhere); "norel" (rel_h = rel_w = 0); "kink" (normal parameters, exact +0.0 / -0.0 planted in x and res).
"""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

import layer_ops_cases as LC
from oracle import fusion_ref as FR

# the kernels' tiles (csrc/attn.hip: AF_TH x AF_TW, AB_TH x AB_TW, the stride of attn_param_reduce_kernel)
FWD_TILE, BWD_TILE, REDUCE_PASS = (16, 32), (6, 30), 256
SAME = "x"
PARAM_KEYS = ("rel_h", "rel_w", "key_conv.weight", "key_conv.bias", "query_conv.weight", "query_conv.bias",
              "value_conv.weight", "value_conv.bias")          # the order of depthcore.ops' parameter tuples
KEY_BIAS = "key_conv.bias"
KEY_BIAS_TOL = 1e-5            # |d key_conv.bias| <= 1e-5 * the case's largest |gradient| (tests/test_fusion_gpu.py)
WIDE_MIN_L = 40.0
_CH = {"p1": 1, "p2": 2, "p4": 4, "ps2": 1, "c1": 1, "w4": 4}

Case = collections.namedtuple("Case", "B C H W x_layout res_layout relu_in relu_res dx_add dres param_style")


def _case(B, C, H, W, x=None, res=None, relu_in=1, relu_res=0, dx_add=0, dres=0, style="normal"):
    x = tuple(x) if x is not None else ("p%d" % C,)
    res = res if res is None or res == SAME else tuple(res)
    assert sum(_CH[k] for k in x) == C and (res in (None, SAME) or sum(_CH[k] for k in res) == C)
    assert not (dres and relu_res and res is None), "dres through a ReLU mask needs the residual"
    return Case(B, C, H, W, x, res, relu_in, relu_res, dx_add, dres, style)


# ---- the table ----------------------------------------------------------------------------------------------------------------
SHAPES = [_case(*s, dx_add=1) for s in [
    (1, 2, 1, 1),          # one pixel: all 8 neighbours are padding
    (1, 4, 1, 33),         # one row, one past the forward tile
    (1, 4, 17, 1),         # one column, one past the forward tile
    (1, 2, 6, 30),         # exactly one backward tile
    (1, 4, 7, 31),         # one past the backward tile in both directions
    (2, 4, 16, 32),        # exactly one forward tile; backward 3 x 2 tiles with ragged last tiles
    (2, 2, 17, 33),        # one past the forward tile in both directions
    (1, 4, 12, 60),        # exact multiples of the backward tile
    (1, 2, 32, 64),        # exact multiples of the forward tile
    (3, 4, 19, 95),        # 4 x 4 backward tiles, 2 x 3 forward tiles, three images: every grid dimension above 2
    (5, 4, 37, 211),       # 7 x 8 x 5 = 280 backward blocks: a second reduction pass with a ragged tail
    (5, 2, 43, 391),       # 8 x 14 x 5 = 560 backward blocks: three passes
]]
DETERMINISM = SHAPES[-1]

PIXEL_SHUFFLE = [
    _case(2, 2, 34, 62, x=["p1", "ps2"], res=SAME, relu_res=1, dres=1),
    _case(2, 2, 34, 62, x=["ps2", "p1"], res=SAME, relu_res=1, dres=1, dx_add=1),          # the first source is pixel-shuffled
    _case(1, 4, 32, 64, x=["ps2"] * 4, res=["ps2"] * 4, relu_res=0, dres=1, dx_add=1),
    _case(2, 4, 18, 36, x=["p1", "ps2", "p2"], res=["w4"], relu_res=1, dres=1),            # res: channels 1..4 of 6
    _case(2, 2, 18, 34, x=["c1", "c1"], dx_add=1),                                         # two chunks of one (3B,1,H,W) tensor
]


def _flag_matrix(B, C, H, W):
    out = []
    for relu_in in (0, 1):
        for res, relu_res in ((None, 0), (("p%d" % C,), 0), (("p%d" % C,), 1)):
            for dx_add in (0, 1):
                for dres in (0, 1):       # without a residual (relu_res = 0) dres is the plain copy of gy
                    out.append(_case(B, C, H, W, res=res, relu_in=relu_in, relu_res=relu_res, dx_add=dx_add, dres=dres))
    return out


FLAG_SHAPES = [(2, 4, 19, 35), (2, 2, 18, 34)]
FLAGS = [c for s in FLAG_SHAPES for c in _flag_matrix(*s)]
KINK = _case(1, 4, 13, 37, res=["p4"], relu_res=1, dx_add=1, dres=1, style="kink")
SOFTMAX = [_case(*s, dx_add=1, style=st) for st in ("wide", "uniform", "norel") for s in ((1, 4, 13, 31), (2, 2, 12, 40))]
CASES = SHAPES + PIXEL_SHUFFLE + FLAGS + [KINK] + SOFTMAX


def case_id(case):
    lay = lambda l: "none" if l is None else "same" if l == SAME else "+".join(l)
    return "%dx%dx%dx%d-x.%s-res.%s-ri%d-rr%d-add%d-dres%d-%s" % (case[:4] + (lay(case.x_layout), lay(case.res_layout)) + case[6:])


def params():
    import pytest
    return [pytest.param(c, id=case_id(c)) for c in CASES]


def ceil_div(a, b):
    return -(-a // b)


def bwd_blocks(case):
    return ceil_div(case.W, BWD_TILE[1]) * ceil_div(case.H, BWD_TILE[0]) * case.B


def param_count(C):
    return 3 * (C * C + C) + 6


def res_layout(case):
    """The residual's layout with SAME resolved (None: no residual)."""
    return case.x_layout if case.res_layout == SAME else case.res_layout


def dres_layout(case):
    """Where dres goes: the residual's layout, or one plain tensor when there is no residual."""
    return res_layout(case) or ("p%d" % case.C,)


def source_shape(kind, B, H, W):
    return (B, 4, H // 2, W // 2) if kind == "ps2" else (B, _CH[kind], H, W)


def gather(layout, srcs):
    """The (B,C,H,W) map a layout stands for."""
    return torch.cat([FR.upscale_ps_shuffle_only(t) if k == "ps2" else t for k, t in zip(layout, srcs)], 1)


# ---- the builder --------------------------------------------------------------------------------------------------------------
def kink_positions(case):
    """(channel, y, x, value) of the planted zeros: corners, the last column, both sides of every backward-tile edge."""
    th, tw = BWD_TILE
    ys = sorted({0, th - 1, th, 2 * th - 1, 2 * th, case.H - 1})
    xs = sorted({0, 1, tw - 1, tw, case.W - 2, case.W - 1})
    return [((i + j) % case.C, y, x, 0.0 if (i + j) % 2 else -0.0) for i, y in enumerate(ys) for j, x in enumerate(xs)]


def _plant(t, case, shift):
    for c, y, x, v in kink_positions(case):
        t[:, (c + shift) % case.C, y, x] = v


def build(case):
    B, C, H, W = case[:4]
    g = torch.Generator().manual_seed(zlib.crc32(repr(("attn", tuple(case))).encode()))
    rn = lambda *shape: torch.randn(*shape, generator=g)
    style = case.param_style
    wscale, xscale = (4.0, 3.0) if style == "wide" else (1.0, 1.0)
    st = {"rel_h": rn(1, 1, 1, 3, 1), "rel_w": rn(1, 1, 1, 1, 3)}
    for n in ("key_conv", "query_conv", "value_conv"):
        st[n + ".weight"] = wscale * rn(C, C, 1, 1)
        st[n + ".bias"] = 0.3 * rn(C)
    if style == "uniform":
        st["query_conv.weight"].zero_(); st["query_conv.bias"].zero_()
    if style == "norel":
        st["rel_h"].zero_(); st["rel_w"].zero_()
    x = [xscale * rn(*source_shape(k, B, H, W)) for k in case.x_layout]
    if case.res_layout == SAME:
        res = [t.clone() for t in x]
    else:
        res = [rn(*source_shape(k, B, H, W)) for k in case.res_layout or ()]
    if style == "kink":
        assert case.x_layout == case.res_layout == ("p%d" % C,)
        _plant(x[0], case, 0)
        _plant(res[0], case, 1)
    inp = {"x": x, "res": res, "params": st, "gy": rn(B, C, H, W), "dx_add": rn(B, C, H, W) if case.dx_add else None}
    to64 = lambda v: None if v is None else v.double() if torch.is_tensor(v) else \
        {k: to64(t) for k, t in v.items()} if isinstance(v, dict) else [to64(t) for t in v]
    return {k: to64(v) for k, v in inp.items()}


# ---- the statement ------------------------------------------------------------------------------------------------------------
def logits(r, st):
    """(B,C,H,W,9) logits and (B,C,H,W,9) value taps of fusion_ref.attention_conv, restated only to measure the logit spread and
    the softmax's underflow (tests/test_attn_cases_cpu.py checks that softmax(logits) . values IS attention_conv's output)."""
    B, C, H, W = r.shape
    conv = lambda n, t: F.conv2d(t, st[n + ".weight"]) + st[n + ".bias"].view(1, C, 1, 1)
    q, rp = conv("query_conv", r), F.pad(r, (1, 1, 1, 1))
    k, v = conv("key_conv", rp), conv("value_conv", rp)
    rh, rw = st["rel_h"].reshape(3), st["rel_w"].reshape(3)
    lg, vt = [], []
    for dy in range(3):
        for dx in range(3):
            rel = torch.cat([rh[dy].expand(C // 2), rw[dx].expand(C - C // 2)]).view(1, C, 1, 1)
            lg.append(q * (k[:, :, dy:dy + H, dx:dx + W] + rel))
            vt.append(v[:, :, dy:dy + H, dx:dx + W])
    return torch.stack(lg, -1), torch.stack(vt, -1)


def _leaf(t, dt):
    return t.detach().to(dt).clone().requires_grad_()


def evaluate(case, inp, dt):
    """Results {name: tensor} and info {"L": largest logit spread, "amin": smallest softmax weight} of the statement in `dt`.
    Names: y; dx.<i> per x source; dres.<i> per residual source (when the case wants dres); the eight parameter keys."""
    xs = [_leaf(t, dt) for t in inp["x"]]
    rs = [_leaf(t, dt) for t in inp["res"]]
    st = {k: _leaf(v, dt) for k, v in inp["params"].items()}
    gy = inp["gy"].to(dt)
    r = gather(case.x_layout, xs)
    if case.relu_in:
        r = F.relu(r)
    y = FR.attention_conv(r, st, "")
    if rs:
        res = gather(res_layout(case), rs)
        y = y + (F.relu(res) if case.relu_res else res)
    want = xs + list(st.values()) + (rs if case.dres and rs else [])
    grads = torch.autograd.grad((y * gy).sum(), want)
    out = {"y": y.detach()}
    add = None if inp["dx_add"] is None else inp["dx_add"].to(dt)
    c0 = 0
    for i, (k, t) in enumerate(zip(case.x_layout, xs)):
        d = grads[i]
        if add is not None:          # dx_add arrives as a (B,C,H,W) map: bring the source's channels into the source's shape
            a = add[:, c0:c0 + _CH[k]]
            d = d + (F.pixel_unshuffle(a, 2) if k == "ps2" else a)
        out["dx.%d" % i] = d
        c0 += _CH[k]
    for k, gr in zip(st, grads[len(xs):len(xs) + len(st)]):
        out[k] = gr
    if case.dres:
        if rs:
            for i, gr in enumerate(grads[len(xs) + len(st):]):
                out["dres.%d" % i] = gr
        else:                        # y = attention_conv(..) + res with res absent: d y / d res is the identity
            out["dres.0"] = gy.clone()
    with torch.no_grad():
        lg, _ = logits(r.detach(), {k: v.detach() for k, v in st.items()})
        info = {"L": float((lg.max(-1).values - lg.min(-1).values).max()), "amin": float(torch.softmax(lg, -1).min())}
    return out, info


@functools.lru_cache(maxsize=None)
def reference(case):
    """(inputs, fp64 results, fp32 results, info) of one case; shared and read-only.  info: L (fp64), amin32, scale = the largest
    |gradient| of the fp64 statement (the yardstick of the key_conv.bias check)."""
    inp = build(case)
    r64, i64 = evaluate(case, inp, torch.float64)
    r32, i32 = evaluate(case, inp, torch.float32)
    scale = max(float(v.abs().max()) for k, v in r64.items() if k != "y")
    info = {"L": i64["L"], "amin32": i32["amin"], "scale": scale}
    if case.param_style == "wide":
        assert info["L"] >= WIDE_MIN_L and info["amin32"] == 0.0, (case_id(case), info)
    return inp, r64, r32, info


def uniform_mean(case, inp):
    """The forward of a "uniform" case stated directly: the plain mean of the 9 value taps, padded ones included (fp64)."""
    r = gather(case.x_layout, inp["x"])
    _, vt = logits(F.relu(r) if case.relu_in else r, inp["params"])
    return vt.mean(-1)


# ---- the gate -----------------------------------------------------------------------------------------------------------------
rel_err = LC.rel_err


def bound(e32, L):
    """rel_err(kernel, fp64) <= gate_bound(e32) + 2 L 2^-24.  The kernel takes exp(x), x = logit - max in [-L, 0], as
    exp2(x log2 e) in fp32: rounding that product moves the result by a relative |x| 2^-24, and the weighted sum and its
    normaliser each carry it."""
    return LC.gate_bound(e32) + 2.0 * L * 2.0 ** -24


def compared(case, r64):
    """The names that go through the gate: everything but key_conv.bias (analytically zero, checked by `key_bias_ok`)."""
    return [k for k in r64 if k != KEY_BIAS]


def key_bias_ok(t, info):
    return float(t.detach().abs().max()) <= KEY_BIAS_TOL * info["scale"]
