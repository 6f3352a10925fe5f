"""Case table, seeded input builder, plain-torch statement and launch-plan transcriptions for ONE BatchNorm-folded Winograd
launch (csrc/wino.hip: dc_wino3x3_fwd_bn / dc_wino3x3_dgrad_bn; csrc/wino_wgrad.hip: dc_wino3x3_wgrad_bn) at the region, group
and mask edges of wino_ps_kernel and wino_wgrad_kernel.  Shared by tests/test_wino_bn_cases_cpu.py (no GPU: the table reaches its
mechanisms, the transcriptions agree with the library's host queries, the cases are well conditioned) and
tests/test_wino_bn_shapes_gpu.py (the kernels against the statement).  DESIGN.md, "The BatchNorm-folded Winograd launches at
their region, group and mask edges", has the table with its reasons, the gates and the measured figures.

    Case                     (kind, B, Ci, Co, H, W, groups, loader, stats, mode, addend)
    build(case)              seeded fp32 inputs whose ReLU decisions are no rounding question (MARGIN), plus planted exact ties
    evaluate(case, inp, dt)  the statement in `dt` (below)
    reference(case)          cached (inputs, fp64 results, fp32 results); nobody may modify what it returns
    mech(case)               what the launch of this case reaches, computed from the transcribed plans

The statement, with g(b) = b // (B / groups) and (s, t) = (in_scale, in_shift), both (groups, channels):
    fwd    a = relu(s[g,c] x + t[g,c]) (loader = 1) or x;  y = conv2d(a, w, padding=1);
           S[g,co] = sum y, Q[g,co] = sum y^2 over the group's images, and the same sums per image (S_img, Q_img)
    dgrad  r = conv2d_input(gy, w) + addend?;  k = [s bn_x + t > 0] (mode 2) or [s bn_x + t + res > 0] (mode 3: the decision
           dc_bn_apply records in its bit mask);  g' = k ? r : 0  (the code adds the addend BEFORE it masks);
           P0[g,ci] = sum g', P1[g,ci] = sum g' (bn_x - mean[g,ci]), and the same per image
    wgrad  dW = conv2d_weight(relu(s x + t), gy)
"""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

import layer_ops_cases as LC

Case = collections.namedtuple("Case", "kind B Ci Co H W groups loader stats mode addend")

MARGIN = 1e-3                 # no pre-activation of a ReLU decision lies in (-MARGIN, MARGIN), planted ties (exactly 0) apart
_PUSH = 1.001e-3              # where a closer one is moved to: a hair beyond, so that rounding the moved element to fp32 keeps it out
TIE = (0.5, 2.0, -1.0)        # x, s, t of a planted tie: s x + t = 0 exactly, in every precision; channel 0 carries (s, t)
TENSOR_TOL = 2e-5             # max|hip - fp64| <= 2e-5 max|fp64|: the bound tests/test_wino_gpu.py holds these kernels to
E32_MAX = 1e-4
EINVAL = -1

# csrc/wino.hip, csrc/weight_cache.h, csrc/wino_wgrad.hip, csrc/conv_bf16.h
PSK = 8                                              # reduction channels per staged chunk (wino_ps_kernel)
PS_REGIONS = [(4, 8), (2, 16), (3, 10), (8, 4)]      # wino_ps_pick_region: 32-tile sub-regions (RH, RW)
WG_REGIONS = [(2, 8), (4, 4), (3, 5)]                # wg_plan: 16-tile sub-regions
WG_KT, WG_SLAB_MR4 = 32, 4 * 4 * 2 * 4 * 3 * 64      # x-side channels per block; floats one MR = 4 block writes
C3B_BC = 32


def _fwd(B, Ci, Co, H, W, groups=1, loader=0, stats=0):
    return Case("fwd", B, Ci, Co, H, W, groups, loader, stats, 0, 0)


def _dgrad(B, Ci, Co, H, W, groups=1, mode=2, addend=0):
    return Case("dgrad", B, Ci, Co, H, W, groups, 0, 0, mode, addend)


def _wgrad(B, Ci, Co, H, W, groups=1):
    return Case("wgrad", B, Ci, Co, H, W, groups, 1, 0, 0, 0)


# ---- the table (DESIGN.md lists what each case is there for; tests/test_wino_bn_cases_cpu.py asserts it from mech()) -------------
FWD = [
    _fwd(2, 8, 16, 8, 16, 1, 1, 1),          # region 4x8 exactly, K = 8: a single chunk
    _fwd(2, 8, 24, 4, 32, 2, 1, 1),          # region 2x16; one image per group; Co = 24 ragged
    _fwd(3, 16, 40, 6, 20, 1, 1, 1),         # region 3x10 (the layer4 map), odd batch, Co = 40
    _fwd(2, 16, 16, 16, 8, 1, 0, 1),         # region 8x4, statistics only
    _fwd(2, 72, 5, 7, 44, 1, 1, 1),          # odd H, K = 72: nine chunks, Co = 5 below one block; hangs over in x
    _fwd(2, 8, 16, 1, 4, 1, 1, 1),           # H = 1: only row 0 of every tile exists
    _fwd(2, 8, 16, 5, 2, 1, 1, 1),           # W = 2, odd H
    _fwd(3, 8, 8, 2, 2, 1, 1, 1),            # one tile: a map smaller than every region
    _fwd(4, 16, 72, 11, 36, 2, 1, 1),        # two groups x two images x several sub-regions, odd H, hangs over in x, Co = 72
    _fwd(4, 16, 24, 11, 36, 2, 1, 0),        # the same map, loader only
    _fwd(4, 16, 24, 11, 36, 2, 0, 1),        # the same map, statistics only
    _fwd(6, 8, 16, 9, 18, 2, 1, 1),          # three images per group, hangs over in both directions
    _fwd(2, 8, 16, 10, 16, 2, 1, 1),         # hangs over in y only
    _fwd(193, 8, 128, 2, 2, 1, 1, 1),        # 32 x 64 tile variant (two sub-regions per block), odd nsub: trailing partial slots
    _fwd(194, 8, 128, 2, 2, 2, 1, 1),        # the same variant, 97 images per group: one block straddles the group boundary
]
DGRAD = [
    _dgrad(2, 16, 8, 8, 16, 1, 2, 0),        # region 4x8, K = 8
    _dgrad(2, 24, 8, 4, 32, 2, 2, 1),        # region 2x16, one image per group, Ci = 24
    _dgrad(3, 40, 16, 6, 20, 1, 2, 1),       # region 3x10, Ci = 40
    _dgrad(2, 16, 16, 16, 8, 1, 3, 0),       # region 8x4, mask with HW = 128 < 256
    _dgrad(2, 5, 72, 7, 44, 1, 3, 1),        # mask with 256 < HW = 308 < 512 and odd H; Ci = 5; K = 72
    _dgrad(2, 5, 72, 7, 44, 1, 2, 1),        # the same through mode 2
    _dgrad(2, 16, 8, 1, 4, 1, 3, 0),         # H = 1, mask with HW = 4
    _dgrad(2, 16, 8, 5, 2, 1, 2, 1),         # W = 2, odd H
    _dgrad(2, 16, 8, 6, 2, 1, 3, 1),         # W = 2 with a mask: HW = 12
    _dgrad(3, 8, 8, 2, 2, 1, 3, 0),          # one tile, HW = 4
    _dgrad(4, 72, 16, 11, 36, 2, 2, 1),      # two groups x two images x several sub-regions, odd H, Ci = 72
    _dgrad(4, 24, 16, 11, 36, 2, 3, 1),      # the same map with a mask: HW = 396
    _dgrad(4, 24, 16, 11, 36, 2, 3, 0),      # ... without the addend
    _dgrad(2, 16, 16, 8, 32, 2, 3, 1),       # mask with HW = 256: exactly one block
    _dgrad(2, 16, 16, 16, 32, 1, 3, 0),      # mask with HW = 512: two blocks (the one shape tests/test_bnfold_gpu.py has)
    _dgrad(6, 16, 8, 9, 18, 2, 2, 0),        # three images per group, hangs over in both directions
    _dgrad(2, 16, 8, 10, 16, 2, 3, 1),       # hangs over in y only; mask with HW = 160
    _dgrad(193, 128, 8, 2, 2, 1, 3, 1),      # 32 x 64 tile variant, odd nsub: trailing partial slots
    _dgrad(194, 128, 8, 2, 2, 2, 2, 0),      # the same variant, a block straddles the group boundary
]
WGRAD = [
    _wgrad(2, 8, 16, 4, 16, 1),              # region 2x8, mr = 2 (16 output channels), one sub-region per image
    _wgrad(2, 16, 64, 8, 8, 2),              # region 4x4, mr = 4 / ng = 1, one image per group
    _wgrad(3, 24, 40, 6, 10, 1),             # region 3x5, mr = 4 with a ragged m-block, K = 24 below one k-block
    _wgrad(3, 40, 72, 6, 30, 1),             # mr = 2 with two m-blocks; 9 sub-regions over 4 splits: a ragged last round
    _wgrad(4, 40, 72, 11, 36, 2),            # odd H, overhang in x, mr = 2, two groups x two images, 16 splits
    _wgrad(6, 72, 128, 7, 44, 2),            # mr = 4 / ng = 1, K = 72: three k-blocks with a ragged last one; three images per group
    _wgrad(8, 128, 256, 12, 40, 2),          # mr = 4 / ng = 2: two 4-wave groups per block, two BatchNorm groups (BNIN 2)
    _wgrad(65, 128, 256, 4, 4, 1),           # ng = 2, 65 sub-regions over 16 splits x 2 groups: a ragged last round (BNIN 1)
    _wgrad(66, 128, 256, 4, 4, 2),           # the same with two BatchNorm groups: the 4-wave groups of a block sit in different ones
    _wgrad(2, 8, 16, 1, 4, 1),               # H = 1
    _wgrad(3, 8, 8, 2, 2, 1),                # one tile
]
CASES = FWD + DGRAD + WGRAD
DETERMINISM = {"fwd": _fwd(4, 16, 72, 11, 36, 2, 1, 1), "dgrad": _dgrad(4, 24, 16, 11, 36, 2, 3, 1), "wgrad": _wgrad(4, 40, 72, 11, 36, 2)}
BATCH_SPLIT = {"fwd": _fwd(3, 16, 40, 6, 20, 1, 1, 1), "dgrad": _dgrad(2, 5, 72, 7, 44, 1, 3, 1)}
PLAIN_WGRAD = _wgrad(4, 40, 72, 11, 36, 2)       # dc_wino3x3_wgrad_bn without a fold is dc_wino3x3_wgrad, bitwise
SPLIT_REDUCTION = (1, 512, 512, 6, 20)           # a shape whose reduction wino_plan splits: no epilogue, no fold


def case_id(c):
    tail = {"fwd": "ld%d-st%d" % (c.loader, c.stats), "dgrad": "m%d-add%d" % (c.mode, c.addend), "wgrad": "ld1"}[c.kind]
    return "%s-%dx%dto%dx%dx%d-g%d-%s" % (c.kind, c.B, c.Ci, c.Co, c.H, c.W, c.groups, tail)


def params(cases):
    import pytest
    return [pytest.param(c, id=case_id(c)) for c in cases]


def ceil_div(a, b):
    return -(-a // b)


# ---- the launch plans, transcribed ------------------------------------------------------------------------------------------------
def _pick(regions, tiles, TH, TW):
    """The candidate of the highest utilisation TH TW / (covered tiles); the first one wins ties (util > best + 1e-9)."""
    best, out = -1.0, None
    for rh, rw in regions:
        util = float(TH * TW) / (float(ceil_div(TH, rh)) * ceil_div(TW, rw) * float(tiles))
        if util > best + 1e-9:
            best, out = util, (rh, rw)
    return out


def ps_region(H, W):
    """wino_ps_pick_region on an H x W output map: (RH, RW) in 2x2 tiles."""
    return _pick(PS_REGIONS, 32, ceil_div(H, 2), W // 2)


def _ps_cost(v, ks, nsub, M, nchunks, nout):
    P, A, Bc = (3.28, 3.51, 4.33), (0.614, 0.598, 0.893), (0.213, 0.460, 0.994)
    bpc, mt, g = (4, 3, 2), (16, 32, 32), (1, 1, 2)
    blocks = ceil_div(nsub, g[v]) * ceil_div(M, mt[v]) * ks
    chunks = ceil_div(nchunks, ks)
    slots = 256 * bpc[v]
    full, rem = blocks // slots, blocks % slots
    t = float(full) * (P[v] + chunks * (A[v] + Bc[v] * bpc[v]))
    if rem:
        t += P[v] + chunks * (A[v] + Bc[v] * float(ceil_div(rem, 256)))
    if ks > 1:
        t += 6.5 + 0.124 * float(nout) * 4.0 * (ks + 1) * 1e-6
    return t


PsPlan = collections.namedtuple("PsPlan", "RH RW regs_x regs_y per_img nsub nchunks MT G ksplit")


def ps_plan(B, K, M, H, W):
    """wino_plan: sub-region shape, tile variant (MT output channels x G sub-regions per block) and reduction split of a
    wino_ps_kernel launch with K reduction and M output channels."""
    RH, RW = ps_region(H, W)
    regs_x, regs_y = ceil_div(W // 2, RW), ceil_div(ceil_div(H, 2), RH)
    nsub, nchunks, nout = regs_x * regs_y * B, ceil_div(K, PSK), B * M * H * W
    cap = (8 if nout * 4 <= (2 << 20) else 2) if (H * W) % 4 == 0 and nchunks >= 2 else 1
    best, pick = 1e30, (32, 2, 1)
    for v in range(3):
        ks = 1
        while ks <= cap:
            if ks > 1 and nchunks < 2 * ks:
                break
            t = _ps_cost(v, ks, nsub, M, nchunks, nout)
            if t < best:
                best, pick = t, (16 if v == 0 else 32, 2 if v == 2 else 1, ks)
            ks *= 2
    return PsPlan(RH, RW, regs_x, regs_y, regs_x * regs_y, nsub, nchunks, *pick)


WgPlan = collections.namedtuple("WgPlan", "RH RW regs_x regs_y per_img nsub mr ng mblocks kblocks splits ws_bytes")


def wg_plan(B, Ci, Co, H, W):
    """wg_plan of csrc/wino_wgrad.hip: region, channel tile (mr), 4-wave groups per block (ng), reduction splits, workspace."""
    RH, RW = _pick(WG_REGIONS, 16, ceil_div(H, 2), W // 2)
    regs_x, regs_y = ceil_div(W // 2, RW), ceil_div(ceil_div(H, 2), RH)
    nsub = regs_x * regs_y * B
    mr = 2 if (Co % 64 != 0 and Co % 64 <= 32) else 4
    mblocks, kblocks = ceil_div(Co, 16 * mr), ceil_div(Ci, WG_KT)
    nmk = mblocks * kblocks
    ng = 2 if (mr == 4 and nsub >= 4 * ceil_div(256, nmk)) else 1
    target = 768 if (mr == 2 and nsub >= 4096) else 512 // ng
    splits = max(1, min(max(1, nsub // (2 * ng)), ceil_div(target, nmk)))
    ws = splits * nmk * (WG_SLAB_MR4 // 4 * mr) * 4
    return WgPlan(RH, RW, regs_x, regs_y, regs_x * regs_y, nsub, mr, ng, mblocks, kblocks, splits, ws)


def wgrad_bf16_bytes(B, Ci, Co, H, W):
    """The other term of dc_wino3x3_wgrad_workspace (it sizes for the bf16 policy's weight gradient too): c3b_wgrad_split slabs."""
    ntiles = ceil_div(W, 32) * ceil_div(H, 8) * B
    outer = ceil_div(Co, 64) * ceil_div(Ci, C3B_BC)
    return min(max(1, min(ntiles, 512 // max(outer, 1))), 256) * Co * Ci * 9 * 4


def conv_dims(c):
    """(K, M) of the wino_ps_kernel launch of a fwd / dgrad case: the data gradient reduces over Co and writes Ci channels."""
    return (c.Co, c.Ci) if c.kind == "dgrad" else (c.Ci, c.Co)


def mech(c):
    """What the launch reaches, from the transcriptions alone."""
    TH, TW = ceil_div(c.H, 2), c.W // 2
    m = {"odd_H": c.H % 2 == 1, "HW": c.H * c.W, "npg": c.B // c.groups}
    if c.kind == "wgrad":
        p = wg_plan(c.B, c.Ci, c.Co, c.H, c.W)
        m.update(plan=p, ragged_round=p.splits > 1 and p.nsub % (2 * p.ng * p.splits) != 0, bnin=c.groups)
    else:
        K, M = conv_dims(c)
        p = ps_plan(c.B, K, M, c.H, c.W)
        m.update(plan=p, K=K, M=M, ragged_M=M % 16 != 0 and M % 32 != 0, nparts=2 * ceil_div(p.nsub, p.G) * p.G,
                 ppg=2 * p.per_img * (c.B // c.groups))
        m["trailing"] = m["nparts"] > 2 * p.nsub
        # a two-sub-region block whose halves lie in different BatchNorm groups
        m["straddles_groups"] = p.G == 2 and c.groups == 2 and (p.per_img * (c.B // 2)) % 2 == 1
    m.update(hang_x=p.regs_x * p.RW > TW, hang_y=p.regs_y * p.RH > TH, sub_region=TH < p.RH and TW < p.RW)
    return m


# ---- the builder ------------------------------------------------------------------------------------------------------------------
def tie_positions(c):
    """(b, y, x) of the planted ties, all in channel 0: the corners of the first and the last image, and -- odd H: the row that
    only has a row 0 in its tile -- the middle of the last row."""
    H, W, B = c.H, c.W, c.B
    pos = {(0, 0, 0), (0, 0, W - 1), (B - 1, H - 1, 0), (B - 1, H - 1, W - 1), (B - 1, H - 1, W // 2), (B // 2, H // 2, W // 2)}
    return sorted(pos)


def _scale_shift(groups, C, g):
    s = torch.rand(groups, C, generator=g) + 0.5
    t = 0.3 * torch.randn(groups, C, generator=g)
    s[:, 0], t[:, 0] = TIE[1], TIE[2]
    return s, t


def _group_of(c):
    return torch.arange(c.B) // (c.B // c.groups)


def preact(c, x, s, t, res=None):
    """fp64 pre-activation s[g(b), ch] x + t[g(b), ch] (+ res) of the fp32 inputs."""
    gi = _group_of(c)
    p = s.double()[gi][:, :, None, None] * x.double() + t.double()[gi][:, :, None, None]
    return p if res is None else p + res.double()


def _clear_margin(c, x, s, t, res=None):
    """Move every element of x whose pre-activation lies within MARGIN of zero out to +-_PUSH, then plant the ties."""
    gi = _group_of(c)
    p = preact(c, x, s, t, res)
    near = p.abs() < MARGIN
    target = torch.where(p >= 0, _PUSH, -_PUSH).double() - t.double()[gi][:, :, None, None]
    if res is not None:
        target = target - res.double()
    moved = (target / s.double()[gi][:, :, None, None]).float()
    x = torch.where(near, moved, x)
    for b, yy, xx in tie_positions(c):
        x[b, 0, yy, xx] = TIE[0]
        if res is not None:
            res[b, 0, yy, xx] = 0.0
    return x


def tie_mask(c, C):
    m = torch.zeros(c.B, C, c.H, c.W, dtype=torch.bool)
    for b, yy, xx in tie_positions(c):
        m[b, 0, yy, xx] = True
    return m


def build(c, ksize=3, tag="wino_bn"):
    """fp32 inputs of one case (a dict of CPU tensors; absent operands are None).  ksize, tag: the kernel size and the seed's name
    (tests/pointwise_bn_cases.py builds the 1x1 cases with the same builder)."""
    B, Ci, Co, H, W = c.B, c.Ci, c.Co, c.H, c.W
    g = torch.Generator().manual_seed(zlib.crc32(repr((tag, tuple(c))).encode()))
    rn = lambda *shape: torch.randn(*shape, generator=g)
    inp = {"w": rn(Co, Ci, ksize, ksize) * (2.0 / (ksize * ksize * Ci)) ** 0.5, "x": None, "gy": None, "s": None, "t": None, "bn_x": None,
           "mean": None, "res": None, "addend": None}
    if c.kind in ("fwd", "wgrad"):
        inp["x"] = rn(B, Ci, H, W)
        if c.loader:
            inp["s"], inp["t"] = _scale_shift(c.groups, Ci, g)
            inp["x"] = _clear_margin(c, inp["x"], inp["s"], inp["t"])
    if c.kind in ("dgrad", "wgrad"):
        inp["gy"] = rn(B, Co, H, W)
    if c.kind == "dgrad":
        inp["bn_x"] = rn(B, Ci, H, W)
        inp["mean"] = 0.2 * rn(c.groups, Ci)
        inp["s"], inp["t"] = _scale_shift(c.groups, Ci, g)
        if c.mode == 3:
            inp["res"] = 0.5 * rn(B, Ci, H, W)
        if c.addend:
            inp["addend"] = rn(B, Ci, H, W)
        inp["bn_x"] = _clear_margin(c, inp["bn_x"], inp["s"], inp["t"], inp["res"])
    return inp


def decision_preact(c, inp):
    """fp64 pre-activation of the case's ReLU decisions, or None (a forward without the loader fold)."""
    if c.kind == "dgrad":
        return preact(c, inp["bn_x"], inp["s"], inp["t"], inp["res"])
    return preact(c, inp["x"], inp["s"], inp["t"]) if c.loader else None


# ---- the statement ----------------------------------------------------------------------------------------------------------------
def _per_group(c, per_img):
    return per_img.view(c.groups, c.B // c.groups, -1).sum(1)


def evaluate(c, inp, dt, padding=1):
    """{name: tensor} of the statement in `dt` (padding = 1: the 3x3 convolution; 0 with 1x1 weights: tests/pointwise_bn_cases.py)."""
    to = lambda k: None if inp[k] is None else inp[k].to(dt)
    gi = _group_of(c)
    w = to("w")
    bc = lambda v: v[gi][:, :, None, None]
    if c.kind in ("fwd", "wgrad"):
        a = to("x")
        if c.loader:
            a = F.relu(bc(to("s")) * a + bc(to("t")))
        if c.kind == "wgrad":
            return {"dW": torch.nn.grad.conv2d_weight(a, w.shape, to("gy"), padding=padding)}
        y = F.conv2d(a, w, padding=padding)
        s_img, q_img = y.sum((2, 3)), (y * y).sum((2, 3))
        return {"y": y, "S_img": s_img, "Q_img": q_img, "S": _per_group(c, s_img), "Q": _per_group(c, q_img)}
    r = torch.nn.grad.conv2d_input((c.B, c.Ci, c.H, c.W), w, to("gy"), padding=padding)
    if c.addend:
        r = r + to("addend")
    bx = to("bn_x")
    pre = bc(to("s")) * bx + bc(to("t"))
    if c.mode == 3:
        pre = pre + to("res")
    keep = pre > 0
    gx = torch.where(keep, r, torch.zeros_like(r))
    p0_img, p1_img = gx.sum((2, 3)), (gx * (bx - bc(to("mean")))).sum((2, 3))
    return {"gx": gx, "r": r, "keep": keep, "P0_img": p0_img, "P1_img": p1_img, "P0": _per_group(c, p0_img), "P1": _per_group(c, p1_img)}


@functools.lru_cache(maxsize=None)
def reference(c):
    """(inputs, fp64 results, fp32 results) of one case; shared and read-only."""
    inp = build(c)
    return inp, evaluate(c, inp, torch.float64), evaluate(c, inp, torch.float32)


rel_err = LC.rel_err
TENSORS = {"fwd": "y", "dgrad": "gx", "wgrad": "dW"}


def assert_well_conditioned(case, inp, r64, r32):
    """The case is fit to judge a kernel with: finite, torch's fp32 evaluation of the statement within E32_MAX of fp64, no ReLU
    decision a rounding question (MARGIN), the planted ties exactly zero and "off" in both precisions.  (Shared with
    tests/test_pointwise_bn_cases_cpu.py.)"""
    name = TENSORS[case.kind]
    for k, v in r64.items():
        assert bool(torch.isfinite(v.double()).all()) and bool(torch.isfinite(r32[k].double()).all()), k
    e32 = rel_err(r32[name], r64[name])
    assert e32 < E32_MAX, e32
    assert float(r64[name].abs().max()) > 0.1
    pre = decision_preact(case, inp)
    if pre is None:
        return
    # the decision margin: nothing within MARGIN of zero but the planted ties, which are exactly zero
    ties = tie_mask(case, pre.shape[1])
    assert int(ties.sum()) >= (2 if case.H * case.W > 1 else 1)
    assert bool((pre[ties] == 0).all())
    assert bool((pre[~ties].abs() >= MARGIN).all()), float(pre[~ties].abs().min())
    # a tie is "off": torch's ReLU and the kernels' `> 0` agree, in both precisions
    pre32 = preact(case, *[inp[k] for k in (("bn_x", "s", "t", "res") if case.kind == "dgrad" else ("x", "s", "t"))]).float()
    assert bool((pre32[ties] == 0).all()) and not bool((pre32[ties] > 0).any()) and bool((torch.relu(pre32[ties]) == 0).all())
    if case.kind == "dgrad":
        for r in (r64, r32):
            assert not bool(r["keep"][ties].any()) and bool((r["gx"][ties] == 0).all())
        assert bool((r64["keep"] == r32["keep"]).all())
        assert 0.2 < float(r64["keep"].double().mean()) < 0.8
        # the tie matters: the unmasked gradient there is not zero, so `>=` for `>` would show
        assert float(r64["r"][ties].abs().min()) > 1e-3 * float(r64["gx"].abs().max())
    if case.kind == "dgrad" and case.mode == 3:
        assert bool((inp["res"][ties] == 0).all())
        # the residual takes part in the decision: it differs from the decision without it somewhere
        assert bool(((preact(case, inp["bn_x"], inp["s"], inp["t"]) > 0) != r64["keep"]).any())


# ---- the gates --------------------------------------------------------------------------------------------------------------------
def sum_bound(n, abs_sum):
    """Worst case of an fp32 sum of n terms in any order, each term itself one rounded fp32 operation: (n + 2) 2^-24 sum|term|."""
    return (n + 2) * 2.0 ** -24 * abs_sum


def stat_bounds(n, delta, abs_y_sum):
    """How far the sums of a tensor that is within delta of the statement's may be from the statement's sums over n elements:
    n delta for sum y; delta (2 sum|y| + n delta) for sum y^2 (|y'^2 - y^2| = |y' - y| |y' + y|)."""
    return n * delta, delta * (2.0 * abs_y_sum + n * delta)


def host_lib():
    from depthcore import _lib
    return _lib.lib()


def parts_query(c):
    """(nparts, ppg) from the library for a fwd / dgrad case."""
    import ctypes
    ppg = ctypes.c_int(0)
    fn = host_lib().dc_wino3x3_bwd_parts if c.kind == "dgrad" else host_lib().dc_wino3x3_stat_parts
    n = fn(c.B, c.Ci, c.Co, c.H, c.W, c.groups, ctypes.byref(ppg))
    return n, ppg.value


assert TIE[0] * TIE[1] + TIE[2] == 0.0
