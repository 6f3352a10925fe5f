"""Case tables, the bf16 plan transcribed from the host code, the rounded-operand fp64 statement, launchers and gates for the bf16
matrix-core 3x3 convolutions (csrc/conv_bf16.hip: c3b_conv_kernel<MR, S, DPAD>, c3b_wgrad_kernel<S>) at the edges of their staging
and of their tiles: the weight gradient's tile walk, channel raggedness in the patch stager, the reflected overhang column, the
padded-domain data gradient, the hybrids the plan produces below 16 output channels, the null-pointer patterns and the stride-2
instantiations.  Shared by tests/test_conv_bf16_cases_cpu.py (no GPU: route() agrees with the library's plans under the policy, the
tables reach every mechanism, the rounding is visible, a single wrong tap or channel is seen, the rows are well conditioned) and
tests/test_conv_bf16_shapes_gpu.py (the kernels against the statement).  DESIGN.md, "The bf16 convolutions at their staging and tile
edges", has the tables with their reasons, the predicates, the gates and the measured figures.

    BLOCK / BLOCK_NULLS / HEAD_FIRST    conv_block_cases.Case rows: one dc_conv3x3_fwd + one dc_conv3x3_bwd_add under DC_PREC_BF16
    TRUNK                               (B, Ci, Co, H, W, addend): dc_wino3x3_fwd, _dgrad / _dgrad_add, _wgrad under DC_PREC_BF16
    S2                                  convs2_cases.Case rows (k = 3): dc_convs2_fwd / _wgrad / _dgrad under DC_PREC_BF16
    route(case)                         the plan and the geometry the kernels derive, transcribed (never asks the library)
    evaluate(case, inp, rounded, dt)    the statement: operands rounded to bf16 (rounded) or left as they are, evaluated in `dt`
    launch(case, inp) / gate(...)       the launches between guards under the policy; the project's gates for this contract

The contract is exact: operands rounded to bf16 (nearest even), products exact in fp32, fp32 sums.  What is left between a correct
kernel and the fp64 statement on the SAME rounded operands is fp32 summation order, so a wrong tap, channel or column cannot hide
behind a "bf16 tolerance".  With rb(t) = t.to(bfloat16).double(), u = nearest x2 upsample or identity, P = the padding:
    forward   y = act(conv2d(P(cat(u(rb x0), rb x1)), rb w) + b)
    backward  g' = gy act'(y_given) formed in fp32 (the expression of conv_block_cases.act_prime; tanh: 1 - y^2 with ONE rounding --
              the compiled kernels evaluate it as fma(-y, y, 1), which is the correctly rounded value); data gradient and bf16 weight
              gradient on rb(g'); bias gradient = the sum of the unrounded fp32 g'; a DW_DIRECT weight gradient (Co < 16: the fp32
              direct kernel fed by conv_gprime_kernel) on unrounded operands; the addends as conv_block_cases.evaluate has them
    stride 2 and trunk: the same with stride = 2 / padding = 1, no activation, no bias."""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

import conv_block_cases as CC
import convs2_cases as S
from conv_block_cases import ALL, REFLECT, ZERO, K
from helpers import rel_l2

NONE, ELU, SIGMOID, RELU, TANH = CC.ACT_NONE, CC.ACT_ELU, CC.ACT_SIGMOID, CC.ACT_RELU, CC.ACT_TANH
PREC_F32, PREC_BF16 = 0, 1                      # include/depthcore.h: DC_PREC_*
Y_GATE, G_GATE = 2e-6, 5e-6                     # rel-L2 against the rounded-operand fp64 statement (tests/test_conv_bf16_gpu.py)
VISIBLE, SENSITIVITY, CONDITION = 100.0, 10.0, 0.25
BC, TW = CC.C3B_BC, 32                          # csrc/conv_bf16.hip: reduction channels per chunk, tile width
B16_DW_MIN = 16                                 # csrc/conv3x3.hip: conv_plan (DC_B16_DW_MIN unset)

Trunk = collections.namedtuple("Trunk", "B Ci Co H W addend")
ceil_div = CC.ceil_div
bits = CC.bits

# ---- the tables ---------------------------------------------------------------------------------------------------------------------
BLOCK = [
    K(3, 16, 0, 0, 16, 88, 260, ELU, REFLECT),            # split 256, 297 tiles: the weight gradient's walk with refl_over
    K(3, 32, 1, 16, 16, 88, 264, ELU, REFLECT),           # the walk with up0 plus a ragged x1 chunk, two channel blocks
    K(2, 40, 0, 0, 1, 8, 12, SIGMOID, REFLECT),           # M = 1 forward, K = 1 padded data gradient, DW_DIRECT
    K(1, 5, 0, 0, 7, 2, 4, NONE, ZERO),                   # odd K, H = 2, W = 4, GP_GY
    K(2, 32, 0, 8, 40, 9, 36, ELU, REFLECT, add0=1, add1="separate"),    # C1 = 8 behind a full chunk, Co = 40 in an MR = 4 block, W = 36, odd H, fold, both addends
    K(2, 24, 0, 0, 72, 10, 68, TANH, ZERO, add0=1),       # two m-blocks, the second ragged; W = 68; direct DX_BF16 with the addend on an overhanging tile
    K(1, 16, 1, 0, 24, 6, 40, ELU, REFLECT),              # up0 with xx + 8 == W; H + 2 = 8 fills exactly one padded tile row
    K(1, 16, 0, 0, 8, 8, 32, RELU, ZERO),                 # W = 32: the edge-column path, padded width 34, Co < 16, ReLU ties
    K(1, 16, 0, 0, 16, 8, 12, ELU, REFLECT),              # W = 12: three inside quads, refl_over in the only tile; Co = 16 exactly
    K(1, 8, 0, 0, 16, 8, 28, SIGMOID, REFLECT),           # W = 28: seven inside quads; K = 8
    K(1, 16, 1, 0, 16, 4, 8, ELU, REFLECT),               # W = 8 with up0: the half-resolution row is one quad, xx + 8 == W in quad 0
    K(1, 16, 0, 0, 16, 8, 32, ELU, REFLECT),              # W = 32 reflect: column W comes from the edge-column load, no refl_over
    K(1, 16, 0, 0, 16, 8, 64, RELU, REFLECT),             # W = 64 reflect: the edge column of tile 0 is an interior column
    K(1, 40, 0, 0, 24, 8, 16, ELU, ZERO),                 # Cin = 40 single source: M = 40 in the direct data gradient (MR = 4, ragged)
    K(1, 24, 0, 0, 32, 8, 16, ELU, REFLECT),              # Co = 32 exactly: a full MR = 2 block; M = 24 in the padded data gradient (MR = 2, ragged)
    K(1, 16, 0, 0, 17, 8, 16, SIGMOID, ZERO),             # Co = 17: one row in the second half of the MR = 2 block
    K(1, 64, 1, 32, 16, 8, 16, ELU, REFLECT, add1="inplace"),            # C0 = 64 upsampled, C1 = 32: three chunks, the last from x1; dx1 in place
    K(1, 16, 0, 0, 16, 8, 16, NONE, ZERO, bias=0),        # no bias, no activation: db alone from the g' pass
    K(1, 16, 0, 0, 16, 2, 8, ELU, REFLECT),               # H = 2 under reflection: every row of the padded domain (4 rows) is on the border
]
_NULL_PATTERNS = (("x0",), ("x1",), ("x0", "x1"), ("w",), ("b",), ("w", "b"))
NULL_FAMILIES = {
    "reflect-concat": K(2, 32, 1, 16, 16, 8, 16, ELU, REFLECT),
    "zero": K(2, 16, 0, 0, 16, 8, 16, ELU, ZERO),
}
BLOCK_NULLS = []
for _base in NULL_FAMILIES.values():
    for _g in _NULL_PATTERNS:
        _c = K(*_base[:10], grads=_g)
        if _c.grads and _c not in BLOCK_NULLS:            # (a single-source block has no x1: that pattern is empty there)
            BLOCK_NULLS.append(_c)
# the head-first rule: a single-channel head keeps its fp32 plain-FMA kernels under the policy (the plan is its fp32 plan)
HEAD_FIRST = [K(2, 16, 0, 0, 1, 12, 28, ELU, ZERO)]
BLOCK_ALL = BLOCK + list(NULL_FAMILIES.values()) + BLOCK_NULLS

TRUNK = [
    Trunk(2, 24, 40, 9, 36, 1),         # ragged chunk and ragged MR = 4 block, odd H, one-quad overhang; the addend in the store epilogue
    Trunk(1, 64, 64, 8, 32, 0),         # two full chunks, MR = 4 both ways, W = 32 exactly
    Trunk(2, 16, 16, 2, 4, 0),          # H = 2, W = 4: one quad, every row on the border
    Trunk(1, 7, 5, 10, 68, 0),          # odd Ci and odd Co: the channel-pair guard in both passes; three tiles in x, two in y
    Trunk(3, 16, 16, 88, 260, 0),       # the weight gradient's walk with zero padding
]

S2 = [
    S.K(3, 8, 16, 88, 520, 3),          # walk: 297 tiles on 256 blocks, no data gradient
    S.K(1, 40, 64, 2, 8, 3),            # OH = 1, OW = 4, ragged chunk, dilated data gradient
    S.K(1, 5, 7, 4, 8, 3),              # odd Ci, Co = 7
    S.K(2, 64, 128, 10, 72, 3),         # OH = 5, OW = 36, data gradient with two tiles
    S.K(3, 8, 32, 688, 8, 3),           # a walk that has a data gradient: 258 one-quad tiles (OW = 4) on 256 blocks, 86 tile rows in the dilated data gradient
]
S2 += [c for c in S.TRIP + S.GATHER3 if c not in S2 and c.B * c.Co * (c.H // 2) * (c.W // 2) < 10 ** 5]
WALK = {"block": BLOCK[0], "block-up0": BLOCK[1], "trunk": TRUNK[4], "s2": S2[0], "s2-dx": S2[4]}


def kind(c):
    return "block" if isinstance(c, CC.Case) else ("trunk" if isinstance(c, Trunk) else "s2")


def case_id(c):
    if kind(c) == "block":
        return CC.case_id(c)
    if kind(c) == "trunk":
        return "trunk-b%d-%dto%d-%dx%d-add%d" % tuple(c)
    return "s2-" + S.case_id(c)


def params(cases):
    import pytest
    return [pytest.param(c, id=case_id(c)) for c in cases]


# ---- the plan and the geometry, transcribed (csrc/conv_bf16.hip, csrc/conv3x3.hip: conv_plan, csrc/wino.hip, csrc/convgemm.hip) ----
def c3b_eligible(C0, C1, up0, H, W, stride=1):
    if stride == 1:
        return W % 4 == 0 and W >= 4 and H >= 2 and (C1 == 0 or C0 % BC == 0) and (not up0 or (W % 8 == 0 and H % 2 == 0))
    return stride == 2 and W % 8 == 0 and H % 2 == 0 and C1 == 0 and not up0


def c3b_wgrad_split(B, OH, OW, Co, Cin, stride=1):
    ntiles = ceil_div(OW, TW) * ceil_div(OH, 8 if stride == 1 else 4) * B
    outer = ceil_div(Co, 64) * ceil_div(Cin, BC)
    return min(max(1, min(ntiles, 512 // max(outer, 1))), 256)


def c3b_dpad_pitch(W):
    return (W + 2 + 3) & ~3


def conv_geometry(M, Kred, OH, OW, TH=8):
    """One c3b_conv_kernel launch: M output rows, Kred reduction channels, OH x OW output maps."""
    mr = CC.pick_mr(M)
    return {"M": M, "K": Kred, "mr": mr, "mblocks": ceil_div(M, 16 * mr), "ragged_m": M % (16 * mr) != 0, "chunks": ceil_div(Kred, BC),
            "tiles_x": ceil_div(OW, TW), "tiles_y": ceil_div(OH, TH), "OH": OH, "OW": OW, "overhang": OW % TW != 0,
            "last_quads": ((OW - 1) % TW) // 4 + 1, "ragged_y": OH % TH != 0}


def wgrad_geometry(B, OH, OW, Co, Cin, stride=1):
    """One c3b_wgrad_kernel launch: block i of `split` walks tiles i, i + split, ...; which blocks meet the overhanging tile (the
    last in x where OW % 32 != 0) first and which meet it second, and whether a block's two tiles lie in different images."""
    TH = 8 if stride == 1 else 4
    tx, ty = ceil_div(OW, TW), ceil_div(OH, TH)
    ntiles, split = tx * ty * B, c3b_wgrad_split(B, OH, OW, Co, Cin, stride)
    over = lambda t: OW % TW != 0 and (t % (tx * ty)) % tx == tx - 1
    walkers = range(max(0, ntiles - split)) if ntiles <= 2 * split else range(split)
    return {"ntiles": ntiles, "split": split, "per_block": ceil_div(ntiles, split), "walkers": len(walkers), "tiles_x": tx, "tiles_y": ty,
            "over_first": any(over(t) and not over(t + split) for t in walkers),
            "over_second": any(over(t + split) and not over(t) for t in walkers),
            "cross_image": any(t // (tx * ty) != (t + split) // (tx * ty) for t in walkers),
            "outer": (ceil_div(Co, 64), ceil_div(Cin, BC)), "ragged_co": Co % 64 != 0, "ragged_ci": Cin % BC != 0}


def sources(C0, C1):
    """Channel raggedness of the two staged sources: (K of the source, its last chunk's channel count) for x0 and x1."""
    return {"k0": C0, "k1": C1, "rag0": C0 % BC, "rag1": C1 % BC}


def block_plan(c, grads=None):
    """dc_conv3x3_plan of a block under DC_PREC_BF16, field by field, for the request `grads` (default: the case's)."""
    grads = c.grads if grads is None else tuple(g for g in ALL if g in grads)
    B, C0, up0, C1, Co, H, W, act, pad = c[:9]
    if not c3b_eligible(C0, C1, up0, H, W):
        return CC.plan_of(CC.route(c._replace(grads=grads)))
    Cin, HW = C0 + C1, H * W
    want_dx0, dx_any = "x0" in grads, "x0" in grads or "x1" in grads
    want_w, want_b = "w" in grads, "b" in grads
    dw_any = want_w or want_b
    head = CC.head_eligible(C0, C1, up0, Co, H, W)                    # the heads come first: plain FMAs in fp32
    b16_dw = Co >= B16_DW_MIN
    fused_db = want_b and b16_dw and HW % 4 == 0
    fast = W % 16 == 0 and (C1 == 0 or C0 % CC.CK == 0) and (C1 == 0 or C0 % CC.CW == 0)
    head_dx = want_dx0 and head
    head_dw = (dw_any and head and C0 in (16, 32) and HW % 4 == 0 and
               B * ceil_div(HW, CC.DWP) * (C0 * 9 + 1) * 4 <= CC.al256(B * Cin * (H + 2) * (W + 5) * 4))
    p = dict(fwd=CC.FWD_HEAD if head else CC.FWD_BF16, fwd_v2=0, fwd_mr=0, ring=0, bwd_v2=int(fast), dx_mr=0, dw_mr=0, split=0)
    if (head_dx or not dx_any) and (head_dw or not dw_any):
        p["gprime"] = CC.GP_UNUSED
    elif fused_db:
        p["gprime"] = CC.GP_DBIAS_KERNEL
    else:                                                             # (W % 4 == 0: whole float4s, conv_gprime_kernel always fits)
        p["gprime"] = CC.GP_KERNEL if act != NONE else CC.GP_GY
    p["dx"] = CC.DX_HEAD if head_dx else (CC.DX_NONE if not dx_any else
                                          (CC.DX_BF16 if pad == ZERO and not up0 and C1 == 0 else CC.DX_BF16_FOLD))
    p["dw"], p["db"] = CC.DW_NONE, CC.DB_NONE
    if head_dw:
        p["dw"], p["db"] = CC.DW_HEAD, CC.DB_SLABS if want_b else CC.DB_NONE
    elif b16_dw and dw_any:
        p["dw"] = CC.DW_BF16 if want_w else CC.DW_NONE
        p["db"] = CC.DB_GPRIME if fused_db else (CC.DB_KERNEL if want_b else CC.DB_NONE)
        p["split"] = c3b_wgrad_split(B, H, W, Co, Cin) if want_w else 0
    elif dw_any:
        p.update(dw=CC.DW_DIRECT, db=CC.DB_SLABS if want_b else CC.DB_NONE, dw_mr=CC.pick_mr_w(Co), split=CC.pick_split(B, H, W, Co, Cin))
    return p


def route(c, grads=None):
    """The plan (block and stride-2 rows: the fields of the library's plan struct) and the geometry of every bf16 launch of the row:
    fwd / dx / dw are conv_geometry / wgrad_geometry dicts or None where that pass is not a bf16 kernel."""
    k = kind(c)
    r = {"kind": k, "fwd": None, "dx": None, "dxpad": None, "dw": None, "stride": 1}
    if k == "block":
        p = block_plan(c, grads)
        Cin = c.C0 + c.C1
        r.update(plan=p, src=sources(c.C0, c.C1), up0=c.up0, pad=c.pad, W=c.W, H=c.H)
        if p["fwd"] == CC.FWD_BF16:
            r["fwd"] = conv_geometry(c.Co, Cin, c.H, c.W)
        if p["dx"] == CC.DX_BF16:
            r["dx"] = conv_geometry(Cin, c.Co, c.H, c.W)
        if p["dx"] == CC.DX_BF16_FOLD:
            r["dxpad"] = dict(conv_geometry(Cin, c.Co, c.H + 2, c.W + 2), pitch=c3b_dpad_pitch(c.W))
        if p["dw"] == CC.DW_BF16:
            r["dw"] = wgrad_geometry(c.B, c.H, c.W, c.Co, Cin)
            assert r["dw"]["split"] == p["split"]
    elif k == "trunk":
        assert c3b_eligible(c.Ci, 0, 0, c.H, c.W) and c3b_eligible(c.Co, 0, 0, c.H, c.W)
        r.update(src=sources(c.Ci, 0), up0=0, pad=ZERO, W=c.W, H=c.H, fwd=conv_geometry(c.Co, c.Ci, c.H, c.W),
                 dx=conv_geometry(c.Ci, c.Co, c.H, c.W), dw=wgrad_geometry(c.B, c.H, c.W, c.Co, c.Ci))
    else:
        s = S.route(c, bf16=True)
        assert s is not None and c.k == 3 and c3b_eligible(c.Ci, 0, 0, c.H, c.W, 2)
        OH, OW = c.H // 2, c.W // 2
        r.update(plan=S.plan_of(s), s2=s, src=sources(c.Ci, 0), up0=0, pad=ZERO, W=c.W, H=c.H, stride=2,
                 fwd=conv_geometry(c.Co, c.Ci, OH, OW, 4), dw=wgrad_geometry(c.B, OH, OW, c.Co, c.Ci, 2))
        if s["dx"] == "bf16":          # the stride-1 kernel over the dilated g' (up0 = 3): W % 8 == 0 and even H hold for every stride-2 shape
            assert c3b_eligible(c.Co, 0, 1, c.H, c.W)
            r["dx"] = dict(conv_geometry(c.Ci, c.Co, c.H, c.W), dilated=True)
    return r


def dw_is_bf16(c):
    return kind(c) != "block" or block_plan(c, ALL)["dw"] == CC.DW_BF16


def is_head(c):
    return kind(c) == "block" and block_plan(c, ALL)["fwd"] == CC.FWD_HEAD


def output_kernels(c):
    """What decides each backward output's bits of a block row, as far as the plan names it (the null-pattern comparison's key).  g'
    is the same expression in conv_gprime_kernel and conv_gprime_dbias_kernel: which of the two formed it is not part of the key."""
    p = block_plan(c)
    return {"dx0": (p["dx"],), "dx1": (p["dx"],), "dw": (p["dw"], p["split"], p["dw_mr"], p["bwd_v2"]),
            "db": (p["db"], p["split"] if p["db"] == CC.DB_SLABS else 0)}


# ---- inputs and the statement -------------------------------------------------------------------------------------------------------
def rb(t):
    return t.to(torch.bfloat16).double()


def _seed(c):
    return zlib.crc32(repr(("conv_bf16", kind(c), tuple(c))).encode())


def build(c):
    """fp32 inputs of one row (CPU tensors).  Block rows: conv_block_cases.build (with its planted ties and the backward's given y);
    stride-2 rows: convs2_cases.build; trunk rows: x, w scaled by (9 Ci)^-1/2, gy and an addend."""
    if kind(c) == "block":
        return CC.build(c)
    if kind(c) == "s2":
        return S.build(c)
    g = torch.Generator().manual_seed(_seed(c))
    rn = lambda *shape: torch.randn(*shape, generator=g)
    return {"x": rn(c.B, c.Ci, c.H, c.W), "w": rn(c.Co, c.Ci, 3, 3) * (1.0 / (9 * c.Ci)) ** 0.5, "gy": rn(c.B, c.Co, c.H, c.W),
            "add": rn(c.B, c.Ci, c.H, c.W)}


def gprime32(c, inp):
    """g' = gy act'(y_given) as the kernels form it, in fp32."""
    y = inp["y"]
    ap = (1.0 - y.double() * y.double()).float() if c.act == TANH else CC.act_prime(y, c.act)      # tanh: fma(-y, y, 1)
    return inp["gy"] * ap


def _evaluate_block(c, inp, rounded, dt, mutate):
    r = (lambda t: rb(t).to(dt)) if rounded else (lambda t: t.to(dt))
    x0 = r(inp["x0"])
    a = F.interpolate(x0, scale_factor=2, mode="nearest") if c.up0 else x0
    if c.C1:
        a = torch.cat([a, r(inp["x1"])], 1)
    a = a.clone().requires_grad_()
    pad = lambda t: F.pad(t, (1, 1, 1, 1), mode="reflect" if c.pad == REFLECT else "constant")
    xp = pad(a)
    if "xp" in mutate:
        xp = mutate["xp"](xp)
    w = r(inp["w"])
    z = F.conv2d(xp, w)
    out = {"y": CC._act(z + inp["b"].to(dt)[None, :, None, None] if c.bias else z, c.act).detach()}
    gp32 = gprime32(c, inp)
    gp = r(gp32)
    if "gp" in mutate:
        gp = mutate["gp"](gp)
    (dxp,) = torch.autograd.grad(z, xp, gp, retain_graph=True)
    if "dxp" in mutate:
        dxp = mutate["dxp"](dxp)
    (da,) = torch.autograd.grad(xp, a, dxp)
    dx0 = da[:, :c.C0]
    if c.up0:
        dx0 = dx0.reshape(c.B, c.C0, c.H // 2, 2, c.W // 2, 2).sum((3, 5))
    out["dx0"] = dx0 + inp["add0"].to(dt) if c.add0 else dx0
    out["dx1"] = None
    if c.C1:
        out["dx1"] = da[:, c.C0:] + inp["add1"].to(dt) if c.add1 else da[:, c.C0:]
    if dw_is_bf16(c) or not rounded:
        out["dw"] = torch.nn.grad.conv2d_weight(xp.detach(), w.shape, gp)
    else:                                  # DW_DIRECT: the fp32 direct kernel on the unrounded input and the unrounded fp32 g'
        au = F.interpolate(inp["x0"].to(dt), scale_factor=2, mode="nearest") if c.up0 else inp["x0"].to(dt)
        if c.C1:
            au = torch.cat([au, inp["x1"].to(dt)], 1)
        out["dw"] = torch.nn.grad.conv2d_weight(pad(au), w.shape, gp32.to(dt))
    out["gp"] = gp32.to(dt)                # the bias gradient sums the unrounded fp32 g'
    out["db"] = out["gp"].sum((0, 2, 3))
    return out


def _evaluate_plain(c, inp, rounded, dt, mutate, stride):
    r = (lambda t: rb(t).to(dt)) if rounded else (lambda t: t.to(dt))
    x = r(inp["x"])
    if "x" in mutate:
        x = mutate["x"](x)
    x, w, gy = x.clone().requires_grad_(), r(inp["w"]).requires_grad_(), r(inp["gy"])
    if "gp" in mutate:
        gy = mutate["gp"](gy)
    y = F.conv2d(x, w, None, stride, 1)
    dx, dw = torch.autograd.grad(y, [x, w], gy)
    out = {"y": y.detach(), "dw": dw, "dx": dx}
    if kind(c) == "trunk" and c.addend:
        out["dx"] = dx + inp["add"].to(dt)
    if kind(c) == "s2" and route(c)["dx"] is None:
        out["dx"] = None
    return out


def evaluate(c, inp, rounded=True, dt=torch.float64, mutate=None):
    """The statement of every output the row checks (block: y, dx0, dx1, dw, db, gp; trunk and stride 2: y, dx, dw).  `mutate`: hooks
    {"xp" | "x": on the (padded) input, "gp": on the rounded g', "dxp": on the padded-domain data gradient} for the sensitivity checks."""
    mutate = mutate or {}
    if kind(c) == "block":
        return _evaluate_block(c, inp, rounded, dt, mutate)
    return _evaluate_plain(c, inp, rounded, dt, mutate, 2 if kind(c) == "s2" else 1)


@functools.lru_cache(maxsize=None)
def _reference(c):
    inp = build(c)
    return inp, evaluate(c, inp), evaluate(c, inp, rounded=False)


def reference(c):
    """(inputs, the rounded-operand fp64 statement, the unrounded fp64 statement) of one row; shared and read-only.  Block rows that
    differ only in what they request share one entry."""
    if kind(c) == "block":
        c = c._replace(grads=ALL if c.C1 else ("x0", "w", "b"), dsplit=1)
    return _reference(c)


def checked(c):
    """{output: (gate, norm, statement)}: norm "l2" or "max"; statement "rounded" or "unrounded".  db has its own bound."""
    if kind(c) == "block":
        out = {"y": (Y_GATE, "l2", "rounded"), "dx0": (G_GATE, "l2", "rounded")}
        if c.C1:
            out["dx1"] = (G_GATE, "l2", "rounded")
        out["dw"] = (G_GATE, "l2", "rounded") if dw_is_bf16(c) else (CC.DIRECT_TOL, "max", "unrounded")
        return out
    out = {"y": (Y_GATE, "l2", "rounded"), "dw": (G_GATE, "l2", "rounded")}
    if route(c)["dx"] is not None:
        out["dx"] = (G_GATE, "l2", "rounded")
    return out


def distance(a, ref, norm):
    return rel_l2(a, ref) if norm == "l2" else CC.rel_err(a, ref)


# ---- the launches under the policy and their gate (GPU) -------------------------------------------------------------------------------
class bf16_policy:
    """with bf16_policy(): the calling thread's matrix precision is DC_PREC_BF16, restored on the way out."""

    def __enter__(self):
        self.prev = CC.host_lib().dc_set_matrix_precision(PREC_BF16)
        assert self.prev in (PREC_F32, PREC_BF16)

    def __exit__(self, *exc):
        CC.host_lib().dc_set_matrix_precision(self.prev)


def _launch_trunk(c, inp):
    """dc_wino3x3_fwd, _dgrad (or _dgrad_add) and _wgrad of a trunk row.  Outputs and workspaces -- exactly the bytes of
    dc_wino3x3_workspace / dc_wino3x3_wgrad_workspace -- sit between guards and start as NaN."""
    from depthcore import _lib
    from depthcore._lib import ptr
    L = _lib.lib()
    B, Ci, Co, H, W = c[:5]
    x, w, gy, add = (inp[n].to(CC.DEV).contiguous() for n in ("x", "w", "gy", "add"))
    st = _lib.stream(w)
    keep = add.clone()
    res = {}
    for name, n, query in (("y", B * Co * H * W, L.dc_wino3x3_workspace), ("dx", B * Ci * H * W, L.dc_wino3x3_workspace),
                           ("dw", Co * Ci * 9, L.dc_wino3x3_wgrad_workspace)):
        nbytes = query(B, Ci, Co, H, W)
        assert nbytes > 0 and nbytes % 4 == 0, (name, nbytes)
        out, ws = CC.Guarded(n), CC.Guarded(nbytes // 4)
        if name == "y":
            rc = L.dc_wino3x3_fwd(ptr(x), ptr(w), out.ptr(), ws.ptr(), B, Ci, Co, H, W, st)
        elif name == "dx" and c.addend:
            rc = L.dc_wino3x3_dgrad_add(ptr(gy), ptr(w), out.ptr(), ptr(add), ws.ptr(), B, Ci, Co, H, W, st)
        elif name == "dx":
            rc = L.dc_wino3x3_dgrad(ptr(gy), ptr(w), out.ptr(), ws.ptr(), B, Ci, Co, H, W, st)
        else:
            rc = L.dc_wino3x3_wgrad(ptr(x), ptr(gy), out.ptr(), ws.ptr(), B, Ci, Co, H, W, st)
        assert rc == 0, (name, rc)
        torch.cuda.synchronize()
        assert out.intact() and ws.intact(), "%s: the launch wrote outside a buffer" % name
        res[name] = out.body.cpu()
        assert bool(torch.isfinite(res[name]).all()), "%s has an element that is not finite (left unwritten?)" % name
    assert torch.equal(bits(keep), bits(add)), "the addend was modified"
    res["y"], res["dx"], res["dw"] = res["y"].view(B, Co, H, W), res["dx"].view(B, Ci, H, W), res["dw"].view(Co, Ci, 3, 3)
    return res


def launch(c, inp):
    """The row's launches through the C ABI under DC_PREC_BF16 (restored afterwards, whatever happens): conv_block_cases.launch,
    convs2_cases.launch or the trunk launcher above -- guards, NaN-filled outputs, exact workspace bytes, addends checked."""
    with bf16_policy():
        if kind(c) == "block":
            return CC.launch(c, inp)
        if kind(c) == "s2":
            return S.launch(c, inp, what=("y", "dw") + (("dx",) if route(c)["dx"] is not None else ()))
        return _launch_trunk(c, inp)


def gate(c, res, rnd, unr, tag="conv_bf16_parity"):
    """Prints the share of its gate every output of `res` uses (and the operand rounding next to it), then asserts.  Returns
    {output: share}."""
    share, parts = {}, []
    for k, (g, norm, which) in checked(c).items():
        if res.get(k) is None:
            continue
        ref = rnd[k] if which == "rounded" else unr[k]
        err = distance(res[k], ref, norm)
        share[k] = err / g
        parts.append("%s %.2e (%.0f%% of %.0e %s, %s)" % (k, err, 100 * err / g, g, norm, which))
    if res.get("db") is not None:
        bound = CC.sum_bound(c.B * c.H * c.W, rnd["gp"].abs().sum((0, 2, 3))).clamp_min(1e-300)
        share["db"] = float(((res["db"].double() - rnd["db"]).abs() / bound).max())
        parts.append("db %.1f%% of its sum bound" % (100 * share["db"]))
    print("%s %-50s %s" % (tag, case_id(c), "; ".join(parts)))
    for k, s in share.items():
        assert s < 1.0, (case_id(c), k, s)
    return share
