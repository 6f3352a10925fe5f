"""Case table, seeded input builder, plain-torch statement and host-dispatch transcription for ONE fused 3x3 block launch pair
(csrc/conv3x3.hip: dc_conv3x3_fwd / dc_conv3x3_bwd_add, fp32 policy) at the edges of its dispatch: the single-channel head
kernels (csrc/dispconv.hip), the fused Winograd launches (csrc/wino.hip, csrc/wino_wgrad.hip), the direct implicit GEMMs, the two
folds, the reflection ring, the split weight-gradient reductions and the four ways g' = gy act'(y) comes about.  Shared by
tests/test_conv_block_cases_cpu.py (no GPU: the table reaches every mechanism, route() agrees with the library's workspace
queries and, field by field, with the plan the launches themselves follow (dc_conv3x3_plan_query), the cases are well conditioned,
the refusals are host-side), tests/test_conv_block_shapes_gpu.py (the kernels against the statement), tests/conv_block_direct_child.py
(the same with DC_CONV_WINO=0) and tests/conv_block_plan_child.py (the plan agreement with DC_CONV_WINO=0).  DESIGN.md, "The fused 3x3 block at its dispatch
edges", has the table with its reasons, the predicates, the gates and the measured figures.

    Case                     (B, C0, up0, C1, Co, H, W, act, pad, bias, grads, add0, add1, dsplit)
                             grads: the outputs of the backward launch whose pointers are non-null, a tuple out of x0, x1, w, b
                             add1: 0, "inplace" (dx1 preloaded and passed as its own addend) or "separate"; dsplit: dc_set_dgrad_split
    build(case)              seeded fp32 inputs x0, x1, w, b, gy, add0, add1 and the backward's INPUT y (below)
    evaluate(case, inp, dt)  the statement in `dt`
    reference(case)          cached (inputs, fp64 results, fp32 results); nobody may modify what it returns
    route(case, wino)        the kernels the two launches run, transcribed from the host code (independent of the library: it never
                             asks dc_conv3x3_plan_query, plan_mismatches() compares the two)

The statement, with u = nearest x2 upsample (up0) or the identity, P = ReflectionPad2d(1) (pad 0) or ZeroPad2d(1) (pad 1):
    forward   y = act(conv2d(P(cat(u(x0), x1)), w) + b)
    backward  g' = gy act'(y_given), act' expressed through the OUTPUT: [y > 0] (ReLU), y > 0 ? 1 : y + 1 (ELU), y (1 - y)
              (sigmoid), 1 - y^2 (tanh);  dx0, dx1 by autograd through P, cat and u, plus the addends;
              dw = conv2d_weight(P(cat(u(x0), x1)), g');  db = sum g'
The backward entry takes y as an input, so it is given one: the fp64 statement's y rounded to fp32, with exact zeros planted for
ReLU and ELU (ReLU's derivative there is 0, ELU's is 1).  No activation derivative is a rounding question that way."""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

import layer_ops_cases as LC
import wino_bn_cases as WC
from wino_split_cases import al256, uhat_bytes, slab_bytes as _wino_slab_bytes      # the Winograd workspace layout is transcribed there

Case = collections.namedtuple("Case", "B C0 up0 C1 Co H W act pad bias grads add0 add1 dsplit")

ACT_NONE, ACT_ELU, ACT_SIGMOID, ACT_RELU, ACT_TANH = range(5)
REFLECT, ZERO = 0, 1
ALL = ("x0", "x1", "w", "b")
WINO_TOL = WC.TENSOR_TOL      # max|hip - fp64| <= 2e-5 max|fp64| behind a Winograd kernel (tests/test_wino_gpu.py)
DIRECT_TOL = 1e-5             # ... <= 1e-5 max|fp64| behind a direct or plain-FMA kernel (tests/test_convs2_gpu.py)
E32_MAX = 1e-4
EINVAL = -1

# csrc/conv3x3.hip, csrc/dispconv.hip, csrc/conv_bf16.hip, csrc/wino.hip
CT, CK, CW = 16, 8, 16
RING_MAXCO, RING_CB, RING_SEG = 64, 8, 128
DWP, DB_SPLIT = 2048, 8
DGRAD_SPLIT_MIN_PIXELS, DGRAD_SPLIT_MIN_ELEMS = 6000, 4 << 20
WINO_DX_MIN_CIN, WINO_DW_MIN_CIN, WINO_DW_MIN_CO = 16, 32, 32
C3B_BC = WC.C3B_BC

ceil_div = WC.ceil_div
rel_err = LC.rel_err
sum_bound = WC.sum_bound


def K(B, C0, up0, C1, Co, H, W, act, pad, bias=1, grads=ALL, add0=0, add1=0, dsplit=1):
    grads = tuple(g for g in ALL if g in grads and (g != "x1" or C1 > 0))
    return Case(B, C0, up0, C1, Co, H, W, act, pad, bias, grads, add0, add1, dsplit)


# ---- the table (DESIGN.md lists what each case is there for; tests/test_conv_block_cases_cpu.py asserts it from route()) ---------
HEAD = [
    K(2, 16, 0, 0, 1, 48, 50, 2, REFLECT, add0=1),          # tile forward (W = 50), dispconv_dx + addend, wgrad<4> over 2400 > 2048 pixels
    K(2, 32, 0, 0, 1, 48, 50, 2, ZERO),                     # wgrad<8> over a ragged second 2048-pixel block, zero pad
    K(2, 16, 0, 0, 1, 12, 28, 1, ZERO),                     # fwd4; 336 pixels: a ragged second block of dispconv_dx; wgrad<4> below 2048
    K(1, 32, 0, 0, 1, 18, 20, 3, REFLECT, add0=1),          # fwd4; 360 pixels; wgrad<8> below 2048; ReLU ties
    K(2, 5, 0, 0, 1, 9, 13, 0, REFLECT),                    # odd W = 13: tile forward below one tile; C0 = 5: direct weight gradient, nW = 45
    K(2, 16, 0, 0, 1, 9, 13, 2, ZERO, add0=1),              # HW % 4 != 0: wgrad<4> refused
    K(2, 32, 0, 0, 1, 9, 13, 4, REFLECT),                   # HW % 4 != 0: wgrad<8> refused
    K(2, 16, 0, 0, 1, 10, 18, 2, REFLECT, bias=0),          # W = 18: tile forward with a ragged second tile, no bias
    K(2, 40, 0, 0, 1, 8, 12, 2, REFLECT),                   # C0 = 40: the head kernels refuse, Winograd forward with Co = 1
    K(2, 16, 0, 0, 1, 3, 12, 2, ZERO),                      # H = 3: refused, Winograd
    K(2, 40, 0, 0, 1, 8, 13, 2, REFLECT),                   # C0 = 40 and odd W: refused, direct
]
HEAD_NULLS = [K(2, C0, 0, 0, 1, 12, 28, 1, ZERO, grads=g) for C0 in (16, 32) for g in (("x0",), ("w", "b"), ("w",), ("b",))]
HEAD_NULLS += [K(2, 32, 0, 0, 1, 12, 28, 1, ZERO)]
HEAD_NULLS += [K(2, C0, 0, 0, 1, 48, 50, 2, pad, grads=g) for C0, pad in ((16, REFLECT), (32, ZERO)) for g in (("w",), ("b",))]

WINO = [
    # the fused forward: {up0, concat, up0 + concat} x {reflect, zero}, activations 0-4, a null bias; split store with and without ring
    K(2, 16, 1, 0, 24, 8, 12, 1, REFLECT, dsplit=2),                                    # up0; ring on a half-resolution plane
    K(2, 16, 1, 0, 24, 8, 12, 1, ZERO),                                                 # split store, no ring
    K(2, 16, 0, 8, 24, 12, 8, 2, REFLECT, add0=1, add1="separate", dsplit=2),           # concat, H > W
    K(2, 16, 0, 8, 24, 8, 20, 4, ZERO, add0=1, add1="inplace"),                         # concat, zero: addends in the store epilogue
    K(2, 16, 1, 8, 24, 12, 8, 1, REFLECT, add0=1, add1="inplace", dsplit=2),            # up0 + concat, H > W
    K(2, 16, 1, 8, 24, 8, 20, 3, REFLECT, add0=1, add1="separate", dsplit=2),           # up0 + concat, W > H
    K(2, 16, 1, 8, 24, 8, 20, 0, ZERO, bias=0),                                         # up0 + concat, zero, no bias, no activation
    K(1, 20, 0, 0, 16, 6, 10, 0, REFLECT, dsplit=2),                                    # Cin = 20: a ragged last ring chunk
    K(2, 40, 0, 24, 64, 4, 12, 3, REFLECT, dsplit=2),                                   # H = 4; Co = 64 exactly; 40 + 24
    K(1, 16, 0, 0, 8, 10, 4, 2, REFLECT, dsplit=2),                                     # W = 4
    K(1, 16, 1, 0, 8, 4, 4, 1, REFLECT, add0=1, dsplit=2),                              # 4 x 4 with up0: a 2 x 2 plane, every element on the ring
    # split refused: full correlation + fold
    K(2, 24, 0, 0, 72, 8, 12, 1, REFLECT, dsplit=2),                                    # Co = 72 > RING_MAXCO; fold4
    K(2, 24, 0, 0, 72, 8, 12, 1, ZERO, dsplit=2),                                       # ... zero pad takes the split store
    K(2, 16, 0, 8, 24, 7, 12, 2, REFLECT, add0=1, add1="separate", dsplit=2),           # odd H; fold4 with concat and addends
    K(2, 16, 0, 8, 24, 7, 10, 2, ZERO, add0=1, add1="inplace", dsplit=2),               # odd H; W % 4 != 0: conv_fold_kernel, zero
    K(2, 16, 1, 8, 24, 12, 8, 1, REFLECT, add0=1, add1="inplace", dsplit=0),            # dsplit = 0 twins of the ring cases
    K(2, 16, 1, 8, 24, 8, 20, 3, REFLECT, add0=1, add1="separate", dsplit=0),           # (W >> 1) % 4 != 0: conv_fold_kernel with up0
    K(2, 16, 1, 0, 24, 8, 24, 1, REFLECT, dsplit=0),                                    # W = 24 with up0: 12-wide rows, fold4 on the half plane
    K(2, 16, 1, 0, 24, 8, 24, 1, ZERO, add0=1, dsplit=0),                               # fold4, zero, up0, addend
    K(2, 16, 1, 8, 24, 8, 16, 0, ZERO, dsplit=0),                                       # fold4, zero, up0 + concat, no addend
    K(1, 20, 0, 0, 16, 6, 10, 0, REFLECT, dsplit=0),                                    # conv_fold_kernel, reflect, no addend
    K(2, 16, 0, 8, 24, 12, 8, 2, REFLECT, add0=1, add1="separate", dsplit=0),           # fold4, reflect, concat, addends
    # dsplit = 1 (the default): the ring only from 6000 pixels and 4 Mi elements
    K(8, 88, 0, 0, 8, 64, 96, 1, REFLECT, grads=("x0",), dsplit=1),                     # 6144 pixels, 4.1 Mi elements: the ring
    K(2, 16, 1, 8, 24, 12, 8, 1, REFLECT, add0=1, add1="inplace", dsplit=1),            # below: full correlation + fold
    # the fused weight gradient (Cin >= 32, Co >= 32) and the bias gradient's two ways
    K(2, 16, 1, 16, 32, 8, 12, 1, REFLECT, dsplit=2),                                   # up0 + concat + reflect; g' fused with db
    K(2, 16, 1, 16, 32, 8, 12, 0, REFLECT, dsplit=2),                                   # ... without an activation: db alone from that pass
    K(2, 32, 0, 0, 32, 7, 6, 1, REFLECT),                                               # HW % 4 != 0: conv_dbias_kernel
    K(2, 32, 0, 0, 32, 7, 6, 0, ZERO),                                                  # ... without an activation, zero pad
    K(2, 24, 1, 16, 40, 10, 12, 4, ZERO, bias=0),                                       # ragged Cin = 40 and Co = 40 in the fused weight gradient
]
WINO_NULLS = [K(2, 16, 1, 16, 32, 8, 12, 1, REFLECT, grads=g, dsplit=2)
              for g in (("x0", "x1"), ("w", "b"), ("w",), ("b",), ("x0",), ("x1",))]

DIRECT = [
    K(2, 7, 0, 0, 5, 9, 13, 1, REFLECT),                    # below one tile; Co = 5, Cin = 7: nW = 315, conv_wreduce_kernel; g' on the fly
    K(2, 20, 0, 0, 20, 17, 19, 2, ZERO),                    # ragged second tile both ways; <2> everywhere; 8 tiles: two slabs
    K(3, 20, 0, 0, 7, 17, 19, 3, REFLECT, add0=1),          # 12 tiles: three slabs; conv_gemm<1>, wgrad<1>
    K(3, 7, 0, 0, 5, 17, 19, 4, ZERO),                      # nW = 315 over three slabs: conv_wreduce_kernel's slab loop
    K(1, 12, 0, 8, 40, 9, 34, 3, REFLECT, add0=1, add1="separate"),   # even W refused by the ragged concat; <4> forward; three tiles in x
    K(2, 12, 1, 8, 7, 10, 14, 1, REFLECT, add0=1, add1="inplace"),    # up0 + ragged concat, W / 2 = 7
    K(2, 12, 1, 8, 20, 10, 14, 1, ZERO),                    # ... zero pad, <2>
    K(2, 12, 0, 8, 20, 8, 16, 4, ZERO, add1="separate"),    # C0 = 12, C1 = 8, W = 16: fold4 behind the direct kernel
    K(1, 40, 0, 0, 40, 17, 19, 0, ZERO, bias=0),            # <4> forward and <4> data gradient
    K(1, 16, 0, 0, 5, 7, 6, 1, REFLECT),                    # even W, B Co H W % 4 != 0 with an activation: wino_gp_ok refuses both gradients
    K(2, 8, 0, 0, 20, 8, 16, 1, REFLECT),                   # Cin = 8 < 16, W % 16 == 0: conv_gemm_v2<1, dgrad>, conv_wgrad_v2<2>
    K(4, 8, 0, 0, 7, 16, 32, 2, ZERO, add0=1),              # conv_wgrad_v2<1> with two slabs
    K(2, 7, 0, 0, 5, 9, 13, 1, REFLECT, grads=("b",)),      # the direct weight-gradient kernel with dw == nullptr
    K(2, 7, 0, 0, 5, 9, 13, 1, REFLECT, grads=("w",)),      # ... and with db == nullptr
    K(2, 8, 0, 0, 20, 8, 16, 1, REFLECT, grads=("b",)),     # conv_wgrad_v2 with dw == nullptr
    K(2, 8, 0, 0, 20, 8, 16, 1, REFLECT, grads=("w",)),     # conv_wgrad_v2 with db == nullptr
]
DIRECT_NULLS = [K(2, 12, 1, 8, 20, 10, 14, 1, ZERO, grads=g) for g in (("x0", "x1"), ("w", "b"), ("w",), ("b",), ("x0",), ("x1",))]

# W % 16 == 0: with DC_CONV_WINO=0 these reach conv_gemm_v2_kernel<1 | 2 | 4, false> (and the v2 gradients) -- tests/conv_block_direct_child.py
V2 = [
    K(2, 16, 1, 16, 7, 8, 16, 1, REFLECT, add0=1, add1="separate"),      # <1>: up0 + concat + reflect, Co = 7
    K(2, 16, 1, 16, 20, 8, 32, 2, REFLECT),                              # <2>: Co = 20, two tiles in x
    K(1, 16, 1, 32, 40, 16, 16, 3, REFLECT, add1="inplace"),             # <4>: Co = 40
]
CASES = HEAD + HEAD_NULLS + WINO + WINO_NULLS + DIRECT + DIRECT_NULLS + V2

# one shape per routing family: every null pattern of NULL_FAMILIES[base] is compared with the all-gradients launch of base
NULL_FAMILIES = {
    "wino": (K(2, 16, 1, 16, 32, 8, 12, 1, REFLECT, dsplit=2), WINO_NULLS),
    "direct": (K(2, 12, 1, 8, 20, 10, 14, 1, ZERO), DIRECT_NULLS),
    "head4": (K(2, 16, 0, 0, 1, 12, 28, 1, ZERO), [c for c in HEAD_NULLS if c.C0 == 16 and c.H == 12]),
    "head8": (K(2, 32, 0, 0, 1, 12, 28, 1, ZERO), [c for c in HEAD_NULLS if c.C0 == 32 and c.H == 12 and len(c.grads) < 3]),
}
# dsplit = 2 cases whose dsplit = 0 twin is in the table and takes another data-gradient kernel
DSPLIT_PAIRS = [K(2, 16, 1, 8, 24, 12, 8, 1, REFLECT, add0=1, add1="inplace", dsplit=2),
                K(2, 16, 1, 8, 24, 8, 20, 3, REFLECT, add0=1, add1="separate", dsplit=2),
                K(1, 20, 0, 0, 16, 6, 10, 0, REFLECT, dsplit=2)]
DETERMINISM = {"split_wgrad": K(3, 20, 0, 0, 7, 17, 19, 3, REFLECT, add0=1),
               "ring": K(2, 16, 1, 8, 24, 8, 20, 3, REFLECT, add0=1, add1="separate", dsplit=2),
               "head_wgrad": K(2, 32, 0, 0, 1, 48, 50, 2, ZERO)}


def case_id(c):
    return "b%d-%d%s+%dto%d-%dx%d-a%d-%s-%s-g.%s-add%d%s-ds%d" % (
        c.B, c.C0, "u" if c.up0 else "", c.C1, c.Co, c.H, c.W, c.act, "zero" if c.pad else "refl", "b" if c.bias else "nb",
        "".join(c.grads), c.add0, {0: "0", "inplace": "i", "separate": "s"}[c.add1], c.dsplit)


def params(cases):
    import pytest
    return [pytest.param(c, id=case_id(c)) for c in cases]


# ---- the dispatch, transcribed ------------------------------------------------------------------------------------------------------
def pick_mr(M):
    return 4 if M > 32 else (2 if M > 16 else 1)


def pick_mr_w(M):
    return 2 if M > 16 else 1


def pick_split(B, H, W, Co, Cin):
    ntiles = ceil_div(W, CT) * ceil_div(H, CT) * B
    outer = ceil_div(Co, 16 * pick_mr_w(Co)) * ceil_div(Cin, CW)
    split = max(1, min(ntiles, 2048 // max(outer, 1)))
    split = min(split, max(1, ntiles // 4))
    return min(split, 512)


def gpd_split(Co):
    return max(8, min(256, 2048 // max(Co, 1)))


def c3b_weights_bytes(Ci, Co):
    a, b = ceil_div(Co, 16 * pick_mr(Co)) * 16 * pick_mr(Co), ceil_div(Ci, 16 * pick_mr(Ci)) * 16 * pick_mr(Ci)
    return al256(max(a * ceil_div(Ci, C3B_BC) * C3B_BC * 9 * 2, b * ceil_div(Co, C3B_BC) * C3B_BC * 9 * 2))


def c3b_wgrad_split(B, H, W, Co, Cin):
    ntiles = ceil_div(W, 32) * ceil_div(H, 8) * B
    outer = ceil_div(Co, 64) * ceil_div(Cin, C3B_BC)
    return min(max(1, min(ntiles, 512 // max(outer, 1))), 256)


def wino_conv_ws_bytes(B, Ci, Co, H, W):
    return uhat_bytes(Ci, Co) + al256(max(_wino_slab_bytes(B * Co * H * W), _wino_slab_bytes(B * Ci * (H + 2) * (W + 2))))


def wino_eligible(C0, C1, H, W):
    return W >= 2 and W % 2 == 0 and H >= 2 and (C1 == 0 or C0 % WC.PSK == 0)


def wino_fits(B, C0, C1, Co, H, W):
    return B * max(C0, C1, Co) * H * W * 4 < 0x7fffffff


def wino_gp_ok(B, Co, H, W, act):
    return act == ACT_NONE or (B * Co * H * W) % 4 == 0


def head_eligible(C0, C1, up0, Co, H, W):
    return Co == 1 and C1 == 0 and not up0 and H >= 4 and W >= 4 and C0 <= 32


def dgrad_split_ok(B, C0, C1, Co, H, W):
    if H < 4 or W < 4 or H % 2 or W % 2 or C0 <= 0 or B * Co * H * W * 4 >= 0x7fffffff:
        return False
    return WC.ps_plan(B, Co, C0 + C1, H, W).ksplit == 1


def shape_routes(c, wino_enabled=True, act=ACT_NONE):
    """(wino_fwd, wino_dx, wino_dw) of the shape alone -- what the workspace queries ask (act = ACT_NONE there)."""
    B, C0, C1, Co, H, W = c.B, c.C0, c.C1, c.Co, c.H, c.W
    base = wino_enabled and wino_eligible(C0, C1, H, W) and wino_fits(B, C0, C1, Co, H, W)
    gp = wino_gp_ok(B, Co, H, W, act)
    return (base, base and C0 + C1 >= WINO_DX_MIN_CIN and gp,
            base and C0 + C1 >= WINO_DW_MIN_CIN and Co >= WINO_DW_MIN_CO and gp)


WINO_KERNELS = ("wino_conv_fused_fwd", "wino_conv_dgrad_split", "wino_conv_full_dgrad", "wino_wgrad_fused")


def route(c, wino_enabled=True):
    """The kernels behind each result of the case's two launches (fp32 policy, 16-byte aligned buffers):
    fwd, gprime, dx (kernel, ring, fold), dw (kernel, reduce), db, and the flags the host code derives them from."""
    B, C0, up0, C1, Co, H, W, act, pad = c.B, c.C0, c.up0, c.C1, c.Co, c.H, c.W, c.act, c.pad
    Cin, HW = C0 + C1, H * W
    head = wino_enabled and head_eligible(C0, C1, up0, Co, H, W)
    wf, _, _ = shape_routes(c, wino_enabled)
    _, wdx_shape, wdw_shape = shape_routes(c, wino_enabled, act)
    r = {}
    # dc_conv3x3_fwd
    fast_f = W % 16 == 0 and (C1 == 0 or C0 % CK == 0)
    if head:
        r["fwd"] = "dispconv_fwd4_kernel" if W % 4 == 0 else "dispconv_fwd_kernel"
    elif wf:
        r["fwd"] = "wino_conv_fused_fwd"
    else:
        r["fwd"] = "conv_gemm%s_kernel<%d, false>" % ("_v2" if fast_f else "", pick_mr(Co))
    # dc_conv3x3_bwd_add
    want_dx0, want_dx = "x0" in c.grads, "x0" in c.grads or "x1" in c.grads
    want_w, want_b = "w" in c.grads, "b" in c.grads
    w_dx, w_dw = want_dx and wdx_shape, want_w and wdw_shape
    fused_db = want_b and w_dw and HW % 4 == 0
    fast = W % 16 == 0 and (C1 == 0 or C0 % CK == 0) and (C1 == 0 or C0 % CW == 0)
    head_dx = want_dx0 and head
    dxpad_bytes = al256(B * Cin * (H + 2) * (W + 5) * 4)
    head_dw = ((want_w or want_b) and head and C0 in (16, 32) and HW % 4 == 0 and
               B * ceil_div(HW, DWP) * (C0 * 9 + 1) * 4 <= dxpad_bytes)
    gp_unused = (head_dx or not want_dx) and (head_dw or not (want_w or want_b))
    if gp_unused:
        r["gprime"] = "unused"
    elif fused_db:
        r["gprime"] = "conv_gprime_dbias_kernel"
    elif (fast or w_dx or w_dw) and act != ACT_NONE and (B * Co * HW) % 4 == 0:
        r["gprime"] = "conv_gprime_kernel"
    else:
        r["gprime"] = "on the fly" if act != ACT_NONE else "gy"
    quads = H >= 4 and W >= 4 and W % 4 == 0 and (W >> up0) % 4 == 0
    fold = "conv_fold4_kernel" if quads else "conv_fold_kernel"
    r["dx"], r["ring"], r["fold"] = None, False, None
    if head_dx:
        r["dx"] = "dispconv_dx_kernel"
    elif w_dx and c.dsplit and dgrad_split_ok(B, C0, C1, Co, H, W) and (
            pad == ZERO or (Co <= RING_MAXCO and (c.dsplit == 2 or (HW >= DGRAD_SPLIT_MIN_PIXELS and B * Cin * HW >= DGRAD_SPLIT_MIN_ELEMS)))):
        r["dx"], r["ring"] = "wino_conv_dgrad_split", pad == REFLECT
    elif w_dx:
        r["dx"], r["fold"] = "wino_conv_full_dgrad", fold
    elif want_dx:
        r["dx"], r["fold"] = "conv_gemm%s_kernel<%d, true>" % ("_v2" if fast else "", pick_mr(Cin)), fold
    r["dw"], r["reduce"], r["db"], r["split"] = None, None, None, 0
    nW = Co * Cin * 9
    if head_dw:
        r["dw"] = "dispconv_wgrad_kernel<%d>" % (C0 // 4)
        r["reduce"] = "conv_wreduce4_kernel" if want_w else "conv_wreduce_kernel"       # (nW = 9 C0: whole quads)
        r["split"] = B * ceil_div(HW, DWP)
        r["db"] = r["dw"] if want_b else None
    elif w_dw:
        r["dw"], r["reduce"] = "wino_wgrad_fused", None
        if want_b:
            r["db"] = "conv_gprime_dbias_kernel" if fused_db else "conv_dbias_kernel"
    elif want_w or want_b:
        r["dw"] = "conv_wgrad%s_kernel<%d>" % ("_v2" if fast else "", pick_mr_w(Co))
        r["reduce"] = "conv_wreduce4_kernel" if want_w and nW % 4 == 0 else "conv_wreduce_kernel"
        r["split"] = pick_split(B, H, W, Co, Cin)
        r["db"] = r["dw"] if want_b else None
    r.update(head=head, head_dx=head_dx, head_dw=head_dw, w_dx=bool(w_dx), w_dw=bool(w_dw), fused_db=bool(fused_db), fast=fast,
             gp_unused=gp_unused, dw_null=r["dw"] is not None and not want_w, db_null=r["dw"] is not None and not want_b)
    return r


def output_kernels(c, wino_enabled=True):
    """What decides each backward output's bits, as far as route() names it (the null-pattern comparison's key)."""
    r = route(c, wino_enabled)
    dx = (r["dx"], r["ring"], r["fold"])
    return {"dx0": dx, "dx1": dx, "dw": (r["dw"], r["reduce"], r["split"]), "db": (r["db"], r["reduce"] if r["dw"] != "wino_wgrad_fused" else None)}


def tol(kernel):
    return WINO_TOL if kernel in WINO_KERNELS else DIRECT_TOL


# ---- the library's own plan (include/depthcore.h: dc_conv3x3_plan, the DC_C3_* enums) against route() -------------------------------
FWD_HEAD, FWD_BF16, FWD_WINO, FWD_DIRECT = range(4)
GP_UNUSED, GP_GY, GP_ON_THE_FLY, GP_KERNEL, GP_DBIAS_KERNEL = range(5)
DX_NONE, DX_HEAD, DX_BF16, DX_BF16_FOLD, DX_WINO_SPLIT, DX_WINO_FOLD, DX_DIRECT_FOLD = range(7)
DW_NONE, DW_HEAD, DW_BF16, DW_WINO, DW_DIRECT = range(5)
DB_NONE, DB_SLABS, DB_GPRIME, DB_KERNEL = range(4)
WANT = {"x0": 1, "x1": 2, "w": 4, "b": 8}
# route()'s kernel names, template arguments stripped, as plan values (the bf16 values have no name: route() is the fp32 policy)
PLAN_FWD = {"dispconv_fwd4_kernel": FWD_HEAD, "dispconv_fwd_kernel": FWD_HEAD, "wino_conv_fused_fwd": FWD_WINO,
            "conv_gemm_kernel": FWD_DIRECT, "conv_gemm_v2_kernel": FWD_DIRECT}
PLAN_GP = {"unused": GP_UNUSED, "gy": GP_GY, "on the fly": GP_ON_THE_FLY, "conv_gprime_kernel": GP_KERNEL,
           "conv_gprime_dbias_kernel": GP_DBIAS_KERNEL}
PLAN_DX = {None: DX_NONE, "dispconv_dx_kernel": DX_HEAD, "wino_conv_dgrad_split": DX_WINO_SPLIT, "wino_conv_full_dgrad": DX_WINO_FOLD,
           "conv_gemm_kernel": DX_DIRECT_FOLD, "conv_gemm_v2_kernel": DX_DIRECT_FOLD}
PLAN_DW = {None: DW_NONE, "dispconv_wgrad_kernel": DW_HEAD, "wino_wgrad_fused": DW_WINO, "conv_wgrad_kernel": DW_DIRECT,
           "conv_wgrad_v2_kernel": DW_DIRECT}
PLAN_DB = {None: DB_NONE, "conv_gprime_dbias_kernel": DB_GPRIME, "conv_dbias_kernel": DB_KERNEL}


def _kernel(name):
    """(name without template arguments, first template argument or 0)"""
    if name is None or "<" not in name:
        return name, 0
    return name[:name.index("<")], int(name[name.index("<") + 1:].rstrip(">").split(",")[0])


def plan_of(r):
    """route()'s answer as the fields of dc_conv3x3_plan.  fwd_v2 / fwd_mr, dx_mr and dw_mr are 0 unless the direct kernel of that pass
    runs; `split` counts the direct weight gradient's slabs (the head's and Winograd's are chosen inside their own files: 0)."""
    (fwd, fwd_mr), (dx, dx_mr), (dw, dw_mr) = _kernel(r["fwd"]), _kernel(r["dx"]), _kernel(r["dw"])
    direct_f, direct_dx, direct_dw = PLAN_FWD[fwd] == FWD_DIRECT, PLAN_DX[dx] == DX_DIRECT_FOLD, PLAN_DW[dw] == DW_DIRECT
    assert not direct_dx or dx.endswith("_v2_kernel") == r["fast"]
    assert not direct_dw or dw.endswith("_v2_kernel") == r["fast"]
    return {"fwd": PLAN_FWD[fwd], "fwd_v2": int(direct_f and fwd.endswith("_v2_kernel")), "fwd_mr": fwd_mr if direct_f else 0,
            "gprime": PLAN_GP[r["gprime"]], "dx": PLAN_DX[dx], "ring": int(r["ring"]), "dw": PLAN_DW[dw],
            "db": DB_SLABS if r["db"] is not None and r["db"] == r["dw"] else PLAN_DB[r["db"]], "bwd_v2": int(r["fast"]),
            "dx_mr": dx_mr if direct_dx else 0, "dw_mr": dw_mr if direct_dw else 0, "split": r["split"] if direct_dw else 0}


def plan_query(c, grads=None):
    """dc_conv3x3_plan_query of the case (`grads`: another request than the case's) under the mode and precision in effect:
    (return code, {field: value})."""
    import ctypes
    from depthcore import _lib
    p = _lib.Conv3x3Plan()
    want = sum(WANT[g] for g in (c.grads if grads is None else grads))
    rc = host_lib().dc_conv3x3_plan_query(c.C0, c.up0, c.C1, c.B, c.Co, c.H, c.W, c.act, c.pad, want, ctypes.byref(p))
    return rc, {n: getattr(p, n) for n, _ in p._fields_}


def plan_mismatches(c, wino_enabled=True):
    """[(field, the library's value, route()'s value)] of the case under its own dsplit mode -- empty when they agree."""
    L = host_lib()
    prev = L.dc_set_dgrad_split(c.dsplit)
    try:
        rc, got = plan_query(c)
    finally:
        L.dc_set_dgrad_split(prev)
    assert rc == 0, rc
    want = plan_of(route(c, wino_enabled))
    assert set(want) == set(got)
    return [(k, got[k], want[k]) for k in sorted(want) if got[k] != want[k]]


def fwd_workspace(c, wino_enabled=True):
    """dc_conv3x3_fwd_workspace rebuilt from the transcription."""
    Cin = c.C0 + c.C1
    direct = max(al256(9 * Cin * c.Co * 4), c3b_weights_bytes(Cin, c.Co))
    return max(direct, wino_conv_ws_bytes(c.B, Cin, c.Co, c.H, c.W)) if shape_routes(c, wino_enabled)[0] else direct


def bwd_workspace(c, wino_enabled=True):
    """dc_conv3x3_bwd_workspace rebuilt from the transcription: the direct layout (weights, padded-domain scratch, weight and bias
    slabs, g'), the Winograd scratch of either gradient behind it, the bias partials of conv_gprime_dbias_kernel last."""
    B, Co, H, W = c.B, c.Co, c.H, c.W
    Cin = c.C0 + c.C1
    nW = Co * Cin * 9
    split = max(pick_split(B, H, W, Co, Cin), c3b_wgrad_split(B, H, W, Co, Cin))
    total = (max(al256(nW * 4), c3b_weights_bytes(Cin, Co)) + al256(B * Cin * (H + 2) * (W + 5) * 4) + al256(split * nW * 4) +
             al256(max(split, DB_SPLIT) * Co * 4) + al256(B * Co * H * W * 4))
    _, wdx, wdw = shape_routes(c, wino_enabled)
    if wdx:
        total += al256(wino_conv_ws_bytes(B, Cin, Co, H, W))
    if wdw:
        total += al256(WC.wg_plan(B, Cin, Co, H, W).ws_bytes) + al256(DB_SPLIT * Co * 4)
    return total + al256(256 * Co * 4)


# ---- the builder ------------------------------------------------------------------------------------------------------------------
def tie_positions(c):
    """(b, co, y, x) of the exact zeros planted into the backward's y (ReLU and ELU cases): the first and the last pixel of a
    plane among them."""
    B, Co, H, W = c.B, c.Co, c.H, c.W
    return sorted({(0, 0, 0, 0), (0, 0, H - 1, W - 1), (B - 1, Co - 1, 0, 0), (B - 1, Co - 1, H - 1, W - 1), (B - 1, Co // 2, H // 2, W // 2),
                   (0, Co - 1, H - 1, 0), (B // 2, 0, 0, W - 1)})


def tie_mask(c):
    m = torch.zeros(c.B, c.Co, c.H, c.W, dtype=torch.bool)
    if c.act in (ACT_ELU, ACT_RELU):
        for b, co, y, x in tie_positions(c):
            m[b, co, y, x] = True
    return m


def _act(v, act):
    return [v, F.elu(v), torch.sigmoid(v), F.relu(v), torch.tanh(v)][act] if act else v


def act_prime(y, act):
    """act' through the activated output, the comparisons as the kernels make them (`> 0`)."""
    one = torch.ones_like(y)
    if act == ACT_ELU:
        return torch.where(y > 0, one, y + 1)
    if act == ACT_SIGMOID:
        return y * (1 - y)
    if act == ACT_RELU:
        return torch.where(y > 0, one, torch.zeros_like(y))
    if act == ACT_TANH:
        return 1 - y * y
    return one


def _padded_input(c, x0, x1):
    a = F.interpolate(x0, scale_factor=2, mode="nearest") if c.up0 else x0
    if c.C1:
        a = torch.cat([a, x1], 1)
    return F.pad(a, (1, 1, 1, 1), mode="reflect" if c.pad == REFLECT else "constant")


def forward(c, inp, dt):
    z = F.conv2d(_padded_input(c, inp["x0"].to(dt), None if inp["x1"] is None else inp["x1"].to(dt)), inp["w"].to(dt))
    if c.bias:
        z = z + inp["b"].to(dt)[None, :, None, None]
    return _act(z, c.act)


def build(c):
    """fp32 inputs of one case (a dict of CPU tensors; absent operands are None)."""
    B, C0, C1, Co, H, W = c.B, c.C0, c.C1, c.Co, c.H, c.W
    g = torch.Generator().manual_seed(zlib.crc32(repr(("conv_block", tuple(c[:10]))).encode()))
    rn = lambda *shape: torch.randn(*shape, generator=g)
    inp = {"x0": rn(B, C0, H >> c.up0, W >> c.up0), "x1": rn(B, C1, H, W) if C1 else None,
           "w": rn(Co, C0 + C1, 3, 3) * (2.0 / (9 * (C0 + C1))) ** 0.5, "b": 0.3 * rn(Co), "gy": rn(B, Co, H, W)}
    inp["add0"] = rn(B, C0, H >> c.up0, W >> c.up0)
    inp["add1"] = rn(B, C1, H, W) if C1 else None
    y = forward(c, inp, torch.float64).float()
    ties = tie_mask(c)
    y[ties] = 0.0
    inp["gy"][ties] = 1.5           # the tie matters: ReLU's 0 and ELU's 1 are 1.5 apart in g'
    inp["y"] = y
    return inp


# ---- the statement ----------------------------------------------------------------------------------------------------------------
def evaluate(c, inp, dt):
    """{y, gp, dx0, dx1, dw, db} of the statement in `dt` (every gradient, whatever the case requests; the addends as the case
    has them)."""
    x0 = inp["x0"].to(dt).requires_grad_()
    x1 = inp["x1"].to(dt).requires_grad_() if c.C1 else None
    w = inp["w"].to(dt)
    xp = _padded_input(c, x0, x1)
    z = F.conv2d(xp, w)
    yb = z + inp["b"].to(dt)[None, :, None, None] if c.bias else z
    out = {"y": _act(yb, c.act).detach()}
    gp = inp["gy"].to(dt) * act_prime(inp["y"].to(dt), c.act)
    grads = torch.autograd.grad(z, [x0] + ([x1] if c.C1 else []), gp)
    out["gp"] = gp
    out["dx0"] = grads[0] + inp["add0"].to(dt) if c.add0 else grads[0]
    out["dx1"] = None
    if c.C1:
        out["dx1"] = grads[1] + inp["add1"].to(dt) if c.add1 else grads[1]
    out["dw"] = torch.nn.grad.conv2d_weight(xp.detach(), w.shape, gp)
    out["db"] = gp.sum((0, 2, 3))
    return out


@functools.lru_cache(maxsize=None)
def _reference(key):
    c = key
    inp = build(c)
    return inp, evaluate(c, inp, torch.float64), evaluate(c, inp, torch.float32)


def reference(c):
    """(inputs, fp64 results, fp32 results) of one case; shared and read-only.  Cases that differ only in what they request
    (grads) or in dsplit share one entry."""
    return _reference(c._replace(grads=ALL if c.C1 else ("x0", "w", "b"), dsplit=0))


def db_bound(c, r64):
    """The worst case of an fp32 sum of the n = B H W rounded products gy act'(y) of one channel, in any order."""
    return sum_bound(c.B * c.H * c.W, r64["gp"].abs().sum((0, 2, 3)))


def host_lib():
    return WC.host_lib()


# ---- the launch pair and its gates (GPU; shared by tests/test_conv_block_shapes_gpu.py and tests/conv_block_direct_child.py) ------
DEV = "cuda:0"
GUARD = 256                      # floats on either side of an output or of the workspace
SENTINEL = -7.0312e28
OUTPUTS = {"x0": "dx0", "x1": "dx1", "w": "dw", "b": "db"}


def bits(t):
    return t.contiguous().view(torch.int32)


class Guarded:
    """`n` floats between two guard bands of sentinels; the body starts as NaN."""

    def __init__(self, n):
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
        self.body = self.buf[GUARD:GUARD + n]
        self.body.fill_(float("nan"))
        self.n = n

    def ptr(self):
        return self.body.data_ptr()

    def intact(self):
        want = int(bits(torch.tensor([SENTINEL]))[0])
        return bool((bits(self.buf[:GUARD]) == want).all()) and bool((bits(self.buf[GUARD + self.n:]) == want).all())


def launch(c, inp):
    """One dc_conv3x3_fwd and one dc_conv3x3_bwd_add of `c` on the fp32 inputs `inp`.  Every output and both workspaces (exactly
    the bytes the queries return) sit between guard bands and start as NaN; null outputs get no buffer.  Returns the outputs as
    CPU tensors {y, dx0, dx1, dw, db} (None where not requested); asserts return codes, guards, finiteness and the addends."""
    from depthcore import _lib
    from depthcore._lib import ptr
    L = _lib.lib()
    B, C0, C1, Co, H, W = c.B, c.C0, c.C1, c.Co, c.H, c.W
    d = {k: (None if v is None else v.to(DEV).contiguous()) for k, v in inp.items()}
    st = _lib.stream(d["w"])
    nbytes = L.dc_conv3x3_fwd_workspace(C0, C1, B, Co, H, W)
    assert nbytes > 0 and nbytes % 4 == 0
    y, ws = Guarded(B * Co * H * W), Guarded(nbytes // 4)
    rc = L.dc_conv3x3_fwd(ptr(d["x0"]), C0, c.up0, ptr(d["x1"]), C1, ptr(d["w"]), ptr(d["b"]) if c.bias else None, y.ptr(), ws.ptr(),
                          B, Co, H, W, c.act, c.pad, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert y.intact() and ws.intact(), "the forward wrote outside a buffer"
    shapes = {"dx0": d["x0"].shape, "dx1": (B, C1, H, W), "dw": d["w"].shape, "db": (Co,)}
    out = {k: Guarded(int(torch.Size(shapes[k]).numel())) for g, k in OUTPUTS.items() if g in c.grads}
    add0 = d["add0"].clone() if c.add0 else None
    add1 = None
    if c.add1 == "separate":
        add1 = d["add1"].clone()
    elif c.add1 == "inplace":
        out["dx1"].body.copy_(d["add1"].reshape(-1))
    nbytes = L.dc_conv3x3_bwd_workspace(C0, C1, B, Co, H, W)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = Guarded(nbytes // 4)
    op = lambda k: out[k].ptr() if k in out else None
    prev = L.dc_set_dgrad_split(c.dsplit)
    try:
        rc = L.dc_conv3x3_bwd_add(ptr(d["x0"]), C0, c.up0, ptr(d["x1"]), C1, ptr(d["w"]), ptr(d["y"]), ptr(d["gy"]), op("dx0"), op("dx1"),
                                  ptr(add0), op("dx1") if c.add1 == "inplace" else ptr(add1), op("dw"), op("db"), ws.ptr(),
                                  B, Co, H, W, c.act, c.pad, st)
    finally:
        L.dc_set_dgrad_split(prev)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert ws.intact() and all(g.intact() for g in out.values()), "the backward wrote outside a buffer"
    if add0 is not None:
        assert torch.equal(bits(add0), bits(d["add0"])), "addend0 was modified"
    if add1 is not None:
        assert torch.equal(bits(add1), bits(d["add1"])), "addend1 was modified"
    res = {k: None for k in ("dx0", "dx1", "dw", "db")}
    res["y"] = y.body.cpu().view(B, Co, H, W)
    for k, g in out.items():
        res[k] = g.body.cpu().view(shapes[k])
    for k, v in res.items():
        assert v is None or bool(torch.isfinite(v).all()), "%s has an element that is not finite (left unwritten?)" % k
    return res


def gate(c, res, r64, r32, wino_enabled=True, tag="conv_block_parity"):
    """Prints the share of its bound every output of `res` uses, then asserts them.  Returns {output: share}."""
    r = route(c, wino_enabled)
    kernel = {"y": r["fwd"], "dx0": r["dx"], "dx1": r["dx"], "dw": r["dw"]}
    share, parts = {}, []
    for k in ("y", "dx0", "dx1", "dw"):
        if res[k] is None:
            continue
        t = tol(kernel[k])
        err = rel_err(res[k], r64[k])
        share[k] = err / t
        parts.append("%s %.2e (%.0f%% of %.0e; torch fp32 %.1e)" % (k, err, 100 * err / t, t, rel_err(r32[k], r64[k])))
    if res["db"] is not None:
        bound = db_bound(c, r64).clamp_min(1e-300)
        share["db"] = float(((res["db"].double() - r64["db"]).abs() / bound).max())
        parts.append("db %.1f%% of its sum bound" % (100 * share["db"]))
    print("%s %-58s %s | fwd %s, g' %s, dx %s%s%s, dw %s%s, db %s" % (
        tag, case_id(c), "; ".join(parts), r["fwd"], r["gprime"], r["dx"], " + ring" if r["ring"] else "", " + " + r["fold"] if r["fold"] else "",
        r["dw"], " + %s x%d" % (r["reduce"], r["split"]) if r["reduce"] else "", r["db"]))
    for k, s in share.items():
        assert s <= 1.0, (k, s, kernel.get(k, r["db"]))
    return share


def direct_child_cases():
    """What tests/conv_block_direct_child.py runs under DC_CONV_WINO=0: every table case whose route differs from the default one,
    with all gradients requested (the null patterns of one shape fall together)."""
    seen, out = set(), []
    for c in CASES:
        if route(c, False) == route(c):
            continue
        full = c._replace(grads=ALL if c.C1 else ("x0", "w", "b"))
        if full[:13] not in seen and full in CASES:      # (dsplit means nothing without Winograd)
            seen.add(full[:13])
            out.append(full)
    return out
