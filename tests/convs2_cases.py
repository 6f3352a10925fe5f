"""Case table, seeded input builder, fp64 statement and host-dispatch transcription for the strided trunk convolutions
(csrc/convgemm.hip: dc_convs2_fwd / _wgrad / _dgrad and dc_stem_fwd / _wgrad) at the edges of their dispatch and of their tiles: the
patch-staged 7x7 stem (fp32 and split-operand forward, raw-frame loader, the weight gradient's tile walk), the triple-gather 3x3
kernels (tile picks, even and uneven reduction slabs), the general gather kernels (every tile pick of both kernel sizes, padded
weight rows, the scalar slab reduce) and the parity data gradient (output-channel slabs, Ci off the 64-row tile).  Shared by
tests/test_convs2_cases_cpu.py (no GPU: the table reaches every mechanism, route() agrees field by field with the plan the launches
follow (dc_convs2_plan_query) and with the three workspace queries, the rows are well conditioned and the gate sees a single dropped
term, the refusals are host-side), tests/test_convs2_shapes_gpu.py (the kernels against the statement) and
tests/convs2_gather_child.py (the triple-gather and stem rows on the gather kernels, DC_STEM_PATCH=0 DC_CONV_TRIP=0).  DESIGN.md, "The
strided convolutions at their dispatch edges", has the table with its reasons, the predicates, the gate and the measured figures.

    Case                         (B, Ci, Co, H, W, k, only): `only` names the outputs that are checked (None: all the plan has)
    build(case)                  seeded fp32 inputs x, w, gy (stem rows: rand frames too; x is their normalised concat)
    evaluate(case, inp, dt)      the statement in `dt`: y = conv2d(x, w, None, 2, k // 2), dx and dw by autograd
    reference(case)              cached (inputs, fp64 results, fp32 results); nobody may modify what it returns
    route(case, split_mode, env, raw, bf16)
                                 what the launches run, transcribed from the host code (independent of the library: it never asks
                                 dc_convs2_plan_query; plan_mismatches() compares the two).  DC_FWD3_SPLIT / DC_DGRAD3_SPLIT
                                 (experiments) are taken as unset.
    launch(case, inp, ...)       the launches through the C ABI between guards, NaN-prefilled"""
import collections
import ctypes
import functools
import zlib

import torch
import torch.nn.functional as F

import conv_block_cases as CC

Case = collections.namedtuple("Case", "B Ci Co H W k only")

GATE = CC.DIRECT_TOL            # max|hip - fp64| <= 1e-5 max|fp64| for y, dx and dw (tests/test_convs2_gpu.py)
CONDITION = 0.25                # torch's fp32 evaluation of the statement stays within this share of the gate
SENSITIVITY = 10.0              # a single dropped term misses the gate by at least this factor
EINVAL = -1
MEAN, STD = 0.45, 0.225         # networks/resnet_encoder.py:89

# csrc/gemm_tiles.h, csrc/convgemm.hip, csrc/gemm1x1_x3.hip
GKC, KC3, ST_TH, ST_TW, STEM_MAX_BLOCKS, X3_KC = 32, 96, 2, 64, 512, 32

ceil_div = CC.ceil_div
rel_err = CC.rel_err
al256 = CC.al256
bits = CC.bits


def K(B, Ci, Co, H, W, k, only=None):
    return Case(B, Ci, Co, H, W, k, only)


# ---- the table (DESIGN.md lists what each row is there for; tests/test_convs2_cases_cpu.py asserts it from route()) ---------------
TRIP = [
    K(1, 32, 64, 2, 8, 3),          # Ho = 1, Wo = 4, N = 4: every gather group touches the padding; forward unsplit; one partial chunk
    K(1, 32, 256, 12, 8, 3),        # forward unsplit; data gradient over 4 output-channel slabs
    K(1, 64, 128, 6, 8, 3),         # forward 2 slabs; data gradient 2 slabs; N = 12
    K(1, 128, 128, 6, 8, 3),        # forward 4 slabs (12 super-chunks, 3 each)
    K(2, 288, 40, 6, 8, 3),         # 27 super-chunks over 4 slabs (7/7/7/6); Co = 40: a ragged row tile; no data gradient
    K(1, 96, 64, 10, 16, 3),        # 9 super-chunks over 2 slabs (5/4)
    K(3, 64, 64, 6, 24, 3),         # P = 36: 64-pixel tiles span images; N = 108: partial last chunk; 4 weight-gradient slabs
    K(1, 64, 64, 20, 136, 3),       # <2,4> with 2 slabs; N = 680: ragged last pixel tile; 22 weight-gradient slabs
    K(1, 32, 40, 20, 136, 3),       # <2,4> unsplit
]
GATHER3 = [
    K(1, 5, 7, 4, 8, 3),            # K = 45 padded to 64; Co = 7, N = 8: everything ragged; one weight-gradient slab
    K(2, 5, 7, 12, 16, 3),          # 3 weight-gradient slabs of 315 elements: the scalar slab reduce
    K(3, 36, 64, 10, 24, 3),        # <2,2,3>; 6 slabs, 16-byte reduce; data gradient with Ci = 36
    K(1, 8, 32, 20, 24, 3),         # data gradient with Ci = 8, one chunk of output channels per tap
    K(1, 20, 160, 6, 8, 3),         # three row tiles, the last ragged (160 = 64 + 64 + 32)
    K(1, 12, 8, 64, 160, 3),        # <2,4,3>
    K(1, 4, 96, 512, 512, 3, only=("y",)),    # <4,4,3>; forward only (its fp32 CPU weight gradient uses 0.89 of the gate itself)
]
SEVEN = [
    K(1, 3, 64, 2, 8, 7),           # stem: one tile, one output row, 4 of 64 columns
    K(1, 6, 64, 2, 8, 7),
    K(19, 3, 64, 108, 8, 7),        # 513 tiles on 512 blocks: 2 per block, block 256 gets one, 255 blocks write zero slabs
    K(2, 3, 64, 6, 136, 7),         # Ho = 3 (odd), Wo = 68: the second tile is 4 columns wide
    K(2, 6, 64, 6, 136, 7),
    K(1, 3, 16, 6, 8, 7),           # gather <2,2,7>, Co = 16
    K(1, 4, 64, 8, 16, 7),          # gather <2,2,7>: Co = 64 but Ci = 4
    K(2, 3, 96, 20, 24, 7),         # gather <2,2,7>, Co = 96: two row tiles
    K(1, 3, 16, 16, 64, 7),         # gather <2,4,7>
    K(1, 3, 96, 512, 512, 7, only=("y",)),    # gather <4,4,7>; forward only (the 65536-pixel weight gradient is the 3x3 row's question)
]
CASES = TRIP + GATHER3 + SEVEN
SPLIT3 = {"eligible": K(1, 64, 64, 16, 32, 3), "ineligible": K(1, 64, 128, 6, 8, 3)}     # Ho Wo = 128 (N % 32 == 0) / Ho Wo = 12
DETERMINISM = {"stem": K(2, 6, 64, 6, 136, 7), "trip": K(3, 64, 64, 6, 24, 3), "gather": K(3, 36, 64, 10, 24, 3)}
NO_ENV = {}
GATHER_ENV = {"DC_STEM_PATCH": "0", "DC_CONV_TRIP": "0"}


def case_id(c):
    return "b%d-%dto%d-%dx%d-k%d" % c[:6]


def params(cases):
    import pytest
    return [pytest.param(c, id=case_id(c)) for c in cases]


# ---- the dispatch, transcribed ------------------------------------------------------------------------------------------------------
def supported(B, Ci, Co, H, W, k):
    if min(B, Ci, Co, H, W) <= 0 or k not in (3, 7) or H % 2 or W % 2 or (W // 2) % 4:
        return False
    return B * max(Ci, Co) * H * W < 1 << 29


def _on(env, name):
    """A DC_* switch: on unless set to something atoi() reads as 0."""
    v = env.get(name)
    if v is None:
        return True
    digits = v.strip()
    sign = digits[:1] in "+-"
    n = ""
    for ch in digits[1 if sign else 0:]:
        if not ch.isdigit():
            break
        n += ch
    return int(n or "0") != 0


def cg_pick(M, N):
    blocks = lambda mt, nt: ceil_div(M, 32 * mt) * ceil_div(N, 32 * nt)
    if M > 64 and blocks(4, 4) >= 500:
        return 4, 4
    if blocks(2, 4) >= 300 or N >= 8 * M:
        return 2, 4
    return 2, 2


def cg_wsplits(tiles, chunks):
    s = max(1, min(chunks, ceil_div(768, tiles), 512))
    return ceil_div(chunks, ceil_div(chunks, s))


def fwd3_plan(Ci, Co, N):
    tile = (2, 4) if ceil_div(Co, 64) * ceil_div(N, 128) >= 300 or N >= 8 * Co else (2, 2)
    blocks, nsc, s = ceil_div(Co, 64) * ceil_div(N, 32 * tile[1]), Ci * 9 // KC3, 1
    while s < 4 and blocks * s * 2 <= 768 and nsc // (s * 2) >= 3:
        s *= 2
    return tile, s


def dgrad3_splits(B, Ci, Co, H, W):
    blocks, s = ceil_div(Ci, 64) * ceil_div(B * (H // 2) * (W // 2), 64) * 2, 1
    while s < 4 and blocks * s * 2 <= 768 and (Co // GKC) % (s * 2) == 0 and (Co // GKC) // (s * 2) >= 2:
        s *= 2
    return s


def g1x3_ok(split_mode, B, Ci, Co, H, W):
    if not split_mode or Ci % 32 or Co < 32:
        return False
    return ((H // 2) * (W // 2)) % 16 == 0 and B * max(Ci, Co) * H * W < 1 << 31


def g1x3_wslabs(npx, Co, Kc):
    chunks, mt, nt = npx // X3_KC, 4 if Co >= 128 else 2, 4 if Kc >= 128 else 2
    target = 256 * (2 if mt * nt >= 16 else (3 if mt * nt >= 8 else 4))
    s = max(1, min(chunks, ceil_div(target, ceil_div(Co, 32 * mt) * ceil_div(Kc, 32 * nt)), 512))
    splits = ceil_div(chunks, ceil_div(chunks, s))
    return splits * Co * Kc * 4 if splits > 1 else 16


def c3b_wgrad_split_s2(B, Ho, Wo, Co, Ci):
    ntiles, outer = ceil_div(Wo, 32) * ceil_div(Ho, 4) * B, ceil_div(Co, 64) * ceil_div(Ci, CC.C3B_BC)
    return min(max(1, min(ntiles, 512 // max(outer, 1))), 256)


def route(c, split_mode=1, env=NO_ENV, raw=0, bf16=False):
    """The plan of one shape as csrc/convgemm.hip: cg_plan decides it, with the geometry the coverage test asks about.  `raw`: through
    dc_stem_* (None when that entry refuses the shape).  Families: fwd stem_x3 | stem_f32 | trip | gather | g1x3 | bf16; dw stem | trip |
    gather | g1x3 | bf16; dx None | parity | bf16; reduce None | scalar | 16b."""
    B, Ci, Co, H, W, k = c[:6]
    if not supported(B, Ci, Co, H, W, k):
        return None
    Ho, Wo = H // 2, W // 2
    P, N, Kk = Ho * Wo, B * Ho * Wo, Ci * k * k
    Kp = ceil_div(Kk, GKC) * GKC
    stem = _on(env, "DC_STEM_PATCH") and k == 7 and Co == 64 and Ci in (3, 6)
    trip = not stem and _on(env, "DC_CONV_TRIP") and k == 3 and Ci % 32 == 0
    if raw and not stem:
        return None
    r = dict(Ho=Ho, Wo=Wo, P=P, N=N, K=Kk, Kp=Kp, stem=stem, trip=trip, raw=raw, wpad_f32=Kp != Kk)
    b16 = bf16 and k == 3                       # (c3b_eligible holds for every supported stride-2 shape: W % 8 == 0, H % 2 == 0)
    x3_f = not b16 and k == 3 and bool(split_mode & 2) and g1x3_ok(split_mode, B, Ci, Co, H, W)
    x3_w = x3_f and N % 32 == 0
    # forward
    r.update(fwd_mt=0, fwd_nt=0, fwd_slabs=0, fwd_wpad=0, f32_slabs=1)
    if stem:
        r["fwd"] = "stem_x3" if _on(env, "DC_STEM_X3") and split_mode != 0 else "stem_f32"
        r["fwd_wpad"] = 1
        tx, ty = ceil_div(Wo, ST_TW), ceil_div(Ho, ST_TH)
        nt = B * ty * tx
        nb = min(nt, STEM_MAX_BLOCKS)
        per = ceil_div(nt, nb)
        r.update(tiles_x=tx, tiles_y=ty, ntiles=nt, nblocks=nb, per=per, working=ceil_div(nt, per), last_tiles=nt - (ceil_div(nt, per) - 1) * per)
    else:
        tile, r["f32_slabs"] = fwd3_plan(Ci, Co, N) if trip else (cg_pick(Co, N), 1)
        r["f32_tile"] = tile
        if trip:
            nsc, sp = Kk // KC3, r["f32_slabs"]
            per = ceil_div(nsc, sp)
            r["slab_chunks"] = [max(0, min(per, nsc - z * per)) for z in range(sp)]
        r["fwd"] = "trip" if trip else "gather"
        r.update(fwd_mt=tile[0], fwd_nt=tile[1], fwd_slabs=r["f32_slabs"] if trip else 0, fwd_wpad=int(Kp != Kk))
        r.update(fwd_mtiles=ceil_div(Co, 64 if trip else 32 * tile[0]), fwd_ntiles=ceil_div(N, 32 * tile[1]))
    if b16 or x3_f:
        r.update(fwd="bf16" if b16 else "g1x3", fwd_mt=0, fwd_nt=0, fwd_slabs=0, fwd_wpad=0)
    # weight gradient
    r.update(dw_slabs=0, dw_blocks=0, dw_tiles_per_block=0, reduce=None, f32_wsplits=0)
    if stem:
        r.update(dw="stem", dw_blocks=r["nblocks"], dw_tiles_per_block=r["per"], reduce="16b")
    else:
        r["w_mtiles"], r["w_ntiles"], r["chunks"] = ceil_div(Co, 64), ceil_div(Kk, KC3 if trip else 64), ceil_div(N, GKC)
        r["f32_wsplits"] = cg_wsplits(r["w_mtiles"] * r["w_ntiles"], r["chunks"])
        r.update(dw="trip" if trip else "gather", dw_slabs=r["f32_wsplits"])
        if r["f32_wsplits"] > 1:
            r["reduce"] = "16b" if (Co * Kk) % 4 == 0 else "scalar"
    if b16 or x3_w:
        r.update(dw="bf16" if b16 else "g1x3", dw_slabs=0, dw_blocks=0, dw_tiles_per_block=0, reduce=None)
    # data gradient
    has_dx = k == 3 and Ci % 4 == 0 and Co % GKC == 0
    r["f32_dxsp"] = dgrad3_splits(B, Ci, Co, H, W) if has_dx else 0
    r["dx"] = None if not has_dx else ("bf16" if b16 else "parity")
    r["dx_slabs"] = r["f32_dxsp"] if r["dx"] == "parity" else 0
    # the three workspace queries (they cover the fp32 family, the bf16 route and -- while dc_get_gemm_split() != 0 -- the split one)
    wb = CC.c3b_weights_bytes(Ci, Co) if k == 3 else 0
    wpad = 16 if Kp == Kk else Co * Kp * 4 + (Co * Kp * 6 + 512 if k == 7 else 0)
    x3ok = k == 3 and g1x3_ok(split_mode, B, Ci, Co, H, W)
    r["fwd_ws"] = max(wpad, wb, r["f32_slabs"] * B * Co * P * 4 if r["f32_slabs"] > 1 else 0,
                      ceil_div(Co, 128) * 128 * 9 * Ci * 6 + 512 if x3ok else 0)
    if stem:
        r["wgrad_ws"] = r["nblocks"] * 64 * Kp * 4
    else:
        r["wgrad_ws"] = max(r["f32_wsplits"] * Co * Kk * 4 if r["f32_wsplits"] > 1 else 16,
                            c3b_wgrad_split_s2(B, Ho, Wo, Co, Ci) * Co * Kk * 4 if k == 3 else 0,
                            g1x3_wslabs(N, Co, 9 * Ci) if x3ok and N % 32 == 0 else 0)
    r["dgrad_ws"] = max(al256(9 * Co * Ci * 4) + (r["f32_dxsp"] * B * Ci * H * W * 4 if r["f32_dxsp"] > 1 else 0), wb) if has_dx else 0
    return r


# ---- the library's own plan (include/depthcore.h: dc_convs2_plan, the DC_S2_* enums) against route() -------------------------------
PLAN_FWD = {"stem_x3": 0, "stem_f32": 1, "trip": 2, "gather": 3, "g1x3": 4, "bf16": 5}
PLAN_DW = {"stem": 0, "trip": 1, "gather": 2, "g1x3": 3, "bf16": 4}
PLAN_RED = {None: 0, "scalar": 1, "16b": 2}
PLAN_DX = {None: 0, "parity": 1, "bf16": 2}


def plan_of(r):
    """route()'s answer as the fields of dc_convs2_plan."""
    return {"fwd": PLAN_FWD[r["fwd"]], "fwd_mt": r["fwd_mt"], "fwd_nt": r["fwd_nt"], "fwd_slabs": r["fwd_slabs"], "fwd_wpad": r["fwd_wpad"],
            "dw": PLAN_DW[r["dw"]], "dw_slabs": r["dw_slabs"], "dw_blocks": r["dw_blocks"], "dw_tiles_per_block": r["dw_tiles_per_block"],
            "dw_reduce": PLAN_RED[r["reduce"]], "dx": PLAN_DX[r["dx"]], "dx_slabs": r["dx_slabs"]}


def host_lib():
    return CC.host_lib()


def plan_query(c, raw=0):
    """dc_convs2_plan_query under the split mode and precision in effect: (return code, {field: value})."""
    from depthcore import _lib
    p = _lib.ConvS2Plan()
    rc = host_lib().dc_convs2_plan_query(c.B, c.Ci, c.Co, c.H, c.W, c.k, int(bool(raw)), ctypes.byref(p))
    return rc, {n: getattr(p, n) for n, _ in p._fields_}


class split_mode:
    """with split_mode(m): dc_set_gemm_split(m), restored on the way out."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = host_lib().dc_get_gemm_split()
        host_lib().dc_set_gemm_split(self.mode)

    def __exit__(self, *exc):
        host_lib().dc_set_gemm_split(self.prev)


def plan_mismatches(c, mode=1, env=NO_ENV, raw=0):
    """[(field, the library's value, route()'s value)] -- plan fields and the three workspace queries -- empty when they agree.  The
    process must have been started under `env`."""
    L = host_lib()
    want = route(c, mode, env, raw)
    with split_mode(mode):
        rc, got = plan_query(c, raw)
        ws = {"fwd_ws": L.dc_convs2_fwd_workspace(*c[:6]), "wgrad_ws": L.dc_convs2_wgrad_workspace(*c[:6]),
              "dgrad_ws": L.dc_convs2_dgrad_workspace(*c[:6])}
    if want is None:
        return [] if rc == EINVAL else [("rc", rc, EINVAL)]
    if rc != 0:
        return [("rc", rc, 0)]
    wp = plan_of(want)
    assert set(wp) == set(got)
    return [(k, got[k], wp[k]) for k in sorted(wp) if got[k] != wp[k]] + [(k, ws[k], want[k]) for k in sorted(ws) if ws[k] != want[k]]


def stem_rows(cases=None):
    return [c for c in (CASES if cases is None else cases) if route(c)["stem"]]


def raw_modes(c):
    """The nf of dc_stem_* that feed the row's shape: 1 (3 channels); 2, and 3 where the batch is two pair groups (6 channels)."""
    return (1,) if c.Ci == 3 else ((2, 3) if c.B % 2 == 0 else (2,))


def outputs(c, r=None):
    """The outputs of the row that are checked: y, dw, and dx where the plan has a data gradient -- less what `only` leaves out."""
    r = route(c) if r is None else r
    out = ("y", "dw") + (("dx",) if r["dx"] else ())
    return tuple(o for o in out if c.only is None or o in c.only)


# ---- the builder and the statement ------------------------------------------------------------------------------------------------
def build(c):
    """fp32 inputs of one row (CPU tensors): x, w scaled by (Ci k^2)^-1/2, gy.  Stem rows: x is (cat(frames) - 0.45) / 0.225 of rand
    frames, computed on the CPU (a subtraction and a true division, as the kernels' loader does it); `frames[nf]` are what dc_stem_*
    gets -- for nf = 2 and 3 they describe the SAME x (nf = 3: the pairs (g0, g1), (g1, g2) stacked along the batch)."""
    B, Ci, Co, H, W, k = c[:6]
    g = torch.Generator().manual_seed(zlib.crc32(repr(("convs2", tuple(c[:6]))).encode()))
    inp = {"frames": {}}
    if route(c)["stem"]:
        if Ci == 3:
            f = torch.rand(B, 3, H, W, generator=g)
            inp["frames"][1], raw = (f,), f
        elif B % 2 == 0:
            g0, g1, g2 = (torch.rand(B // 2, 3, H, W, generator=g) for _ in range(3))
            inp["frames"][3] = (g0, g1, g2)
            inp["frames"][2] = (torch.cat([g0, g1], 0), torch.cat([g1, g2], 0))
            raw = torch.cat([torch.cat([g0, g1], 1), torch.cat([g1, g2], 1)], 0)
        else:
            f0, f1 = torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g)
            inp["frames"][2], raw = (f0, f1), torch.cat([f0, f1], 1)
        inp["x"] = ((raw - MEAN) / STD).contiguous()
    else:
        inp["x"] = torch.randn(B, Ci, H, W, generator=g)
    inp["w"] = torch.randn(Co, Ci, k, k, generator=g) * (1.0 / (Ci * k * k)) ** 0.5
    inp["gy"] = torch.randn(B, Co, H // 2, W // 2, generator=g)
    return inp


def evaluate(c, inp, dt):
    """{y, dw, dx} of the statement in `dt` (y and the outputs the row checks; the others None)."""
    want = outputs(c)
    with_dx = "dx" in want
    x, w = inp["x"].to(dt).clone().requires_grad_(with_dx), inp["w"].to(dt).clone().requires_grad_("dw" in want)
    y = F.conv2d(x, w, None, 2, c.k // 2)
    out = {"y": y.detach(), "dw": None, "dx": None}
    need = ([w] if "dw" in want else []) + ([x] if with_dx else [])
    if need:
        grads = list(torch.autograd.grad(y, need, inp["gy"].to(dt)))
        if "dw" in want:
            out["dw"] = grads.pop(0)
        if with_dx:
            out["dx"] = grads.pop(0)
    return out


@functools.lru_cache(maxsize=None)
def reference(c):
    """(inputs, fp64 results, fp32 results) of one row; shared and read-only."""
    inp = build(c)
    return inp, evaluate(c, inp, torch.float64), evaluate(c, inp, torch.float32)


def single_term(c, inp, r64, name):
    """The fp64 statement of output `name` with ONE term removed, as (mutated tensor, the term): the smallest error a wrong tap, a
    missed pixel or a skipped channel can make at this shape.  The term sits at the last pixel of the last image and the centre tap
    (inside the image at every shape); among the channels it could belong to, the one of median magnitude is taken -- a typical
    term, neither the largest nor one that happens to vanish.
        y   one (ci, tap) product of channel Co - 1;  dw  one pixel's gy x product;  dx  one (co, tap) product of channel Ci - 1"""
    B, Ci, Co, H, W, k = c[:6]
    x, w, gy = inp["x"].double(), inp["w"].double(), inp["gy"].double()
    b, oy, ox, t = B - 1, H // 2 - 1, W // 2 - 1, k // 2
    iy, ix = 2 * oy, 2 * ox                              # the centre tap's input pixel: 2 o + t - k // 2
    out = r64[name].clone()
    if name == "y":
        terms = w[Co - 1, :, t, t] * x[b, :, iy, ix]
        j = int(terms.abs().argsort()[len(terms) // 2])
        out[b, Co - 1, oy, ox] -= terms[j]
        return out, float(terms[j])
    if name == "dw":
        terms = gy[b, :, oy, ox, None] * x[b, None, :, iy, ix]
        flat = terms.abs().flatten().argsort()
        j = int(flat[len(flat) // 2])
        out[j // Ci, j % Ci, t, t] -= terms[j // Ci, j % Ci]
        return out, float(terms[j // Ci, j % Ci])
    terms = w[:, Ci - 1, t, t] * gy[b, :, oy, ox]
    j = int(terms.abs().argsort()[len(terms) // 2])
    out[b, Ci - 1, iy, ix] -= terms[j]
    return out, float(terms[j])


# ---- the launches and their gate (GPU; shared by tests/test_convs2_shapes_gpu.py and tests/convs2_gather_child.py) ------------------
DEV = CC.DEV
Guarded = CC.Guarded


def launch(c, inp, what=("y", "dw", "dx"), raw=0):
    """dc_convs2_fwd / _wgrad / _dgrad of `c` (raw = nf > 0: dc_stem_fwd / _wgrad on inp["frames"][nf]) for the outputs named in
    `what`, under the split mode in effect.  Every output and every workspace -- exactly the bytes its query returns -- sits between
    guard bands and starts as NaN.  Returns CPU tensors {y, dw, dx} (None where not run); asserts return codes, guards, finiteness."""
    from depthcore import _lib
    from depthcore._lib import ptr
    L = _lib.lib()
    B, Ci, Co, H, W, k = c[:6]
    Ho, Wo = H // 2, W // 2
    x, w, gy = (inp[n].to(DEV).contiguous() for n in ("x", "w", "gy"))
    st = _lib.stream(w)
    if raw:
        fr = [f.to(DEV).contiguous() for f in inp["frames"][raw]]
        fptr = (ctypes.c_void_p * raw)(*[ptr(f) for f in fr])
        Bf = fr[0].shape[0]
        assert L.dc_stem_supported(raw, Bf, Co, H, W) == 1
    shapes = {"y": (B, Co, Ho, Wo), "dw": (Co, Ci, k, k), "dx": (B, Ci, H, W)}
    query = {"y": L.dc_convs2_fwd_workspace, "dw": L.dc_convs2_wgrad_workspace, "dx": L.dc_convs2_dgrad_workspace}
    res = {n: None for n in shapes}
    for name in ("y", "dw", "dx"):
        if name not in what:
            continue
        nbytes = query[name](B, Ci, Co, H, W, k)
        assert nbytes > 0 and nbytes % 4 == 0, (name, nbytes)
        out, ws = Guarded(int(torch.Size(shapes[name]).numel())), Guarded(nbytes // 4)
        if name == "y" and raw:
            rc = L.dc_stem_fwd(fptr, raw, MEAN, STD, ptr(w), out.ptr(), ws.ptr(), Bf, H, W, Co, st)
        elif name == "y":
            rc = L.dc_convs2_fwd(ptr(x), ptr(w), out.ptr(), ws.ptr(), B, Ci, Co, H, W, k, st)
        elif name == "dw" and raw:
            rc = L.dc_stem_wgrad(fptr, raw, MEAN, STD, ptr(gy), out.ptr(), ws.ptr(), Bf, H, W, Co, st)
        elif name == "dw":
            rc = L.dc_convs2_wgrad(ptr(x), ptr(gy), out.ptr(), ws.ptr(), B, Ci, Co, H, W, k, st)
        else:
            assert not raw
            rc = L.dc_convs2_dgrad(ptr(gy), ptr(w), out.ptr(), ws.ptr(), B, Ci, Co, H, W, k, st)
        assert rc == 0, (name, rc)
        torch.cuda.synchronize()
        assert out.intact() and ws.intact(), "%s: the launch wrote outside a buffer" % name
        res[name] = out.body.cpu().view(shapes[name])
        assert bool(torch.isfinite(res[name]).all()), "%s has an element that is not finite (left unwritten?)" % name
    return res


def gate(c, res, r64, r32, tag="convs2_parity", note=""):
    """Prints the figures of every output of `res` the row checks, then asserts the gate.  Returns {output: err / max}."""
    errs = {}
    for name in outputs(c):
        if res.get(name) is None:
            continue
        errs[name] = rel_err(res[name], r64[name])
        print("%s %s %s err/max %.3e (%.0f%% of %.0e; torch fp32 %.1e) %s" % (
            tag, case_id(c), name, errs[name], 100 * errs[name] / GATE, GATE, rel_err(r32[name], r64[name]), note))
    for name, e in errs.items():
        assert e <= GATE, (case_id(c), name, e)
    return errs


def describe(r):
    return "fwd %s<%d,%d> x%d%s, dw %s x%d %s, dx %s x%d" % (
        r["fwd"], r["fwd_mt"], r["fwd_nt"], r["fwd_slabs"], " wpad" if r["fwd_wpad"] else "", r["dw"], r["dw_slabs"] or r["dw_blocks"],
        r["reduce"], r["dx"], r["dx_slabs"])


def gather_child_cases():
    """What tests/convs2_gather_child.py runs under DC_STEM_PATCH=0 DC_CONV_TRIP=0: the rows whose route changes."""
    return [c for c in CASES if route(c, 1, GATHER_ENV) != route(c)]
