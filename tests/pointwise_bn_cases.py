"""Case table, seeded input builder, plain-torch statement and tile-choice transcriptions for ONE BatchNorm-folded 1x1 GEMM launch
of either tiled kernel family -- fp32-MFMA (csrc/gemm1x1.hip: dc_conv1x1_fwd_bn / _dgrad_bn / _wgrad_bn) and split bf16
(csrc/gemm1x1_x3.hip through dc_pointwise_* under dc_set_gemm_split(1)) -- at the tile, group and mask edges of g1_fwd_kernel,
g1_dgrad_kernel, g1_wgrad_kernel, g1x3_kernel and g1x3_wgrad_kernel.  Shared by tests/test_pointwise_bn_cases_cpu.py (no GPU: the
table reaches its mechanisms, the transcriptions agree with the library's host queries, the cases are well conditioned) and
tests/test_pointwise_bn_shapes_gpu.py (the kernels against the statement).  DESIGN.md, "The BatchNorm-folded 1x1 GEMMs at their
tile, group and mask edges", has the table with its reasons, the gates and the measured figures.

    Case                     (family, kind, B, Ci, Co, H, W, groups, loader, stats, mode, addend)
    build(case)              the builder of tests/wino_bn_cases.py with 1x1 weights: MARGIN, planted exact ties
    evaluate(case, inp, dt)  the statement of tests/wino_bn_cases.py's docstring with conv2d(., w) the 1x1 convolution at stride 1
    reference(case)          cached (inputs, fp64 results, fp32 results); nobody may modify what it returns
    mech(case)               what the launch of this case reaches, computed from the transcribed tile choices

Both families flatten the pixels over the batch (n = b P + p), cut them into tiles of 32 NT pixels, and give each of a block's two
wave columns (16 NT pixels: `cover`) one partial slot: slot s covers the flattened pixels [s cover, (s + 1) cover) that exist."""
import collections
import functools

import torch

import wino_bn_cases as WC

Case = collections.namedtuple("Case", "family kind B Ci Co H W groups loader stats mode addend")

MARGIN, TIE = WC.MARGIN, WC.TIE
TENSOR_TOL = 5e-6             # max|hip - fp64| <= 5e-6 max|fp64|: the bound tests/test_conv1x1_gpu.py holds both families to
EINVAL = -1
TENSORS = {"fwd": "y", "dgrad": "gx", "wgrad": "dW"}
GKC = 32                      # reduction chunk of both families


def _fwd(fam, B, Ci, Co, H, W, groups=1, loader=1, stats=1):
    return Case(fam, "fwd", B, Ci, Co, H, W, groups, loader, stats, 0, 0)


def _dgrad(fam, B, Ci, Co, H, W, groups=1, mode=2, addend=0):
    return Case(fam, "dgrad", B, Ci, Co, H, W, groups, 0, 0, mode, addend)


def _wgrad(fam, B, Ci, Co, H, W, groups=1):
    return Case(fam, "wgrad", B, Ci, Co, H, W, groups, 1, 0, 0, 0)


def _both(make, *a):
    return [make("g1", *a), make("x3", *a)]


# ---- the table (DESIGN.md lists what each case is there for; tests/test_pointwise_bn_cases_cpu.py asserts it from mech()) --------
FWD = (
    [_fwd("g1", 8, 32, 32, 2, 6),                 # P = 12, N = 96: one and a half 64-pixel tiles; 2.67 images per wave column
     _fwd("g1", 3, 32, 40, 2, 2),                 # N = 12 below one wave column, P = 4, Co = 40 ragged
     _fwd("x3", 2, 32, 64, 4, 4),                 # N = 32 below one wave column of the split family's NT = 4 tile (the ppg = 0 shape)
     _fwd("g1", 2, 32, 64, 4, 4),                 # the same shape on the fp32-MFMA family: one wave column, the other empty
     _fwd("g1", 16, 32, 32, 2, 2, 2),             # N / groups = 32: the group boundary between the two wave columns of the one block
     _fwd("g1", 16, 32, 32, 2, 2, 2, 1, 0),       # ... loader only
     _fwd("g1", 16, 32, 32, 2, 2, 2, 0, 1)]       # ... statistics only
    + _both(_fwd, 5, 64, 96, 4, 4)                # N = 80 ragged, P = 16: two images per wave column
    + _both(_fwd, 5, 64, 96, 4, 4, 1, 1, 0)       # ... loader only
    + _both(_fwd, 5, 64, 96, 4, 4, 1, 0, 1)       # ... statistics only
    + _both(_fwd, 3, 32, 64, 4, 12)               # N = 144 ragged, P = 48
    + _both(_fwd, 4, 64, 96, 4, 8, 2)             # two groups, boundary at a block edge
    + _both(_fwd, 4, 64, 96, 4, 8, 2, 1, 0)       # ... loader only
    + _both(_fwd, 4, 64, 96, 4, 8, 2, 0, 1)       # ... statistics only
    + _both(_fwd, 3, 32, 64, 4, 8, 3)             # three groups, one wave column each: a boundary inside the first block
    + _both(_fwd, 6, 64, 96, 4, 4, 3)             # three groups of two images, P = 16
    + _both(_fwd, 4, 32, 96, 128, 128)            # 128 x 128 tiles in both families
    + _both(_fwd, 6, 32, 32, 128, 128, 2)         # 64 x 128 tiles, two groups
    + _both(_fwd, 3, 32, 160, 128, 64)            # x3: 128 x 64 tiles, Co = 160 ragged against 128-row tiles (g1: 64 x 128)
    + _both(_fwd, 3, 32, 160, 128, 64, 3)         # ... three groups
    + [_fwd("g1", 4, 32, 96, 4, 4097)]            # N = 65552: a ragged 128-pixel last tile, NT = 4 lanes past the end (P % 16 != 0: g1 only)
)
DGRAD = (
    [_dgrad("g1", 8, 32, 32, 2, 6, 1, 2, 0),      # P = 12, ragged N, 2.67 images per wave column
     _dgrad("g1", 8, 32, 32, 2, 6, 1, 3, 1),      # ... mask with P = 12, addend
     _dgrad("g1", 8, 32, 32, 2, 6, 1, 3, 0),
     _dgrad("g1", 3, 40, 32, 2, 2, 1, 3, 1),      # N = 12 below one wave column, mask with P = 4, Ci = 40 ragged in the epilogue's reads
     _dgrad("g1", 3, 40, 32, 2, 2, 1, 3, 0),
     _dgrad("g1", 3, 40, 32, 2, 2, 1, 2, 0),
     _dgrad("x3", 2, 64, 32, 4, 4, 1, 2, 0),      # N = 32 below one wave column of the split family's NT = 4 tile
     _dgrad("x3", 2, 64, 32, 4, 4, 1, 3, 1),      # ... mask with P = 16 under NT = 4
     _dgrad("x3", 2, 64, 32, 4, 4, 1, 3, 0),
     _dgrad("g1", 16, 32, 32, 2, 2, 2, 2, 0),     # the group boundary between the two wave columns of the one block
     _dgrad("g1", 16, 32, 32, 2, 2, 2, 3, 1)]
    + _both(_dgrad, 5, 96, 64, 4, 4, 1, 2, 0)     # N = 80 ragged, Ci = 96
    + _both(_dgrad, 7, 96, 64, 4, 4, 1, 3, 1)     # N = 112: mask with P = 16, addend
    + _both(_dgrad, 5, 96, 64, 4, 4, 1, 3, 0)
    + _both(_dgrad, 3, 64, 32, 4, 12, 1, 3, 1)    # N = 144 ragged, P = 48
    + _both(_dgrad, 4, 96, 64, 4, 8, 2, 2, 0)     # two groups
    + _both(_dgrad, 4, 96, 64, 4, 8, 2, 3, 1)
    + _both(_dgrad, 3, 64, 32, 4, 8, 3, 2, 0)     # three groups, one wave column each
    + _both(_dgrad, 6, 96, 64, 4, 4, 3, 3, 1)     # three groups of two images, P = 16
    + _both(_dgrad, 2, 64, 32, 16, 16, 1, 3, 1)   # mask with P = 256: exactly one block
    + _both(_dgrad, 2, 64, 32, 16, 16, 1, 3, 0)
    + _both(_dgrad, 2, 40, 32, 4, 76, 1, 3, 1)    # mask with P = 304: two blocks, the second partial; Ci = 40 ragged
    + _both(_dgrad, 2, 40, 32, 4, 76, 1, 3, 0)
    + _both(_dgrad, 4, 96, 32, 128, 128, 2, 3, 1)     # 128 x 128 tiles in both families, NT = 4 against the mask words
    + _both(_dgrad, 4, 96, 32, 128, 128, 2, 3, 0)     # ... the null-addend arm of the NT = 4 epilogue
    + _both(_dgrad, 4, 96, 32, 128, 128, 2, 2, 0)
    + _both(_dgrad, 6, 160, 32, 64, 64, 3, 3, 1)      # x3: 128 x 64 tiles (NT = 2: w0 in {0, 2}), Ci = 160 ragged
    + _both(_dgrad, 6, 160, 32, 64, 64, 3, 3, 0)
    + _both(_dgrad, 6, 160, 32, 64, 64, 3, 2, 0)
    + _both(_dgrad, 4, 32, 96, 128, 128, 1, 3, 1)     # g1: 64 x 128 tiles; x3: 64 x 64 (twice the fp32-MFMA family's partial count)
    + [_dgrad("g1", 4, 32, 96, 4, 4097, 1, 3, 1),     # ragged 128-pixel last tile
       _dgrad("g1", 4, 32, 96, 4, 4097, 1, 2, 0)]
)
WGRAD = (
    _both(_wgrad, 2, 32, 32, 4, 12, 2)            # P = 48: the second 32-pixel chunk lies in both images = both groups
    + _both(_wgrad, 6, 64, 96, 4, 4, 3)           # ragged rows (Co = 96 on 64-row tiles), P = 16: two images per chunk, three groups
    + _both(_wgrad, 2, 96, 96, 16, 257)           # 257 chunks over 129 splits: a ragged last round
    + _both(_wgrad, 4, 128, 128, 8, 8, 2)         # the 128 x 128 tile, two groups
    + _both(_wgrad, 2, 128, 160, 16, 515, 2)      # the 128 x 128 tile, ragged rows, 515 chunks: a ragged last round, two groups
    + [_wgrad("g1", 8, 32, 32, 2, 6, 2)]          # P = 12: every chunk spans 2.67 images; the group boundary inside chunk 1
)
CASES = FWD + DGRAD + WGRAD
DETERMINISM = _both(_fwd, 5, 64, 96, 4, 4) + _both(_dgrad, 7, 96, 64, 4, 4, 1, 3, 1) + _both(_wgrad, 6, 64, 96, 4, 4, 3)
PLAIN_WGRAD = _both(_wgrad, 2, 32, 32, 4, 12, 2)
# refusals: (what, case)
NO_GROUP_LAYOUT = _both(_fwd, 6, 64, 96, 4, 4, 2)                 # N / groups = 48 is no multiple of a wave column: *_parts returns 0
NO_DGRAD = _dgrad("g1", 3, 32, 40, 2, 2, 1, 2, 0)                 # Co = 40 is no multiple of the reduction chunk
NO_WGRAD = _both(_wgrad, 3, 32, 64, 4, 12)                        # N = 144 is no multiple of the reduction chunk: no tiled weight gradient
MODE2_ADDEND = _both(_dgrad, 5, 96, 64, 4, 4, 1, 2, 1)            # the re-derived decision takes no addend
MODULE_SHAPE = (2, 32, 64, 4, 4)                                  # bnfold.conv1x1 under the default split mode: the ppg = 0 shape
# the stride-2 data gradient with 0, 1 and 2 addends: (B, Ci, Co, Hi, Wi); the second shape has a ragged last pixel tile
STRIDE2 = [(2, 32, 32, 4, 8), (5, 64, 32, 8, 8), (3, 96, 64, 8, 24)]


def case_id(c):
    return c.family + "-" + WC.case_id(c)


def params(cases):
    import pytest
    return [pytest.param(c, id=case_id(c)) for c in cases]


ceil_div = WC.ceil_div


# ---- the host side, transcribed -----------------------------------------------------------------------------------------------------
def _common(B, Ci, Co, H, W, s=1):
    return min(B, Ci, Co, H, W) > 0 and s in (1, 2) and not (s == 2 and (H % 2 or W % 2))


def g1_common(B, Ci, Co, H, W, s=1):
    """g1_common of csrc/gemm1x1.hip."""
    if not _common(B, Ci, Co, H, W, s):
        return False
    Ho, Wo = H // s, W // s
    return not (s == 2 and Wo % 4) and (Ho * Wo) % 4 == 0 and Ci % 4 == 0 and B * max(Ci, Co) * H * W < 2 ** 31


def x3_common(B, Ci, Co, H, W, s=1):
    """g1x3_common of csrc/gemm1x1_x3.hip."""
    if not _common(B, Ci, Co, H, W, s) or (s == 2 and (W // 2) % 4):
        return False
    return ((H // s) * (W // s)) % 16 == 0 and B * max(Ci, Co) * H * W < 2 ** 31


def pass_ok(fam, kind, B, Ci, Co, H, W, s=1):
    """dc_gemm1x1_{fwd,dgrad,wgrad}_ok / dc_gemm1x1x3_{fwd,dgrad,wgrad}_ok."""
    N = B * (H // s) * (W // s)
    if fam == "g1":
        return g1_common(B, Ci, Co, H, W, s) and {"fwd": Ci % GKC == 0, "dgrad": Co % GKC == 0, "wgrad": N % GKC == 0}[kind]
    return x3_common(B, Ci, Co, H, W, s) and {"fwd": Ci % 32 == 0 and Co >= 32, "dgrad": Co % 32 == 0 and Ci >= 32,
                                              "wgrad": Ci % 4 == 0 and Co >= 32 and Ci >= 32 and N % 32 == 0}[kind]


def _g1_lds(kind, mt, nt):
    w = lambda t: 128 if t == 4 else 80
    if kind == "fwd":
        return 2 * (32 * mt * (GKC + 2) + GKC * w(nt)) * 4
    return 2 * GKC * (w(mt) + w(nt)) * 4


def g1_pick(M, N, kind):
    """g1_pick: (MT, NT) of a forward (M = Co) or data-gradient (M = Ci) launch over N flattened pixels."""
    best, pick = 1e300, (2, 2)
    for (mt, nt), penalty in (((4, 4), 1.0), ((2, 4), 1.12), ((2, 2), 1.3)):
        if mt == 4 and M <= 64:
            continue
        blocks = ceil_div(M, 32 * mt) * ceil_div(N, 32 * nt)
        per_cu = max(1, min(4, (150 << 10) // _g1_lds(kind, mt, nt)))
        slots = 256 * per_cu
        rounds = ceil_div(blocks, slots)
        fill = float(blocks) / float(rounds * slots)
        t = float(rounds) * per_cu * mt * nt * penalty * (0.5 + fill if fill < 0.5 and rounds == 1 else 1.0)
        if t < best:
            best, pick = t, (mt, nt)
    return pick


def x3_pick(M, N, stride=1):
    """x3_pick: the split family's (MT, NT)."""
    eff = (0.8, 1.0, 0.75, 0.85) if stride == 2 else (1.0, 0.97, 0.9, 0.85)
    best, pick = -1.0, (2, 2)
    for i, ((mt, nt), per_cu) in enumerate((((4, 4), 2), ((4, 2), 3), ((2, 4), 3), ((2, 2), 4))):
        if mt == 4 and M <= 64:
            continue
        blocks = ceil_div(M, 32 * mt) * ceil_div(N, 32 * nt)
        slots = 256 * per_cu
        rounds = ceil_div(blocks, slots)
        fill = float(blocks) / float(rounds * slots)
        pad = float(M) / float(ceil_div(M, 32 * mt) * 32 * mt)
        score = eff[i] * fill * pad
        if score > best:
            best, pick = score, (mt, nt)
    return pick


def gemm_parts(nt, B, P, groups):
    """gemm_parts of csrc/gemm_tiles.h: (nparts, ppg); (0, 0) = no epilogue with this group layout.  One group owns every partial,
    so its ppg is at least 1 even where N is below one wave column."""
    if groups < 1 or B % groups:
        return 0, 0
    N, cover = B * P, 16 * nt
    if groups > 1 and (N // groups) % cover:
        return 0, 0
    return ceil_div(N, 32 * nt) * 2, max(1, (N // groups) // cover)


def wgrad_plan(fam, B, Ci, Co, H, W):
    """(MT, NT, chunks, splits) of the weight gradient: g1_wpick / g1_wsplits, g1x3_wplan."""
    chunks = B * H * W // GKC
    if fam == "g1":
        mt = nt = 4 if (Co >= 128 and Ci >= 128) else 2
        target = 512 if mt == 4 else 1024
    else:
        mt, nt = (4 if Co >= 128 else 2), (4 if Ci >= 128 else 2)
        target = 256 * (2 if mt * nt >= 16 else (3 if mt * nt >= 8 else 4))
    tiles = ceil_div(Co, 32 * mt) * ceil_div(Ci, 32 * nt)
    s = max(1, min(chunks, ceil_div(target, tiles), 512))
    return mt, nt, chunks, ceil_div(chunks, ceil_div(chunks, s))


def dims(c):
    """(M, K) of a fwd / dgrad launch: output rows and reduction extent."""
    return (c.Ci, c.Co) if c.kind == "dgrad" else (c.Co, c.Ci)


def tile(c):
    N = c.B * c.H * c.W
    if c.kind == "wgrad":
        return wgrad_plan(c.family, c.B, c.Ci, c.Co, c.H, c.W)[:2]
    return g1_pick(dims(c)[0], N, c.kind) if c.family == "g1" else x3_pick(dims(c)[0], N)


def takes(c):
    """the family takes the pass of this case (for x3: and the dispatcher under split mode 1 therefore gives it the pass)."""
    ok = pass_ok(c.family, c.kind, c.B, c.Ci, c.Co, c.H, c.W)
    if ok and c.kind != "wgrad":
        ok = gemm_parts(tile(c)[1], c.B, c.H * c.W, c.groups)[0] > 0
    return ok


def mech(c):
    """What the launch reaches, from the transcriptions alone."""
    P = c.H * c.W
    N, npg = c.B * P, c.B // c.groups
    mt, nt = tile(c)
    m = {"tile": (32 * mt, 32 * nt), "MT": mt, "NT": nt, "P": P, "N": N, "npg": npg}
    if c.kind == "wgrad":
        _, _, chunks, splits = wgrad_plan(c.family, c.B, c.Ci, c.Co, c.H, c.W)
        per = ceil_div(chunks, splits)
        bounds = [g * npg * P for g in range(1, c.groups)]
        m.update(chunks=chunks, splits=splits, ragged_round=splits > 1 and chunks % per != 0,
                 chunk_straddles_groups=any(b % GKC for b in bounds), chunk_straddles_images=P % GKC != 0,
                 ragged_rows=c.Co % (32 * mt) != 0 or c.Ci % (32 * nt) != 0)
        return m
    M = dims(c)[0]
    BN, cover = 32 * nt, 16 * nt
    nparts, ppg = gemm_parts(nt, c.B, P, c.groups)
    bounds = [g * npg * P for g in range(1, c.groups)]
    m.update(M=M, cover=cover, nparts=nparts, ppg=ppg,
             ragged=N % BN,                                          # pixels of the last tile that exist (0: the tile is full)
             empty_column=0 < N % BN <= cover,                        # the last tile's second wave column lies wholly outside N
             below_column=N < cover,                                  # not even one wave column is full
             lanes_past_end=(cover - N % cover) % cover // nt,        # lanes of the last live wave column whose pixels do not exist
             images_per_column=float(cover) / P,
             boundary_in_block=[b % BN == cover for b in bounds],     # a group boundary between the two wave columns of one block
             boundary_at_block=[b % BN == 0 for b in bounds],
             ragged_rows=M % (32 * mt) != 0,
             mask_blocks=ceil_div(P, 256), mask_partial=P % 256 != 0)
    return m


# ---- builder and statement: those of tests/wino_bn_cases.py with 1x1 weights ------------------------------------------------------
tie_positions, tie_mask, decision_preact, rel_err, sum_bound, stat_bounds = (
    WC.tie_positions, WC.tie_mask, WC.decision_preact, WC.rel_err, WC.sum_bound, WC.stat_bounds)


def build(c):
    return WC.build(c, ksize=1, tag="pointwise_bn")


def evaluate(c, inp, dt):
    return WC.evaluate(c, inp, dt, padding=0)


@functools.lru_cache(maxsize=6)
def _reference(c):
    inp = build(c)
    return inp, evaluate(c, inp, torch.float64), evaluate(c, inp, torch.float32)


def reference(c):
    """(inputs, fp64 results, fp32 results) of one case, the same for both families (cached without the family: the g1 and x3 twins
    of a shape share one evaluation); shared and read-only."""
    return _reference(c._replace(family=""))


# ---- the library's queries ---------------------------------------------------------------------------------------------------------
def host_lib():
    return WC.host_lib()


def parts_query(c, which=None):
    """(nparts, ppg) from the library: which = "g1" (dc_conv1x1_*_parts), "x3" (dc_gemm1x1x3_*_parts) or "pw" (dc_pointwise_*_parts
    under the current split mode); default: the case's family, x3 through the dispatcher."""
    import ctypes
    L, ppg = host_lib(), ctypes.c_int(-7)
    which = which or {"g1": "g1", "x3": "pw"}[c.family]
    a = (c.B, c.Ci, c.Co, c.H, c.W)
    if c.kind == "dgrad":
        n = {"g1": lambda: L.dc_conv1x1_bwd_parts(*a, c.groups, ctypes.byref(ppg)),
             "x3": lambda: L.dc_gemm1x1x3_bwd_parts(*a, c.groups, ctypes.byref(ppg)),
             "pw": lambda: L.dc_pointwise_bwd_parts(*a, 1, c.groups, ctypes.byref(ppg))}[which]()
    else:
        n = {"g1": L.dc_conv1x1_stat_parts, "x3": L.dc_gemm1x1x3_stat_parts, "pw": L.dc_pointwise_stat_parts}[which](
            *a, 1, c.groups, ctypes.byref(ppg))
    return n, ppg.value
