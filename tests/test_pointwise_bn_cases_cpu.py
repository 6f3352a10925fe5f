"""The cases of tests/pointwise_bn_cases.py are fit to judge the BatchNorm-folded 1x1 GEMM launches with: the table reaches every
mechanism it is there for in BOTH kernel families (computed from transcriptions of g1_pick / x3_pick / gemm_parts and the
weight-gradient plans, which are cross-checked against the library's own host queries), the dispatcher under dc_set_gemm_split(1)
gives the split family every pass of an x3 case, every *_parts query that returns a count returns at least one partial per group,
and every case is finite and well conditioned with no ReLU decision a rounding question.  Needs no GPU."""
import ctypes

import pytest

import pointwise_bn_cases as PC
import wino_bn_cases as WC

CONV = PC.FWD + PC.DGRAD
FAMILIES = ("g1", "x3")


@pytest.fixture
def L():
    lib = PC.host_lib()
    prev = lib.dc_get_gemm_split()
    try:
        yield lib
    finally:
        lib.dc_set_gemm_split(prev)


def test_case_table_reaches_every_mechanism():
    assert len(set(PC.CASES)) == len(PC.CASES) == len({PC.case_id(c) for c in PC.CASES})
    assert all(PC.takes(c) for c in PC.CASES)
    for fam in FAMILIES:
        for kind, cases in (("fwd", PC.FWD), ("dgrad", PC.DGRAD)):
            cases = [c for c in cases if c.family == fam]
            mm = [PC.mech(c) for c in cases]
            both = list(zip(cases, mm))
            where = (fam, kind)
            # a last pixel tile that is partly outside N: lanes of a live wave column without pixels, and a wholly empty wave column
            assert any(m["lanes_past_end"] > 0 for m in mm) and any(m["empty_column"] for m in mm), where
            assert any(m["lanes_past_end"] > 0 and m["empty_column"] for m in mm), where
            # N below one wave column: the partial count is positive and every partial is group 0's (the ppg >= 1 contract)
            assert any(m["below_column"] and m["nparts"] == 2 and m["ppg"] == 1 for m in mm), where
            # a wave column that spans several images
            assert any(m["images_per_column"] >= 2 for m in mm), where
            # BatchNorm groups: 1, 2 and 3; a boundary between the two wave columns of one block, and one at a block edge
            assert {1, 2, 3} <= {c.groups for c in cases}, where
            assert any(any(m["boundary_in_block"]) for m in mm) and any(any(m["boundary_at_block"]) for m in mm), where
            assert any(c.groups == 3 and m["npg"] == 2 and m["P"] == 16 for c, m in both), where
            # ragged output rows
            assert any(m["ragged_rows"] and m["M"] > 32 * m["MT"] for m in mm) and any(m["ragged_rows"] and m["tile"][0] == 128 for m in mm), where
        # the tiles each family instantiates with a fold, reached through the pickers' own choices
        ftiles = {PC.mech(c)["tile"] for c in PC.FWD if c.family == fam}
        dtiles = {PC.mech(c)["tile"] for c in PC.DGRAD if c.family == fam}
        if fam == "g1":
            assert ftiles == {(64, 64), (64, 128), (128, 128)} == dtiles
        else:
            assert ftiles == {(64, 64), (64, 128), (128, 64), (128, 128)} and dtiles >= {(64, 64), (64, 128), (128, 64), (128, 128)}
        # forward: loader only / statistics only / both, on a ragged shape and on a grouped one
        fw = [(c, PC.mech(c)) for c in PC.FWD if c.family == fam]
        for pick in (lambda c, m: m["lanes_past_end"] > 0, lambda c, m: c.groups > 1):
            assert {(c.loader, c.stats) for c, m in fw if pick(c, m)} == {(1, 1), (1, 0), (0, 1)}, fam
        assert any(c.Co in (40, 96, 160) and m["ragged_rows"] for c, m in fw)
        # data gradient: both decisions; the mask with and without the addend at every plane size
        dg = [(c, PC.mech(c)) for c in PC.DGRAD if c.family == fam]
        assert {(c.mode, c.addend) for c, m in dg} == {(2, 0), (3, 0), (3, 1)}
        planes = {}
        for c, m in dg:
            if c.mode == 3:
                planes.setdefault(m["P"], set()).add(c.addend)
        assert all(p % 4 == 0 for p in planes)
        need = [16, 256, 304] + ([4, 12] if fam == "g1" else [])           # (the split kernels take P % 16 == 0 only)
        assert all(planes.get(p) == {0, 1} for p in need), (fam, planes)
        assert any(m["mask_blocks"] == 2 and m["mask_partial"] for c, m in dg if c.mode == 3)
        # ... and under large tiles: NT = 4, and NT = 2 (w0 in {0, 2}), each with and without the addend (the null-addend arm of the
        # epilogue is a line of its own per NT)
        big = {(m["NT"], c.addend) for c, m in dg if c.mode == 3 and m["N"] >= 16384}
        assert {(4, 0), (4, 1)} <= big and (fam == "g1" or {(2, 0), (2, 1)} <= big), (fam, big)
        assert fam == "g1" or any(m["tile"] == (128, 64) and c.addend == a for a in (0, 1) for c, m in dg if c.mode == 3)
        assert any(m["NT"] == 2 and m["P"] % 4 == 0 and m["P"] % 8 for c, m in dg if c.mode == 3) or fam == "x3"     # p & 3 == 2 starts a row
        # ragged Ci in the epilogue's clamped bn_x / mask reads
        assert all(any(m["ragged_rows"] and c.mode == mode and c.Ci in (40, 96, 160) for c, m in dg) for mode in (2, 3))
        # weight gradient
        wm = [(c, PC.mech(c)) for c in PC.WGRAD if c.family == fam]
        assert any(m["chunk_straddles_groups"] and m["splits"] <= 4 for c, m in wm), fam
        assert any(m["ragged_round"] and m["tile"] == (64, 64) for c, m in wm) and any(m["ragged_round"] and m["tile"] == (128, 128) for c, m in wm)
        assert any(m["tile"] == (128, 128) and c.groups == 2 for c, m in wm) and any(m["ragged_rows"] for c, m in wm)
    assert (2, 32, 32, 4, 12, 2) in {tuple(c[2:8]) for c in PC.WGRAD}
    # the special-purpose cases: table cases, one per kind and family
    assert all(c in PC.CASES for c in PC.DETERMINISM + PC.PLAIN_WGRAD)
    assert {(c.family, c.kind) for c in PC.DETERMINISM} == {(f, k) for f in FAMILIES for k in ("fwd", "dgrad", "wgrad")}
    # nothing large: every tensor of every case stays below 32 MB, the largest case is N = 98304 pixels
    assert max(c.B * max(c.Ci, c.Co) * c.H * c.W * 4 for c in PC.CASES) <= 32 << 20
    assert max(c.B * c.H * c.W for c in PC.CASES) == 98304


def _ok(L, fam, kind, a):
    """the library's word on whether `fam` takes the pass (the fp32-MFMA predicates are exported through their queries only)"""
    if fam == "x3":
        return bool(getattr(L, "dc_gemm1x1x3_%s_ok" % kind)(*a, 1))
    if kind == "fwd":
        return L.dc_conv1x1_stat_parts(*a, 1, 1, None) > 0
    if kind == "dgrad":
        return L.dc_conv1x1_bwd_parts(*a, 1, None) > 0
    return None


SHAPES = sorted({tuple(c[2:7]) for c in PC.CASES + PC.NO_GROUP_LAYOUT + [PC.NO_DGRAD] + PC.NO_WGRAD} | {PC.MODULE_SHAPE})


def test_predicates_agree_with_the_library(L):
    for a in SHAPES:
        for fam in FAMILIES:
            for kind in ("fwd", "dgrad", "wgrad"):
                got = _ok(L, fam, kind, a)
                if got is not None:
                    assert got == PC.pass_ok(fam, kind, *a), (fam, kind, a)
        assert bool(L.dc_conv1x1_bn_ok(*a)) == all(PC.pass_ok("g1", k, *a) for k in ("fwd", "dgrad", "wgrad")), a
    for c in PC.NO_WGRAD:
        assert not PC.pass_ok(c.family, "wgrad", *c[2:7]) and PC.pass_ok(c.family, "fwd", *c[2:7])
    assert not PC.pass_ok("g1", "dgrad", *PC.NO_DGRAD[2:7]) and PC.pass_ok("g1", "fwd", *PC.NO_DGRAD[2:7])


@pytest.mark.parametrize("case", PC.params(CONV))
def test_tile_transcription_agrees_with_the_parts_queries(L, case):
    """count and partials per group, from the family's own query and -- x3 cases -- from the dispatcher under split mode 1, which
    must therefore have chosen the split family; under mode 0 the dispatcher answers with the fp32-MFMA family's layout"""
    m = PC.mech(case)
    want = (m["nparts"], m["ppg"])
    assert want[0] > 0 and want == PC.gemm_parts(m["NT"], case.B, m["P"], case.groups)
    assert PC.parts_query(case, case.family) == want
    g1 = case._replace(family="g1")
    g1_want = PC.gemm_parts(PC.tile(g1)[1], case.B, m["P"], case.groups) if PC.pass_ok("g1", case.kind, *case[2:7]) else (0, -7)
    assert PC.parts_query(case, "g1") == (g1_want if g1_want[0] else (0, -7))
    L.dc_set_gemm_split(0)
    assert PC.parts_query(case, "pw") == PC.parts_query(case, "g1")
    L.dc_set_gemm_split(1)
    x3 = PC.parts_query(case, "x3")
    assert PC.parts_query(case, "pw") == (x3 if x3[0] else PC.parts_query(case, "g1"))
    if case.family == "x3":
        assert x3 == want and bool(getattr(L, "dc_gemm1x1x3_%s_ok" % case.kind)(*case[2:7], 1))
    if case.kind == "dgrad" and case.mode == 3:
        assert L.dc_bn_mask_bytes(case.B, case.Ci, m["P"]) == case.B * case.Ci * m["mask_blocks"] * 32


def test_the_families_lay_their_partials_out_differently_where_the_table_says(L):
    """what makes `x3 through the dispatcher` a statement about the chosen family: on these shapes the two layouts differ"""
    differ = [c for c in CONV if c.family == "x3" and PC.parts_query(c, "x3") != PC.parts_query(c, "g1")]
    assert {c.kind for c in differ} == {"fwd", "dgrad"}


@pytest.mark.parametrize("case", PC.params(PC.WGRAD))
def test_weight_gradient_plan_agrees_with_the_workspace_queries(L, case):
    a = case[2:7]
    m = PC.mech(case)
    want = m["splits"] * case.Co * case.Ci * 4 if m["splits"] > 1 else 16
    if case.family == "g1":
        assert L.dc_conv1x1_wgrad_workspace(*a, 1) == want
    else:
        assert L.dc_gemm1x1x3_wgrad_ok(*a, 1) and L.dc_gemm1x1x3_wgrad_workspace(*a, 1) == want
        from depthcore import _lib
        f = _lib.BnFold()
        f.groups = case.groups
        L.dc_set_gemm_split(1)
        assert L.dc_pointwise_workspace(2, ctypes.byref(f), *a, 1) == want          # the dispatcher gives the pass to the split family


@pytest.mark.parametrize("mode", [0, 1])
def test_every_positive_partial_count_has_a_positive_ppg(L, mode):
    """The contract of include/depthcore.h -- partial p belongs to group min(p / ppg, groups - 1) -- needs ppg >= 1 wherever a count
    is returned; dc_bn_finalize and dc_bn_bwd_finalize refuse ppg < 1.  N below one wave column (32 or 64 pixels) with one group
    used to return ppg = 0 with a positive count: the table's shapes, the module-level shape, and a sweep of small maps."""
    L.dc_set_gemm_split(mode)
    shapes = set(SHAPES)
    for B in (1, 2, 3, 4):
        for hw in ((2, 2), (2, 4), (2, 6), (4, 4), (2, 8), (4, 12)):
            for Ci, Co in ((32, 32), (32, 64), (64, 32), (64, 256), (2048, 512)):
                shapes.add((B, Ci, Co) + hw)
    seen_small = 0
    for a in sorted(shapes):
        B = a[0]
        for groups in (1, 2, 3):
            for name, fn, args in (("conv1x1_stat", L.dc_conv1x1_stat_parts, a + (1, groups)), ("conv1x1_bwd", L.dc_conv1x1_bwd_parts, a + (groups,)),
                                   ("x3_stat", L.dc_gemm1x1x3_stat_parts, a + (1, groups)), ("x3_bwd", L.dc_gemm1x1x3_bwd_parts, a + (groups,)),
                                   ("pointwise_stat", L.dc_pointwise_stat_parts, a + (1, groups)), ("pointwise_bwd", L.dc_pointwise_bwd_parts, a + (1, groups))):
                ppg = ctypes.c_int(-7)
                n = fn(*args, ctypes.byref(ppg))
                assert n >= 0
                if n > 0:
                    assert ppg.value >= 1, (name, a, groups, n, ppg.value)
                    assert B % groups == 0 and (groups - 1) * ppg.value < n, (name, a, groups, n, ppg.value)     # every group owns a partial
                    seen_small += B * a[3] * a[4] < 32
    assert seen_small >= 8
    ppg = ctypes.c_int(-7)
    assert L.dc_pointwise_stat_parts(*PC.MODULE_SHAPE, 1, 1, ctypes.byref(ppg)) == 2 and ppg.value == 1


def test_group_layouts_without_an_epilogue_return_zero(L):
    for mode in (0, 1):
        L.dc_set_gemm_split(mode)
        for c in PC.NO_GROUP_LAYOUT:
            assert not PC.takes(c)
            for which in ("g1", "x3", "pw"):
                assert PC.parts_query(c, which)[0] == 0
                assert PC.parts_query(c._replace(kind="dgrad"), which)[0] == 0
    assert PC.parts_query(PC.NO_DGRAD)[0] == 0 and not PC.takes(PC.NO_DGRAD)


UNIQUE = sorted({c._replace(family="") for c in PC.CASES})


@pytest.mark.parametrize("case", [pytest.param(c, id=WC.case_id(c)) for c in UNIQUE])
def test_case_is_well_conditioned(case):
    WC.assert_well_conditioned(case, *PC.reference(case))
