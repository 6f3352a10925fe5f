"""The cases of tests/wino_bn_cases.py are fit to judge the BatchNorm-folded Winograd launches with: the table reaches every
mechanism it is there for (computed from transcriptions of wino_plan / wg_plan, which are cross-checked against the library's own
host queries), every case is finite and well conditioned (torch's fp32 evaluation of the statement is within 1e-4 of fp64), no
ReLU decision is a rounding question, the planted ties are "off" in both precisions -- and the entries refuse what they cannot
run (host-side checks: DC_EINVAL before anything is launched).  Needs no GPU."""
import ctypes

import pytest
import torch

import wino_bn_cases as WC

CONV = WC.FWD + WC.DGRAD


def test_case_table_reaches_every_mechanism():
    assert len(set(WC.CASES)) == len(WC.CASES) == len({WC.case_id(c) for c in WC.CASES})
    for kind, cases in (("fwd", WC.FWD), ("dgrad", WC.DGRAD)):
        mm = [WC.mech(c) for c in cases]
        # every sub-region shape; odd H; H = 1; W = 2; a map below one region; overhang in x only, y only, both
        assert {(m["plan"].RH, m["plan"].RW) for m in mm} == set(WC.PS_REGIONS), kind
        assert any(m["odd_H"] for m in mm) and any(c.H == 1 for c in cases) and any(c.W == 2 for c in cases)
        assert any(m["sub_region"] for m in mm)
        assert {(True, False), (False, True), (True, True), (False, False)} <= {(m["hang_x"], m["hang_y"]) for m in mm}, kind
        assert any(m["odd_H"] and m["hang_x"] and m["plan"].per_img > 1 for m in mm)
        # the unsplit reduction everywhere (the epilogues exist for it only), one chunk and nine chunks
        assert all(m["plan"].ksplit == 1 for m in mm)
        assert {1, 9} <= {m["plan"].nchunks for m in mm}, kind
        # a last channel block that is ragged whichever tile the cost model picks
        assert sum(1 for m in mm if m["ragged_M"]) >= 3 and {5, 24, 40, 72} <= {m["M"] for m in mm if m["ragged_M"]}
        # BatchNorm groups: one image per group; >= 2 images per group with >= 2 sub-regions per image; three images per group
        g2 = [m for c, m in zip(cases, mm) if c.groups == 2]
        assert any(m["npg"] == 1 for m in g2) and any(m["npg"] >= 2 and m["plan"].per_img >= 2 for m in g2) and any(m["npg"] == 3 for m in g2)
        # the two-sub-region tile: trailing partial slots (odd nsub), and a block whose halves lie in different groups
        assert any(m["plan"].G == 2 and m["trailing"] for m in mm) and any(m["straddles_groups"] for m in mm)
        assert {16, 32} <= {m["plan"].MT for m in mm}
        assert all(c.Ci <= 128 and c.Co <= 128 for c in cases)
    # forward: the three forms; the loader fold needs whole chunks
    assert {(c.loader, c.stats) for c in WC.FWD} == {(1, 1), (1, 0), (0, 1)}
    assert all(c.Ci % WC.PSK == 0 for c in WC.FWD if c.loader)
    # data gradient: both modes with and without the addend, on one group and on two
    assert {(c.mode, c.addend) for c in WC.DGRAD} == {(2, 0), (2, 1), (3, 0), (3, 1)}
    assert {(c.mode, c.groups) for c in WC.DGRAD} == {(2, 1), (2, 2), (3, 1), (3, 2)}
    # masks: HW % 4 == 0 always; below one 256-element block; between one and two with a ragged tail and odd H; whole blocks
    hw = {c.H * c.W: c for c in WC.DGRAD if c.mode == 3}
    assert all(k % 4 == 0 for k in hw)
    assert any(k < 256 for k in hw) and any(k < 32 for k in hw) and {256, 512} <= set(hw)
    assert any(256 < k < 512 and k % 256 and c.H % 2 for k, c in hw.items())
    assert any(c.W % 4 for c in hw.values())            # rows that start at e & 3 == 2
    # weight gradient: regions, channel tiles, 4-wave groups, splits with a ragged last round, both BNIN variants of each
    wm = [WC.mech(c) for c in WC.WGRAD]
    assert {(m["plan"].RH, m["plan"].RW) for m in wm} == set(WC.WG_REGIONS)
    combos = {(m["plan"].mr, m["plan"].ng, m["bnin"]) for m in wm}
    assert combos == {(2, 1, 1), (2, 1, 2), (4, 1, 1), (4, 1, 2), (4, 2, 1), (4, 2, 2)}
    for ng in (1, 2):
        assert any(m["ragged_round"] and m["plan"].ng == ng for m in wm)
    assert any(m["ragged_round"] and m["plan"].ng == 2 and m["bnin"] == 2 for m in wm)
    assert any(m["plan"].kblocks > 1 and c.Ci % WC.WG_KT for c, m in zip(WC.WGRAD, wm))
    assert any(m["plan"].mblocks > 1 and c.Co % (16 * m["plan"].mr) for c, m in zip(WC.WGRAD, wm))
    assert any(m["odd_H"] for m in wm) and any(c.H == 1 for c in WC.WGRAD) and any(m["hang_x"] for m in wm)
    assert all(c.Ci <= 128 and c.Co <= 128 for c, m in zip(WC.WGRAD, wm) if m["plan"].ng == 1)
    # nothing large: every tensor of every case stays below 6 MB
    assert max(c.B * max(c.Ci, c.Co) * c.H * c.W * 4 for c in WC.CASES) <= 6 << 20
    # the special-purpose cases are table cases
    assert all(c in WC.CASES for c in list(WC.DETERMINISM.values()) + list(WC.BATCH_SPLIT.values()) + [WC.PLAIN_WGRAD])
    assert all(c.groups == 2 for c in WC.DETERMINISM.values()) and all(c.groups == 1 and c.B >= 2 for c in WC.BATCH_SPLIT.values())
    for c in WC.BATCH_SPLIT.values():       # the B = 1 launch runs the same tile variant, so the arithmetic per output is the same
        K, M = WC.conv_dims(c)
        assert WC.ps_plan(1, K, M, c.H, c.W)[:5] + WC.ps_plan(1, K, M, c.H, c.W)[6:] == WC.mech(c)["plan"][:5] + WC.mech(c)["plan"][6:]


@pytest.mark.parametrize("case", WC.params(CONV))
def test_plan_transcription_agrees_with_the_parts_queries(case):
    m = WC.mech(case)
    p = m["plan"]
    nparts, ppg = WC.parts_query(case)
    assert nparts > 0, "the library gives this shape no epilogue"
    assert ppg == 2 * p.regs_x * p.regs_y * (case.B // case.groups) == m["ppg"]
    assert nparts in (2 * p.nsub, 2 * (p.nsub + 1)) and nparts == m["nparts"]
    assert (nparts > 2 * p.nsub) == (p.G == 2 and p.nsub % 2 == 1)
    if case.kind == "dgrad" and case.mode == 3:
        assert WC.host_lib().dc_bn_mask_bytes(case.B, case.Ci, case.H * case.W) == case.B * case.Ci * WC.ceil_div(case.H * case.W, 256) * 32


@pytest.mark.parametrize("case", WC.params(WC.WGRAD))
def test_plan_transcription_agrees_with_the_workspace_query(case):
    p = WC.mech(case)["plan"]
    slab = WC.WG_SLAB_MR4 // 4 * p.mr * 4
    assert p.ws_bytes == p.splits * p.mblocks * p.kblocks * slab
    # (the query also covers the bf16 policy's weight gradient of the same shape: the larger of the two)
    want = max(p.ws_bytes, WC.wgrad_bf16_bytes(case.B, case.Ci, case.Co, case.H, case.W))
    assert WC.host_lib().dc_wino3x3_wgrad_workspace(case.B, case.Ci, case.Co, case.H, case.W) == want


def test_region_transcription_on_the_trunk_maps():
    """The picks the kernels' headers name: 48x160 and 24x80 -> 4x8 / 2x8, 12x40 and 6x20 -> 3x10 / 3x5."""
    assert WC.ps_region(48, 160) == (4, 8) and WC.ps_region(12, 40) == (3, 10) and WC.ps_region(6, 20) == (3, 10)
    assert WC.wg_plan(1, 64, 64, 12, 40)[:2] == (3, 5) and WC.wg_plan(1, 64, 64, 48, 160)[:2] == (2, 8)
    assert WC.ps_plan(*((1,) + WC.SPLIT_REDUCTION[1:])).ksplit > 1


@pytest.mark.parametrize("case", WC.params(WC.CASES))
def test_case_is_well_conditioned(case):
    WC.assert_well_conditioned(case, *WC.reference(case))


# ---- refusals: host-side, DC_EINVAL before anything is launched -------------------------------------------------------------------
class _Mem:
    """Scratch memory an entry point could legally touch if it wrongly accepted a call: device memory where there is a GPU (so a
    regression shows as a wrong return code, not as a launch on host pointers), host memory otherwise."""

    def __init__(self):
        self.keep = []

    def __call__(self, nbytes):
        nbytes = max(int(nbytes), 256)
        if torch.cuda.is_available():
            t = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
            self.keep.append(t)
            return t.data_ptr()
        b = ctypes.create_string_buffer(nbytes + 256)
        self.keep.append(b)
        return (ctypes.addressof(b) + 255) & ~255


def _fold(mem, B, Ci, Co, H, W, groups=1, **on):
    """A dc_bn_fold with every field named in `on` pointing at memory large enough for the shape."""
    from depthcore import _lib
    f = _lib.BnFold()
    f.groups = groups
    size = {"in_scale": 2 * max(Ci, Co) * 4, "in_shift": 2 * max(Ci, Co) * 4, "bn_mean": 2 * max(Ci, Co) * 4,
            "stat_part": Co * 4 * (B * H * W + 8) * 4, "bwd_part": Ci * 4 * (B * H * W + 8) * 4,
            "bn_x": B * Ci * H * W * 4, "bn_mask": B * Ci * WC.ceil_div(H * W, 256) * 32}
    for k, v in on.items():
        if v:
            setattr(f, k, mem(size[k]))
    return f


def _call(entry, fold, B, Ci, Co, H, W, mem, addend_offset=None):
    L = WC.host_lib()
    x, y, w = mem(B * max(Ci, Co) * H * W * 4), mem(B * max(Ci, Co) * H * W * 4), mem(Co * Ci * 36)
    fp = ctypes.byref(fold) if fold is not None else None
    if entry == "fwd":
        return L.dc_wino3x3_fwd_bn(x, w, y, mem(L.dc_wino3x3_workspace(B, Ci, Co, H, W)), B, Ci, Co, H, W, fp, None)
    if entry == "dgrad":
        add = None if addend_offset is None else mem(B * Ci * H * W * 4 + 64) + addend_offset
        return L.dc_wino3x3_dgrad_bn(x, w, y, add, mem(L.dc_wino3x3_workspace(B, Ci, Co, H, W)), B, Ci, Co, H, W, fp, None)
    return L.dc_wino3x3_wgrad_bn(x, y, w, mem(L.dc_wino3x3_wgrad_workspace(B, Ci, Co, H, W)), B, Ci, Co, H, W, fp, None)


REFUSALS = [
    # name, entry, (B, Ci, Co, H, W), groups, fields of the fold that are set
    ("loader fold with Ci % 8 != 0", "fwd", (2, 12, 8, 4, 4), 1, ("in_scale", "in_shift")),
    ("in_scale without in_shift", "fwd", (2, 8, 8, 4, 4), 1, ("in_scale",)),
    ("in_scale without in_shift (weight gradient)", "wgrad", (2, 8, 8, 4, 4), 1, ("in_scale",)),
    ("three groups", "fwd", (3, 8, 8, 4, 4), 3, ("in_scale", "in_shift")),
    ("three groups (statistics)", "fwd", (3, 8, 8, 4, 4), 3, ("stat_part",)),
    ("three groups (data gradient)", "dgrad", (3, 8, 8, 4, 4), 3, ("in_scale", "in_shift", "bn_x", "bn_mean", "bwd_part")),
    ("three groups (weight gradient)", "wgrad", (3, 8, 8, 4, 4), 3, ("in_scale", "in_shift")),
    ("B % groups != 0", "fwd", (3, 8, 8, 4, 4), 2, ("in_scale", "in_shift")),
    ("B % groups != 0 (data gradient)", "dgrad", (3, 8, 8, 4, 4), 2, ("in_scale", "in_shift", "bn_x", "bn_mean", "bwd_part")),
    ("B % groups != 0 (weight gradient)", "wgrad", (3, 8, 8, 4, 4), 2, ("in_scale", "in_shift")),
    ("bwd_part without bn_x", "dgrad", (2, 8, 8, 4, 4), 1, ("in_scale", "in_shift", "bn_mean", "bwd_part")),
    ("bwd_part without bn_mean", "dgrad", (2, 8, 8, 4, 4), 1, ("in_scale", "in_shift", "bn_x", "bwd_part")),
    ("bwd_part with neither a mask nor scale / shift", "dgrad", (2, 8, 8, 4, 4), 1, ("bn_x", "bn_mean", "bwd_part")),
    ("bwd_part with a scale but no shift and no mask", "dgrad", (2, 8, 8, 4, 4), 1, ("in_scale", "bn_x", "bn_mean", "bwd_part")),
    ("a mask with HW % 4 != 0", "dgrad", (2, 8, 8, 3, 2), 1, ("bn_x", "bn_mean", "bn_mask", "bwd_part")),
    ("stat_part together with bwd_part", "dgrad", (2, 8, 8, 4, 4), 1, ("in_scale", "in_shift", "stat_part", "bn_x", "bn_mean", "bwd_part")),
    ("stat_part together with bwd_part (forward entry)", "fwd", (2, 8, 8, 4, 4), 1, ("in_scale", "in_shift", "stat_part", "bn_x", "bn_mean", "bwd_part")),
    ("odd W", "fwd", (2, 8, 8, 4, 5), 1, ("in_scale", "in_shift")),
    ("a split reduction with stat_part", "fwd", WC.SPLIT_REDUCTION, 1, ("stat_part",)),
    ("a split reduction with bwd_part", "dgrad", WC.SPLIT_REDUCTION, 1, ("in_scale", "in_shift", "bn_x", "bn_mean", "bwd_part")),
    # (300000 sub-regions of one tile each: the block index leaves the range in which the kernel's multiply-high division is exact)
    ("sub-region index beyond the exact-division range", "fwd", (300000, 1, 1, 2, 2), 1, ("stat_part",)),
]


@pytest.mark.parametrize("name,entry,shape,groups,fields", [pytest.param(*r, id=r[0].replace(" ", "_")) for r in REFUSALS])
def test_refusals_are_host_side(name, entry, shape, groups, fields):
    L = WC.host_lib()
    L.dc_clear_error()
    idle = L.dc_clear_error()               # 0 with a GPU; without one HIP reports "no device" on every query
    mem = _Mem()
    fold = _fold(mem, *shape, groups=groups, **{k: 1 for k in fields})
    assert _call(entry, fold, *shape, mem=mem) == WC.EINVAL, name
    assert L.dc_clear_error() == idle       # no HIP call failed on the way: nothing was attempted


def test_misaligned_addend_is_refused():
    mem = _Mem()
    shape = (2, 8, 8, 4, 4)
    fold = _fold(mem, *shape, in_scale=1, in_shift=1, bn_x=1, bn_mean=1, bwd_part=1)
    for off in (4, 8, 12):
        assert _call("dgrad", fold, *shape, mem=mem, addend_offset=off) == WC.EINVAL
        assert _call("dgrad", None, *shape, mem=mem, addend_offset=off) == WC.EINVAL       # the plain launch behind a NULL fold too


def test_split_reduction_shape_has_no_epilogue():
    L = WC.host_lib()
    B, Ci, Co, H, W = WC.SPLIT_REDUCTION
    ppg = ctypes.c_int(-1)
    assert L.dc_wino3x3_stat_parts(B, Ci, Co, H, W, 1, ctypes.byref(ppg)) == 0
    assert L.dc_wino3x3_bwd_parts(B, Ci, Co, H, W, 1, ctypes.byref(ppg)) == 0
    assert L.dc_wino3x3_bn_ok(B, Ci, Co, H, W, 1) == 0
    # and the queries' own refusals: three groups, a batch the groups do not divide, odd W
    assert L.dc_wino3x3_stat_parts(3, 8, 8, 4, 4, 3, None) == 0 and L.dc_wino3x3_bwd_parts(3, 8, 8, 4, 4, 2, None) == 0
    assert L.dc_wino3x3_stat_parts(2, 8, 8, 4, 5, 1, None) == 0 and L.dc_wino3x3_bn_ok(2, 12, 8, 4, 4, 1) == 0
    assert L.dc_wino3x3_bn_ok(2, 8, 8, 4, 4, 2) == 1 and L.dc_bn_mask_bytes(2, 8, 6) == 0
