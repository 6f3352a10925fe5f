"""The cases of tests/wino_split_cases.py are fit to judge the split Winograd reductions with: the tables reach every slab
mechanism they are there for (computed from the transcribed plan and workspace layout), the transcription agrees with the library
where the library can be asked (the epilogue queries refuse exactly the launches that split; dc_wino3x3_workspace byte for byte,
also under plan streams), every slab's channel range is what it should be, and every case is well conditioned (torch's fp32
evaluation of the statement within 1e-4 of fp64 -- a condition on the inputs, not on the kernel).  Needs no GPU."""
import pytest

import conv_block_cases as CC
import wino_bn_cases as WC
import wino_split_cases as WS


def _hit(cases, **want):
    """The cases whose mech() has every given value (a callable is a predicate on the value)."""
    out = []
    for c in cases:
        m = WS.mech(c)
        if all(v(m[k]) if callable(v) else m[k] == v for k, v in want.items()):
            out.append(c)
    return out


def test_case_tables_reach_every_mechanism():
    everything = WS.CASES + WS.FORCED
    assert len(set(everything)) == len(everything) == len({WS.case_id(c) for c in everything})
    for kind, cases in (("fwd", WS.FWD), ("dgrad", [c for c in WS.DGRAD if not c.addend]), ("dgrad", [c for c in WS.DGRAD if c.addend])):
        assert all(c.kind == kind for c in cases) and len(cases) == len(WS.SHAPES)
        by_shape = {(c.B,) + WS.conv_dims(c) + (c.H, c.W): WS.mech(c) for c in cases}
        # the rows of the issue's table, each with the plan claimed for it
        m = by_shape[(1, 128, 5, 2, 2)]
        assert (m["ksplit"], m["slab_chunks"], m["MT"], m["m_fast"], m["nsub"]) == (8, [2] * 8, 16, False, 1)
        m = by_shape[(1, 129, 5, 2, 2)]
        assert (m["nchunks"], m["cps"], m["slab_chunks"], m["empty"], m["beyond"], m["K_mod_8"]) == (17, 3, [3, 3, 3, 3, 3, 2, 0, 0], 2, 2, 1)
        assert m["ragged_last"] and [lo for lo, _ in m["ranges"]][6:] == [129, 129]
        for K in (128, 129):
            a, b = by_shape[(1, K, 5, 2, 2)], by_shape[(1, K, 5, 6, 20)]
            assert b["m_fast"] and not a["m_fast"] and b["slab_chunks"] == a["slab_chunks"]
            assert (b["plan"].RH, b["plan"].RW) == (3, 10)
        m = by_shape[(3, 129, 512, 10, 16)]
        assert (m["ksplit"], m["slab_chunks"], m["MT"], m["ragged_last"]) == (4, [5, 5, 5, 2], 16, True)
        m = by_shape[(3, 128, 512, 7, 44)]
        assert (m["ksplit"], m["MT"], m["G"], m["nchunks"], m["odd_H"]) == (4, 32, 1, 16, True)
        m = by_shape[(3, 128, 512, 10, 16)]
        assert (m["ksplit"], m["MT"], m["G"]) == (8, 32, 1)
        m = by_shape[(3, 256, 512, 12, 40)]
        assert m["nout"] * 4 > WS.SMALL_OUT and (m["ksplit"], m["nchunks"]) == (2, 32)
        assert by_shape[(1,) + WC.SPLIT_REDUCTION[1:]]["ksplit"] == 8
        # found by searching with the transcription: an empty slab that begins exactly at nchunks, next to one beyond it
        assert _hit(cases, at_end=1, beyond=1, ksplit=8)
        # every case splits; every slab count the cap allows; both tiles; ragged and whole M; one and several sub-regions
        mm = list(by_shape.values())
        assert all(m["ksplit"] > 1 for m in mm) and {m["ksplit"] for m in mm} == {2, 4, 8}
        assert {m["MT"] for m in mm} == {16, 32} and {m["ragged_M"] for m in mm} == {True, False}
        assert any(m["nsub"] == 1 for m in mm) and any(m["nsub"] > 3 for m in mm)
    # the cost model picks no split on the 32 x 64 variant and none of 9 chunks over 4 slabs: the forced plans reach them
    assert not _hit(WS.CASES, G=2)
    assert not _hit(WS.CASES, nchunks=9)
    assert _hit(WS.FORCED, G=2, ksplit=4, ragged_last=True, ragged_M=True, nsub=3)
    for kind in ("fwd", "dgrad"):
        assert _hit([c for c in WS.FORCED if c.kind == kind], nchunks=9, ksplit=4, slab_chunks=[3, 3, 3, 0], at_end=1, beyond=0)
        assert _hit([c for c in WS.FORCED if c.kind == kind], G=2)
    assert _hit(WS.FORCED, MT=32, G=1, beyond=2)
    g2 = [c for c in _hit(WS.FORCED, G=2) if c.kind == "loader"]
    assert g2 and all(c.groups == 2 and c.B == 2 and WS.mech(c)["nsub"] == 2 for c in g2)        # one block, two BatchNorm groups
    assert all(c.force and WS.parse_force(c.force) for c in WS.FORCED) and all(c.force is None for c in WS.CASES)
    # without the forced plan, none of the forced cases reaches what it is there for
    for c in WS.FORCED:
        free, forced = WS.mech(c._replace(force=None)), WS.mech(c)
        assert (free["MT"], free["G"], free["ksplit"]) != (forced["MT"], forced["G"], forced["ksplit"])
    # the loader fold: whole chunks; groups 1 and 2; the 17-chunk edge through 136 channels; one and two images per group; both tiles
    assert all(c.Ci % WS.PSK == 0 and c.B % c.groups == 0 for c in WS.LOADER)
    assert {c.groups for c in WS.LOADER} == {1, 2}
    for groups in (1, 2):
        assert _hit([c for c in WS.LOADER if c.groups == groups and c.Ci == 136], nchunks=17, empty=2, beyond=2)
    assert {c.B // c.groups for c in WS.LOADER if c.groups == 2} == {1, 2}
    assert {WS.mech(c)["MT"] for c in WS.LOADER} == {16, 32} and any(WS.mech(c)["m_fast"] for c in WS.LOADER)
    # the special-purpose cases are table cases
    assert all(c in WS.CASES for c in WS.DETERMINISM.values())
    assert any(WS.mech(c)["ragged_last"] for c in WS.DETERMINISM.values()) and any(WS.mech(c)["empty"] for c in WS.DETERMINISM.values())
    # nothing large: every tensor below 6 MB
    assert max(c.B * max(c.Ci, c.Co) * c.H * c.W * 4 for c in everything) <= 6 << 20


def test_fused_cases_reach_their_launches_split():
    cases = WS.fused_cases()
    assert len(set(cases)) == len(cases)
    mm = [(c, WS.block_mech(c), CC.route(c)) for c in cases]
    for c, bm, r in mm:
        assert r["fwd"] == "wino_conv_fused_fwd" and bm["fwd"]["ksplit"] > 1, CC.case_id(c)
        assert c.dsplit == 2 and r["w_dx"]
    # the fused slab sum: bias present and null, activations 0-4, a plain, an upsampled and a concatenated source
    assert {c.act for c in cases} == {0, 1, 2, 3, 4} and {c.bias for c in cases} == {0, 1}
    assert {(0, 0), (1, 0), (0, 1), (1, 1)} <= {(c.up0, int(c.C1 > 0)) for c in cases}
    assert all(c.C0 % WS.PSK == 0 for c in cases if c.C1)
    assert any(c.act and not c.bias for c in cases) and any(c.bias and not c.act for c in cases) and any(not c.bias and not c.act for c in cases)
    assert any(bm["fwd"]["empty"] for _, bm, _ in mm) and any(bm["fwd"]["m_fast"] for _, bm, _ in mm)
    # the bias index (i / plane4) % M: M that is no power of two, over more than one image
    assert any(c.Co in (5, 24) and c.B > 1 and c.bias for c in cases)
    # the data gradient: the split of its P = 1 plan is the ONLY reason the split store is refused, and the P = 2 launch splits too
    full = cases[-WS.FUSED_FULL_DGRAD:]
    for c, bm, r in mm:
        # everything else wino_dgrad_split_ok asks for holds
        assert c.H >= 4 and c.W >= 4 and c.H % 2 == 0 and c.W % 2 == 0 and c.C0 > 0
        assert CC.dgrad_split_ok(c.B, c.C0, c.C1, c.Co, c.H, c.W) == (c not in full)
        if c in full:
            assert bm["dgrad_same"]["ksplit"] > 1 and bm["dgrad_full"]["ksplit"] > 1
            assert (r["dx"], r["ring"]) == ("wino_conv_full_dgrad", False) and r["fold"] is not None
        else:
            assert bm["dgrad_same"]["ksplit"] == 1 and r["dx"] == "wino_conv_dgrad_split"
    # (zero padding takes the split store whatever Co: there the split of the plan is the one reason it is refused)
    assert sum(1 for c in full if c.pad == CC.ZERO) >= 3
    assert {bool(c.add0) for c in full} == {True, False} and any(c.add1 for c in full) and any(c.up0 for c in full)
    assert any(bm["dgrad_full"]["empty"] for c, bm, _ in mm if c in full)
    assert {c.pad for c in full} == {CC.REFLECT, CC.ZERO}


def _stream_cases():
    return [WS.Case(kind, B, Ci, Co, H, W, 1, 0, None) for B, Ci, Co, H, W in WS.LOCKSTEP_SHAPES for kind in ("fwd", "dgrad")]


def test_plan_streams_in_the_transcription():
    """dc_set_wino_plan_streams(3): tile variant and split are those of ONE stream's launch.  On (3, 512, 512, 6, 20) the batch
    of three takes that plan anyway; on (3, 512, 512, 12, 40) it would take 2 slabs (a 2.9 MB output) where one stream takes 8."""
    for c in _stream_cases():
        one, three, lock = WS.mech(c._replace(B=1)), WS.mech(c), WS.mech(c, streams=WS.LOCKSTEP)
        pick = lambda m: (m["MT"], m["G"], m["ksplit"])
        assert pick(lock) == pick(one) and lock["ksplit"] == 8 and lock["nsub"] == three["nsub"] == 3 * one["nsub"]
        assert (pick(three) != pick(one)) == ((c.H, c.W) == (12, 40)), WS.case_id(c)
    assert WS.mech(_stream_cases()[-1])["ksplit"] == 2


@pytest.mark.parametrize("case", WS.params(WS.CASES + WS.FORCED))
def test_transcription_agrees_with_the_library(case, monkeypatch):
    """The epilogue queries return 0 exactly when the transcribed plan splits (asked with and, for a forced case, without the
    forced plan), and dc_wino3x3_workspace is the transcribed total."""
    L = WS.host_lib()
    free = case._replace(force=None)
    monkeypatch.delenv("DC_WINO_FORCE", raising=False)
    assert (WS.parts_query(free) == 0) == (WS.mech(free)["ksplit"] > 1)
    if case.force:
        monkeypatch.setenv("DC_WINO_FORCE", case.force)       # (read per query)
        assert WS.parts_query(case) == 0 and WS.mech(case)["ksplit"] > 1
        monkeypatch.delenv("DC_WINO_FORCE")
    else:
        assert WS.mech(case)["ksplit"] > 1, "a table case that does not split"
    assert L.dc_wino3x3_workspace(case.B, case.Ci, case.Co, case.H, case.W) == WS.workspace_bytes(case.B, case.Ci, case.Co, case.H, case.W)
    # the slabs of the split the plan picks (or is forced to) fit behind the transformed weights
    m = WS.mech(case)
    assert WS.slab_offset_floats(case.Ci, case.Co, m["ksplit"], m["nout"]) * 4 <= WS.workspace_bytes(case.B, case.Ci, case.Co, case.H, case.W)


@pytest.mark.parametrize("shape", [(1, 5, 128, 6, 20), (2, 24, 16, 8, 12), (1, 40, 72, 6, 20), (1, 72, 40, 6, 20)])
def test_unsplit_launches_keep_their_epilogue(shape):
    """The other direction of the equivalence: where the transcribed plan does not split, the queries grant partials."""
    for kind in ("fwd", "dgrad"):
        c = WS.case_of(kind, *shape)                   # (B, K, M, H, W) in either role
        assert WS.mech(c)["ksplit"] == 1 and WS.parts_query(c) > 0


@pytest.mark.parametrize("case", WS.params(_stream_cases()))
def test_workspace_under_plan_streams(case):
    L = WS.host_lib()
    B, Ci, Co, H, W = case[1:6]
    prev = L.dc_set_wino_plan_streams(WS.LOCKSTEP)
    try:
        got = L.dc_wino3x3_workspace(B, Ci, Co, H, W)
    finally:
        assert L.dc_set_wino_plan_streams(prev) == WS.LOCKSTEP
    assert got == WS.workspace_bytes(B, Ci, Co, H, W, streams=WS.LOCKSTEP)
    assert L.dc_wino3x3_workspace(B, Ci, Co, H, W) == WS.workspace_bytes(B, Ci, Co, H, W)
    # (the 12 x 40 shape tells the two apart: a stream's third of the output is below 2 MB, the whole is not)
    assert (got != WS.workspace_bytes(B, Ci, Co, H, W)) == ((H, W) == (12, 40))
    m = WS.mech(case, streams=WS.LOCKSTEP)
    assert WS.slab_offset_floats(Ci, Co, m["ksplit"], m["nout"]) * 4 <= got


@pytest.mark.parametrize("case", WS.params(WS.CASES + WS.FORCED))
def test_slab_ranges_partition_the_reduction(case):
    m = WS.mech(case)
    K = m["K"]
    assert len(m["ranges"]) == len(m["slab_chunks"]) == m["ksplit"] and sum(m["slab_chunks"]) == m["nchunks"]
    at = 0
    for (lo, hi), n in zip(m["ranges"], m["slab_chunks"]):
        assert lo <= hi <= K and (hi > lo) == (n > 0)
        if n:
            assert lo == at and lo % WS.PSK == 0 and WS.ceil_div(hi - lo, WS.PSK) == n
            at = hi
    assert at == K
    assert m["empty"] == m["at_end"] + m["beyond"] == sum(1 for lo, hi in m["ranges"] if lo == hi)
    assert m["cps"] * m["ksplit"] >= m["nchunks"] and m["cps"] >= 2


@pytest.mark.parametrize("case", WS.params(WS.CASES + WS.FORCED))
def test_case_is_well_conditioned(case):
    WS.assert_well_conditioned(case)


@pytest.mark.parametrize("case", CC.params(WS.fused_cases()))
def test_fused_case_is_well_conditioned_and_routed_as_transcribed(case):
    assert CC.plan_mismatches(case) == []
    L = CC.host_lib()
    assert L.dc_conv3x3_fwd_workspace(case.C0, case.C1, case.B, case.Co, case.H, case.W) == CC.fwd_workspace(case)
    assert L.dc_conv3x3_bwd_workspace(case.C0, case.C1, case.B, case.Co, case.H, case.W) == CC.bwd_workspace(case)
    inp, r64, r32 = CC.reference(case)
    for k, v in r64.items():
        if v is not None and k != "db":
            assert CC.rel_err(r32[k], v) < CC.E32_MAX, (k, CC.rel_err(r32[k], v))
    assert float(r64["y"].abs().max()) > 0.1
