"""The rows of tests/convs2_cases.py are fit to judge the strided trunk convolutions with: the table reaches every mechanism it is
there for (computed by route(), the transcription of csrc/convgemm.hip: cg_plan) and every row is the only witness of one of them;
route() agrees field by field with the plan the launches themselves follow (dc_convs2_plan_query) and with the three workspace
queries, for every row, split mode and entry, in this process and under the DC_* switches in fresh ones; every checked output is
well conditioned (torch's fp32 evaluation of the statement stays within a quarter of the gate) and the gate sees a single dropped
term at every shape; and the entries refuse what they cannot run before any HIP call.  Needs no GPU."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import convs2_cases as S
from convs2_cases import K

MODES = (0, 1, 3)


def _nsc(c, r):
    return r["K"] // S.KC3


# name -> predicate(case, default route).  Each names one thing the suite did not launch before this table (the list in DESIGN.md).
MECHANISMS = {
    # ---- triple-gather forward (cg_fwd3_kernel)
    "trip: Ho = 1 and Wo = 4 (N = 4: every gather group touches the padding)": lambda c, r: r["fwd"] == "trip" and (r["Ho"], r["Wo"], r["N"]) == (1, 4, 4),
    "trip forward <2,2> unsplit with more than one row tile": lambda c, r: r["fwd"] == "trip" and r["f32_tile"] == (2, 2) and r["fwd_slabs"] == 1 and r["fwd_mtiles"] > 1,
    "trip forward 2 slabs, even": lambda c, r: r["fwd"] == "trip" and r["f32_tile"] == (2, 2) and r["slab_chunks"] == [3, 3],
    "trip forward 4 slabs, even": lambda c, r: r["fwd"] == "trip" and r["fwd_slabs"] == 4 and len(set(r["slab_chunks"])) == 1,
    "trip forward 4 uneven slabs (7/7/7/6) and a ragged row tile (Co = 40)": lambda c, r: r["fwd"] == "trip" and r["slab_chunks"] == [7, 7, 7, 6] and c.Co % 64 == 40,
    "trip forward 2 uneven slabs (5/4)": lambda c, r: r["fwd"] == "trip" and r["slab_chunks"] == [5, 4],
    "trip: pixel tiles span images (P = 36, N = 108 over two 64-pixel tiles)": lambda c, r: r["fwd"] == "trip" and c.B > 1 and r["P"] % 64 and r["fwd_ntiles"] > 1 and r["N"] % 32,
    "trip forward <2,4> with slabs and a ragged last pixel tile": lambda c, r: r["fwd"] == "trip" and r["f32_tile"] == (2, 4) and r["fwd_slabs"] == 2 and r["N"] % 128,
    "trip forward <2,4> unsplit": lambda c, r: r["fwd"] == "trip" and r["f32_tile"] == (2, 4) and r["fwd_slabs"] == 1,
    # ---- triple-gather weight gradient (cg_wgrad3_kernel)
    "trip weight gradient: 4 slabs, partial last chunk": lambda c, r: r["dw"] == "trip" and r["dw_slabs"] == 4 and r["N"] % 32,
    "trip weight gradient: 22 slabs of one chunk": lambda c, r: r["dw"] == "trip" and r["dw_slabs"] == 22 == r["chunks"] and c.Co == 64,
    # ---- parity data gradient (cg_dgrad3_kernel)
    "data gradient over 4 output-channel slabs": lambda c, r: r["dx"] == "parity" and r["dx_slabs"] == 4,
    "data gradient over 2 output-channel slabs": lambda c, r: r["dx"] == "parity" and r["dx_slabs"] == 2 and c.Ci == 64,
    "data gradient with Ci % 64 != 0, Ci > 32 (Ci = 36)": lambda c, r: r["dx"] == "parity" and c.Ci % 64 and c.Ci > 32 and c.Ci % 32,
    "data gradient with Ci = 8 and one output-channel chunk per tap": lambda c, r: r["dx"] == "parity" and c.Ci == 8 and c.Co == 32,
    "3x3 without a data gradient on the triple-gather kernels (Co % 32 != 0)": lambda c, r: c.k == 3 and r["dx"] is None and r["fwd"] == "trip" and r["fwd_slabs"] > 1,
    # ---- general gather kernels, 3x3 (cg_fwd_kernel<.,.,3>, cg_wgrad_kernel<2,2,3>, cg_wpad_kernel before a 3x3)
    "gather 3x3 <2,2,3> below one tile, K = 45 padded to 64, one weight-gradient slab": lambda c, r: c.k == 3 and r["fwd"] == "gather" and r["f32_tile"] == (2, 2) and (r["K"], r["Kp"]) == (45, 64) and r["dw_slabs"] == 1,
    "scalar slab reduce (Co K % 4 != 0 over 3 slabs)": lambda c, r: r["reduce"] == "scalar" and r["dw_slabs"] == 3,
    "gather 3x3 <2,2,3> with 6 weight-gradient slabs and the 16-byte reduce": lambda c, r: c.k == 3 and r["fwd"] == "gather" and r["f32_tile"] == (2, 2) and r["fwd_wpad"] and r["dw"] == "gather" and r["dw_slabs"] == 6 and r["reduce"] == "16b",
    "gather 3x3: three row tiles, the last ragged": lambda c, r: c.k == 3 and r["fwd"] == "gather" and r["fwd_mtiles"] == 3 and c.Co % 64,
    "gather 3x3 <2,4,3> over several pixel tiles": lambda c, r: c.k == 3 and r["fwd"] == "gather" and r["f32_tile"] == (2, 4) and r["fwd_ntiles"] > 1,
    "gather 3x3 <4,4,3>": lambda c, r: c.k == 3 and r["fwd"] == "gather" and r["f32_tile"] == (4, 4),
    # ---- patch-staged stem (stem_fwd_*_kernel, stem_wgrad_kernel)
    "stem, 3 channels: a single tile, one output row, 4 of 64 columns": lambda c, r: r["stem"] and c.Ci == 3 and r["ntiles"] == 1 and (r["Ho"], r["Wo"]) == (1, 4),
    "stem, 6 channels: a single tile, one output row, 4 of 64 columns": lambda c, r: r["stem"] and c.Ci == 6 and r["ntiles"] == 1 and (r["Ho"], r["Wo"]) == (1, 4),
    "stem tile walk: more tiles than blocks, a last working block with fewer tiles, trailing zero slabs":
        lambda c, r: r["stem"] and r["ntiles"] > S.STEM_MAX_BLOCKS and 0 < r["last_tiles"] < r["per"] and r["working"] < r["nblocks"],
    "stem, 3 channels: odd Ho, second tile 4 columns wide": lambda c, r: r["stem"] and c.Ci == 3 and r["Ho"] % 2 and r["tiles_x"] == 2 and r["Wo"] - S.ST_TW == 4,
    "stem, 6 channels: odd Ho, second tile 4 columns wide (nf = 2 and nf = 3)": lambda c, r: r["stem"] and c.Ci == 6 and r["Ho"] % 2 and r["Wo"] - S.ST_TW == 4 and S.raw_modes(c) == (2, 3),
    # ---- general gather kernels, 7x7 (cg_fwd_kernel<.,.,7>, cg_wgrad_kernel<2,2,7>)
    "gather 7x7 <2,2,7> with Co = 16": lambda c, r: c.k == 7 and r["fwd"] == "gather" and r["f32_tile"] == (2, 2) and c.Co == 16,
    "gather 7x7 <2,2,7> with Co = 64, Ci = 4": lambda c, r: c.k == 7 and r["fwd"] == "gather" and c.Co == 64 and c.Ci == 4,
    "gather 7x7 <2,2,7> with two row tiles (Co = 96)": lambda c, r: c.k == 7 and r["fwd"] == "gather" and r["f32_tile"] == (2, 2) and r["fwd_mtiles"] == 2,
    "gather 7x7 <2,4,7> with Co below a row tile": lambda c, r: c.k == 7 and r["fwd"] == "gather" and r["f32_tile"] == (2, 4) and c.Co < 64,
    "gather 7x7 <4,4,7>": lambda c, r: c.k == 7 and r["fwd"] == "gather" and r["f32_tile"] == (4, 4),
}


def unreached(cases):
    R = [(c, S.route(c)) for c in cases]
    return [name for name, pred in MECHANISMS.items() if not any(pred(c, r) for c, r in R)]


def test_case_table_reaches_every_mechanism():
    assert len(set(S.CASES)) == len(S.CASES) == len({S.case_id(c) for c in S.CASES})
    assert all(S.supported(*c[:6]) for c in S.CASES)
    assert unreached(S.CASES) == []
    # what the modes and entries add to the rows (asserted from route(), launched by tests/test_convs2_shapes_gpu.py)
    stems = S.stem_rows()
    assert {c.Ci for c in stems} == {3, 6} and len(stems) == 5
    for c in stems:
        assert S.route(c, 0)["fwd"] == "stem_f32" and S.route(c, 1)["fwd"] == "stem_x3"
        for nf in S.raw_modes(c):
            assert S.route(c, 0, raw=nf)["fwd"] == "stem_f32"              # stem_fwd_kernel<true>: raw frames without split operands
            assert S.route(c, 1, raw=nf)["fwd"] == "stem_x3"
    assert {nf for c in stems for nf in S.raw_modes(c)} == {1, 2, 3}
    assert any(S.route(c)["Ho"] % 2 and S.route(c)["tiles_x"] == 2 for c in stems)       # raw frames at odd Ho, second tile not 32 wide
    # dc_set_gemm_split(3): one row goes to the split-operand kernels, one stays
    e, n = S.route(S.SPLIT3["eligible"], 3), S.route(S.SPLIT3["ineligible"], 3)
    assert (e["fwd"], e["dw"], e["dx"]) == ("g1x3", "g1x3", "parity") and (n["fwd"], n["dw"]) == ("trip", "trip")
    assert S.route(S.SPLIT3["eligible"], 1)["fwd"] == "trip" and S.SPLIT3["ineligible"] in S.CASES
    # the bf16 policy's stride-2 route (tests/test_conv_bf16_gpu.py launches it) is named, not run here
    b = S.route(K(1, 64, 128, 6, 8, 3), bf16=True)
    assert (b["fwd"], b["dw"], b["dx"]) == ("bf16", "bf16", "bf16")
    # the child's rows: every triple-gather and stem row, on the gather kernels with Kp == K (3x3) and at Co = 64 (7x7)
    child = S.gather_child_cases()
    assert set(child) == set(S.TRIP) | set(stems)
    rg = [S.route(c, 1, S.GATHER_ENV) for c in child]
    assert all(r["fwd"] == "gather" and r["dw"] == "gather" for r in rg)
    assert any(c.k == 3 and not r["fwd_wpad"] for c, r in zip(child, rg)) and any(c.k == 7 and c.Co == 64 for c in child)
    assert {r["f32_tile"] for c, r in zip(child, rg) if c.k == 3} == {(2, 2), (2, 4)}


@pytest.mark.parametrize("case", S.params(S.CASES))
def test_every_row_is_the_only_witness_of_a_mechanism(case):
    """Deleting the row leaves a mechanism unreached -- and the failure names it."""
    gone = unreached([c for c in S.CASES if c != case])
    print("without %s: %s" % (S.case_id(case), gone))
    assert gone, "the table reaches every mechanism without %s" % S.case_id(case)


# ---- the plan the launches follow (dc_convs2_plan_query) and the workspace queries against route() ----------------------------------
@pytest.mark.parametrize("case", S.params(S.CASES + [S.SPLIT3["eligible"]]))
def test_plan_and_workspaces_agree_with_route(case):
    """Every field of dc_convs2_plan and the bytes of dc_convs2_fwd_workspace / _wgrad_workspace / _dgrad_workspace are what route()
    predicts, under dc_set_gemm_split 0, 1 and 3, through dc_convs2_* and (stem rows) through dc_stem_*.  A threshold changed in
    csrc/convgemm.hip fails here, not silently at the GPU."""
    L = S.host_lib()
    before = L.dc_get_gemm_split()
    for mode in MODES:
        for raw in (0,) + (S.raw_modes(case) if S.route(case)["stem"] else ()):
            assert S.plan_mismatches(case, mode, S.NO_ENV, raw) == [], (mode, raw)
    assert L.dc_get_gemm_split() == before
    if not S.route(case)["stem"]:
        assert S.plan_query(case, raw=1)[0] == S.EINVAL          # dc_stem_* refuse what the patch-staged stem does not take


def test_plan_tells_the_modes_apart():
    e, n = S.SPLIT3["eligible"], S.SPLIT3["ineligible"]
    with S.split_mode(3):
        pe, pn = S.plan_query(e)[1], S.plan_query(n)[1]
    with S.split_mode(1):
        p1 = S.plan_query(e)[1]
    assert (pe["fwd"], pe["dw"], pe["dx"]) == (S.PLAN_FWD["g1x3"], S.PLAN_DW["g1x3"], S.PLAN_DX["parity"])
    assert (pn["fwd"], pn["dw"]) == (S.PLAN_FWD["trip"], S.PLAN_DW["trip"]) == (p1["fwd"], p1["dw"])
    stem = S.stem_rows()[0]
    with S.split_mode(0):
        assert S.plan_query(stem)[1]["fwd"] == S.plan_query(stem, raw=1)[1]["fwd"] == S.PLAN_FWD["stem_f32"]
    with S.split_mode(1):
        assert S.plan_query(stem)[1]["fwd"] == S.plan_query(stem, raw=1)[1]["fwd"] == S.PLAN_FWD["stem_x3"]


def test_plan_under_the_bf16_policy():
    L = S.host_lib()
    c = K(1, 64, 128, 6, 8, 3)
    prev = L.dc_set_matrix_precision(1)
    try:
        rc, got = S.plan_query(c)
        rc7, got7 = S.plan_query(S.stem_rows()[0])
    finally:
        L.dc_set_matrix_precision(prev)
    assert rc == 0 and got == S.plan_of(S.route(c, bf16=True)) and got != S.plan_of(S.route(c))
    assert rc7 == 0 and got7 == S.plan_of(S.route(S.stem_rows()[0]))            # the stem has no reduced-precision kernel
    assert L.dc_get_matrix_precision() == prev


@pytest.mark.parametrize("env", [S.GATHER_ENV, {"DC_STEM_X3": "0"}, {"DC_STEM_PATCH": "0"}, {"DC_CONV_TRIP": "0"}],
                         ids=lambda e: "-".join("%s=%s" % kv for kv in sorted(e.items())))
def test_plan_agrees_with_route_under_the_switches(env):
    """DC_STEM_PATCH, DC_CONV_TRIP and DC_STEM_X3 are read once per process: tests/convs2_gather_child.py `plan` compares plan and
    workspaces with route(case, mode, env) for every row, mode and entry in a fresh process (no GPU there either)."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "convs2_gather_child.py")
    clean = {k: v for k, v in os.environ.items() if k not in ("DC_STEM_PATCH", "DC_CONV_TRIP", "DC_STEM_X3")}
    p = subprocess.run([sys.executable, child, "plan"], env={**clean, **env}, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("convs2_plan ")]
    assert {ln.split()[1] for ln in lines} == {S.case_id(c) for c in S.CASES} and len(lines) == len(S.CASES)
    assert p.stdout.rstrip().endswith("convs2_plan_done %d" % len(S.CASES))
    changed = [c for c in S.CASES if S.plan_of(S.route(c, 1, env)) != S.plan_of(S.route(c))]
    assert changed, "the switch changes no row's plan"
    for c in changed:             # the child saw the library follow the switch
        assert any(ln.split()[1] == S.case_id(c) and " differs" in ln for ln in lines), S.case_id(c)


# ---- conditioning and sensitivity -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.params(S.CASES))
def test_rows_are_well_conditioned_and_the_gate_sees_one_dropped_term(case):
    """torch's fp32 evaluation of the statement stays within 0.25 of the gate of fp64 for every checked output (the gate judges the
    kernel, not the shape); and the fp64 statement with ONE term removed -- one tap of one channel (y), one pixel's product (dw), one
    (co, tap) term (dx) -- misses the gate by at least 10x: the smallest possible error at that shape is seen."""
    inp, r64, r32 = S.reference(case)
    assert S.outputs(case) and S.outputs(case)[0] == "y"
    for name in S.outputs(case):
        assert bool(torch.isfinite(r64[name]).all()) and float(r64[name].abs().max()) > 0
        e32 = S.rel_err(r32[name], r64[name])
        mutated, term = S.single_term(case, inp, r64, name)
        assert int((mutated != r64[name]).sum()) == 1
        miss = S.rel_err(mutated, r64[name]) / S.GATE
        print("convs2_fitness %s %s torch fp32 %.2e (%.0f%% of the gate), one term %.2e misses the gate %.0fx" % (
            S.case_id(case), name, e32, 100 * e32 / S.GATE, term, miss))
        assert e32 <= S.CONDITION * S.GATE, (name, e32)
        assert miss >= S.SENSITIVITY, (name, miss)
    for name in ("dw", "dx"):
        if name not in S.outputs(case):
            assert r64[name] is None


def test_reference_inputs_are_what_the_issue_states():
    inp = S.build(K(2, 6, 64, 6, 136, 7))
    g0, g1, g2 = inp["frames"][3]
    f0, f1 = inp["frames"][2]
    assert torch.equal(f0, torch.cat([g0, g1], 0)) and torch.equal(f1, torch.cat([g1, g2], 0))
    x = (torch.cat([torch.cat([g0, g1], 1), torch.cat([g1, g2], 1)], 0) - S.MEAN) / S.STD
    assert torch.equal(inp["x"], x) and torch.equal(inp["x"], (torch.cat([f0, f1], 1) - S.MEAN) / S.STD)
    assert 0 <= float(g0.min()) and float(g0.max()) < 1
    inp = S.build(K(1, 32, 64, 2, 8, 3))
    assert not inp["frames"] and abs(float(inp["w"].std()) * (32 * 9) ** 0.5 - 1) < 0.1 and not inp["x"].requires_grad
    a, b = S.reference(K(1, 32, 64, 2, 8, 3)), S.reference(K(1, 32, 64, 2, 8, 3))
    assert a is b and not a[0]["x"].requires_grad and not a[0]["w"].requires_grad


# ---- refusals: host-side, before any HIP call ---------------------------------------------------------------------------------------
UNSUPPORTED = [
    ("odd Hi", (1, 32, 64, 7, 8, 3)), ("odd Wi", (1, 32, 64, 8, 9, 3)), ("Wo % 4 != 0", (1, 32, 64, 8, 12, 3)),
    ("ks = 5", (1, 32, 64, 8, 8, 5)), ("ks = 1", (1, 32, 64, 8, 8, 1)), ("2^29 elements", (1, 32, 64, 4096, 4096, 3)),
    ("2^29 elements by Co", (2, 3, 64, 2048, 2048, 7)), ("B = 0", (0, 32, 64, 8, 8, 3)),
]
NO_DGRAD = [("ks = 7", (1, 4, 64, 8, 16, 7)), ("Ci % 4 != 0", (1, 6, 64, 8, 8, 3)), ("Co % 32 != 0", (1, 32, 40, 8, 8, 3))]


def test_entries_refuse_what_they_cannot_run():
    L = S.host_lib()
    L.dc_clear_error()
    idle = L.dc_clear_error()
    one = ctypes.c_void_p(4096)          # never dereferenced: every call below returns before a launch
    assert (1 << 29) - 1 < 1 * 32 * 4096 * 4096 and 2 * 64 * 2048 * 2048 >= 1 << 29 > 2 * 3 * 2048 * 2048
    for name, s in UNSUPPORTED:
        assert not S.supported(*s) and S.route(K(*s)) is None, name
        assert L.dc_convs2_supported(*s) == 0, name
        assert L.dc_convs2_fwd_workspace(*s) == L.dc_convs2_wgrad_workspace(*s) == L.dc_convs2_dgrad_workspace(*s) == 0, name
        assert L.dc_convs2_fwd(one, one, one, one, *s, None) == S.EINVAL, name
        assert L.dc_convs2_wgrad(one, one, one, one, *s, None) == S.EINVAL, name
        assert L.dc_convs2_dgrad(one, one, one, one, *s, None) == S.EINVAL, name
        assert S.plan_query(K(*s))[0] == S.EINVAL, name
    for name, s in NO_DGRAD:
        assert L.dc_convs2_supported(*s) == 1 and S.route(K(*s))["dx"] is None, name
        assert L.dc_convs2_dgrad_workspace(*s) == 0, name
        assert L.dc_convs2_dgrad(one, one, one, one, *s, None) == S.EINVAL, name
        rc, got = S.plan_query(K(*s))
        assert rc == 0 and got["dx"] == S.PLAN_DX[None] and got["dx_slabs"] == 0, name
    ok = (1, 32, 64, 8, 8, 3)
    assert L.dc_convs2_supported(*ok) == 1 and L.dc_convs2_dgrad_workspace(*ok) > 0
    for k in range(4):                   # a null pointer in each position
        a = [one] * 4
        a[k] = None
        assert L.dc_convs2_fwd(*a, *ok, None) == S.EINVAL
        assert L.dc_convs2_wgrad(*a, *ok, None) == S.EINVAL
        assert L.dc_convs2_dgrad(*a, *ok, None) == S.EINVAL
    assert L.dc_convs2_plan_query(*ok, 0, None) == S.EINVAL
    from depthcore import _lib
    assert L.dc_convs2_plan_query(*ok, 1, ctypes.byref(_lib.ConvS2Plan())) == S.EINVAL      # not a stem
    # dc_stem_*: frames missing, a shape off the patch-staged stem
    fr = (ctypes.c_void_p * 3)(4096, 4096, 4096)
    assert L.dc_stem_supported(1, 1, 64, 8, 16) == 1 and L.dc_stem_supported(1, 1, 32, 8, 16) == 0 and L.dc_stem_supported(4, 1, 64, 8, 16) == 0
    assert L.dc_stem_fwd(fr, 1, S.MEAN, S.STD, one, one, one, 1, 8, 16, 32, None) == S.EINVAL
    assert L.dc_stem_fwd(None, 1, S.MEAN, S.STD, one, one, one, 1, 8, 16, 64, None) == S.EINVAL
    assert L.dc_stem_fwd(fr, 1, S.MEAN, S.STD, one, None, one, 1, 8, 16, 64, None) == S.EINVAL
    assert L.dc_stem_wgrad(fr, 1, S.MEAN, 0.0, one, one, one, 1, 8, 16, 64, None) == S.EINVAL
    assert L.dc_stem_wgrad(fr, 1, S.MEAN, S.STD, one, one, one, 1, 7, 16, 64, None) == S.EINVAL
    assert L.dc_clear_error() == idle    # nothing above made a HIP call that failed, on a machine without a GPU or with one
