"""The cases of tests/conv_block_cases.py are fit to judge the fused 3x3 block's fp32 dispatch with: the table reaches every
mechanism it is there for (computed by route(), the transcription of the host code in dc_conv3x3_fwd / dc_conv3x3_bwd_add, which
is cross-checked against the library's own workspace queries and, field by field, against the plan the launches themselves follow
(dc_conv3x3_plan_query) for every case), every case is finite and well conditioned (torch's
fp32 evaluation of the statement is within 1e-4 of fp64, no result is all zero, the planted ties are there) -- and the entries
refuse what they cannot run (host-side checks: DC_EINVAL before anything is launched).  Needs no GPU."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import conv_block_cases as CC
from conv_block_cases import ACT_NONE, REFLECT, ZERO

R = [(c, CC.route(c)) for c in CC.CASES]


def _some(pred):
    return any(pred(c, r) for c, r in R)


def test_case_table_reaches_every_mechanism():
    assert len(set(CC.CASES)) == len(CC.CASES) == len({CC.case_id(c) for c in CC.CASES})
    addends = lambda c: bool(c.add0 or c.add1)
    # ---- forward
    assert _some(lambda c, r: r["fwd"] == "dispconv_fwd4_kernel" and c.W % 4 == 0)
    assert _some(lambda c, r: r["fwd"] == "dispconv_fwd_kernel" and c.W == 18) and _some(lambda c, r: r["fwd"] == "dispconv_fwd_kernel" and c.W == 13)
    # the head refused (C0 = 40; H = 3): a Co = 1 launch on Winograd and on the direct kernel
    assert _some(lambda c, r: c.Co == 1 and c.C0 == 40 and r["fwd"] == "wino_conv_fused_fwd")
    assert _some(lambda c, r: c.Co == 1 and c.H == 3 and r["fwd"] == "wino_conv_fused_fwd")
    assert _some(lambda c, r: c.Co == 1 and r["fwd"] == "conv_gemm_kernel<1, false>")
    wf = [c for c, r in R if r["fwd"] == "wino_conv_fused_fwd"]
    assert {(bool(c.up0), c.C1 > 0, c.pad) for c in wf} >= {(u, k, p) for u, k in ((1, 0), (0, 1), (1, 1)) for p in (REFLECT, ZERO)}
    assert {c.act for c in wf} == {0, 1, 2, 3, 4} and any(not c.bias for c in wf)
    for mr, Co in ((1, 7), (2, 20), (4, 40)):
        assert _some(lambda c, r: r["fwd"] == "conv_gemm_kernel<%d, false>" % mr and c.Co == Co)
    dg = [c for c, r in R if r["fwd"].startswith("conv_gemm_kernel")]
    assert any(c.W % 2 for c in dg) and any(c.C1 and c.C0 == 12 and c.C1 == 8 and c.W == 16 for c in dg)
    assert any(c.H < 16 and c.W < 16 for c in dg)
    assert any((c.H, c.W) == (17, 19) for c in dg) and any((c.H, c.W) == (9, 34) for c in dg)
    assert any(c.up0 and c.C1 and c.C0 % 8 and (c.W // 2) % 2 for c in dg)
    assert not _some(lambda c, r: "conv_gemm_v2_kernel" in r["fwd"])           # unreachable with Winograd enabled below 2 GiB
    # ---- data gradient
    hd = [c for c, r in R if r["dx"] == "dispconv_dx_kernel"]
    assert {c.C0 for c in hd} >= {5, 16, 32} and {c.add0 for c in hd} == {0, 1} and {c.pad for c in hd} == {REFLECT, ZERO}
    assert any(c.H * c.W > 256 and (c.H * c.W) % 256 for c in hd)
    assert _some(lambda c, r: r["dx"] == "wino_conv_dgrad_split" and c.pad == ZERO and not r["ring"])
    ring = [c for c, r in R if r["ring"]]
    assert all(c.pad == REFLECT and c.Co <= CC.RING_MAXCO and c.dsplit for c in ring)
    r2 = [c for c in ring if c.dsplit == 2]
    assert any(c.H > c.W for c in r2) and any(c.W > c.H for c in r2)
    assert any((c.C0 + c.C1) % 8 for c in r2) and any((c.C0, c.C1) == (40, 24) for c in r2)
    assert {c.add1 for c in r2 if c.up0 and c.C1 and c.add0} >= {"inplace", "separate"}
    assert any(c.H == 4 for c in r2) and any(c.W == 4 for c in r2) and any(c.Co == 64 for c in r2)
    full = [(c, r) for c, r in R if r["dx"] == "wino_conv_full_dgrad"]
    assert any(c.Co == 72 and c.pad == REFLECT and c.dsplit == 2 for c, _ in full)
    assert any(c.H % 2 and c.dsplit == 2 for c, _ in full) and any(c.dsplit == 0 and c.H % 2 == 0 and c.Co <= 64 for c, _ in full)
    for fold in ("conv_fold4_kernel", "conv_fold_kernel"):
        ff = [c for c, r in R if r["fold"] == fold]
        assert {c.pad for c in ff} == {REFLECT, ZERO}, fold
        assert any(c.up0 for c in ff) and any(c.C1 for c in ff) and {addends(c) for c in ff} == {True, False}, fold
        assert any(c.up0 and c.pad == REFLECT for c in ff) and any(c.up0 and c.pad == ZERO for c in ff), fold
    assert _some(lambda c, r: r["fold"] == "conv_fold_kernel" and c.W % 4 == 0 and c.up0 and (c.W >> 1) % 4)
    assert _some(lambda c, r: r["fold"] == "conv_fold4_kernel" and c.up0 and c.W == 24)
    direct = [(c, r) for c, r in R if r["dx"] and r["dx"].startswith("conv_gemm_kernel")]
    assert {r["dx"] for _, r in direct} == {"conv_gemm_kernel<%d, true>" % m for m in (1, 2, 4)}
    assert any(c.W % 2 for c, _ in direct) and any(c.C0 + c.C1 < 16 for c, _ in direct)
    assert any(c.W % 2 == 0 and c.act != ACT_NONE and (c.B * c.Co * c.H * c.W) % 4 and c.C0 + c.C1 >= 16 for c, _ in direct)
    assert _some(lambda c, r: r["dx"] == "conv_gemm_v2_kernel<1, true>" and c.W % 16 == 0 and c.C0 + c.C1 < 16)
    one = [(c, r) for c, r in R if c.dsplit == 1 and c.pad == REFLECT and r["w_dx"] and not r["head_dx"]]
    big = [c for c, r in one if r["ring"]]
    assert len(big) == 1 and big[0].H * big[0].W >= 6000 and big[0].B * (big[0].C0 + big[0].C1) * big[0].H * big[0].W >= 4 << 20
    assert big[0].B * (big[0].C0 + big[0].C1) * big[0].H * big[0].W < 1.1 * (4 << 20) and big[0].H * big[0].W < 1.1 * 6000
    assert any(not r["ring"] and CC.route(c._replace(dsplit=2))["ring"] for c, r in one)
    # ---- weight and bias gradient
    for n in (4, 8):
        hw = [(c, r) for c, r in R if r["dw"] == "dispconv_wgrad_kernel<%d>" % n]
        assert any(c.H * c.W > 2048 and (c.H * c.W) % 2048 for c, _ in hw) and any(c.H * c.W < 2048 for c, _ in hw)
        assert {tuple(g for g in c.grads if g in "wb") for c, _ in hw} == {("w", "b"), ("w",), ("b",)}
        assert _some(lambda c, r: c.Co == 1 and c.C0 == 4 * n and (c.H * c.W) % 4 and r["dw"].startswith("conv_wgrad_kernel"))
    ww = [(c, r) for c, r in R if r["dw"] == "wino_wgrad_fused"]
    assert any(c.up0 and c.C1 and c.pad == REFLECT for c, _ in ww)
    for db in ("conv_gprime_dbias_kernel", "conv_dbias_kernel"):
        assert {c.act != ACT_NONE for c, r in ww if r["db"] == db} == {True, False}, db
    assert any((c.H, c.W, c.Co) == (7, 6, 32) for c, r in ww if r["db"] == "conv_dbias_kernel")
    dw = [(c, r) for c, r in R if r["dw"] and r["dw"].startswith("conv_wgrad")]
    assert {r["dw"] for _, r in dw} == {"conv_wgrad%s_kernel<%d>" % (v, m) for v in ("", "_v2") for m in (1, 2)}
    for v in ("conv_wgrad_kernel", "conv_wgrad_v2_kernel"):
        assert {r["split"] > 1 for _, r in dw if r["dw"].startswith(v)} == {True, False}, v
    assert any((c.C0 + c.C1) % CC.CW for c, _ in dw)
    assert any((c.Co, c.C0 + c.C1) == (5, 7) and r["reduce"] == "conv_wreduce_kernel" and "w" in c.grads for c, r in dw)
    assert any(r["reduce"] == "conv_wreduce_kernel" and "w" in c.grads and r["split"] > 1 for c, r in dw)
    assert any(r["reduce"] == "conv_wreduce4_kernel" and r["split"] > 1 for c, r in dw)
    for v in ("conv_wgrad_kernel", "conv_wgrad_v2_kernel"):
        assert any(r["dw_null"] and r["dw"].startswith(v) for _, r in dw) and any(r["db_null"] and r["dw"].startswith(v) for _, r in dw)
    # ---- g' and the null patterns
    assert {r["gprime"] for _, r in R} == {"unused", "conv_gprime_dbias_kernel", "conv_gprime_kernel", "on the fly", "gy"}
    full_list = {("x0", "x1", "w", "b"), ("x0", "x1"), ("w", "b"), ("w",), ("b",), ("x0",), ("x1",)}
    for fam, single in (("wino", False), ("direct", False), ("head4", True), ("head8", True)):
        base, nulls = CC.NULL_FAMILIES[fam]
        assert base in CC.CASES and all(n in CC.CASES and n[:10] == base[:10] for n in nulls)
        want = {("x0", "w", "b"), ("x0",), ("w", "b"), ("w",), ("b",)} if single else full_list
        assert {base.grads} | {n.grads for n in nulls} == want, fam
    rb = CC.route(CC.NULL_FAMILIES["wino"][0])
    assert rb["fwd"] == "wino_conv_fused_fwd" and rb["dx"] == "wino_conv_dgrad_split" and rb["dw"] == "wino_wgrad_fused"
    rb = CC.route(CC.NULL_FAMILIES["direct"][0])
    assert rb["fwd"].startswith("conv_gemm_kernel") and rb["dx"].startswith("conv_gemm_kernel") and rb["dw"].startswith("conv_wgrad_kernel")
    # `b` without `w` on the Winograd shape runs the whole direct kernel with dw == nullptr
    assert _some(lambda c, r: c[:10] == CC.NULL_FAMILIES["wino"][0][:10] and c.grads == ("b",) and r["dw"] == "conv_wgrad_kernel<2>" and r["dw_null"])
    # ---- the special-purpose cases are table cases; nothing large
    assert all(c in CC.CASES and c._replace(dsplit=0) in CC.CASES for c in CC.DSPLIT_PAIRS) and all(c in CC.CASES for c in CC.DETERMINISM.values())
    for c in CC.DSPLIT_PAIRS:
        assert CC.route(c)["dx"] == "wino_conv_dgrad_split" and CC.route(c._replace(dsplit=0))["dx"] == "wino_conv_full_dgrad"
    d = {k: CC.route(c) for k, c in CC.DETERMINISM.items()}
    assert d["split_wgrad"]["split"] > 1 and d["ring"]["ring"] and d["head_wgrad"]["dw"].startswith("dispconv_wgrad") and d["head_wgrad"]["split"] > 1
    assert sum(1 for c in CC.CASES if c.B * c.Co * c.H * c.W > 50000) == 1


def test_head_null_patterns_flip_the_flags():
    """{w} without {x0} on a head shape: no data-gradient kernel, and g' is never materialised."""
    base, nulls = CC.NULL_FAMILIES["head4"]
    rb = CC.route(base)
    # (w_dx is on for the 16-channel head with all gradients -- the shape is Winograd's too -- but head_dx goes first)
    assert rb["head_dx"] and rb["head_dw"] and rb["gp_unused"] and rb["w_dx"] and rb["dx"] == "dispconv_dx_kernel"
    w = CC.route(base._replace(grads=("w",)))
    assert not w["head_dx"] and not w["w_dx"] and w["dx"] is None and w["head_dw"] and w["gp_unused"]
    # where the head's weight-gradient kernel refuses (HW % 4 != 0), g' is unused only as long as no weight gradient is asked for
    r9 = CC.K(2, 16, 0, 0, 1, 9, 13, 2, ZERO, add0=1)
    assert not CC.route(r9)["gp_unused"] and CC.route(r9._replace(grads=("x0",)))["gp_unused"]
    # a head the weight-gradient kernel refuses (C0 = 5) needs g' for the direct kernel: not unused
    odd = CC.route(CC.K(2, 5, 0, 0, 1, 9, 13, 0, REFLECT))
    assert odd["head_dx"] and not odd["head_dw"] and not odd["gp_unused"]
    # the Winograd shape: w_dx follows the request
    wb, _ = CC.NULL_FAMILIES["wino"]
    assert CC.route(wb)["w_dx"] and not CC.route(wb._replace(grads=("w",)))["w_dx"] and not CC.route(wb._replace(grads=("w",)))["gp_unused"]


def test_wino_disabled_routes_reach_the_v2_forward_kernels():
    """With DC_CONV_WINO=0 (tests/conv_block_direct_child.py) the table reaches conv_gemm_v2_kernel<1 | 2 | 4, false>, each with
    up0 + concat + reflect and with a ragged Co, and the v2 data gradients <2> and <4> no Winograd-enabled launch below 2 GiB can."""
    off = [(c, CC.route(c, False)) for c in CC.CASES if CC.route(c, False) != CC.route(c)]
    for mr in (1, 2, 4):
        hit = [c for c, r in off if r["fwd"] == "conv_gemm_v2_kernel<%d, false>" % mr]
        assert any(c.up0 and c.C1 and c.pad == REFLECT for c in hit) and any(c.Co % (16 * mr) for c in hit), mr
    assert {"conv_gemm_v2_kernel<%d, true>" % m for m in (1, 2, 4)} <= {r["dx"] for _, r in off}
    assert not any(r["head"] or r["fwd"].startswith("wino") or r["w_dx"] or r["w_dw"] for _, r in off)
    assert sum(1 for c in CC.V2) <= 3 and all(c.W % 16 == 0 and c.C0 % 16 == 0 for c in CC.V2)


@pytest.mark.parametrize("case", CC.params(CC.CASES))
def test_route_agrees_with_the_workspace_queries(case):
    """dc_conv3x3_fwd_workspace / dc_conv3x3_bwd_workspace rebuilt from route()'s wino_fwd / wino_dx / wino_dw and the transcribed
    plans: a mismatch means the transcription (or the layout the header describes) is wrong."""
    L = CC.host_lib()
    c = case
    Cin = c.C0 + c.C1
    assert L.dc_conv3x3_fwd_workspace(c.C0, c.C1, c.B, c.Co, c.H, c.W) == CC.fwd_workspace(c)
    assert L.dc_conv3x3_bwd_workspace(c.C0, c.C1, c.B, c.Co, c.H, c.W) == CC.bwd_workspace(c)
    wf, wdx, wdw = CC.shape_routes(c)
    if wdw:     # the Winograd queries wino_bn_cases uses: the weight gradient's is the larger of the fp32 plan and the bf16 slabs
        assert L.dc_wino3x3_wgrad_workspace(c.B, Cin, c.Co, c.H, c.W) == max(CC.WC.wg_plan(c.B, Cin, c.Co, c.H, c.W).ws_bytes,
                                                                          CC.WC.wgrad_bf16_bytes(c.B, Cin, c.Co, c.H, c.W))
    if wf:      # ... and the convolution's differs from the block's only in the padded-domain slabs and the other kernels' weights
        assert L.dc_wino3x3_workspace(c.B, Cin, c.Co, c.H, c.W) <= CC.wino_conv_ws_bytes(c.B, Cin, c.Co, c.H, c.W) + max(
            CC.c3b_weights_bytes(Cin, c.Co), CC.al256(CC.ceil_div(Cin, 16) * 16 * CC.ceil_div(c.Co, 16) * 16 * 36 * 4))
    # the ring's strips fit the padded-domain scratch they borrow
    if CC.route(c)["ring"]:
        assert 4 * (max(c.H, c.W) + 2) <= (c.H + 2) * (c.W + 5)


UNIQUE = sorted({c._replace(grads=CC.ALL if c.C1 else ("x0", "w", "b"), dsplit=0) for c in CC.CASES})


@pytest.mark.parametrize("case", CC.params(UNIQUE))
def test_case_is_well_conditioned(case):
    inp, r64, r32 = CC.reference(case)
    for k, v in r64.items():
        if v is None:
            continue
        assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(r32[k]).all()), k
        assert float(v.abs().max()) > 0, k
        if k != "db":
            assert CC.rel_err(r32[k], v) < CC.E32_MAX, (k, CC.rel_err(r32[k], v))
    assert bool(((r32["db"].double() - r64["db"]).abs() <= CC.db_bound(case, r64)).all())
    assert float(r64["y"].abs().max()) > 0.1 and float(r64["dw"].abs().max()) > 0.1
    ties = CC.tie_mask(case)
    if case.act in (CC.ACT_ELU, CC.ACT_RELU):
        assert int(ties.sum()) >= 4 and ties[0, 0, 0, 0] and ties[-1, -1, -1, -1]
        assert bool((inp["y"][ties] == 0).all())
        want = 0.0 if case.act == CC.ACT_RELU else 1.5
        for r in (r64, r32):
            assert bool((r["gp"][ties] == want).all())
    else:
        assert int(ties.sum()) == 0
    # the backward's y is the statement's, ties apart
    assert CC.rel_err(inp["y"][~ties], r64["y"][~ties]) < 1e-7


# ---- refusals: host-side, DC_EINVAL before anything is launched -------------------------------------------------------------------
def _buf(keep, nbytes):
    nbytes = max(int(nbytes), 256)
    if torch.cuda.is_available():
        keep.append(torch.zeros(nbytes, dtype=torch.uint8, device="cuda"))
        return keep[-1].data_ptr()
    keep.append(ctypes.create_string_buffer(nbytes + 256))
    return (ctypes.addressof(keep[-1]) + 255) & ~255


REFUSALS = [
    # name, (B, C0, up0, C1, Co, H, W, act, pad), operands withheld
    ("up0 with odd H", (2, 8, 1, 0, 8, 7, 8, 1, 0), ()),
    ("up0 with odd W", (2, 8, 1, 8, 8, 8, 7, 1, 0), ()),
    ("H below 2", (2, 8, 0, 0, 8, 1, 8, 1, 0), ()),
    ("act = 5", (2, 8, 0, 0, 8, 8, 8, 5, 0), ()),
    ("pad = 2", (2, 8, 0, 0, 8, 8, 8, 1, 2), ()),
    ("addend0 with dx0 == nullptr", (2, 8, 0, 8, 8, 8, 8, 1, 0), ("dx0",)),
    ("C1 > 0 with x1 == nullptr", (2, 8, 0, 8, 8, 8, 8, 1, 0), ("x1",)),
]


@pytest.mark.parametrize("name,shape,withheld", [pytest.param(*r, id=r[0].replace(" ", "_")) for r in REFUSALS])
def test_refusals_are_host_side(name, shape, withheld):
    L = CC.host_lib()
    B, C0, up0, C1, Co, H, W, act, pad = shape
    keep = []
    n = B * max(C0, C1, Co) * (H + 2) * (W + 2) * 4
    m = lambda: _buf(keep, n)
    x0, x1, w, b, y, gy, dx0, dx1, a0, a1, dw, db = m(), m(), _buf(keep, Co * (C0 + C1) * 36), m(), m(), m(), m(), m(), m(), m(), _buf(keep, Co * (C0 + C1) * 36), m()
    if "x1" in withheld:
        x1 = None
    if "dx0" in withheld:
        dx0 = None
    ws = _buf(keep, max(L.dc_conv3x3_bwd_workspace(C0, C1, B, Co, H, W), L.dc_conv3x3_fwd_workspace(C0, C1, B, Co, H, W), 1 << 20))
    L.dc_clear_error()
    idle = L.dc_clear_error()               # 0 with a GPU; without one HIP reports "no device" on every query
    if "dx0" not in withheld:
        assert L.dc_conv3x3_fwd(x0, C0, up0, x1, C1, w, b, y, ws, B, Co, H, W, act, pad, None) == CC.EINVAL, name
    assert L.dc_conv3x3_bwd_add(x0, C0, up0, x1, C1, w, y, gy, dx0, dx1 if C1 else None, a0, a1 if C1 else None, dw, db, ws, B, Co, H, W, act, pad,
                                None) == CC.EINVAL, name
    assert L.dc_clear_error() == idle       # no HIP call failed on the way: nothing was attempted
    assert L.dc_set_dgrad_split(3) == CC.EINVAL


# ---- the plan the launches follow (dc_conv3x3_plan_query) against route() -----------------------------------------------------------
@pytest.mark.parametrize("case", CC.params(CC.CASES))
def test_plan_agrees_with_route(case):
    """fwd, fwd_v2, fwd_mr, gprime, dx, ring, dw, db, bwd_v2, dx_mr, dw_mr and split of the library's plan -- what dc_conv3x3_fwd and
    dc_conv3x3_bwd_add switch on -- are what route() names, under the case's dsplit mode and with the case's gradients requested."""
    assert CC.plan_mismatches(case) == []


@pytest.mark.parametrize("family", sorted(CC.NULL_FAMILIES))
def test_plan_agrees_with_route_for_every_null_pattern(family):
    base, nulls = CC.NULL_FAMILIES[family]
    seen = set()
    for c in [base] + list(nulls):
        assert CC.plan_mismatches(c) == [], CC.case_id(c)
        seen.add(tuple(sorted(CC.plan_query(c)[1].items())))
    assert len(seen) > 1        # the request is part of the plan: the patterns do not fall together
    # the forward's plan is that of the shape alone
    assert len({CC.plan_query(c)[1]["fwd"] for c in [base] + list(nulls)}) == 1


def test_plan_agrees_with_route_with_winograd_disabled():
    """DC_CONV_WINO is read once per process: tests/conv_block_plan_child.py compares the plan with route(case, False) for every
    case of direct_child_cases() in a fresh process (no GPU there either)."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_block_plan_child.py")
    p = subprocess.run([sys.executable, child], env={**os.environ, "DC_CONV_WINO": "0"}, timeout=300, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-4000:]
    want = {CC.case_id(c) for c in CC.direct_child_cases()}
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("conv_block_plan ")]
    assert {ln.split()[1] for ln in lines} == want and len(lines) == len(want)
    assert {m for ln in lines for m in (1, 2, 4) if "fwd_v2=1 fwd_mr=%d " % m in ln} == {1, 2, 4}
    assert p.stdout.rstrip().endswith("conv_block_plan_done %d" % len(want))


@pytest.mark.parametrize("name,shape", [pytest.param(r[0], r[1], id=r[0].replace(" ", "_")) for r in REFUSALS if not r[2]])
def test_plan_query_refuses_what_the_launches_refuse(name, shape):
    L = CC.host_lib()
    assert sum(1 for r in REFUSALS if not r[2]) == 5
    B, C0, up0, C1, Co, H, W, act, pad = shape
    c = CC.K(B, C0, up0, C1, Co, H, W, act, pad)
    L.dc_clear_error()
    idle = L.dc_clear_error()
    for grads in ((), c.grads, ("w",)):
        assert CC.plan_query(c, grads)[0] == CC.EINVAL, name
    assert L.dc_conv3x3_plan_query(C0, up0, C1, B, Co, H, W, act, pad, 15, None) == CC.EINVAL
    assert L.dc_clear_error() == idle       # the query makes no HIP call
    ok = CC.K(2, 8, 0, 8, 8, 8, 8, 1, 0)    # (the two rows that withhold an operand: their shape is fine)
    assert CC.plan_query(ok)[0] == 0 and L.dc_conv3x3_plan_query(8, 0, 8, 2, 8, 8, 8, 1, 0, 15, None) == CC.EINVAL
    assert L.dc_clear_error() == idle


PREC_F32, PREC_BF16 = 0, 1


def _plan_under(precision, c):
    L = CC.host_lib()
    prev = L.dc_set_matrix_precision(precision)         # (per calling thread)
    assert prev in (PREC_F32, PREC_BF16)
    try:
        rc, got = CC.plan_query(c)
    finally:
        L.dc_set_matrix_precision(prev)
    assert rc == 0
    return got


def test_plan_under_the_bf16_policy():
    """dc_set_matrix_precision(DC_PREC_BF16) on the calling thread: the plan names the bf16 kernels where their 16-byte staging takes
    the shape, the direct fp32 weight gradient below DC_B16_DW_MIN output channels, the head kernels before either -- and is the
    fp32 plan where c3b_eligible refuses."""
    ELU, SIGMOID = CC.ACT_ELU, CC.ACT_SIGMOID
    # zero pad, single source, no upsample: the data gradient straight from the bf16 kernel; g' and the bias partials in one pass
    p = _plan_under(PREC_BF16, CC.K(2, 16, 0, 0, 32, 8, 16, ELU, ZERO))
    assert (p["fwd"], p["dx"], p["dw"], p["gprime"], p["db"]) == (CC.FWD_BF16, CC.DX_BF16, CC.DW_BF16, CC.GP_DBIAS_KERNEL, CC.DB_GPRIME)
    assert p["split"] == CC.c3b_wgrad_split(2, 8, 16, 32, 16) and not p["ring"] and (p["fwd_mr"], p["dx_mr"], p["dw_mr"]) == (0, 0, 0)
    # upsample + concat + reflect: over the padded domain, then the fold
    p = _plan_under(PREC_BF16, CC.K(2, 32, 1, 32, 32, 8, 16, ELU, REFLECT))
    assert (p["fwd"], p["dx"], p["dw"], p["gprime"], p["db"]) == (CC.FWD_BF16, CC.DX_BF16_FOLD, CC.DW_BF16, CC.GP_DBIAS_KERNEL, CC.DB_GPRIME)
    # Co = 8 < DC_B16_DW_MIN: conv_wgrad_v2_kernel<1> fed by conv_gprime_kernel, not Winograd; the bias gradient from its slabs
    c8 = CC.K(2, 16, 0, 0, 8, 8, 16, ELU, ZERO)
    p = _plan_under(PREC_BF16, c8)
    assert (p["fwd"], p["dx"], p["dw"], p["gprime"], p["db"]) == (CC.FWD_BF16, CC.DX_BF16, CC.DW_DIRECT, CC.GP_KERNEL, CC.DB_SLABS)
    assert (p["bwd_v2"], p["dw_mr"], p["split"]) == (1, 1, CC.pick_split(2, 8, 16, 8, 16))
    # the single-channel head goes first, in both passes
    p = _plan_under(PREC_BF16, CC.K(2, 16, 0, 0, 1, 8, 16, SIGMOID, REFLECT))
    assert (p["fwd"], p["dx"], p["dw"], p["gprime"], p["db"]) == (CC.FWD_HEAD, CC.DX_HEAD, CC.DW_HEAD, CC.GP_UNUSED, CC.DB_SLABS)
    # W = 18: c3b_eligible refuses -- the fp32 plan, which is route()'s
    c18 = CC.K(2, 16, 0, 0, 32, 8, 18, ELU, ZERO)
    p = _plan_under(PREC_BF16, c18)
    assert p == _plan_under(PREC_F32, c18) == CC.plan_of(CC.route(c18)) and p["fwd"] == CC.FWD_WINO and p["dx"] == CC.DX_WINO_SPLIT
    # ... and each bf16 plan above differs from its fp32 one, which is route()'s
    for c in (CC.K(2, 16, 0, 0, 32, 8, 16, ELU, ZERO), CC.K(2, 32, 1, 32, 32, 8, 16, ELU, REFLECT), c8):
        f = _plan_under(PREC_F32, c)
        assert f == CC.plan_of(CC.route(c)) and f != _plan_under(PREC_BF16, c)
    assert CC.host_lib().dc_get_matrix_precision() == PREC_F32
