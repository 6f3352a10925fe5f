"""The rows of tests/conv_bf16_cases.py are fit to judge the bf16 matrix-core convolutions with: route() -- the bf16 plan written
from the host code -- equals the plan the launches follow (dc_conv3x3_plan_query / dc_convs2_plan_query under DC_PREC_BF16) field by
field for every request pattern and differs from the fp32 plan; the tables reach every mechanism they are there for (predicates over
route(), not by eye); the operand rounding is visible (the rounded-operand statement and the unrounded one differ by more than 100x
the gate on every output), a single dropped tap at the outermost column or row and a single zeroed channel of a ragged chunk miss the
gate by more than 10x, and torch's fp32 evaluation of the rounded-operand statement stays within a quarter of each gate.  Needs no
GPU."""
import itertools

import pytest
import torch

import conv_block_cases as CC
import conv_bf16_cases as BF
import convs2_cases as S

ROWS = BF.BLOCK + list(BF.NULL_FAMILIES.values()) + BF.TRUNK + BF.S2


def _requests(c):
    names = [g for g in CC.ALL if g != "x1" or c.C1]
    return [tuple(g for g, on in zip(names, mask) if on) for mask in itertools.product((0, 1), repeat=len(names))]


def _under(prec, fn):
    L = CC.host_lib()
    prev = L.dc_set_matrix_precision(prec)
    try:
        return fn()
    finally:
        L.dc_set_matrix_precision(prev)


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BF.params(BF.BLOCK + list(BF.NULL_FAMILIES.values()) + BF.HEAD_FIRST))
def test_block_plan_agrees_with_route_for_every_request(case):
    before = CC.host_lib().dc_get_matrix_precision()
    for grads in _requests(case):
        rc, got = _under(BF.PREC_BF16, lambda: CC.plan_query(case, grads))
        want = BF.block_plan(case, grads)
        assert rc == 0 and set(got) == set(want)
        assert [(k, got[k], want[k]) for k in sorted(want) if got[k] != want[k]] == [], grads
        rc32, got32 = _under(BF.PREC_F32, lambda: CC.plan_query(case, grads))
        assert rc32 == 0 and got32 == CC.plan_of(CC.route(case._replace(grads=grads)))
        if BF.is_head(case):
            assert got == got32                   # the heads come first: the policy leaves them their fp32 kernels
        else:
            assert got != got32 and got["fwd"] == CC.FWD_BF16 != got32["fwd"]
    assert CC.host_lib().dc_get_matrix_precision() == before


@pytest.mark.parametrize("case", BF.params(BF.S2))
def test_stride2_plan_agrees_with_route(case):
    rc, got = _under(BF.PREC_BF16, lambda: S.plan_query(case))
    rc32, got32 = _under(BF.PREC_F32, lambda: S.plan_query(case))
    r = BF.route(case)
    assert rc == 0 and got == r["plan"] and rc32 == 0 and got32 == S.plan_of(S.route(case)) and got != got32
    assert (got["fwd"], got["dw"]) == (S.PLAN_FWD["bf16"], S.PLAN_DW["bf16"])
    assert got["dx"] == (S.PLAN_DX["bf16"] if r["dx"] is not None else S.PLAN_DX[None])


def test_every_eligible_shape_takes_the_bf16_backward():
    """conv_plan's `b16 = b16_shape && wino_gp_ok(...)`: c3b_eligible needs W % 4 == 0, which makes B Co H W % 4 == 0 and wino_gp_ok
    true -- the second clause is dead (DESIGN says so; there is no shape to test it with)."""
    for c in BF.BLOCK_ALL:
        assert BF.c3b_eligible(c.C0, c.C1, c.up0, c.H, c.W) and CC.wino_gp_ok(c.B, c.Co, c.H, c.W, c.act)
    for W in range(4, 132, 4):
        for B, Co, H, act in itertools.product((1, 3), (1, 5, 7), (2, 3, 9), range(5)):
            assert CC.wino_gp_ok(B, Co, H, W, act)
    for shape, ok in (((16, 0, 0, 8, 10), False), ((16, 0, 0, 1, 8), False), ((16, 8, 0, 8, 8), False), ((32, 8, 0, 8, 8), True),
                      ((16, 0, 1, 8, 12), False), ((16, 0, 1, 6, 8), True), ((16, 0, 1, 7, 8), False)):
        assert BF.c3b_eligible(*shape) == ok, shape


# ---- the tables reach every mechanism -----------------------------------------------------------------------------------------------
def _passes(rows):
    """[(row, pass name, geometry)] of every c3b_conv_kernel launch of the rows."""
    out = []
    for c in rows:
        r = BF.route(c)
        out += [(c, r, n, r[n]) for n in ("fwd", "dx", "dxpad") if r[n] is not None]
    return out


def test_tables_reach_every_mechanism():
    ids = [BF.case_id(c) for c in ROWS + BF.BLOCK_NULLS]
    assert len(set(ids)) == len(ids)
    P = _passes(ROWS)
    R = [(c, BF.route(c)) for c in ROWS]
    s1 = [(c, r, n, g) for c, r, n, g in P if r["stride"] == 1 or n != "fwd"]
    # every MR of the forward, the plain data gradient and the padded one, and a ragged M in each
    for n in ("fwd", "dx", "dxpad"):
        assert {g["mr"] for c, r, m, g in s1 if m == n} == {1, 2, 4}, n
        assert {g["mr"] for c, r, m, g in s1 if m == n and g["ragged_m"]} >= {1, 4}, n
        assert any(g["mblocks"] > 1 and g["ragged_m"] for c, r, m, g in s1 if m == n) or n != "fwd"
    assert {g["mr"] for c, r, m, g in P if r["stride"] == 2 and m == "fwd"} == {1, 2, 4}
    assert any(g["M"] == 1 for c, r, m, g in P if m == "fwd") and any(g["M"] == 40 and g["mr"] == 4 for c, r, m, g in P if m == "dx")
    assert any(g["M"] == 17 for c, r, m, g in P if m == "fwd") and {16, 32} <= {g["M"] for c, r, m, g in P if m == "fwd"}
    # the channel-pair guard and the chunk guard: odd K, K = 1, K < 32, K % 32 != 0 in both sources, ragged x1 behind a full x0 chunk
    ks = [g["K"] for c, r, m, g in P]
    assert any(k % 2 and k > 1 for k in ks) and 1 in ks and any(k < 32 for k in ks) and any(k > 32 and k % 32 for k in ks)
    assert any(g["K"] == 1 for c, r, m, g in P if m == "dxpad")
    assert any(r["src"]["rag0"] and r["src"]["k0"] > 32 for c, r in R) and any(r["src"]["rag1"] for c, r in R)
    assert any(r["src"]["k0"] % 32 == 0 and r["src"]["k0"] and r["src"]["rag1"] for c, r in R)
    assert any(r["kind"] == "block" and r["up0"] and r["src"]["k0"] == 64 and r["src"]["k1"] == 32 for c, r in R)
    assert any(r["dw"] is not None and r["dw"]["ragged_ci"] and r["dw"]["outer"][1] > 1 for c, r in R)
    # the reflected overhang: inside quads of the last tile, without and with up0 (8-wide quads), and the widths without an overhang
    refl = [(c, r) for c, r in R if r["kind"] == "block" and r["pad"] == CC.REFLECT and r["fwd"] is not None]
    assert {r["fwd"]["last_quads"] for c, r in refl if r["fwd"]["overhang"] and not r["up0"]} >= {1, 3, 4, 7}       # (2 and 5: W = 40 and 20 in tests/test_conv_bf16_gpu.py)
    assert {c.W for c, r in refl if r["fwd"]["overhang"] and not r["up0"]} >= {12, 28, 36, 260}
    assert {c.W % 32 for c, r in refl if r["fwd"]["overhang"] and r["up0"]} >= {8}
    assert {c.W for c, r in refl if r["up0"]} >= {8, 40, 264} and {c.W for c, r in refl if not r["fwd"]["overhang"]} >= {32, 64}
    assert any(c.W == 68 and r["dx"] is not None and r["dx"]["last_quads"] == 1 and c.add0 for c, r in R if r["kind"] == "block")
    # the padded-domain data gradient: width 34 (a second tile two columns wide), exactly one tile row, every row on the border
    pads = [(c, g) for c, r, m, g in P if m == "dxpad"]
    assert any(g["OW"] == 34 and g["tiles_x"] == 2 and g["pitch"] == 36 for c, g in pads)
    assert any(g["OH"] == 8 and g["tiles_y"] == 1 for c, g in pads) and any(g["OH"] % 8 and g["tiles_y"] > 1 for c, g in pads)
    assert any(c.H == 2 for c, r, m, g in P if m == "dx") and any(g["OH"] == 4 and c.H == 2 for c, g in pads)
    # the weight gradient's walk, both strides: more tiles than blocks, the overhanging tile first and second, across images
    for stride in (1, 2):
        walks = [r["dw"] for c, r in R if r["dw"] is not None and r["stride"] == stride and r["dw"]["per_block"] > 1]
        assert walks and all(w["split"] == 256 and w["per_block"] == 2 and w["cross_image"] for w in walks)
        assert any(w["ntiles"] == 297 and w["walkers"] == 41 and w["over_first"] and w["over_second"] for w in walks), stride
    assert any(r["dw"] is not None and r["dw"]["per_block"] > 1 and r["pad"] == CC.REFLECT and r["up0"] for c, r in R)
    assert any(r["dw"] is not None and r["dw"]["per_block"] > 1 and r["pad"] == CC.REFLECT and not r["up0"] for c, r in R)
    assert all(BF.route(c)["dw"]["per_block"] > 1 for c in BF.WALK.values())
    assert BF.route(BF.WALK["s2"])["dx"] is None and BF.route(BF.WALK["s2-dx"])["dx"]["tiles_y"] == 86 and BF.route(BF.WALK["s2-dx"])["dw"]["walkers"] == 2
    # stride 2: OH = 1, 3, 5; OW = 4 and 36; odd Ci; Ci = 40; a dilated data gradient at H = 2
    s2 = [(c, r) for c, r in R if r["kind"] == "s2"]
    assert {r["fwd"]["OH"] for c, r in s2} >= {1, 3, 5} and {r["fwd"]["OW"] for c, r in s2} >= {4, 36}
    assert any(c.Ci % 2 for c, r in s2) and any(c.Ci == 40 and r["dx"] is not None and c.H == 2 for c, r in s2)
    assert any(r["dx"] is not None and r["dx"]["tiles_y"] == 2 and r["dx"]["ragged_y"] and r["dx"]["chunks"] == 4 for c, r in s2)
    # every g' and bias-gradient value the policy can produce, the hybrids, both data-gradient routes, every null pattern
    plans = [BF.block_plan(c, g) for c in BF.BLOCK_ALL + BF.HEAD_FIRST for g in _requests(c)]
    assert {p["gprime"] for p in plans} == {CC.GP_UNUSED, CC.GP_GY, CC.GP_KERNEL, CC.GP_DBIAS_KERNEL}
    assert {p["db"] for p in plans} == {CC.DB_NONE, CC.DB_SLABS, CC.DB_GPRIME}
    own = [BF.block_plan(c) for c in BF.BLOCK_ALL]
    assert {p["gprime"] for p in own} == {CC.GP_GY, CC.GP_KERNEL, CC.GP_DBIAS_KERNEL} and {p["dx"] for p in own} == {CC.DX_NONE, CC.DX_BF16, CC.DX_BF16_FOLD}
    assert {p["dw"] for p in own} == {CC.DW_NONE, CC.DW_BF16, CC.DW_DIRECT}
    hybrids = [c for c in BF.BLOCK if BF.block_plan(c)["dw"] == CC.DW_DIRECT]
    assert all(BF.block_plan(c)["fwd"] == CC.FWD_BF16 and BF.block_plan(c)["db"] == CC.DB_SLABS for c in hybrids)
    assert {BF.block_plan(c)["gprime"] for c in hybrids} == {CC.GP_GY, CC.GP_KERNEL} and any(c.Co == 1 and c.C0 == 40 for c in hybrids)
    for base in BF.NULL_FAMILIES.values():
        got = {c.grads for c in BF.BLOCK_NULLS if c[:10] == base[:10]}
        assert got == {tuple(g for g in CC.ALL if g in pat and (g != "x1" or base.C1)) for pat in BF._NULL_PATTERNS} - {()}
    nb = BF.block_plan(BF.K(*BF.NULL_FAMILIES["zero"][:10], grads=("b",)))          # only db: no weight-gradient launch at all
    assert (nb["dw"], nb["split"], nb["db"], nb["gprime"]) == (CC.DW_NONE, 0, CC.DB_GPRIME, CC.GP_DBIAS_KERNEL)


# ---- rounding visibility, sensitivity, conditioning -----------------------------------------------------------------------------------
def _moved(c, base, mutated, names):
    """{output: distance(mutated, base) / gate} for the outputs of `names` the row checks against the rounded statement."""
    ck = BF.checked(c)
    return {k: BF.distance(mutated[k], base[k], ck[k][1]) / ck[k][0] for k in names if k in ck and ck[k][2] == "rounded" and base[k] is not None}


def _zero_at(index):
    def f(t):
        m = torch.ones_like(t)
        m[index] = 0
        return t * m
    return f


@pytest.mark.parametrize("case", BF.params(ROWS))
def test_rounding_is_visible_and_the_rows_are_well_conditioned(case):
    inp, rnd, unr = BF.reference(case)
    e32 = {"rounded": BF.evaluate(case, inp, True, torch.float32)}
    if any(w == "unrounded" for _, _, w in BF.checked(case).values()):
        e32["unrounded"] = BF.evaluate(case, inp, False, torch.float32)
    for k, (g, norm, which) in BF.checked(case).items():
        ref = rnd[k] if which == "rounded" else unr[k]
        assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
        cond = BF.distance(e32[which][k], ref, norm)
        seen = BF.distance(unr[k], rnd[k], norm) / g if which == "rounded" else float("nan")
        print("conv_bf16_fitness %s %s torch fp32 %.2e (%.0f%% of the gate), operand rounding %.0fx the gate" % (
            BF.case_id(case), k, cond, 100 * cond / g, seen))
        assert cond <= BF.CONDITION * g, (k, cond)
        if which == "rounded":
            assert seen > BF.VISIBLE, (k, seen)


@pytest.mark.parametrize("case", BF.params([c for c in ROWS if BF.kind(c) == "block" and c.pad == CC.REFLECT]))
def test_a_dropped_tap_at_the_outermost_column_or_row_is_seen(case):
    """The padded input's outermost column (the reflected column W, which the overhang commit or the edge-column load supplies) and
    outermost row, one element of the last channel zeroed: y and the bf16 weight gradient move by more than 10x their gates; the same
    element of the padded-domain data gradient dropped before the fold: that channel's data gradient does."""
    inp, rnd, _ = BF.reference(case)
    c = case
    Cin = c.C0 + c.C1
    xp = _padded(case, inp)
    col = int(xp[c.B - 1, Cin - 1, 1:c.H + 1, c.W + 1].abs().argmax()) + 1
    row = int(xp[c.B - 1, Cin - 1, c.H + 1, 1:c.W + 1].abs().argmax()) + 1
    dxk = "dx1" if c.C1 else "dx0"
    for where, index in (("column", (c.B - 1, Cin - 1, col, c.W + 1)), ("row", (c.B - 1, Cin - 1, c.H + 1, row))):
        fw = _moved(c, rnd, BF.evaluate(c, inp, mutate={"xp": _zero_at(index)}), ("y", "dw"))
        bw = _moved(c, rnd, BF.evaluate(c, inp, mutate={"dxp": _zero_at(index)}), (dxk,))
        print("conv_bf16_sensitivity %s outermost %s: %s" % (BF.case_id(c), where, {k: "%.0fx" % v for k, v in {**fw, **bw}.items()}))
        assert "y" in fw and dxk in bw and all(v > BF.SENSITIVITY for v in {**fw, **bw}.values()), (where, fw, bw)


def _padded(c, inp):
    a = BF.rb(inp["x0"])
    if c.up0:
        a = torch.nn.functional.interpolate(a, scale_factor=2, mode="nearest")
    if c.C1:
        a = torch.cat([a, BF.rb(inp["x1"])], 1)
    return torch.nn.functional.pad(a, (1, 1, 1, 1), mode="reflect" if c.pad == CC.REFLECT else "constant")


def _ragged_rows():
    return [c for c in ROWS if (BF.route(c)["src"]["k0"] + BF.route(c)["src"]["k1"]) % BF.BC or c.Co % BF.BC]


@pytest.mark.parametrize("case", BF.params(_ragged_rows()))
def test_the_last_channel_of_a_ragged_chunk_is_seen(case):
    """Zeroing ONE pixel of the last channel of a chunk that is not full -- the input's (K = Cin: forward and weight gradient) or g''s
    (K = Co: data gradient and weight gradient) -- moves the outputs by more than 10x their gates."""
    inp, rnd, _ = BF.reference(case)
    c, r = case, BF.route(case)
    Cin = r["src"]["k0"] + r["src"]["k1"]
    if Cin % BF.BC:
        if BF.kind(c) == "block":
            xp = _padded(c, inp)[c.B - 1, Cin - 1, 1:c.H + 1, 1:c.W + 1].abs()
            iy, ix = divmod(int(xp.argmax()), c.W)
            mut = {"xp": _zero_at((c.B - 1, Cin - 1, iy + 1, ix + 1))}
        else:
            iy, ix = divmod(int(inp["x"][c.B - 1, Cin - 1].abs().argmax()), c.W)
            mut = {"x": _zero_at((c.B - 1, Cin - 1, iy, ix))}
        fw = _moved(c, rnd, BF.evaluate(c, inp, mutate=mut), ("y", "dw"))
        print("conv_bf16_sensitivity %s input channel %d of a ragged chunk: %s" % (BF.case_id(c), Cin - 1, {k: "%.0fx" % v for k, v in fw.items()}))
        assert "y" in fw and all(v > BF.SENSITIVITY for v in fw.values()), fw
    if c.Co % BF.BC:
        gp = BF.gprime32(c, inp) if BF.kind(c) == "block" else inp["gy"]
        iy, ix = divmod(int(gp[c.B - 1, c.Co - 1].abs().argmax()), gp.shape[3])
        bw = _moved(c, rnd, BF.evaluate(c, inp, mutate={"gp": _zero_at((c.B - 1, c.Co - 1, iy, ix))}), ("dx0", "dx1", "dx", "dw"))
        print("conv_bf16_sensitivity %s g' channel %d of a ragged chunk: %s" % (BF.case_id(c), c.Co - 1, {k: "%.0fx" % v for k, v in bw.items()}))
        assert bw and all(v > BF.SENSITIVITY for v in bw.values()), bw


def test_reference_is_shared_and_states_what_the_issue_states():
    c = BF.BLOCK[5]
    a, b = BF.reference(c), BF.reference(c._replace(grads=("w",)))
    assert a is b and c.act == BF.TANH
    inp, rnd, unr = a
    y = inp["y"]
    assert torch.equal(BF.gprime32(c, inp), inp["gy"] * (1.0 - y.double() * y.double()).float())
    assert torch.equal(rnd["db"], BF.gprime32(c, inp).double().sum((0, 2, 3)))        # the bias gradient sums the unrounded fp32 g'
    assert torch.equal(BF.rb(torch.tensor([1.00390625, 1.01171875])), torch.tensor([1.0, 1.015625], dtype=torch.float64))   # nearest even
    d = BF.BLOCK[7]                                                                 # Co < 16: the weight gradient's statement is unrounded
    assert not BF.dw_is_bf16(d) and BF.checked(d)["dw"] == (CC.DIRECT_TOL, "max", "unrounded")
    inp, rnd, unr = BF.reference(d)
    assert torch.equal(rnd["dw"], unr["dw"]) and not torch.equal(rnd["y"], unr["y"])
