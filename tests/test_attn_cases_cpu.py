"""The cases of tests/attn_cases.py are fit to judge the AttentionConv kernels with: the table reaches every mechanism it is
there for (computed from the kernels' tile constants), every case is finite and well conditioned (torch's own fp32 evaluation
of the statement is within 1e-4 of fp64 in every compared tensor), the exact claims (planted zeros, uniform softmax, the
analytically zero key_conv.bias gradient) hold for the statement itself, and the statement is tied to the recorded output of the
reference (tests/golden/fusion_v3.npz).  Needs no GPU."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import attn_cases as AC
import make_golden_r2 as MG2
from helpers import T, close
from oracle import fusion_ref as FR
from test_fusion_oracle import attn_state


def test_case_table_hits_the_mechanisms_it_is_there_for():
    (fh, fw), (bh, bw), P = AC.FWD_TILE, AC.BWD_TILE, AC.REDUCE_PASS
    hw = {(c.H, c.W) for c in AC.CASES}
    assert (1, 1) in hw and (fh, fw) in hw and (bh, bw) in hw
    assert any(h == 1 and w == fw + 1 for h, w in hw) and any(h == fh + 1 and w == 1 for h, w in hw)       # narrower than the ring
    assert (fh + 1, fw + 1) in hw and (bh + 1, bw + 1) in hw                                               # one past, both directions
    assert any(h % bh == 0 and w % bw == 0 and h > bh and w > bw for h, w in hw)
    assert any(h % fh == 0 and w % fw == 0 and h > fh and w > fw for h, w in hw)
    # the flat block index with every grid dimension above 2, forward and backward
    assert any(c.B > 2 and AC.ceil_div(c.W, bw) > 2 and AC.ceil_div(c.H, bh) > 2 and AC.ceil_div(c.W, fw) > 2 for c in AC.CASES)
    nb = [AC.bwd_blocks(c) for c in AC.CASES]
    assert any(P < n < 2 * P and n % P for n in nb) and any(n > 2 * P and n % P for n in nb)
    assert max(c.B * c.C * c.H * c.W for c in AC.CASES) <= 340000
    assert AC.DETERMINISM in AC.CASES and AC.bwd_blocks(AC.DETERMINISM) > 2 * P
    assert {c.C for c in AC.CASES} == {2, 4}
    # pixel shuffle in x (= dx), in res, in dres; as the first source; batch chunks; a batch stride beyond C*H*W
    assert any("ps2" in c.x_layout for c in AC.CASES)
    assert any("ps2" in (AC.res_layout(c) or ()) for c in AC.CASES)
    assert sum(1 for c in AC.CASES if c.dres and "ps2" in AC.dres_layout(c)) >= 2
    assert any(c.x_layout[0] == "ps2" and len(c.x_layout) > 1 for c in AC.CASES)
    assert any(set(c.x_layout) == {"ps2"} and c.C == 4 for c in AC.CASES)
    assert any(c.x_layout.count("c1") == 2 for c in AC.CASES)
    assert any("w4" in (AC.res_layout(c) or ()) for c in AC.CASES)
    assert all(c.H % 2 == 0 and c.W % 2 == 0 for c in AC.CASES if "ps2" in c.x_layout + (AC.res_layout(c) or ()))
    # every legal flag combination on both flag shapes
    full = set(itertools.product((0, 1), ("none", "res", "relu_res"), (0, 1), (0, 1)))
    for B, C, H, W in AC.FLAG_SHAPES:
        seen = {(c.relu_in, "none" if c.res_layout is None else "relu_res" if c.relu_res else "res", c.dx_add, c.dres)
                for c in AC.FLAGS if c[:4] == (B, C, H, W)}
        assert seen == full
    assert all(not (c.dres and c.relu_res and c.res_layout is None) for c in AC.CASES)
    assert len(set(AC.CASES)) == len(AC.CASES) and len({AC.case_id(c) for c in AC.CASES}) == len(AC.CASES)
    # the kink case plants a few dozen zeros of both signs on corners, the last column and backward-tile edges
    pos = AC.kink_positions(AC.KINK)
    assert len(pos) >= 24 and {(y, x) for _, y, x, _ in pos} >= {(0, 0), (0, AC.KINK.W - 1), (AC.KINK.H - 1, 0), (AC.KINK.H - 1, AC.KINK.W - 1)}
    assert any(y % bh == 0 and y for _, y, _, _ in pos) and any(x % bw == 0 and x for _, _, x, _ in pos)
    assert {str(v) for *_, v in pos} == {"0.0", "-0.0"}
    assert {c.param_style for c in AC.SOFTMAX} == {"wide", "uniform", "norel"}


def _planted(case, shift):
    m = torch.zeros(case.B, case.C, case.H, case.W, dtype=torch.bool)
    for c, y, x, _ in AC.kink_positions(case):
        m[:, (c + shift) % case.C, y, x] = True
    return m


@pytest.mark.parametrize("case", AC.params())
def test_case_is_well_conditioned_and_its_exact_claims_hold(case):
    inp, r64, r32, info = AC.reference(case)          # reference() asserts the "wide" preconditions
    assert r64.keys() == r32.keys()
    assert all(not t.requires_grad and t.dtype == torch.float64 and torch.equal(t, t.float().double())
               for t in inp["x"] + inp["res"] + list(inp["params"].values()) + [inp["gy"]])
    want = ["y"] + ["dx.%d" % i for i in range(len(case.x_layout))] + list(AC.PARAM_KEYS)
    want += ["dres.%d" % i for i in range(len(AC.dres_layout(case)))] if case.dres else []
    assert sorted(r64) == sorted(want)
    for name in r64:
        assert r64[name].dtype == torch.float64 and r32[name].dtype == torch.float32
        assert torch.isfinite(r64[name]).all() and torch.isfinite(r32[name]).all(), name
    for name in AC.compared(case, r64):
        e32 = AC.rel_err(r32[name], r64[name])
        assert e32 < 1e-4, (name, e32)
    # gradients arrive in the sources' own shapes
    for i, k in enumerate(case.x_layout):
        assert r64["dx.%d" % i].shape == AC.source_shape(k, case.B, case.H, case.W)
    if case.dres:
        for i, k in enumerate(AC.dres_layout(case)):
            assert r64["dres.%d" % i].shape == AC.source_shape(k, case.B, case.H, case.W)
    # ReLU acts on given inputs: no decision can differ between the precisions
    for t in inp["x"] + inp["res"]:
        assert torch.equal(t > 0, t.float() > 0)
    assert bool((AC.gather(case.x_layout, inp["x"]) > 0).any())          # not a map the input ReLU wipes out
    # the analytically zero gradient, in both precisions
    assert AC.key_bias_ok(r64[AC.KEY_BIAS], info) and AC.key_bias_ok(r32[AC.KEY_BIAS], info)
    assert info["scale"] > 0
    if case.dres and case.res_layout is None:
        for r in (r64, r32):
            assert torch.equal(r["dres.0"].double(), inp["gy"])
    if case.param_style == "kink":
        mx, mr = _planted(case, 0), _planted(case, 1)
        assert bool((inp["x"][0][mx] == 0).all()) and bool((inp["res"][0][mr] == 0).all())
        assert bool(torch.signbit(inp["x"][0][mx]).any()) and not bool(torch.signbit(inp["x"][0][mx]).all())
        for r in (r64, r32):
            assert bool(((r["dx.0"] - inp["dx_add"].to(r["dx.0"].dtype))[mx] == 0).all())
            assert bool((r["dres.0"][mr] == 0).all())
            assert bool((r["dres.0"][~mr & (inp["res"][0] > 0)] != 0).all())
    if case.param_style == "wide":
        assert info["L"] >= AC.WIDE_MIN_L and info["amin32"] == 0.0
    if case.param_style == "uniform":
        assert info["L"] == 0.0
        mean = AC.uniform_mean(case, inp)
        assert AC.rel_err(r64["y"], mean) < 1e-14 and AC.rel_err(r32["y"], mean) <= AC.bound(0.0, 0.0)
        for r in (r64, r32):
            for k in ("key_conv.weight", "rel_h", "rel_w"):
                assert bool((r[k] == 0).all()), k
    if case.param_style == "norel":
        assert not inp["params"]["rel_h"].any() and not inp["params"]["rel_w"].any() and r64["rel_h"].any()


def _gather_by_index(layout, srcs, H, W):
    """The channel map as dc_attn_map addresses it: a pixel-shuffled channel is plane (y&1)*2 + (x&1) at (y>>1, x>>1)."""
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    parts = [t[:, (y & 1) * 2 + (x & 1), y >> 1, x >> 1].unsqueeze(1) if k == "ps2" else t for k, t in zip(layout, srcs)]
    return torch.cat(parts, 1)


@pytest.mark.parametrize("case", [pytest.param(c, id=AC.case_id(c)) for c in AC.PIXEL_SHUFFLE])
def test_layout_gather_is_cat_plus_pixel_shuffle(case):
    inp = AC.reference(case)[0]
    for lay, srcs in ((case.x_layout, inp["x"]), (AC.res_layout(case), inp["res"])):
        if lay:
            want = torch.cat([FR.upscale_ps_shuffle_only(t) if k == "ps2" else t for k, t in zip(lay, srcs)], 1)
            assert want.shape == (case.B, case.C, case.H, case.W)
            assert torch.equal(AC.gather(lay, srcs), want)
            assert torch.equal(_gather_by_index(lay, srcs, case.H, case.W), want)
            assert torch.equal(F.pixel_shuffle(F.pixel_unshuffle(want, 2), 2), want)


def test_statement_reproduces_the_recorded_reference_output(golden):
    """evaluate() fed the fixture's input and parameters gives the reference's own recorded AttentionConv output and gradients
    (the tolerances of tests/test_fusion_oracle.py), and the logits restated for the spread measurement are the oracle's."""
    g = golden["fusion_v3"]
    x, _ = MG2.attn_case()
    case = AC._case(*x.shape, relu_in=0)
    inp = {"x": [x.double()], "res": [], "params": {k: v.double() for k, v in attn_state().items()}, "gy": T(g["ac_cot"]).double(),
           "dx_add": None}
    r32, _ = AC.evaluate(case, inp, torch.float32)
    close(r32["y"], g["ac_y"], rtol=1e-5, atol=1e-6)
    close(r32["dx.0"], g["ac_gx"], rtol=1e-4, atol=1e-6)
    for k in AC.PARAM_KEYS:
        close(r32[k], g["ac_g_" + k], rtol=1e-4, atol=2e-5, msg=k)
    r64, info = AC.evaluate(case, inp, torch.float64)
    lg, vt = AC.logits(inp["x"][0], inp["params"])
    assert AC.rel_err((torch.softmax(lg, -1) * vt).sum(-1), r64["y"]) < 1e-14
    assert info["L"] == float((lg.max(-1).values - lg.min(-1).values).max())


def test_bound_is_the_stated_formula():
    assert AC.bound(0.0, 0.0) == AC.LC.gate_bound(0.0)
    assert AC.bound(1e-6, 50.0) == AC.LC.gate_bound(1e-6) + 2 * 50.0 * 2.0 ** -24
    assert [AC.param_count(C) for C in (2, 4)] == [24, 66]
