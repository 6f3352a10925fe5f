"""The cases of tests/layer_ops_cases.py are fit to judge a kernel with: for every case the builder's kink preconditions hold, the
reference statement is finite in fp32 and fp64, torch's own fp32 evaluation is within 1e-4 of fp64 in every compared tensor (so
the inputs are not ill-conditioned and `4 x the fp32 error` is a tight bound), no element of the fp32 evaluation sits on the
other side of a kink, and the exact-zero claims hold for the fp32 CPU statement too.  Needs no GPU."""
import pytest
import torch

import layer_ops_cases as LC

ALL = [pytest.param(op, c, id="%s-%s" % (op, LC.case_id(c))) for op in LC.OPS for c in LC.CASES[op]]


def test_case_tables_hit_the_mechanisms_they_are_there_for():
    cd = lambda a, b: -(-a // b)
    ssim = LC.CASES["ssim"]
    assert any(H == 3 and W == 3 for _, _, H, W in ssim) and any(H < 8 and W < 32 for _, _, H, W in ssim)
    assert any(H % 8 == 1 and W % 32 == 1 for _, _, H, W in ssim) and any(H % 8 and W % 32 and H > 8 and W > 64 for _, _, H, W in ssim)
    sm = LC.CASES["smooth"]
    assert any(h * w < 2048 for _, _, h, w, _ in sm) and any(h * w == 2048 and C == 1 for _, C, h, w, _ in sm)
    assert any(h * w > 2048 and h * w % 2048 for _, _, h, w, _ in sm) and any(B * cd(h * w, 2048) > 256 for B, _, h, w, _ in sm)
    pj = LC.CASES["project3d"]
    assert any(H * W == 1024 for _, H, W, _ in pj) and any(cd(H * W, 1024) > 64 and H * W % 1024 for _, H, W, _ in pj)
    assert any(d for *_, d in pj)
    assert any(n % 256 and n > 4096 * 256 for (n,) in LC.CASES["disp_to_depth"])
    assert any(B * C > 65535 for B, C, _, _ in LC.CASES["nearest2x"])
    assert all(H * W % 256 for _, H, W in LC.CASES["backproject"] if (H, W) != (16, 16))
    gs = LC.CASES["grid_sample"]
    assert {ac for *_, ac in gs} == {False, True} and any(Ho * Wo > 256 and (Ho, Wo) != (H, W) for _, _, H, W, Ho, Wo, _ in gs)
    assert all(LC.DETERMINISM[op] in LC.CASES[op] for op in LC.OPS)


@pytest.mark.parametrize("op,case", ALL)
def test_case_is_well_conditioned_and_off_the_kinks(op, case):
    inputs, r64, r32 = LC.reference(op, case)          # build() asserts the kink preconditions
    assert r64.keys() == r32.keys() and not any(v.requires_grad for v in inputs.values())
    for name in r64:
        assert r64[name].dtype == torch.float64 and r32[name].dtype == torch.float32
        assert torch.isfinite(r64[name]).all() and torch.isfinite(r32[name]).all(), (op, case, name)
        e_32 = LC.rel_err(r32[name], r64[name])
        assert e_32 < 1e-4, (op, case, name, e_32)
    if op == "grid_sample":
        _, _, H, W, _, _, ac = case
        free = ~LC.grid_corner_mask(inputs["grid"])
        # the same cell and the same side of the clip in fp32 as in fp64
        g = inputs["grid"]
        for k, size in ((0, W), (1, H)):
            u64 = LC.grid_unnormalised(g, H, W, ac)[k]
            u32 = ((g[..., k] + 1) / 2 * (size - 1)) if ac else (((g[..., k] + 1) * size - 1) / 2)
            c64, c32 = u64.clamp(0, size - 1), u32.clamp(0, size - 1)
            assert torch.equal(torch.floor(c64)[free], torch.floor(c32).double()[free])
            assert torch.equal(((u64 <= 0) | (u64 >= size - 1))[free], ((u32 <= 0) | (u32 >= size - 1))[free])
        clamped = LC.grid_clamped(g, H, W, ac)
        for r in (r64, r32):                            # ATen's rule: a clamped coordinate has gradient exactly 0
            assert bool((r["dgrid"][clamped] == 0).all())
        if min(H, W) > 2:
            assert bool((r32["dgrid"][~clamped & free.unsqueeze(-1)] != 0).any())
    if op == "smooth":
        # no flipped sign(): the fp32 gradient differs from fp64 by rounding only, pointwise
        scale = float(r64["ddisp"].abs().max())
        assert float((r32["ddisp"].double() - r64["ddisp"]).abs().max()) < 1e-5 * scale
        if case[4]:
            m = LC.smooth_patch_interior(case)
            assert int(m.sum()) == 36 * case[0] and bool((r32["ddisp"][m] == 0).all()) and bool((r64["ddisp"][m] == 0).all())
            assert bool((r32["ddisp"][~m] != 0).any())
    if op == "nearest2x":
        assert torch.equal(r32["out"], inputs["x"].repeat_interleave(2, 2).repeat_interleave(2, 3))
    if op == "interp" and case == LC.IDENTITY_INTERP:
        assert torch.equal(r32["out"], inputs["x"]) and torch.equal(r32["dx"], inputs["cot"])
    if op == "backproject":
        assert bool((r32["cam"][:, 3] == 1).all())


def test_gate_bound_is_the_stated_formula():
    assert LC.gate_bound(0.0) == 4 * 2.0 ** -23
    assert LC.gate_bound(1e-6) == 4 * 1e-6 + 4 * 2.0 ** -23
    assert LC.rel_err(torch.tensor([1.0, 3.0]), torch.tensor([1.0, 2.0], dtype=torch.float64)) == 0.5
    assert LC.rel_err(torch.tensor([0.25]), torch.zeros(1, dtype=torch.float64)) == 0.25
