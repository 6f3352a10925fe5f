"""The unfused `layers.*` kernels (csrc/layer_ops.hip) against fp64 statements of the same operations at ragged, multi-block and
edge shapes: sizes that are no multiple of a tile / chunk / block, maps smaller than one, and the sizes at which a strided
reduction takes its second trip.  Cases, inputs and references: tests/layer_ops_cases.py (their fitness is the subject of
tests/test_layer_ops_cases_cpu.py).  Forward and gradients (random cotangent, CPU autograd of the fp64 statement) under one
gate, no outlier budget; the piecewise parts (floor, clip, sign) are handled by keeping the inputs off the kinks."""
import pytest
import torch

import layer_ops_cases as LC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# The gate: e_hip = max|hip - f64| / max|f64| <= FACTOR * e_32 + 4 * 2^-23, with e_32 the same figure of torch's fp32 CPU evaluation
# of the statement on the same inputs.  4 is the project's margin for a kernel that contracts multiply-adds and uses the hardware
# reciprocal and __expf where torch rounds every operation (test_adam_gpu.py); the additive term covers statements that fp32
# evaluates exactly.  Measured (profiles/layer_ops_parity.txt), worst e_hip / (e_32 + 2^-23) per operation, to be <= FACTOR:
#   ssim 1.05, smooth 0.61, backproject 0.39, project3d 0.95, grid_sample 0.98, interp 0.84, nearest2x 0.28, disp_to_depth 0.64
# -- no operation needs more than the 4, so none has a factor of its own.
FACTOR = {op: 4.0 for op in LC.OPS}


def _dev(inputs):
    return {k: v.to(DEV) for k, v in inputs.items()}


def _hip_ssim(case, d):
    import layers
    x, y = d["x"].clone().requires_grad_(), d["y"].clone().requires_grad_()
    out = layers.SSIM()(x, y)
    dx, dy = torch.autograd.grad((out * d["cot"]).sum(), [x, y])
    return {"out": out.detach(), "dx": dx, "dy": dy}


def _hip_smooth(case, d):
    import layers
    disp = d["disp"].clone().requires_grad_()
    out = layers.get_smooth_loss(disp, d["img"])
    (dd,) = torch.autograd.grad(out * d["cot"], [disp])
    return {"out": out.detach().reshape(1), "ddisp": dd}


def _hip_backproject(case, d, cot=None):
    import layers
    B, H, W = case
    depth = d["depth"].clone().requires_grad_()
    cam = layers.BackprojectDepth(B, H, W).to(DEV)(depth, d["inv_K"])
    (dd,) = torch.autograd.grad((cam * (d["cot"] if cot is None else cot)).sum(), [depth])
    return {"cam": cam.detach(), "ddepth": dd}


def _hip_project3d(case, d):
    import layers
    B, H, W, _ = case
    p, T = d["points"].clone().requires_grad_(), d["T"].clone().requires_grad_()
    grid = layers.Project3D(B, H, W)(p, d["K"], T)
    dp, dT = torch.autograd.grad((grid * d["cot"]).sum(), [p, T])
    return {"grid": grid.detach(), "dpoints": dp, "dT": dT}


def _hip_grid_sample(case, d):
    import layers
    grid = d["grid"].clone().requires_grad_()
    out = layers.grid_sample(d["img"], grid, padding_mode="border", align_corners=case[6])
    (dg,) = torch.autograd.grad((out * d["cot"]).sum(), [grid])
    return {"out": out.detach(), "dgrid": dg}


def _hip_interp(case, d):
    import layers
    x = d["x"].clone().requires_grad_()
    out = layers.interpolate_bilinear(x, [case[4], case[5]])
    (dx,) = torch.autograd.grad((out * d["cot"]).sum(), [x])
    return {"out": out.detach(), "dx": dx}


def _hip_nearest2x(case, d):
    import layers
    x = d["x"].clone().requires_grad_()
    out = layers.upsample(x)
    (dx,) = torch.autograd.grad((out * d["cot"]).sum(), [x])
    return {"out": out.detach(), "dx": dx}


def _hip_disp_to_depth(case, d):
    import layers
    disp = d["disp"].clone().requires_grad_()
    scaled, depth = layers.disp_to_depth(disp, LC.MIN_DEPTH, LC.MAX_DEPTH)
    ls, ld = (scaled * d["cot_scaled"]).sum(), (depth * d["cot_depth"]).sum()
    grads = [torch.autograd.grad(l, [disp], retain_graph=True)[0] for l in (ls + ld, ls, ld)]
    return {"scaled": scaled.detach(), "depth": depth.detach(), "dd_both": grads[0], "dd_scaled": grads[1], "dd_depth": grads[2]}


_HIP = {"ssim": _hip_ssim, "smooth": _hip_smooth, "backproject": _hip_backproject, "project3d": _hip_project3d,
        "grid_sample": _hip_grid_sample, "interp": _hip_interp, "nearest2x": _hip_nearest2x, "disp_to_depth": _hip_disp_to_depth}


def _check(op, case, edit=None):
    """Run the `layers.*` entry on the device, gate every tensor of the case against the fp64 statement, and compare two runs bit
    for bit at the operation's ragged case.  `edit(name, tensor)`: a last word on a device tensor before it is compared.  Returns
    (inputs, device inputs, device results, fp64 results)."""
    inputs, r64, r32 = LC.reference(op, case)
    d = _dev(inputs)
    got = _HIP[op](case, d)
    assert got.keys() == r64.keys()
    failures = []
    for name in r64:
        assert got[name].shape == r64[name].shape and got[name].dtype == torch.float32, (op, case, name)
        t = got[name].cpu()
        assert torch.isfinite(t).all(), (op, case, name)
        if edit is not None:
            t = edit(name, t)
        e_hip, e_32 = LC.rel_err(t, r64[name]), LC.rel_err(r32[name], r64[name])
        print("layer_ops_parity %-13s %-24s %-9s e_hip=%.3e e_32=%.3e ratio=%.2f" % (
            op, LC.case_id(case), name, e_hip, e_32, e_hip / (e_32 + LC.EPS32)))
        if not e_hip <= LC.gate_bound(e_32, FACTOR[op]):
            failures.append((name, e_hip, e_32))
    assert not failures, (op, case, failures)
    if tuple(case) == LC.DETERMINISM[op]:
        again = _HIP[op](case, d)
        for name in got:
            assert torch.equal(got[name], again[name]), (op, case, name, "differs between two runs")
    return inputs, d, got, r64


@pytest.mark.parametrize("case", LC.params("ssim"))
def test_ssim(case):
    import layers
    _, d, _, _ = _check("ssim", case)
    if case == (2, 3, 9, 33):      # the reference's known answer, SSIM(x, x) == 0, away from the fixture's tile-multiple shape
        assert float(layers.SSIM()(d["x"], d["x"]).abs().max()) < 1e-6
        flat = torch.full_like(d["x"], 0.7311)
        assert float(layers.SSIM()(flat, flat).abs().max()) < 1e-6


@pytest.mark.parametrize("case", LC.params("smooth"))
def test_get_smooth_loss(case):
    _, _, got, _ = _check("smooth", case)
    if case[4]:                    # inside the constant block |d - neighbour| has gradient exactly 0, as torch's abs gives
        m = LC.smooth_patch_interior(case)
        assert bool((got["ddisp"].cpu()[m] == 0).all())


@pytest.mark.parametrize("case", LC.params("backproject"))
def test_backproject_and_pix_coords(case):
    import layers
    from oracle import ref_cpu as R
    B, H, W = case
    inputs, d, got, _ = _check("backproject", case)
    assert torch.equal(layers.BackprojectDepth(B, H, W).to(DEV).pix_coords.cpu(), R.pix_coords(B, H, W))
    assert bool((got["cam"][:, 3] == 1).all())
    cot = d["cot"].clone()         # the homogeneous row is a constant: its cotangent reaches nothing
    cot[:, 3] = torch.randn(B, H * W, generator=torch.Generator().manual_seed(5)).to(DEV) * 100
    assert torch.equal(_hip_backproject(case, d, cot)["ddepth"], got["ddepth"])


@pytest.mark.parametrize("case", LC.params("project3d"))
def test_project3d(case):
    _check("project3d", case)      # d_points in all four rows, the full 4x4 dT


@pytest.mark.parametrize("case", LC.params("grid_sample"))
def test_grid_sample(case):
    _, _, H, W, _, _, ac = case
    inputs = LC.reference("grid_sample", case)[0]
    corners = LC.grid_corner_mask(inputs["grid"])
    seen = {}

    def edit(name, t):
        if name == "dgrid":        # samples exactly on (+-1, +-1): forward only; ATen's rule (x >= size - 1: zero) holds on the device
            seen["corner_grad"] = t[corners].clone()
            t = t.clone()
            t[corners] = 0
        return t

    _, _, got, _ = _check("grid_sample", case, edit)
    assert bool((seen["corner_grad"] == 0).all())
    clamped = LC.grid_clamped(inputs["grid"], H, W, ac) & ~corners.unsqueeze(-1)
    assert bool((got["dgrid"].cpu()[clamped] == 0).all())          # a coordinate held by the border clip: gradient exactly 0


@pytest.mark.parametrize("case", LC.params("interp"))
def test_interpolate_bilinear(case):
    inputs, _, got, _ = _check("interp", case)
    if case == LC.IDENTITY_INTERP:
        assert torch.equal(got["out"].cpu(), inputs["x"]) and torch.equal(got["dx"].cpu(), inputs["cot"])


@pytest.mark.parametrize("case", LC.params("nearest2x"))
def test_upsample_nearest2x(case):
    inputs, _, got, _ = _check("nearest2x", case)
    assert torch.equal(got["out"].cpu(), inputs["x"].repeat_interleave(2, 2).repeat_interleave(2, 3))


@pytest.mark.parametrize("case", LC.params("disp_to_depth"))
def test_disp_to_depth_grid_stride(case):
    _check("disp_to_depth", case)  # both outputs; the backward with both cotangents, with only `scaled` used, with only `depth` used


def test_upsample_nearest2x_takes_views_at_an_odd_float_offset():
    """The kernels move rows as float2, so the C entry points refuse a pointer that is not 8-byte aligned; the autograd wrapper
    meets one when the upstream gradient is a contiguous view that starts at an odd float offset, and copies it."""
    import layers
    B, C, h, w = 2, 3, 5, 7
    g = torch.Generator().manual_seed(11)
    n = B * C * 4 * h * w
    flat = torch.rand(n + 2, generator=g).to(DEV)
    cot = flat[1:1 + n].view(B, C, 2 * h, 2 * w)
    assert cot.is_contiguous() and cot.data_ptr() % 8 == 4
    xflat = torch.rand(B * C * h * w + 2, generator=g).to(DEV)
    x = xflat[1:1 + B * C * h * w].view(B, C, h, w).requires_grad_()
    assert x.data_ptr() % 8 == 4
    out = layers.upsample(x)
    assert torch.equal(out.detach(), x.detach().repeat_interleave(2, 2).repeat_interleave(2, 3))
    (dx,) = torch.autograd.grad(out, [x], grad_outputs=cot)
    want = cot.cpu().double().reshape(B, C, h, 2, w, 2).sum((3, 5))
    assert LC.rel_err(dx, want) <= LC.gate_bound(LC.rel_err(cot.cpu().reshape(B, C, h, 2, w, 2).sum((3, 5)), want))
    (dx2,) = torch.autograd.grad(layers.upsample(x), [x], grad_outputs=cot.clone())          # the aligned copy: same bits
    assert torch.equal(dx, dx2)
