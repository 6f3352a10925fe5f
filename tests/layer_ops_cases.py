"""Case tables, seeded input builders and fp64 reference statements for the unfused `layers.*` kernels (csrc/layer_ops.hip) at
ragged, multi-block and edge shapes.  Shared by tests/test_layer_ops_cases_cpu.py (no GPU: preconditions and conditioning) and
tests/test_layer_ops_shapes_gpu.py (the kernels against these statements).

Every operation has
    CASES[op]             the shapes, each chosen for one mechanism of its kernel (tile / chunk / block remainder, stride trips)
    build(op, case)       seeded fp32 CPU inputs and cotangents; asserts that the inputs stay away from the kinks of the operation
    evaluate(op, case, inputs, dtype)
                          the reference statement, forward and gradients by CPU autograd, in `dtype` (fp64 = the reference,
                          fp32 = the yardstick of the gate)
`reference(op, case)` caches (inputs, fp64 result, fp32 result); nobody may modify what it returns.

The statements are oracle/ref_cpu.py's where it has one (ssim, smooth_loss, backproject, project3d, disp_to_depth) and the torch
functional otherwise (F.grid_sample border, F.interpolate bilinear / nearest).
"""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from helpers import random_poses
from oracle import ref_cpu as R

EPS32 = 2.0 ** -23
MIN_DEPTH, MAX_DEPTH = 0.1, 100.0
KINK_MARGIN, KINK_NUDGE = 1e-3, 2e-3       # grid_sample: distance of an unnormalised coordinate from an integer

CASES = {
    # (B, C, H, W): 32x8 output tiles, halo 1 (forward) / 2 (backward)
    "ssim": [(1, 1, 2, 2), (1, 2, 3, 3), (1, 3, 8, 32), (2, 3, 9, 33), (1, 1, 17, 70), (2, 3, 40, 72)],
    # (B, C, h, w, patch): 2048-pixel chunks, the final kernel strides by 256 partials; patch = an 8x8 constant block
    "smooth": [(1, 3, 2, 2, False), (2, 3, 9, 13, False), (1, 1, 32, 64, False), (1, 3, 33, 67, False),
               (3, 3, 384, 480, False), (1, 3, 33, 67, True)],
    # (B, H, W): one thread per pixel, 256 per block
    "backproject": [(1, 1, 1), (2, 9, 13), (1, 16, 16), (3, 33, 35)],
    # (B, H, W, dense): 1024 pixels per block in the backward, the dT reduction strides by 64 blocks; dense = full 4x4 K and T
    "project3d": [(1, 2, 2, False), (2, 9, 13, False), (2, 32, 32, False), (3, 33, 35, False), (1, 130, 520, False),
                  (3, 33, 35, True)],
    # (B, C, H, W, Ho, Wo, align_corners)
    "grid_sample": [s + (ac,) for s in [(1, 1, 1, 1, 3, 3), (2, 3, 7, 9, 5, 6), (1, 4, 1, 12, 4, 5), (1, 1, 12, 1, 4, 5),
                                        (2, 3, 24, 40, 17, 31), (1, 2, 16, 16, 16, 16)] for ac in (False, True)],
    # (B, C, h, w, Ho, Wo)
    "interp": [(2, 3, 7, 5, 13, 17), (2, 3, 13, 17, 7, 5), (1, 2, 6, 10, 6, 25), (1, 1, 1, 1, 4, 5), (1, 2, 4, 5, 1, 1),
               (1, 1, 24, 80, 192, 640), (1, 3, 5, 6, 5, 6)],
    # (B, C, h, w): one thread per input pixel, grid-y loop beyond 65535 planes
    "nearest2x": [(1, 1, 1, 1), (2, 3, 5, 7), (1, 2, 16, 16), (3, 5, 17, 19), (65539, 1, 1, 1)],
    # n: the grid is capped at 4096 blocks of 256, so the grid-stride loop needs n > 1,048,576
    "disp_to_depth": [(1048576 + 257,)],
}
# one ragged case per operation for the run-to-run bitwise comparison (no kernel here uses atomics)
DETERMINISM = {"ssim": (2, 3, 9, 33), "smooth": (1, 3, 33, 67, False), "backproject": (3, 33, 35),
               "project3d": (1, 130, 520, False), "grid_sample": (2, 3, 24, 40, 17, 31, False), "interp": (2, 3, 13, 17, 7, 5),
               "nearest2x": (3, 5, 17, 19), "disp_to_depth": (1048576 + 257,)}
IDENTITY_INTERP = (1, 3, 5, 6, 5, 6)
N_CORNERS = 4          # grid_sample: the first four samples of image 0 sit exactly on (+-1, +-1)
PATCH = (5, 11, 8)     # smooth: (top, left, size) of the constant block


def case_id(case):
    return "x".join(str(int(v)) if not isinstance(v, bool) else "FT"[v] for v in case)


def _leaf(t, dt):
    """A fresh leaf in `dt` (`.to` alone hands back the shared input itself when the type already matches)."""
    return t.detach().to(dt).clone().requires_grad_()


def _gen(op, case):
    return torch.Generator().manual_seed(zlib.crc32(repr((op, tuple(case))).encode()))


# ---- SSIM ---------------------------------------------------------------------------------------------------------------------
def _build_ssim(case, g):
    B, C, H, W = case
    inp = {"x": torch.rand(B, C, H, W, generator=g), "y": torch.rand(B, C, H, W, generator=g),
           "cot": torch.rand(B, C, H, W, generator=g)}
    v = R.ssim(inp["x"].double(), inp["y"].double())
    # the clamp to [0, 1] is the only kink: independent images sit near 0.5
    assert float(v.min()) > 1e-3 and float(v.max()) < 1 - 1e-3, ("ssim", case, float(v.min()), float(v.max()))
    return inp


def _eval_ssim(case, inp, dt):
    x, y = _leaf(inp["x"], dt), _leaf(inp["y"], dt)
    out = R.ssim(x, y)
    dx, dy = torch.autograd.grad((out * inp["cot"].to(dt)).sum(), [x, y])
    return {"out": out.detach(), "dx": dx, "dy": dy}


# ---- get_smooth_loss ----------------------------------------------------------------------------------------------------------
def smooth_patch_interior(case):
    """Pixels whose four neighbours all lie inside the constant block: their gradient is exactly 0."""
    t, l, s = PATCH
    m = torch.zeros(case[0], 1, case[2], case[3], dtype=torch.bool)
    m[:, :, t + 1:t + s - 1, l + 1:l + s - 1] = True
    return m


def _build_smooth(case, g):
    B, C, h, w, patch = case
    n = h * w
    disp = torch.stack([torch.randperm(n, generator=g).double() / n for _ in range(B)]).reshape(B, 1, h, w)
    inside = torch.zeros(B, 1, h, w, dtype=torch.bool)
    if patch:
        t, l, s = PATCH
        disp[:, :, t:t + s, l:l + s] = (n // 2 + 0.5) / n        # half a step away from every other value
        inside[:, :, t:t + s, l:l + s] = True
    inp = {"disp": disp.float(), "img": torch.rand(B, C, h, w, generator=g), "cot": torch.tensor(1.7)}
    # sign(d - neighbour) is decided: neighbours differ by at least 1/(h w) (half of that at the block's rim), less the rounding of
    # the two values to fp32 (half an ulp of a number below 1 each)
    d = inp["disp"].double()
    step = (0.5 if patch else 1.0) / n - 2.0 ** -24
    assert step > 0.9 * (0.5 if patch else 1.0) / n
    for dim, a, b in ((3, slice(None, -1), slice(1, None)), (2, slice(None, -1), slice(1, None))):
        ia = [slice(None)] * 4; ib = [slice(None)] * 4
        ia[dim], ib[dim] = a, b
        both = inside[tuple(ia)] & inside[tuple(ib)]
        diff = (d[tuple(ia)] - d[tuple(ib)]).abs()
        assert bool((diff[~both] >= step).all()) and bool((diff[both] == 0).all()), ("smooth", case)
    return inp


def _eval_smooth(case, inp, dt):
    d = _leaf(inp["disp"], dt)
    out = R.smooth_loss(d, inp["img"].to(dt))
    (dd,) = torch.autograd.grad(out * inp["cot"].to(dt), [d])
    return {"out": out.detach().reshape(1), "ddisp": dd}


# ---- BackprojectDepth ---------------------------------------------------------------------------------------------------------
def _depth(B, H, W, g):
    return 0.5 + 19.5 * torch.rand(B, 1, H, W, generator=g)


def _build_backproject(case, g):
    B, H, W = case
    return {"depth": _depth(B, H, W, g), "inv_K": torch.randn(B, 4, 4, generator=g),
            "cot": torch.randn(B, 4, H * W, generator=g)}


def _eval_backproject(case, inp, dt):
    d = _leaf(inp["depth"], dt)
    cam = R.backproject(d, inp["inv_K"].to(dt))
    (dd,) = torch.autograd.grad((cam * inp["cot"].to(dt)).sum(), [d])
    return {"cam": cam.detach(), "ddepth": dd}


# ---- Project3D ----------------------------------------------------------------------------------------------------------------
def _synthetic_K(B, H, W):
    K = R.KITTI_K.copy()
    K[0, :] *= W
    K[1, :] *= H
    return (torch.from_numpy(K).unsqueeze(0).repeat(B, 1, 1),
            torch.from_numpy(np.linalg.pinv(K)).unsqueeze(0).repeat(B, 1, 1))


def _build_project3d(case, g):
    B, H, W, dense = case
    K, inv_K = _synthetic_K(B, H, W)
    points = R.backproject(_depth(B, H, W, g), inv_K)
    T = random_poses(B, seed=int(torch.randint(1 << 30, (1,), generator=g)))[0]
    if dense:
        # every entry of K and T takes part: a full fourth column of K, a full fourth row of T.  The third row of K stays positive
        # and dominated by its z entry, so the projective divisor stays away from 0 (asserted below).
        Kd = torch.randn(B, 4, 4, generator=g)
        Kd[:, 0] *= 0.5 * W
        Kd[:, 1] *= 0.5 * H
        Kd[:, 2] = torch.tensor([0.05, 0.05, 0.8, 0.1]) + torch.tensor([0.25, 0.25, 0.4, 0.9]) * torch.rand(B, 4, generator=g)
        K = Kd
        T = T + 0.01 * torch.randn(B, 4, 4, generator=g)
    inp = {"points": points, "K": K, "T": T, "cot": torch.randn(B, H, W, 2, generator=g)}
    z = torch.matmul(torch.matmul(K.double(), T.double())[:, 2:3, :], points.double())
    assert float(z.min()) > 0.1, ("project3d", case, float(z.min()))
    return inp


def _eval_project3d(case, inp, dt):
    B, H, W, _ = case
    p, T = _leaf(inp["points"], dt), _leaf(inp["T"], dt)
    grid = R.project3d(p, inp["K"].to(dt), T, H, W)
    dp, dT = torch.autograd.grad((grid * inp["cot"].to(dt)).sum(), [p, T])
    return {"grid": grid.detach(), "dpoints": dp, "dT": dT}


# ---- grid_sample (bilinear, border) -------------------------------------------------------------------------------------------
def grid_unnormalised(grid, H, W, ac):
    """fp64 unnormalised (x, y) of F.grid_sample's coordinate map, before the clip."""
    g = grid.double()
    if ac:
        return (g[..., 0] + 1) / 2 * (W - 1), (g[..., 1] + 1) / 2 * (H - 1)
    return ((g[..., 0] + 1) * W - 1) / 2, ((g[..., 1] + 1) * H - 1) / 2


def grid_corner_mask(grid):
    m = torch.zeros(grid.shape[:3], dtype=torch.bool)
    m.view(grid.shape[0], -1)[0, :N_CORNERS] = True
    return m


def grid_clamped(grid, H, W, ac):
    """(B, Ho, Wo, 2) bool: components whose coordinate the border clip holds (x <= 0 or x >= size - 1): gradient exactly 0."""
    x, y = grid_unnormalised(grid, H, W, ac)
    return torch.stack([(x <= 0) | (x >= W - 1), (y <= 0) | (y >= H - 1)], -1)


def _offending(u, size):
    if size == 1:            # the output does not depend on this coordinate at all
        return torch.zeros_like(u, dtype=torch.bool)
    near = (u - torch.round(u)).abs() < KINK_MARGIN
    return near & (u > -KINK_MARGIN) & (u < size - 1 + KINK_MARGIN)


def _build_grid_sample(case, g):
    B, C, H, W, Ho, Wo, ac = case
    grid = (torch.rand(B, Ho, Wo, 2, generator=g).double() * 2.6 - 1.3).float().double()
    for k, size in ((0, W), (1, H)):          # nudge a coordinate that sits within 1e-3 of a kink by 2e-3
        if size == 1:
            continue
        u = grid_unnormalised(grid, H, W, ac)[k]
        per_unit = 2.0 / (size - 1) if ac else 2.0 / size
        grid[..., k] = torch.where(_offending(u, size), grid[..., k] + KINK_NUDGE * per_unit, grid[..., k])
    grid = grid.float()
    corners = torch.tensor([[-1.0, -1.0], [1.0, -1.0], [-1.0, 1.0], [1.0, 1.0]])
    grid.view(B, -1, 2)[0, :N_CORNERS] = corners
    inp = {"img": torch.rand(B, C, H, W, generator=g), "grid": grid, "cot": torch.rand(B, C, Ho, Wo, generator=g)}
    free = ~grid_corner_mask(grid)
    for k, size in ((0, W), (1, H)):
        u = grid_unnormalised(grid, H, W, ac)[k]
        assert not bool(_offending(u, size)[free].any()), ("grid_sample", case, k)
    if min(H, W) > 2:                          # the clip is exercised, and so is the interior
        c = grid_clamped(grid, H, W, ac)[free]
        assert 0.05 < float(c.float().mean()) < 0.5, ("grid_sample", case, float(c.float().mean()))
    return inp


def _eval_grid_sample(case, inp, dt):
    ac = case[6]
    grid = _leaf(inp["grid"], dt)
    out = F.grid_sample(inp["img"].to(dt), grid, mode="bilinear", padding_mode="border", align_corners=ac)
    (dg,) = torch.autograd.grad((out * inp["cot"].to(dt)).sum(), [grid])
    # the samples placed exactly on the corners are compared in the forward only (the device must give them a zero gradient)
    return {"out": out.detach(), "dgrid": dg * (~grid_corner_mask(grid)).unsqueeze(-1).to(dt)}


# ---- interpolate_bilinear / upsample / disp_to_depth --------------------------------------------------------------------------
def _build_interp(case, g):
    B, C, h, w, Ho, Wo = case
    return {"x": torch.rand(B, C, h, w, generator=g), "cot": torch.rand(B, C, Ho, Wo, generator=g)}


def _eval_interp(case, inp, dt):
    x = _leaf(inp["x"], dt)
    out = F.interpolate(x, size=[case[4], case[5]], mode="bilinear", align_corners=False)
    (dx,) = torch.autograd.grad((out * inp["cot"].to(dt)).sum(), [x])
    return {"out": out.detach(), "dx": dx}


def _build_nearest2x(case, g):
    B, C, h, w = case
    return {"x": torch.rand(B, C, h, w, generator=g), "cot": torch.rand(B, C, 2 * h, 2 * w, generator=g)}


def _eval_nearest2x(case, inp, dt):
    x = _leaf(inp["x"], dt)
    out = F.interpolate(x, scale_factor=2, mode="nearest")
    (dx,) = torch.autograd.grad((out * inp["cot"].to(dt)).sum(), [x])      # = the 2x2 block sum of the cotangent
    return {"out": out.detach(), "dx": dx}


def _build_disp_to_depth(case, g):
    (n,) = case
    return {"disp": torch.rand(1, 1, 1, n, generator=g), "cot_scaled": torch.randn(1, 1, 1, n, generator=g),
            "cot_depth": torch.randn(1, 1, 1, n, generator=g)}


def _eval_disp_to_depth(case, inp, dt):
    d = _leaf(inp["disp"], dt)
    scaled, depth = R.disp_to_depth(d, MIN_DEPTH, MAX_DEPTH)
    ls, ld = (scaled * inp["cot_scaled"].to(dt)).sum(), (depth * inp["cot_depth"].to(dt)).sum()
    grads = [torch.autograd.grad(l, [d], retain_graph=True)[0] for l in (ls + ld, ls, ld)]
    return {"scaled": scaled.detach(), "depth": depth.detach(), "dd_both": grads[0], "dd_scaled": grads[1], "dd_depth": grads[2]}


_BUILD = {"ssim": _build_ssim, "smooth": _build_smooth, "backproject": _build_backproject, "project3d": _build_project3d,
          "grid_sample": _build_grid_sample, "interp": _build_interp, "nearest2x": _build_nearest2x,
          "disp_to_depth": _build_disp_to_depth}
_EVAL = {"ssim": _eval_ssim, "smooth": _eval_smooth, "backproject": _eval_backproject, "project3d": _eval_project3d,
         "grid_sample": _eval_grid_sample, "interp": _eval_interp, "nearest2x": _eval_nearest2x,
         "disp_to_depth": _eval_disp_to_depth}
OPS = tuple(CASES)


def build(op, case):
    return _BUILD[op](tuple(case), _gen(op, case))


def evaluate(op, case, inputs, dtype):
    return _EVAL[op](tuple(case), inputs, dtype)


@functools.lru_cache(maxsize=None)
def reference(op, case):
    """(inputs, fp64 statement, fp32 statement) of one case; shared and read-only."""
    inputs = build(op, case)
    return inputs, evaluate(op, case, inputs, torch.float64), evaluate(op, case, inputs, torch.float32)


def params(op):
    import pytest
    return [pytest.param(c, id=case_id(c)) for c in CASES[op]]


# ---- the gate -----------------------------------------------------------------------------------------------------------------
def rel_err(a, ref64):
    """max|a - f64| / max|f64| (the plain max|a - f64| for a reference that is identically 0)."""
    ref64 = ref64.double()
    err, den = float((a.detach().cpu().double() - ref64).abs().max()), float(ref64.abs().max())
    return err / den if den > 0 else err


def gate_bound(e_32, factor=4.0):
    """e_hip <= 4 e_32 + 4 * 2^-23: four times the error of torch's own fp32 evaluation of the statement, plus four units of fp32
    roundoff for the statements that fp32 evaluates exactly."""
    return factor * e_32 + 4.0 * EPS32
