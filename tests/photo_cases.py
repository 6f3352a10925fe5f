"""Case table and input conditioning of the pointwise photometric tests (tests/test_photo_cases_cpu.py: the reference alone
satisfies what the GPU test relies on; tests/test_photo_shapes_gpu.py: the HIP kernels against the imposed fp64 oracle).

The photometric loss is piecewise smooth (oracle/photo_kinks.py).  The argmin is recorded by the kernels and imposed on the
oracle; the bilinear cell, the border clamp and the sign of `t - w` are not recorded, so the inputs are CONDITIONED until
no decision of that kind is within reach of an fp32 rounding error: the disparities are nudged, in fp64 and deterministically,
until no full-resolution pixel is "fragile" (`fragile_map`).  What is left is one smooth function that an fp32 evaluation can
be held to pointwise.

Everything here runs on the CPU and is cached per process (`build`): a case is conditioned once however many tests use it.
"""
import ctypes
import functools

import torch
import torch.nn.functional as F

from oracle import ref_cpu as R
from oracle import photo_kinks as PK
from helpers import random_poses

# mode -> (PhotoConfig keywords, dc_set_photo_full mode or None, gradients)
MODES = {
    "full": ({}, 1, True),                # photo_fwdg_kernel<.., FULL> (60-column strips) + disp_grad_kernel
    "split": ({}, 0, True),               # photo_fwdg_kernel + photo_bwdg_kernel (64-column strips, its own row blocks) + disp_grad_kernel
    "eval": ({}, None, False),            # photo_fwd_kernel (62-column strips), no gradient
    "noauto": (dict(disable_automasking=True), None, True),        # the variants: photo_fwdg_kernel<.., -1> + the split backward
    "avg": (dict(avg_reprojection=True), None, True),
    "nossim": (dict(no_ssim=True), None, True),
    "pred_mask": (dict(disable_automasking=True, predictive_mask=True), None, True),
    "align_corners": (dict(align_corners=True), None, True),
}

# name: shape (B, H, W), scales, pose scale, seeds, modes, and the edges it is there for as the plan-query fields that make them
# (strips: [strips, columns the last one owns]; rows: [rows per block, blocks, rows the last one owns]; dg[s]: [tiles x, scale-s
# columns of the last, tiles y, scale-s rows of the last]; chunks: smooth_fwd_kernel blocks per scale-0 image).
CASES = {
    # 60/62/64-column strips with a ragged last one, row blocks 16+16+8 and 8x5, disp_grad seams at full-res x = 128 and y = 32 (y = 8 at
    # scale 0), smoothness chunks of 2048 pixels breaking mid-row (2048 = 15 rows of 136 + 8)
    "seams": dict(shape=(2, 40, 136), ns=3, pose=0.05, seed=5, modes=("full", "split"),
                  plan=dict(g=[3, 16], f=[3, 12], p=[3, 8], rows_g=[16, 3, 8], rows_f=[16, 3, 8], rows_p=[8, 5, 8], rows_id=[8, 5, 8],
                            dg={0: [2, 8, 5, 8], 1: [2, 4, 2, 4], 2: [2, 2, 2, 2]}, chunks=3)),
    # the last 60-strip owns ONE column, x = 60; the reflection fold-back column x = W-2 = 59 sits in the other strip; last row block is one row
    "one_col": dict(shape=(1, 33, 61), ns=1, pose=0.05, seed=20, modes=("full",),
                    plan=dict(g=[2, 1], f=[1, 61], p=[1, 61], rows_g=[16, 3, 1], rows_f=[16, 3, 1], rows_p=[8, 5, 1], rows_id=[8, 5, 1],
                              dg={0: [1, 61, 5, 1]}, chunks=1)),
    # the last 62-strip (evaluation forward, identity_kernel) owns one column; the last row block is 2 rows
    "w63": dict(shape=(1, 18, 63), ns=1, pose=0.05, seed=7, modes=("eval", "full"),
                plan=dict(g=[2, 3], f=[2, 1], p=[1, 63], rows_g=[16, 2, 2], rows_f=[16, 2, 2], rows_p=[8, 3, 2], rows_id=[8, 3, 2],
                          dg={0: [1, 63, 3, 2]}, chunks=1)),
    # the last 64-strip of photo_bwdg_kernel owns one column
    "w65": dict(shape=(1, 18, 65), ns=1, pose=0.05, seed=25, modes=("split",),
                plan=dict(g=[2, 5], f=[2, 3], p=[2, 1], rows_g=[16, 2, 2], rows_f=[16, 2, 2], rows_p=[8, 3, 2], rows_id=[8, 3, 2],
                          dg={0: [1, 65, 3, 2]}, chunks=1)),
    # scale 3: the second disp_grad tile owns one coarse column (17 = 16 + 1); row blocks exact, no ragged tail
    "four": dict(shape=(1, 64, 136), ns=4, pose=0.05, seed=22, modes=("full",),
                 plan=dict(g=[3, 16], f=[3, 12], p=[3, 8], rows_g=[16, 4, 16], rows_f=[16, 4, 16], rows_p=[8, 8, 8], rows_id=[8, 8, 8],
                           dg={0: [2, 8, 8, 8], 1: [2, 4, 2, 16], 2: [2, 2, 2, 8], 3: [2, 1, 2, 4]}, chunks=5)),
    # most samples outside the source image; in batch element 1 frame +1 is translated so that EVERY sample is: whole strips clamped,
    # that frame's warped image one constant colour, its pose gradient exactly zero
    "far_out": dict(shape=(2, 32, 64), ns=3, pose=0.2, seed=26, modes=("full", "split"), all_outside=(1, 1), coverage=False,
                    plan=dict(g=[2, 4], f=[2, 2], p=[1, 64], rows_g=[16, 2, 16], rows_f=[16, 2, 16], rows_p=[8, 4, 8], rows_id=[8, 4, 8],
                              dg={0: [1, 64, 4, 8], 1: [1, 32, 1, 16], 2: [1, 16, 1, 8]}, chunks=1)),
    # the generic forward (SPEC = -1) + the pointwise backward at a strip seam (60 | 12, 64 | 8) and a row-block seam (16 | 8);
    # align_corners=True (the other un-normalisation of the sampling grid)
    "variants": dict(shape=(2, 24, 72), ns=3, pose=0.05, seed=12, modes=("noauto", "avg", "nossim", "pred_mask", "align_corners"),
                     plan=dict(g=[2, 12], f=[2, 10], p=[2, 8], rows_g=[16, 2, 8], rows_f=[16, 2, 8], rows_p=[8, 3, 8], rows_id=[8, 3, 8],
                               dg={0: [1, 72, 3, 8], 1: [1, 36, 1, 12], 2: [1, 18, 1, 6]}, chunks=1)),
}
CASE_MODES = [(n, m) for n, c in CASES.items() for m in c["modes"]]

L1_MARGIN = 1e-4         # |t - w| of a warped pixel that can still move stays at least this far from its kink
DELTA_FACTOR = 8.0       # coordinates stay DELTA_FACTOR x the fp32 oracle's own coordinate error away from every integer
MIN_QZ = 1e-3


def opt_for(name, mode):
    b, h, w = CASES[name]["shape"]
    return R.Opt(height=h, width=w, scales=tuple(range(CASES[name]["ns"])), **MODES[mode][0])


def plan_query(name, mode):
    """dc_photo_plan_query for the desc the op builds for this case and mode (sizes and flags only; needs no GPU)."""
    from depthcore import _lib
    L = _lib.lib()
    kw, full, grad = MODES[mode]
    b, h, w = CASES[name]["shape"]
    d = _lib.PhotoDesc()
    d.B, d.H, d.W, d.num_scales = b, h, w, CASES[name]["ns"]
    d.flags = ((_lib.OPT_NO_AUTOMASK if kw.get("disable_automasking") else 0) | (_lib.OPT_AVG_REPROJ if kw.get("avg_reprojection") else 0)
               | (_lib.OPT_NO_SSIM if kw.get("no_ssim") else 0) | (_lib.OPT_ALIGN_CORNERS if kw.get("align_corners") else 0)
               | (_lib.OPT_PRED_MASK if kw.get("predictive_mask") else 0) | (0 if grad else _lib.OPT_NO_GRAD)
               | ({None: 0, 0: _lib.OPT_PHOTO_SPLIT, 1: _lib.OPT_PHOTO_FULL}[full]))
    p = _lib.PhotoPlan()
    rc = L.dc_photo_plan_query(ctypes.byref(d), ctypes.byref(p))
    assert rc == 0, rc
    return p


def locate(plan, s, y, x, ws):
    """Where element (y, x) of a scale-s gradient map falls in every decomposition of the launches (for failure messages)."""
    k = 1 << s
    fy, fx = y * k, x * k
    return ("scale-%d (y %d, x %d) = full-res (%d, %d): 60-strip %d col %d, 62-strip %d col %d, 64-strip %d col %d; row block fwdg %d row %d, "
            "bwdg %d row %d; disp_grad tile (%d, %d) at (%d, %d); smoothness chunk %d" % (
                s, y, x, fy, fx, fx // plan.strip_g, fx % plan.strip_g, fx // plan.strip_f, fx % plan.strip_f, fx // plan.strip_p,
                fx % plan.strip_p, fy // plan.rows_g, fy % plan.rows_g, fy // plan.rows_p, fy % plan.rows_p,
                y // plan.dg_th[s], x // plan.dg_tw[s], y % plan.dg_th[s], x % plan.dg_tw[s], (y * ws + x) // plan.sm_chunk))


# ---- coordinates and warps of one scale (fp64 or fp32), without the loss -----------------------------------------------------
def coords(inputs, disp_s, Ts, opt, dtype):
    """-> [(ix, iy)] per frame (pixel coordinates before the clamp), [warped image] per frame, min q_z."""
    H, W = opt.height, opt.width
    c = lambda t: t.to(dtype)
    disp = R.upsample_bilinear(c(disp_s), H, W)
    _, depth = R.disp_to_depth(disp, opt.min_depth, opt.max_depth)
    xy, cols = [], []
    cam = R.backproject(depth, c(inputs[("inv_K", 0)]))
    for j, f in enumerate((-1, 1)):
        grid = R.project3d(cam, c(inputs[("K", 0)]), c(Ts[j]), H, W)
        xy.append((PK._unnormalize(grid[..., 0], W, opt.align_corners), PK._unnormalize(grid[..., 1], H, opt.align_corners)))
        cols.append(R.grid_sample_border(c(inputs[("color", f, 0)]), grid, opt.align_corners))
    return xy, cols


def coord_error(inputs, disp_s, Ts, opt):
    """e_c: the fp32 oracle's largest coordinate deviation from fp64 over the samples within one pixel of the image."""
    H, W = opt.height, opt.width
    xy64, _ = coords(inputs, disp_s, Ts, opt, torch.float64)
    xy32, _ = coords(inputs, disp_s.float(), Ts, opt, torch.float32)
    e = 0.0
    for (x64, y64), (x32, y32) in zip(xy64, xy32):
        near = (x64 > -1) & (x64 < W) & (y64 > -1) & (y64 < H)
        if near.any():
            e = max(e, float((x64 - x32.double()).abs()[near].max()), float((y64 - y32.double()).abs()[near].max()))
    return e


def fragile_map(xy, cols, target, H, W, delta):
    """(B,H,W) bool: a pixel where an fp32 evaluation could take a cell, clamp or sign(t - w) decision other than fp64's."""
    m = torch.zeros_like(xy[0][0], dtype=torch.bool)
    for (x, y), col in zip(xy, cols):
        # within delta of an integer while within delta of the image (0 and size-1, the clamp's kinks, are such integers)
        fx = ((x - torch.round(x)).abs() < delta) & (x > -delta) & (x < W - 1 + delta)
        fy = ((y - torch.round(y)).abs() < delta) & (y > -delta) & (y < H - 1 + delta)
        moves = ((x > 0) & (x < W - 1)) | ((y > 0) & (y < H - 1))
        l1 = ((target - col).abs().min(1)[0] < L1_MARGIN) & moves
        m |= fx | fy | l1
    return m


def condition(inputs, disp_s, Ts, opt, s, delta, seed, max_rounds=1200):
    """Nudge scale-s disparities (fp64 holding fp32-representable values) until `fragile_map` is empty.  A coarse pixel that owns a
    fragile pixel gets a seeded step of 1e-3..3e-3; the step is kept only if it leaves fewer fragile pixels in the full-resolution footprint
    of that coarse pixel (the pixels its bilinear taps reach: 2^s x 2^s around it, half a coarse pixel further on each side), and is
    redrawn in a later round otherwise.  Coarse pixels are tried in four interleaved classes (even / odd row and column) whose
    footprints do not overlap, so every accepted step is judged on its own and the fragile set only shrinks."""
    H, W = opt.height, opt.width
    k = 1 << s
    tgt = inputs[("color", 0, 0)].double()
    gen = torch.Generator().manual_seed(seed)
    hh, ww = disp_s.shape[2], disp_s.shape[3]
    cy = torch.arange(hh).view(1, 1, hh, 1)
    cx = torch.arange(ww).view(1, 1, 1, ww)

    def frag(d):
        xy, cols = coords(inputs, d, Ts, opt, torch.float64)
        return fragile_map(xy, cols, tgt, H, W, delta)

    def footprint_count(mm):      # fragile pixels in each coarse pixel's footprint
        mm = mm.double().unsqueeze(1)
        return mm if k == 1 else F.avg_pool2d(F.pad(mm, (k // 2,) * 4), 2 * k, k) * (4 * k * k)

    m = frag(disp_s)
    history = [int(m.sum())]
    for rnd in range(max_rounds):
        if not m.any():
            break
        own = F.max_pool2d(m.double().unsqueeze(1), k) > 0                     # coarse pixels that own a fragile pixel
        cls = rnd % 4
        cand = own & ((cy % 2) == cls // 2) & ((cx % 2) == cls % 2)
        if not cand.any():
            continue
        step = torch.rand(disp_s.shape, generator=gen, dtype=torch.float64) * 2e-3 + 1e-3
        if rnd >= 40:       # the few still left sit where the small steps only trade one fragile pixel for another: up to 64 x larger ones
            step = step * 2.0 ** torch.randint(0, 7, disp_s.shape, generator=gen).double()
        nd = torch.where(cand, disp_s + step, disp_s)
        nd = torch.where(nd > 0.97, nd - 0.5, nd).float().double()
        keep = cand & (footprint_count(frag(nd)) < footprint_count(m))
        disp_s = torch.where(keep, nd, disp_s)
        m = frag(disp_s)
        history.append(int(m.sum()))
    assert not m.any(), "conditioning did not converge at scale %d: fragile pixels per round %s" % (s, history)
    return disp_s, history


class Case:
    pass


@functools.lru_cache(maxsize=None)
def build(name, align_corners=False):
    """The conditioned inputs of a case (shared by all its modes but align_corners, whose coordinates are other ones)."""
    spec = CASES[name]
    b, h, w = spec["shape"]
    ns = spec["ns"]
    opt = R.Opt(height=h, width=w, scales=tuple(range(ns)), align_corners=align_corners)
    c = Case()
    c.name, c.spec, c.shape, c.ns = name, spec, (b, h, w), ns
    c.inputs = R.synthetic_inputs(b, h, w, num_scales=ns, seed=spec["seed"])
    g = torch.Generator().manual_seed(spec["seed"] + 100)
    disps = [(0.05 + 0.9 * torch.rand(b, 1, h >> s, w >> s, generator=g)).double() for s in range(ns)]
    c.Ts = random_poses(b, spec["seed"] + 200, scale=spec["pose"])
    if "all_outside" in spec:
        bi, j = spec["all_outside"]
        c.Ts[j] = c.Ts[j].clone()
        c.Ts[j][bi, 0, 3] += 8.0            # >= 0.58 W x 8 / max depth (1.96) = 2.4 W pixels to the right, 7.8 H down
        c.Ts[j][bi, 1, 3] += 8.0
    c.noise = R.tiebreak_noise(b, h, w, num_scales=ns)
    gm = torch.Generator().manual_seed(spec["seed"] + 300)
    c.masks = [0.1 + 0.8 * torch.rand(b, 2, h, w, generator=gm) for _ in range(ns)]      # predictive masks, full resolution
    c.e_c, c.delta, c.rounds = [], [], []
    c.disps = []
    for s in range(ns):
        e = coord_error(c.inputs, disps[s], c.Ts, opt)
        d, hist = condition(c.inputs, disps[s], c.Ts, opt, s, DELTA_FACTOR * e, spec["seed"] + 400 + s)
        c.e_c.append(e)
        c.delta.append(DELTA_FACTOR * e)
        c.rounds.append(hist)
        assert torch.equal(d.float().double(), d)
        c.disps.append(d.float())
    return c


def case_for(name, mode):
    return build(name, bool(MODES[mode][0].get("align_corners")))


def noise_for(case, mode):
    kw = MODES[mode][0]
    if kw.get("disable_automasking"):
        return None
    if kw.get("avg_reprojection"):
        return [n[:, :1].contiguous() for n in case.noise]
    return case.noise


def oracle(name, mode, dtype, imposed=None, recip_seed=None):
    """photo_eval of a case (cached).  imposed: None (its own decisions), or the identity-hashed holder `Imposed(decisions)`.
    "full", "split" and "eval" are one loss configuration: one evaluation serves the three."""
    return _oracle(name, mode if MODES[mode][0] else "full", dtype, imposed, recip_seed)


@functools.lru_cache(maxsize=None)
def _oracle(name, mode, dtype, imposed, recip_seed):
    case = case_for(name, mode)
    opt = opt_for(name, mode)
    masks = case.masks if MODES[mode][0].get("predictive_mask") else None
    return PK.photo_eval(case.inputs, case.disps, case.Ts, opt, noise_for(case, mode), dtype=dtype,
                         decisions=None if imposed is None else imposed.decisions, pred_masks=masks, recip_seed=recip_seed)


class Imposed:
    """Identity-hashed holder so that imposed evaluations can sit in the lru_cache."""

    def __init__(self, decisions):
        self.decisions = decisions


RECIP_SEED = 4242
FACTOR, FLOOR_GRAD, FLOOR_VALUE = 4.0, 1e-5, 1e-6      # the gate: err <= FACTOR x e32 + floor (oracle/kinks.py: uncalibrated_disagreements)


def relmax(a, ref):
    """max |a - ref| relative to the rms of `ref`."""
    ref = ref.double()
    return float((a.double() - ref).abs().max()) / max(float(ref.pow(2).mean().sqrt()), 1e-300)


def tensors_of(ev, ns):
    """The gated tensors of one evaluation, by name: losses (without the predictive-mask weighting term, which the fused op leaves to
    the caller), d disp[s], d T[f][:, :3, :]."""
    out = {}
    for s in range(ns):
        out["loss/%d" % s] = (ev.losses["loss/%d" % s] - ev.bce[s]).reshape(1)
    out["loss"] = (ev.losses["loss"] - sum(ev.bce[s] for s in range(ns)) / ns).reshape(1)
    for s in range(ns):
        out["d disp%d" % s] = ev.g_disp[s]
    for f in range(2):
        out["d T%+d" % (2 * f - 1)] = ev.g_T[f][:, :3, :]
    return out


def seam_columns(name, mode):
    """Full-resolution columns on both sides of every strip seam of the kernels this mode runs, and rows on both sides of every row-block seam."""
    p = plan_query(name, mode)
    b, h, w = CASES[name]["shape"]
    grad = MODES[mode][2]
    strips = [(p.strip_f, p.strips_f)] + ([(p.strip_g, p.strips_g)] if grad else []) + ([(p.strip_p, p.strips_p)] if grad and not p.full else [])
    rows = [(p.rows_id, p.rowblocks_id)] + ([(p.rows_g, p.rowblocks_g)] if grad else [(p.rows_f, p.rowblocks_f)]) + \
        ([(p.rows_p, p.rowblocks_p)] if grad and not p.full else [])
    cols = sorted({x for wd, n in strips for kk in range(1, n) for x in (kk * wd - 1, kk * wd)})
    rws = sorted({y for r, n in rows for kk in range(1, n) for y in (kk * r - 1, kk * r)})
    return cols, rws
