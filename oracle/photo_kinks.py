"""Imposed kinks for the photometric loss (TEST INFRASTRUCTURE, see oracle/__init__.py; the same idea as oracle/kinks.py).

`generate_images_pred` + `compute_losses` (oracle/ref_cpu.py a14 / a15, reference trainer.py:465-622) are only piecewise
smooth in the disparities and poses.  The kinks:

  1. the bilinear cell `floor(ix)`, `floor(iy)` and the border clamp `0 < ix < W-1` of grid_sample (a9);
  2. the argmin over the candidates of `torch.min(combined, 1)` (a15);
  3. the sign of `t - w` in the L1 term, the SSIM `clamp(., 0, 1)` (a11, a12) and the sign of the neighbour differences of the
     smoothness term (a13).

`photo_eval` restates the two functions with the decisions of (1) and (2) imposable through a `PhotoDecisions`: an fp32 and
an fp64 evaluation that are given the same cells, inside flags and argmin evaluate the SAME smooth function, and every loss and
gradient can be held to a rounding-level bound with no outlier list.  The decisions of (3) are not imposed; the quantities they
are taken on are exposed (`t_minus_w`, `ssim_pre`, `nd_dx` / `nd_dy`) so that a test can assert they are far from their kinks.
With imposed cells the taps are the given `x0, y0` and the weights `wx1 = x - x0`: the same bilinear patch, extended past its
cell when the coordinate lies outside it (it does so by a rounding error only, or the decision was not a legitimate one).

Replaying the decisions an fp32 evaluation recorded reproduces `ref_cpu.generate_images_pred` + `compute_losses` bit for bit:
every expression below is the one of ref_cpu.py, in its order (tests/test_photo_cases_cpu.py asserts it).

`recip_seed`: a second way of rounding the same formulas -- every division `a / b` becomes `a * (r (1 +- 2^-23))` with
r = 1 / b and the sign drawn per element from a seeded generator: the arithmetic of a kernel that multiplies by hardware
reciprocals (1 ulp) instead of dividing.  It calibrates how far an fp32 evaluation may legitimately be from fp64.
"""
import torch

from . import ref_cpu as R


class PhotoDecisions:
    """cell[(s, j, a)]: long (B,H,W), floor of the clamped source coordinate of scale s, frame j (0: -1, 1: +1), axis a (0: x, 1: y);
    inside[(s, j, a)]: bool (B,H,W), `0 < coordinate < size - 1` before the clamp;  argmin[s]: long (B,H,W)."""

    def __init__(self):
        self.cell, self.inside, self.argmin = {}, {}, {}

    def replace(self, argmin=None):
        """A copy with the argmin maps taken from `argmin` ({s: tensor} or a list, any integer dtype)."""
        out = PhotoDecisions()
        out.cell, out.inside, out.argmin = dict(self.cell), dict(self.inside), dict(self.argmin)
        if argmin is not None:
            items = argmin.items() if isinstance(argmin, dict) else enumerate(argmin)
            for s, t in items:
                out.argmin[s] = t.detach().cpu().long()
        return out


class _Div:
    """`a / b`, or its reciprocal-multiply restatement perturbed by one seeded ulp (module docstring)."""

    def __init__(self, seed):
        self.gen = None if seed is None else torch.Generator().manual_seed(seed)

    def __call__(self, a, b):
        if self.gen is None:
            return a / b
        r = 1.0 / (b if torch.is_tensor(b) else torch.tensor(float(b), dtype=a.dtype))
        sign = torch.randint(0, 2, tuple(r.shape), generator=self.gen).to(r.dtype) * 2 - 1
        return a * (r * (1 + sign * 2.0 ** -23))


class PhotoEval:
    """What `photo_eval` returns.  losses: {"loss/s", "loss"} as ref_cpu.compute_losses; bce[s]: the predictive-mask weighting
    term that loss/s contains (0 without predictive_mask);  g_disp / g_T (/ g_mask): autograd of losses["loss"];  rec: the
    decisions this evaluation would take itself;  depth[s], sample[(s, j)] (the grid in [-1, 1]), color[(s, j)];
    ix / iy[(s, j)]: source pixel coordinates before the clamp;  combined[s]: (B,C,H,W) candidates of the min();
    t_minus_w[(s, j)] (B,3,H,W);  ssim_pre[(s, j)] (B,3,H,W): (1 - n/d)/2 before the clamp (absent under no_ssim);
    nd_dx / nd_dy[s]: neighbour differences of the mean-normalised disparity."""


def _unnormalize(g, size, align_corners):
    if align_corners:
        return (g + 1) / 2 * (size - 1)
    return ((g + 1) * size - 1) / 2


def _grid_sample(img, grid, align_corners, key, dec, rec, ev):
    """ref_cpu.grid_sample_border with imposable cells and inside flags."""
    B, C, H, W = img.shape
    Ho, Wo = grid.shape[1], grid.shape[2]
    s, j = key
    xs = []
    for a, size in ((0, W), (1, H)):
        x = _unnormalize(grid[..., a], size, align_corners)
        (ev.ix if a == 0 else ev.iy)[key] = x.detach()
        inside = (x > 0) & (x < size - 1)
        rec.inside[(s, j, a)] = inside
        if dec is not None:
            inside = dec.inside[(s, j, a)]
        xc = x.clamp(0, size - 1)
        x = torch.where(inside, x, xc.detach())
        x0 = torch.floor(x.detach())
        rec.cell[(s, j, a)] = x0.long()
        if dec is not None:
            x0 = dec.cell[(s, j, a)].to(x.dtype)
        xs.append((x, x0))
    (x, x0), (y, y0) = xs
    wx1 = x - x0
    wy1 = y - y0
    wx0 = 1 - wx1
    wy0 = 1 - wy1
    x0 = x0.long()
    y0 = y0.long()
    flat = img.reshape(B, C, H * W)

    def tap(yy, xx):
        ok = ((xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)).to(img.dtype)
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).reshape(B, 1, Ho * Wo)
        val = torch.gather(flat, 2, idx.expand(B, C, Ho * Wo)).reshape(B, C, Ho, Wo)
        return val * ok.unsqueeze(1)

    return (tap(y0, x0) * (wy0 * wx0).unsqueeze(1)
            + tap(y0, x0 + 1) * (wy0 * wx1).unsqueeze(1)
            + tap(y0 + 1, x0) * (wy1 * wx0).unsqueeze(1)
            + tap(y0 + 1, x0 + 1) * (wy1 * wx1).unsqueeze(1))


def _box3(xp, div):
    H, W = xp.shape[2] - 2, xp.shape[3] - 2
    acc = 0
    for dy in range(3):
        for dx in range(3):
            acc = acc + xp[:, :, dy:dy + H, dx:dx + W]
    return div(acc, 9.0)


def _ssim_pre(x, y, div):
    """ref_cpu.ssim without its final clamp."""
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    xp, yp = R._reflect_pad1(x), R._reflect_pad1(y)
    mu_x, mu_y = _box3(xp, div), _box3(yp, div)
    sig_x = _box3(xp * xp, div) - mu_x * mu_x
    sig_y = _box3(yp * yp, div) - mu_y * mu_y
    sig_xy = _box3(xp * yp, div) - mu_x * mu_y
    n = (2 * mu_x * mu_y + C1) * (2 * sig_xy + C2)
    d = (mu_x * mu_x + mu_y * mu_y + C1) * (sig_x + sig_y + C2)
    return (1 - div(n, d)) / 2


def _reprojection_loss(pred, target, no_ssim, div, ev=None, key=None):
    diff = target - pred
    if ev is not None:
        ev.t_minus_w[key] = diff.detach()
    l1 = diff.abs().mean(1, keepdim=True)
    if no_ssim:
        return l1
    pre = _ssim_pre(pred, target, div)
    if ev is not None:
        ev.ssim_pre[key] = pre.detach()
    return 0.85 * torch.clamp(pre, 0, 1).mean(1, keepdim=True) + 0.15 * l1


def photo_eval(inputs, disps, Ts, opt, noise, dtype=torch.float32, decisions=None, pred_masks=None, recip_seed=None, weight=None):
    """One evaluation of the photometric loss and its gradients on the CPU in `dtype`.

    inputs: ref_cpu.synthetic_inputs;  disps[s] (B,1,H>>s,W>>s);  Ts: (T_-1, T_+1), each (B,4,4);  noise[s]: the tie-break
    randn ((B,2,H,W), (B,1,H,W) under avg_reprojection; unused and may be None under disable_automasking);
    pred_masks[s] (B,2,h,w) under opt.predictive_mask (upsampled to (H,W) like the reference does when smaller);
    decisions: a PhotoDecisions to impose (cells, inside flags and argmin), None to take them as they fall;
    weight: {s: tensor broadcastable to (B,H,W)} multiplied into `to_optimise` before its mean -- NOT part of the loss: the tests use it
    to state a deliberately wrong evaluation (a column whose loss terms go missing) and show that their gates catch it."""
    assert not opt.v1_multiscale and opt.pose_model_type != "posecnn", "full-resolution warps with one pose per frame only"
    cast = lambda t: t.detach().cpu().to(dtype)
    div = _Div(recip_seed)
    inputs = {k: cast(v) for k, v in inputs.items()}
    disps = [cast(d).requires_grad_() for d in disps]
    Ts = [cast(t).requires_grad_() for t in Ts]
    masks = [cast(m).requires_grad_() for m in pred_masks] if opt.predictive_mask else []
    noise = None if noise is None else [cast(n) for n in noise]
    H, W = opt.height, opt.width
    ev = PhotoEval()
    ev.rec = rec = PhotoDecisions()
    ev.depth, ev.sample, ev.color, ev.ix, ev.iy = {}, {}, {}, {}, {}
    ev.combined, ev.t_minus_w, ev.ssim_pre, ev.nd_dx, ev.nd_dy, ev.bce = {}, {}, {}, {}, {}, {}
    losses = {}
    total = 0
    for s in opt.scales:
        # ---- a14 generate_images_pred
        disp = R.upsample_bilinear(disps[s], H, W)
        scaled = 1.0 / opt.max_depth + (1.0 / opt.min_depth - 1.0 / opt.max_depth) * disp
        depth = div(1.0, scaled)
        ev.depth[s] = depth.detach()
        target = inputs[("color", 0, 0)]
        warped = []
        for j, f in enumerate((-1, 1)):
            cam = R.backproject(depth, inputs[("inv_K", 0)])
            # a8 Project3D
            P = torch.matmul(inputs[("K", 0)], Ts[j])[:, :3, :]
            q = torch.matmul(P, cam)
            z = q[:, 2:3, :] + 1e-7
            u = div(div(q[:, 0:1, :], z), W - 1)
            v = div(div(q[:, 1:2, :], z), H - 1)
            uv = torch.cat([u, v], 1).reshape(-1, 2, H, W).permute(0, 2, 3, 1)
            grid = (uv - 0.5) * 2
            ev.sample[(s, j)] = grid.detach()
            ev.qz_min = min(getattr(ev, "qz_min", float("inf")), float(q[:, 2].detach().min()))
            w = _grid_sample(inputs[("color", f, 0)], grid, opt.align_corners, (s, j), decisions, rec, ev)
            ev.color[(s, j)] = w.detach()
            warped.append(w)
        # ---- a15 compute_losses
        reproj = torch.cat([_reprojection_loss(warped[j], target, opt.no_ssim, div, ev, (s, j)) for j in range(2)], 1)
        loss = 0
        ev.bce[s] = 0.0
        if not opt.disable_automasking:
            ident = torch.cat([_reprojection_loss(inputs[("color", f, 0)], target, opt.no_ssim, div) for f in (-1, 1)], 1)
            if opt.avg_reprojection:
                ident = ident.mean(1, keepdim=True)
        elif opt.predictive_mask:
            mask = R.upsample_bilinear(masks[s], H, W)
            reproj = reproj * mask
            bce = 0.2 * (-torch.clamp(torch.log(mask), min=-100.0)).mean()
            ev.bce[s] = bce.detach()
            loss = loss + bce
        if opt.avg_reprojection:
            reproj = reproj.mean(1, keepdim=True)
        if not opt.disable_automasking:
            ident = ident + noise[s] * 0.00001
            combined = torch.cat([ident, reproj], 1)
        else:
            combined = reproj
        ev.combined[s] = combined.detach()
        if combined.shape[1] == 1:
            to_opt = combined
        else:
            to_opt, idx = torch.min(combined, dim=1)
            rec.argmin[s] = idx
            if decisions is not None:
                to_opt = torch.gather(combined, 1, decisions.argmin[s].unsqueeze(1))[:, 0]
        if weight is not None and s in weight:
            to_opt = to_opt * weight[s].to(dtype)
        loss = loss + to_opt.mean()
        # a13 get_smooth_loss on the mean-normalised disparity
        mean_disp = disps[s].mean(2, True).mean(3, True)
        norm_disp = div(disps[s], mean_disp + 1e-7)
        img = inputs[("color", 0, s)]
        ddx = norm_disp[:, :, :, :-1] - norm_disp[:, :, :, 1:]
        ddy = norm_disp[:, :, :-1, :] - norm_disp[:, :, 1:, :]
        ev.nd_dx[s], ev.nd_dy[s] = ddx.detach(), ddy.detach()
        gx = (img[:, :, :, :-1] - img[:, :, :, 1:]).abs().mean(1, keepdim=True)
        gy = (img[:, :, :-1, :] - img[:, :, 1:, :]).abs().mean(1, keepdim=True)
        smooth = (ddx.abs() * torch.exp(-gx)).mean() + (ddy.abs() * torch.exp(-gy)).mean()
        loss = loss + opt.disparity_smoothness * smooth / (2 ** s)
        total = total + loss
        losses["loss/{}".format(s)] = loss
    losses["loss"] = total / len(opt.scales)
    grads = torch.autograd.grad(losses["loss"], disps + Ts + masks)
    ns = len(disps)
    ev.losses = {k: v.detach() for k, v in losses.items()}
    ev.g_disp, ev.g_T, ev.g_mask = list(grads[:ns]), list(grads[ns:ns + 2]), list(grads[ns + 2:])
    return ev
