"""The fused photometric kernels (csrc/photo.hip) held POINTWISE to the fp64 oracle at their strip, row-block, tile and border
edges (cases: tests/photo_cases.py; what the reference side guarantees: tests/test_photo_cases_cpu.py).

tests/test_photo_gpu.py compares statistically (outlier budgets, norms) because the loss is piecewise smooth.  Here both sides
evaluate the same smooth function instead: the inputs are conditioned so that no bilinear cell, border clamp or sign(t - w)
decision is within reach of an fp32 rounding error (verified on the kernels' own logged coordinates), and the argmin the
kernels recorded is imposed on the oracle (each disagreement with the oracle's own argmin must be a rounding-level tie).  Every
element of every output is then gated in the max norm, no outlier budget:

    err_hip <= 4 x e32 + floor

with e32 the deviation of the SAME imposed oracle evaluated in fp32 from its fp64 evaluation on that tensor (factor and floor
as oracle/kinks.py: uncalibrated_disagreements; floors 1e-5 of the rms for gradients, 1e-6 for losses, depth and colour; how
the fp32 evaluation rounds: see below).
A seam column is 1.7 % of the pixels and passes every statistical gate; here it fails alone (the CPU file shows it).
"""
import numpy as np
import pytest
import torch

from oracle import photo_kinks as PK
import photo_cases as PC

pytestmark = pytest.mark.gpu

# How e32 is taken: as the larger of the plain fp32 oracle's deviation from fp64 and that of its reciprocal-multiply
# restatement (oracle/photo_kinks.py: recip_seed; every a / b is a * (1/b) with the reciprocal off by one seeded ulp).  Both are
# statements of the reference in fp32; neither looks at a kernel.
# What was measured (MI355X, profiles/photo_pointwise_margins.txt): with the plain e32 every coordinate, depth, colour, argmin
# and gradient gate held (largest err / gate 0.86, d T+1 of far_out), and the LOSSES of every configuration with SSIM missed it by
# 1.05-2.2 x: err_hip 1.5-2.9e-6 relative, the same sign and size at every scale, against e32 = 1e-10..4e-7; without SSIM
# ("nossim") the kernels' losses equal the fp32 oracle's to the last digit printed.  The cause is arithmetic: the kernels form the
# 3x3 box means as sum * k9 with k9 = fl(1/9) (7.5e-9 above 1/9) where the oracle divides by 9, and E[x^2] - mu^2 amplifies that
# common relative offset by mu^2 / sigma ~ 100 in every pixel, with one sign.  Shown on the reference side alone: the fp32
# oracle with `acc * fl(1/9)` in place of `acc / 9` moves its own losses by +1.2..2.1e-6 (tests/test_photo_cases_cpu.py:
# test_multiplying_by_the_rounded_ninth_explains_the_loss_offset).  So, as for every arithmetic-only cause (v_rcp_f32, constants
# held as reciprocals, fma contraction), the calibration was widened on the reference side and for every tensor alike; the
# kernels were not changed.


def run_hip(name, mode):
    from depthcore import ops, _lib
    case = PC.case_for(name, mode)
    kw, full, grad = PC.MODES[mode]
    kw = {k: v for k, v in kw.items() if k != "predictive_mask"}
    dev = torch.device("cuda:0")
    ns = case.ns
    inputs, noise = case.inputs, PC.noise_for(case, mode)
    L = _lib.lib()
    prev = L.dc_set_photo_full(full) if full is not None else None
    try:
        cfg = ops.PhotoConfig(
            inputs[("color", 0, 0)].to(dev), inputs[("color", -1, 0)].to(dev), inputs[("color", 1, 0)].to(dev),
            [inputs[("color", 0, s)].to(dev) for s in range(ns)], inputs[("K", 0)].to(dev), inputs[("inv_K", 0)].to(dev),
            noise=None if noise is None else [n.to(dev) for n in noise], materialize=True, **kw)
        d = [x.to(dev).requires_grad_(grad) for x in case.disps]
        t = [x.to(dev).requires_grad_(grad) for x in case.Ts]
        masks = [m.to(dev) for m in case.masks] if PC.MODES[mode][0].get("predictive_mask") else None
        losses = ops.photometric_loss(cfg, t[0], t[1], d, pred_masks=masks)
        assert losses.requires_grad == grad
        grads = torch.autograd.grad(losses[ns], d + t) if grad else None
        torch.cuda.synchronize()
    finally:
        if prev is not None:
            L.dc_set_photo_full(prev)
    cpu = lambda x: x.detach().cpu()
    ex = cfg.extras
    out = dict(losses=cpu(losses).double(), argmin=[cpu(a) for a in ex["argmin"]], depth=[cpu(x) for x in ex["depth"]],
               sample=[[cpu(x) for x in p] for p in ex["sample"]], color=[[cpu(x) for x in p] for p in ex["color"]],
               idsel=None if ex["identity_selection"] is None else [cpu(x) for x in ex["identity_selection"]])
    if grad:
        out["g_disp"] = [cpu(g) for g in grads[:ns]]
        out["g_T"] = [cpu(g) for g in grads[ns:]]
    return out


def report(name, mode, what, err, e_plain, e_recip, floor):
    e = max(e_plain, e_recip)
    gate = PC.FACTOR * e + floor
    print("photo_pointwise hip %-8s %-13s %-10s e32 %.3e e32_recip %.3e err_hip %.3e err/e32 %.2f err/e32_recip %.2f err/gate %.3f" % (
        name, mode, what, e_plain, e_recip, err, err / max(e_plain, 1e-300), err / max(e_recip, 1e-300), err / gate))
    return gate


@pytest.mark.parametrize("name,mode", PC.CASE_MODES)
def test_pointwise_against_the_imposed_oracle(name, mode):
    case, opt = PC.case_for(name, mode), PC.opt_for(name, mode)
    b, h, w = case.shape
    ns = case.ns
    kw, full, grad = PC.MODES[mode]
    plan = PC.plan_query(name, mode)
    hip = run_hip(name, mode)
    own64 = PC.oracle(name, mode, torch.float64)
    ncand = own64.combined[0].shape[1]
    for s in range(ns):
        assert int(hip["argmin"][s].max()) < ncand
    dec = PC.Imposed(own64.rec.replace(argmin=hip["argmin"]))        # cells and inside flags from fp64, argmin from the kernels
    f64 = PC.oracle(name, mode, torch.float64, dec)
    f32 = PC.oracle(name, mode, torch.float32, dec)
    f32r = PC.oracle(name, mode, torch.float32, dec, PC.RECIP_SEED)
    failures = []

    def gate(what, err, e_plain, e_recip, floor, where=""):
        g = report(name, mode, what, err, e_plain, e_recip, floor)
        if not err <= g:
            failures.append("%s: err %.3e > gate %.3e (e32 %.3e, recip %.3e) %s" % (what, err, g, e_plain, e_recip, where))

    relerr = lambda a, ref: float(((a.double() - ref.double()).abs() / ref.double().abs()).max())
    for s in range(ns):
        # ---- coordinates: the kernels took the fp64 cells (and the projection is right, pointwise)
        for j in range(2):
            g = hip["sample"][s][j].double()
            ix = PK._unnormalize(g[..., 0], w, opt.align_corners)
            iy = PK._unnormalize(g[..., 1], h, opt.align_corners)
            x64, y64 = own64.ix[(s, j)], own64.iy[(s, j)]
            near = (x64 > -1) & (x64 < w) & (y64 > -1) & (y64 < h)
            if near.any():
                dev = max(float((ix - x64).abs()[near].max()), float((iy - y64).abs()[near].max()))
                print("photo_pointwise hip %-8s %-13s coords s%d f%+d |ix_hip - ix_64| max %.3e px, delta/2 %.3e, e_c %.3e" % (
                    name, mode, s, 2 * j - 1, dev, case.delta[s] / 2, case.e_c[s]))
                if not dev <= case.delta[s] / 2:
                    failures.append("coordinates scale %d frame %+d: %.3e px > delta/2 %.3e" % (s, 2 * j - 1, dev, case.delta[s] / 2))
            far = ~near          # far outside: the same side of the image (the clamp decision), whatever the magnitude
            assert torch.equal((ix <= 0)[far], (x64 <= 0)[far]) and torch.equal((ix >= w - 1)[far], (x64 >= w - 1)[far])
            assert torch.equal((iy <= 0)[far], (y64 <= 0)[far]) and torch.equal((iy >= h - 1)[far], (y64 >= h - 1)[far])
            c64 = f64.color[(s, j)]
            crms = float(c64.pow(2).mean().sqrt())
            absmax = lambda a, ref: float((a.double() - ref).abs().max()) / crms
            gate("color s%d f%+d" % (s, 2 * j - 1), absmax(hip["color"][s][j], c64), absmax(f32.color[(s, j)], c64),
                 absmax(f32r.color[(s, j)], c64), PC.FLOOR_VALUE)
        gate("depth s%d" % s, relerr(hip["depth"][s], f64.depth[s]), relerr(f32.depth[s], f64.depth[s]),
             relerr(f32r.depth[s], f64.depth[s]), PC.FLOOR_VALUE)
        # ---- argmin: recorded == logged, and every disagreement with the fp64 oracle's own choice is a tie
        am = hip["argmin"][s].long()
        if hip["idsel"] is not None:
            first_reproj = 1 if kw.get("avg_reprojection") else 2
            assert torch.equal(hip["idsel"][s], (am >= first_reproj).float())
        if ncand > 1:
            comb = own64.combined[s]
            diff = am != own64.rec.argmin[s]
            e_c32 = max(float((PC.oracle(name, mode, torch.float32).combined[s].double() - comb).abs().max()),
                        float((f32r.combined[s].double() - f64.combined[s]).abs().max()))
            gap = (comb.gather(1, am.unsqueeze(1)) - comb.gather(1, own64.rec.argmin[s].unsqueeze(1)))[:, 0].abs()
            worst = float(gap[diff].max()) if diff.any() else 0.0
            print("photo_pointwise hip %-8s %-13s argmin s%d: %d of %d differ from the fp64 oracle's, largest gap %.3e, allowed %.3e" % (
                name, mode, s, int(diff.sum()), diff.numel(), worst, PC.FACTOR * e_c32 + 1e-7))
            if not worst <= PC.FACTOR * e_c32 + 1e-7:
                failures.append("argmin scale %d: a disagreement with a gap of %.3e is no tie (allowed %.3e)" % (s, worst, PC.FACTOR * e_c32 + 1e-7))
    # ---- losses
    t64, t32, t32r = PC.tensors_of(f64, ns), PC.tensors_of(f32, ns), PC.tensors_of(f32r, ns)
    for i in range(ns + 1):
        k = "loss/%d" % i if i < ns else "loss"
        gate(k, PC.relmax(hip["losses"][i:i + 1], t64[k]), PC.relmax(t32[k], t64[k]), PC.relmax(t32r[k], t64[k]), PC.FLOOR_VALUE)
    # ---- gradients: every element
    if grad:
        got = {"d disp%d" % s: hip["g_disp"][s] for s in range(ns)}
        got.update({"d T%+d" % (2 * f - 1): hip["g_T"][f][:, :3, :] for f in range(2)})
        for k, a in got.items():
            ref = t64[k]
            rms = float(ref.pow(2).mean().sqrt())
            err = (a.double() - ref).abs() / rms
            idx = np.unravel_index(int(err.flatten().argmax()), tuple(err.shape))
            where = "worst at %s" % (idx,)
            if k.startswith("d disp"):
                s = int(k[-1])
                where = "worst at batch %d, %s" % (idx[0], PC.locate(plan, s, int(idx[2]), int(idx[3]), w >> s))
            gate(k, float(err.max()), PC.relmax(t32[k], ref), PC.relmax(t32r[k], ref), PC.FLOOR_GRAD, where)
        if "all_outside" in case.spec:
            bi, j = case.spec["all_outside"]
            k = "d T%+d" % (2 * j - 1)
            assert not t64[k][bi].any()
            rms = float(t64[k].pow(2).mean().sqrt())
            z = float(got[k][bi].abs().max()) / rms
            print("photo_pointwise hip %-8s %-13s %s of the all-outside batch element: %.3e of the rms (floor %.1e)" % (name, mode, k, z, PC.FLOOR_GRAD))
            if not z <= PC.FLOOR_GRAD:
                failures.append("%s of batch element %d, whose every sample is clamped: %.3e of the rms, not zero" % (k, bi, z))
    else:
        assert "g_disp" not in hip
    assert not failures, "\n".join(failures)
