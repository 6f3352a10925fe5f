"""The pointwise photometric tests' side of the bargain, checked without a GPU: for every case of tests/photo_cases.py the
REFERENCE ALONE satisfies the conditions tests/test_photo_shapes_gpu.py relies on -- no cell, clamp or sign decision within
reach of an fp32 rounding error, every claimed seam present in the launches' own plan and covered by every kind of pixel --
and the imposed oracle (oracle/photo_kinks.py) is the plain one when it replays its own decisions.  Also: the gate of the GPU
test catches a seam-column error stated on the reference side."""
import ctypes

import pytest
import torch

from oracle import ref_cpu as R
from oracle import photo_kinks as PK
import photo_cases as PC
from helpers import oracle_photo


def _own(name, mode):
    return PC.oracle(name, mode, torch.float64), PC.oracle(name, mode, torch.float32)


@pytest.mark.parametrize("name,mode", PC.CASE_MODES)
def test_reference_takes_no_decision_within_rounding(name, mode):
    case, opt = PC.case_for(name, mode), PC.opt_for(name, mode)
    b, h, w = case.shape
    tgt = case.inputs[("color", 0, 0)].double()
    for s in range(case.ns):
        xy, cols = PC.coords(case.inputs, case.disps[s].double(), case.Ts, opt, torch.float64)
        assert not PC.fragile_map(xy, cols, tgt, h, w, case.delta[s]).any(), (name, s)
        assert 1e-6 < case.e_c[s] < 1e-3, case.e_c           # (the calibration itself: fp32 coordinates are good to 1e-5..1e-4 pixel)
    e64, e32 = _own(name, mode)
    assert e64.qz_min > PC.MIN_QZ, e64.qz_min                # no point behind the camera, no division blows up
    for k in e64.rec.cell:
        assert torch.equal(e64.rec.cell[k], e32.rec.cell[k]) and torch.equal(e64.rec.inside[k], e32.rec.inside[k]), k
    for k, v in e64.ssim_pre.items():
        assert 1e-4 < float(v.min()) and float(v.max()) < 1 - 1e-4, (k, float(v.min()), float(v.max()))
    assert bool(e64.ssim_pre) == (mode != "nossim")
    for s in range(case.ns):
        assert float(e64.nd_dx[s].abs().min()) >= 1e-6 and float(e64.nd_dy[s].abs().min()) >= 1e-6, s
        for j in range(2):                                   # the third fragility condition, on the evaluation the GPU test uses
            moves = e64.rec.inside[(s, j, 0)] | e64.rec.inside[(s, j, 1)]
            assert float(e64.t_minus_w[(s, j)].abs().min(1)[0][moves].min()) >= PC.L1_MARGIN if moves.any() else True


@pytest.mark.parametrize("name,mode", PC.CASE_MODES)
def test_every_claimed_seam_sees_every_kind_of_pixel(name, mode):
    """On the columns on both sides of every strip seam and the rows on both sides of every row-block seam (as the plan query
    places them): every argmin value is taken, and samples inside and outside the source image both occur.  `far_out` claims
    the opposite for one frame instead: every sample of frame +1 of batch element 1 is outside on both axes."""
    case = PC.case_for(name, mode)
    e64, _ = _own(name, mode)
    b, h, w = case.shape
    cols, rows = PC.seam_columns(name, mode)
    assert cols and rows and max(cols) < w and max(rows) < h
    if "all_outside" in case.spec:
        bi, j = case.spec["all_outside"]
        for s in range(case.ns):
            assert not e64.rec.inside[(s, j, 0)][bi].any() and not e64.rec.inside[(s, j, 1)][bi].any()
            col = e64.color[(s, j)][bi]
            assert float((col - col[:, :1, :1]).abs().max()) == 0.0         # one constant colour
            share = 1 - torch.stack([e64.rec.inside[(s, f, 0)] & e64.rec.inside[(s, f, 1)] for f in range(2)]).float().mean()
            assert 0.8 < float(share) < 0.97, float(share)
    if case.spec.get("coverage", True):
        ncand = e64.combined[0].shape[1]
        for s in range(case.ns):
            am = e64.rec.argmin[s]
            ins = torch.stack([e64.rec.inside[(s, j, 0)] & e64.rec.inside[(s, j, 1)] for j in range(2)])      # (2,B,H,W)
            for what, sel in [("column %d" % x, (slice(None), slice(None), x)) for x in cols] + \
                             [("row %d" % y, (slice(None), y, slice(None))) for y in rows]:
                got = set(am[sel].flatten().tolist())
                assert got == set(range(ncand)), (name, mode, s, what, got)
                v = ins[(slice(None),) + sel]
                assert v.any() and not v.all(), (name, mode, s, what)


@pytest.mark.parametrize("name,mode", PC.CASE_MODES)
def test_plan_query_agrees_with_the_case_table(name, mode):
    spec = PC.CASES[name]
    b, h, w = spec["shape"]
    p = PC.plan_query(name, mode)
    want = spec["plan"]
    assert (p.strip_f, p.strip_g, p.strip_p, p.rows_id, p.sm_chunk) == (62, 60, 64, 8, 2048)
    for key, width, n in (("f", p.strip_f, p.strips_f), ("g", p.strip_g, p.strips_g), ("p", p.strip_p, p.strips_p)):
        assert [n, w - (n - 1) * width] == want[key], (key, n)
        assert 0 < w - (n - 1) * width <= width
    for key, r, n in (("rows_f", p.rows_f, p.rowblocks_f), ("rows_g", p.rows_g, p.rowblocks_g), ("rows_p", p.rows_p, p.rowblocks_p),
                      ("rows_id", p.rows_id, p.rowblocks_id)):
        assert [r, n, h - (n - 1) * r] == want[key], (key, r, n)
    for s in range(spec["ns"]):
        ws, hs = w >> s, h >> s
        assert (p.dg_tw[s], p.dg_th[s]) == (128 >> s, 8 if s == 0 else 32 >> s)
        assert [p.dg_tiles_x[s], ws - (p.dg_tiles_x[s] - 1) * p.dg_tw[s], p.dg_tiles_y[s], hs - (p.dg_tiles_y[s] - 1) * p.dg_th[s]] == want["dg"][s], s
    assert p.nchunk == want["chunks"] == -(-h * w // p.sm_chunk)
    if want["chunks"] > 1:
        assert p.sm_chunk % w != 0                           # the chunks break mid-row
    kw, full, grad = PC.MODES[mode]
    if full is not None:
        assert p.full == full
    elif not grad or set(kw) - {"align_corners"}:
        assert p.full == 0                                   # evaluation and the variants never go all the way


def test_plan_query_refusals():
    """DC_EINVAL exactly where the launches' geometry checks refuse (csrc/photo.hip: fill_args), and nothing is written then."""
    from depthcore import _lib
    L = _lib.lib()

    def q(B=2, H=64, W=96, ns=4, flags=0):
        d = _lib.PhotoDesc()
        d.B, d.H, d.W, d.num_scales, d.flags = B, H, W, ns, flags
        p = _lib.PhotoPlan()
        p.strip_f = -7
        rc = L.dc_photo_plan_query(ctypes.byref(d), ctypes.byref(p))
        assert rc == 0 or p.strip_f == -7
        return rc
    assert q() == 0
    assert q(B=0) == -1 and q(H=3) == -1 and q(W=3) == -1 and q(ns=0) == -1 and q(ns=5) == -1
    assert q(H=4, W=4, ns=1) == 0 and q(H=4, W=4, ns=2) == 0 and q(H=4, W=4, ns=3) == -1      # scale 2 would be 1 x 1
    assert q(H=64, W=100, ns=3) == 0 and q(H=64, W=100, ns=4) == -1                            # 100 is no multiple of 8
    assert q(H=33, W=61, ns=1) == 0 and q(H=33, W=62, ns=2) == -1
    assert q(flags=_lib.OPT_PHOTO_SPLIT | _lib.OPT_PHOTO_FULL) == -1
    assert q(flags=_lib.OPT_PRED_MASK) == -1 and q(flags=_lib.OPT_PRED_MASK | _lib.OPT_NO_AUTOMASK) == 0
    d = _lib.PhotoDesc()
    d.B, d.H, d.W, d.num_scales = 2, 64, 96, 4
    assert L.dc_photo_plan_query(ctypes.byref(d), None) == -1 and L.dc_photo_plan_query(None, ctypes.byref(_lib.PhotoPlan())) == -1
    # the process-wide mode decides when the desc pins none; the variants never go all the way
    prev = L.dc_set_photo_full(0)
    try:
        p = _lib.PhotoPlan()
        assert L.dc_photo_plan_query(ctypes.byref(d), ctypes.byref(p)) == 0 and p.full == 0
        L.dc_set_photo_full(1)
        assert L.dc_photo_plan_query(ctypes.byref(d), ctypes.byref(p)) == 0 and p.full == 1
        d.flags = _lib.OPT_NO_SSIM
        assert L.dc_photo_plan_query(ctypes.byref(d), ctypes.byref(p)) == 0 and p.full == 0
    finally:
        L.dc_set_photo_full(prev)


@pytest.mark.parametrize("name,mode", PC.CASE_MODES)
def test_replaying_its_own_decisions_is_the_plain_oracle_bit_for_bit(name, mode):
    case, opt = PC.case_for(name, mode), PC.opt_for(name, mode)
    noise = PC.noise_for(case, mode)
    own = PC.oracle(name, mode, torch.float32)
    rep = PC.oracle(name, mode, torch.float32, PC.Imposed(own.rec))
    if opt.predictive_mask:
        disps = [d.clone().requires_grad_() for d in case.disps]
        Ts = [t.clone().requires_grad_() for t in case.Ts]
        outputs = {("disp", s): disps[s] for s in range(case.ns)}
        outputs[("cam_T_cam", 0, -1)], outputs[("cam_T_cam", 0, 1)] = Ts
        outputs["predictive_mask"] = {("disp", s): case.masks[s] for s in range(case.ns)}
        R.generate_images_pred(case.inputs, outputs, opt)
        ol = R.compute_losses(case.inputs, outputs, opt, noise)
        g = torch.autograd.grad(ol["loss"], disps + Ts)
        ogd, ogT = g[:case.ns], g[case.ns:]
        oo = outputs
    else:
        ol, oo, ogd, ogT = oracle_photo(case.inputs, case.disps, case.Ts, opt, noise)
    for ev in (own, rep):
        for k in ol:
            assert torch.equal(ev.losses[k], ol[k].detach()), k
        for s in range(case.ns):
            assert torch.equal(ev.g_disp[s], ogd[s]), s
            assert torch.equal(ev.depth[s], oo[("depth", 0, s)].detach())
            for j, f in enumerate((-1, 1)):
                assert torch.equal(ev.sample[(s, j)], oo[("sample", f, s)].detach())
                assert torch.equal(ev.color[(s, j)], oo[("color", f, s)].detach())
        for f in range(2):
            assert torch.equal(ev.g_T[f], ogT[f]), f
    for s in rep.rec.argmin:
        assert torch.equal(rep.rec.argmin[s], own.rec.argmin[s])


def _calibration(name, mode):
    """e32 per gated tensor with the fp32 oracle standing in for the kernels: cells from fp64, argmin from fp32."""
    e64, e32 = _own(name, mode)
    dec = PC.Imposed(e64.rec.replace(argmin=e32.rec.argmin))
    case = PC.case_for(name, mode)
    t64 = PC.tensors_of(PC.oracle(name, mode, torch.float64, dec), case.ns)
    t32 = PC.tensors_of(PC.oracle(name, mode, torch.float32, dec), case.ns)
    t32r = PC.tensors_of(PC.oracle(name, mode, torch.float32, dec, PC.RECIP_SEED), case.ns)
    return dec, t64, t32, t32r


@pytest.mark.parametrize("name,mode", PC.CASE_MODES)
def test_calibration_is_at_rounding_level(name, mode):
    """Prints e32 (the fp32 imposed oracle's deviation from the fp64 one, max norm relative to the tensor's rms), plain and with
    reciprocal-multiply divisions, per tensor; both stay far below the size of a gradient element, or the gate of the GPU test
    (4 x e32 + floor) would let a seam error through."""
    dec, t64, t32, t32r = _calibration(name, mode)
    for k in t64:
        e, er = PC.relmax(t32[k], t64[k]), PC.relmax(t32r[k], t64[k])
        print("photo_pointwise e32 %-8s %-13s %-8s plain %.3e recip %.3e" % (name, mode, k, e, er))
        assert max(e, er) < (1e-2 if k.startswith("d ") else 1e-3), (k, e, er)
    if "all_outside" in PC.CASES[name]:
        bi, j = PC.CASES[name]["all_outside"]
        assert not t64["d T%+d" % (2 * j - 1)][bi].any()       # every sample clamped on both axes: exactly no pose gradient


def test_gate_catches_a_dropped_seam_column():
    """Sanity of the tests themselves: the fp32 imposed oracle of `seams`, made wrong on ONE seam column -- the loss terms of
    column 59 (the last one the first 60-column strip owns) are dropped at scale 0, what its neighbours 58..60 would get from a
    strip that loses one halo column -- misses the gate of the GPU test on d disp0 by more than a factor 10, at that column."""
    name, mode = "seams", "full"
    dec, t64, t32, t32r = _calibration(name, mode)
    case = PC.case_for(name, mode)
    b, h, w = case.shape
    wt = torch.ones(1, h, w)
    wt[:, :, 59] = 0
    bad = PK.photo_eval(case.inputs, case.disps, case.Ts, PC.opt_for(name, mode), case.noise, dtype=torch.float32,
                        decisions=dec.decisions, weight={0: wt})
    ref = t64["d disp0"]
    rms = float(ref.pow(2).mean().sqrt())
    gate = PC.FACTOR * max(PC.relmax(t32["d disp0"], ref), PC.relmax(t32r["d disp0"], ref)) + PC.FLOOR_GRAD
    assert PC.relmax(t32["d disp0"], ref) <= gate
    err = (bad.g_disp[0].double() - ref).abs() / rms
    worst = int(err.flatten().argmax())
    assert float(err.max()) > 10 * gate, (float(err.max()), gate)
    assert worst % w in (58, 59, 60)
    err[..., 57:62] = 0                                       # (the 3x3 windows spread it to the neighbours; nothing further away moves)
    assert float(err.max()) <= gate
    for s in (1, 2):
        assert PC.relmax(bad.g_disp[s], t64["d disp%d" % s]) <= gate


def test_multiplying_by_the_rounded_ninth_explains_the_loss_offset(monkeypatch):
    """Why e32 is the larger of two fp32 evaluations (tests/test_photo_shapes_gpu.py): an fp32 evaluation that forms the 3x3 box
    means as sum * fl(1/9) instead of sum / 9 -- as the kernels do -- is a legitimate rounding of the reference, yet its losses
    sit 0.5-5e-6 above fp64, all scales alike, several times the plain fp32 oracle's own deviation (the kernels' measured 1.5-2.9e-6
    miss 4 x that + floor); the reciprocal-multiply restatement covers it.  Every other tensor stays inside the plain gate."""
    name, mode = "variants", "noauto"
    dec, t64, t32, t32r = _calibration(name, mode)
    case = PC.case_for(name, mode)

    def box3_k9(xp, div):
        h, w = xp.shape[2] - 2, xp.shape[3] - 2
        acc = 0
        for dy in range(3):
            for dx in range(3):
                acc = acc + xp[:, :, dy:dy + h, dx:dx + w]
        return acc * torch.tensor(1.0 / 9.0, dtype=xp.dtype)
    monkeypatch.setattr(PK, "_box3", box3_k9)
    k9 = PC.tensors_of(PK.photo_eval(case.inputs, case.disps, case.Ts, PC.opt_for(name, mode), None, dtype=torch.float32,
                                     decisions=dec.decisions), case.ns)
    for k in t64:
        plain, recip = PC.relmax(t32[k], t64[k]), PC.relmax(t32r[k], t64[k])
        floor = PC.FLOOR_GRAD if k.startswith("d ") else PC.FLOOR_VALUE
        err = PC.relmax(k9[k], t64[k])
        print("photo_pointwise k9 %-8s err %.3e plain gate %.3e recip gate %.3e" % (k, err, PC.FACTOR * plain + floor, PC.FACTOR * recip + floor))
        assert err <= PC.FACTOR * max(plain, recip) + floor, k
        if k.startswith("loss"):
            assert float(k9[k]) > float(t64[k]) and 5e-7 < err < 5e-6 and err > 2 * plain, (k, err, plain)
        else:
            assert err <= PC.FACTOR * plain + floor, k
