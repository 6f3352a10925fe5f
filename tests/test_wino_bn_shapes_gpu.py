"""The BatchNorm-folded Winograd launches through the C ABI -- ONE dc_wino3x3_fwd_bn, dc_wino3x3_dgrad_bn or dc_wino3x3_wgrad_bn per
case, with a dc_bn_fold built by ctypes -- against the fp64 statement of tests/wino_bn_cases.py at the region, group and mask
edges of wino_ps_kernel and wino_wgrad_kernel.  The fitness of the cases and the refusals are the subject of
tests/test_wino_bn_cases_cpu.py; the case table with its reasons, the derivation of the gates and the measured figures are in
DESIGN.md, "The BatchNorm-folded Winograd launches at their region, group and mask edges".  Every test prints its figures
(`wino_bn_parity ...`: the error and the share of each bound that was used) before it asserts.

Gates
    tensor    max|hip - fp64| <= 2e-5 max|fp64| (y, gx, dW: the bound of tests/test_wino_gpu.py); every element finite; every
              element the statement masks is bitwise +0.0 in gx
    own       the partials against the launch's OWN output: per image (slots [b ppi, (b+1) ppi)) and per group (slots
              [g ppg, (g+1) ppg), the last group takes the tail), every channel: |sum of slots - fp64 sum over the launch's own
              tensor| <= (n + 2) 2^-24 sum|term| (the worst case of an fp32 sum of n terms); slots past 2 nsub are exactly 0.0; no NaN
    ref       the per-group sums against the statement's, with the tensor gate propagated (delta = 2e-5 max|fp64|):
              n delta for sum y and sum g'; delta (2 sum|y| + n delta) for sum y^2; delta sum|x - mean| for sum g' (x - mean)
Outputs and partial buffers sit between sentinel guards that must come back intact, and start as NaN."""
import ctypes

import pytest
import torch

import wino_bn_cases as WC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256                      # floats on either side of an output
SENTINEL = -7.0312e28
NAN = float("nan")


def _bits(t):
    return t.view(torch.int32)


class _Guarded:
    """`n` floats between two guard bands of sentinels; the body starts as NaN."""

    def __init__(self, n):
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
        self.body = self.buf[GUARD:GUARD + n]
        self.body.fill_(NAN)
        self.n = n

    def intact(self):
        want = int(_bits(torch.tensor([SENTINEL]))[0])
        return bool((_bits(self.buf[:GUARD]) == want).all()) and bool((_bits(self.buf[GUARD + self.n:]) == want).all())


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _launch(case, inp, fold_fields=True):
    """One launch of `case` on the fp32 inputs `inp`.  Returns {"out": CPU tensor, "part": CPU (M, nparts, 2) or None}; asserts
    the return code and the guards."""
    from depthcore import _lib
    from depthcore._lib import ptr
    L = _lib.lib()
    B, Ci, Co, H, W = case.B, case.Ci, case.Co, case.H, case.W
    d = {k: _dev(v) for k, v in inp.items()}
    st = _lib.stream(d["w"])
    fold = _lib.BnFold()
    fold.groups = case.groups
    part = None
    if case.kind == "wgrad":
        out = _Guarded(Co * Ci * 9)
        ws = _Guarded(L.dc_wino3x3_wgrad_workspace(B, Ci, Co, H, W) // 4)
        fold.in_scale, fold.in_shift = ptr(d["s"]), ptr(d["t"])
        rc = L.dc_wino3x3_wgrad_bn(ptr(d["x"]), ptr(d["gy"]), out.body.data_ptr(), ws.body.data_ptr(), B, Ci, Co, H, W, ctypes.byref(fold), st)
        shape = (Co, Ci, 3, 3)
    else:
        nparts, _ = WC.parts_query(case)
        ws = _Guarded(L.dc_wino3x3_workspace(B, Ci, Co, H, W) // 4 + 1)
        if case.kind == "fwd":
            out, shape = _Guarded(B * Co * H * W), (B, Co, H, W)
            if case.loader:
                fold.in_scale, fold.in_shift = ptr(d["s"]), ptr(d["t"])
            if case.stats:
                part = _Guarded(Co * nparts * 2)
                fold.stat_part = part.body.data_ptr()
            rc = L.dc_wino3x3_fwd_bn(ptr(d["x"]), ptr(d["w"]), out.body.data_ptr(), ws.body.data_ptr(), B, Ci, Co, H, W, ctypes.byref(fold), st)
        else:
            out, shape = _Guarded(B * Ci * H * W), (B, Ci, H, W)
            part = _Guarded(Ci * nparts * 2)
            fold.bn_x, fold.bn_mean, fold.bwd_part = ptr(d["bn_x"]), ptr(d["mean"]), part.body.data_ptr()
            if case.mode == 2:
                fold.in_scale, fold.in_shift = ptr(d["s"]), ptr(d["t"])
            else:
                # the decision can only come from the bits: no scale / shift in the fold.  The mask is dc_bn_apply's own.
                nbytes = L.dc_bn_mask_bytes(B, Ci, H * W)
                assert nbytes > 0
                mask = _Guarded(nbytes // 4)
                ybn = _Guarded(B * Ci * H * W)
                assert L.dc_bn_apply(ptr(d["bn_x"]), ptr(d["res"]), ptr(d["s"]), ptr(d["t"]), ybn.body.data_ptr(), mask.body.data_ptr(),
                                     B, Ci, H * W, 1, case.groups, st) == 0
                torch.cuda.synchronize()
                assert mask.intact() and ybn.intact()
                fold.bn_mask = mask.body.data_ptr()
            rc = L.dc_wino3x3_dgrad_bn(ptr(d["gy"]), ptr(d["w"]), out.body.data_ptr(), ptr(d["addend"]), ws.body.data_ptr(), B, Ci, Co, H, W,
                                       ctypes.byref(fold), st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert out.intact() and ws.intact() and (part is None or part.intact()), "a write outside the buffer"
    res = {"out": out.body.cpu().view(shape), "part": None}
    if part is not None:
        res["part"] = part.body.cpu().view(shape[1], -1, 2)
    return res


def _tensor_gate(case, got, ref64, keep=None):
    name = WC.TENSORS[case.kind]
    assert bool(torch.isfinite(got).all()), "%s has a non-finite element" % name
    err = WC.rel_err(got, ref64)
    if keep is not None:
        assert bool((_bits(got)[~keep] == 0).all()), "a masked element of gx is not +0.0"
    return err


def _slot_sums(part, lo, hi):
    return part[:, lo:hi].double().sum(1)            # (M, 2)


def _partials_gate(case, got, part, ref):
    """The `own` and `ref` gates.  Returns the largest share of each bound that was used: (own image, own group, ref sum, ref second)."""
    m = WC.mech(case)
    p, B, groups, npg, HW = m["plan"], case.B, case.groups, m["npg"], case.H * case.W
    nparts, ppg = part.shape[1], m["ppg"]
    ppi = ppg // npg
    assert (nparts, ppg) == WC.parts_query(case) and ppi == 2 * p.per_img
    assert not bool(torch.isnan(part).any()), "a partial slot was not written"
    assert bool((_bits(part[:, 2 * p.nsub:].contiguous()) == 0).all()), "a trailing slot is not +0.0"
    o = got.double()
    if case.kind == "fwd":
        t0, t1 = o, o * o
        names = ("S", "Q")
    else:
        gi = torch.arange(B) // npg
        xm = ref["inp"]["bn_x"].double() - ref["inp"]["mean"].double()[gi][:, :, None, None]
        t0, t1 = o, o * xm
        names = ("P0", "P1")
    img = [(t.sum((2, 3)), t.abs().sum((2, 3))) for t in (t0, t1)]          # (B, M) sums and sums of magnitudes
    share = [0.0, 0.0, 0.0, 0.0]
    for b in range(B):
        s = _slot_sums(part, b * ppi, (b + 1) * ppi)
        for q in range(2):
            bound = WC.sum_bound(HW, img[q][1][b])
            diff = (s[:, q] - img[q][0][b]).abs()
            share[0] = max(share[0], float((diff / bound.clamp_min(1e-300)).max()))
            assert bool((diff <= bound).all()), ("image", b, names[q], float(diff.max()), float(bound.min()))
    r64 = ref["r64"]
    delta = WC.TENSOR_TOL * float(r64[WC.TENSORS[case.kind]].abs().max())
    n = npg * HW
    for g in range(groups):
        lo, hi = g * ppg, (nparts if g == groups - 1 else (g + 1) * ppg)
        s = _slot_sums(part, lo, hi)
        rows = slice(g * npg, (g + 1) * npg)
        for q in range(2):
            own, mag = img[q][0][rows].sum(0), img[q][1][rows].sum(0)
            bound = WC.sum_bound(n, mag)
            diff = (s[:, q] - own).abs()
            share[1] = max(share[1], float((diff / bound.clamp_min(1e-300)).max()))
            assert bool((diff <= bound).all()), ("group", g, names[q], float(diff.max()))
        # against the statement, the tensor gate propagated
        if case.kind == "fwd":
            yabs = r64["y"].abs()[rows].sum((0, 2, 3))
            b0, b1 = WC.stat_bounds(n, delta, yabs)
            b0 = torch.full_like(yabs, b0)
        else:
            b0 = torch.full((s.shape[0],), n * delta, dtype=torch.float64)
            b1 = delta * xm.abs()[rows].sum((0, 2, 3))
        for q, bound in ((0, b0), (1, b1)):
            diff = (s[:, q] - r64[names[q]][g]).abs()
            share[2 + q] = max(share[2 + q], float((diff / bound.clamp_min(1e-300)).max()))
            assert bool((diff <= bound).all()), ("statement", g, names[q], float(diff.max()), float(bound.min()))
    return share


def _check(case):
    inp, r64, r32 = WC.reference(case)
    name = WC.TENSORS[case.kind]
    res = _launch(case, inp)
    e32 = WC.rel_err(r32[name], r64[name])
    err = _tensor_gate(case, res["out"], r64[name], r64.get("keep"))
    line = "wino_bn_parity %-44s %s rel_err %.2e (%.0f%% of %.0e; torch fp32 %.1e)" % (
        WC.case_id(case), name, err, 100 * err / WC.TENSOR_TOL, WC.TENSOR_TOL, e32)
    share = None
    if res["part"] is not None and err <= WC.TENSOR_TOL:
        print(line, end="")
        share = _partials_gate(case, res["out"], res["part"], {"inp": inp, "r64": r64})
        line = "  partials: own image %.0f%% group %.0f%%, statement sum %.1f%% second %.1f%%" % tuple(100 * v for v in share)
    print(line)
    assert err <= WC.TENSOR_TOL, (name, err)
    return res


@pytest.mark.parametrize("case", WC.params(WC.FWD))
def test_forward(case):
    _check(case)


@pytest.mark.parametrize("case", WC.params(WC.DGRAD))
def test_data_gradient(case):
    _check(case)


@pytest.mark.parametrize("case", WC.params(WC.WGRAD))
def test_weight_gradient(case):
    _check(case)


@pytest.mark.parametrize("kind", ["fwd", "dgrad", "wgrad"])
def test_two_launches_are_bitwise_equal(kind):
    case = WC.DETERMINISM[kind]
    inp = WC.reference(case)[0]
    a, b = _launch(case, inp), _launch(case, inp)
    assert torch.equal(_bits(a["out"]), _bits(b["out"]))
    if kind != "wgrad":
        assert torch.equal(_bits(a["part"]), _bits(b["part"]))


@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
def test_batch_decomposition(kind):
    """groups = 1: the arithmetic per output does not depend on B -- image b of the batched launch and its slot range
    [b ppi, (b+1) ppi) are bitwise the B = 1 launch on image b alone."""
    case = WC.BATCH_SPLIT[kind]
    inp = WC.reference(case)[0]
    full = _launch(case, inp)
    ppi = 2 * WC.mech(case)["plan"].per_img
    one = case._replace(B=1)
    assert WC.parts_query(one)[0] == ppi
    for b in range(case.B):
        sub = {k: (v[b:b + 1] if v is not None and k in ("x", "gy", "bn_x", "res", "addend") else v) for k, v in inp.items()}
        r = _launch(one, sub)
        assert torch.equal(_bits(r["out"][0]), _bits(full["out"][b])), b
        assert torch.equal(_bits(r["part"]), _bits(full["part"][:, b * ppi:(b + 1) * ppi].contiguous())), b


def test_wgrad_bn_without_a_fold_is_the_plain_weight_gradient():
    """dc_wino3x3_wgrad_bn with bn == NULL, or with a fold whose in_scale is NULL, is dc_wino3x3_wgrad, bitwise."""
    from depthcore import _lib
    from depthcore._lib import ptr
    L = _lib.lib()
    case = WC.PLAIN_WGRAD
    inp, r64, _ = WC.reference(case)
    B, Ci, Co, H, W = case.B, case.Ci, case.Co, case.H, case.W
    x, gy = _dev(inp["x"]), _dev(inp["gy"])
    st = _lib.stream(x)
    empty = _lib.BnFold()
    empty.groups = case.groups
    outs = []
    for how in ("plain", "null", "no_scale"):
        out = _Guarded(Co * Ci * 9)
        ws = _Guarded(L.dc_wino3x3_wgrad_workspace(B, Ci, Co, H, W) // 4)
        if how == "plain":
            rc = L.dc_wino3x3_wgrad(ptr(x), ptr(gy), out.body.data_ptr(), ws.body.data_ptr(), B, Ci, Co, H, W, st)
        else:
            rc = L.dc_wino3x3_wgrad_bn(ptr(x), ptr(gy), out.body.data_ptr(), ws.body.data_ptr(), B, Ci, Co, H, W,
                                       None if how == "null" else ctypes.byref(empty), st)
        assert rc == 0
        torch.cuda.synchronize()
        assert out.intact() and ws.intact()
        outs.append(out.body.cpu())
    assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(outs[2]))
    # and it is the weight gradient of the RAW input, not of the folded one
    ref = torch.nn.grad.conv2d_weight(inp["x"].double(), (Co, Ci, 3, 3), inp["gy"].double(), padding=1)
    assert WC.rel_err(outs[0].view(Co, Ci, 3, 3), ref) <= WC.TENSOR_TOL
    assert WC.rel_err(outs[0].view(Co, Ci, 3, 3), r64["dW"]) > 100 * WC.TENSOR_TOL
