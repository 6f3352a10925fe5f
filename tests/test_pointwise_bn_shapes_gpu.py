"""The BatchNorm-folded 1x1 GEMM launches through the C ABI -- ONE launch per case with a dc_bn_fold built by ctypes: the fp32-MFMA
family through the pinned dc_conv1x1_fwd_bn / _dgrad_bn / _wgrad_bn, the split-bf16 family through dc_pointwise_* under
dc_set_gemm_split(1) -- against the fp64 statement of tests/pointwise_bn_cases.py at the tile, group and mask edges of both families.
The fitness of the cases is the subject of tests/test_pointwise_bn_cases_cpu.py; the case table with its reasons, the derivation of
the gates and the measured figures are in DESIGN.md, "The BatchNorm-folded 1x1 GEMMs at their tile, group and mask edges".  Every
test prints its figures (`pointwise_bn_parity ...`: the error and the share of each bound that was used) before it asserts.

Gates
    tensor    max|hip - fp64| <= 5e-6 max|fp64| (y, gx, dW: the bound of tests/test_conv1x1_gpu.py); every element finite; every
              element the statement masks is bitwise +0.0 in gx
    own       the partials against the launch's OWN output.  Slot s holds the flattened pixels [s cover, (s + 1) cover) that exist
              (cover = 16 NT): per slot, per image (where P is a multiple of cover: slots [b P / cover, (b + 1) P / cover)) and per
              group (slots [g ppg, (g + 1) ppg), the last group takes the tail), every channel: |sum of slots - fp64 sum over the
              launch's own tensor| <= (n + 2) 2^-24 sum|term| (the worst case of an fp32 sum of n terms); the slots of wave columns
              wholly outside N are exactly 0.0; no NaN
    ref       the per-group sums against the statement's, with the tensor gate propagated (delta = 5e-6 max|fp64|):
              n delta for sum y and sum g'; delta (2 sum|y| + n delta) for sum y^2; delta sum|x - mean| for sum g' (x - mean)
Outputs, partial buffers and workspaces sit between sentinel guards that must come back intact, and start as NaN."""
import ctypes

import pytest
import torch

import pointwise_bn_cases as PC
from test_wino_bn_shapes_gpu import _Guarded, _bits, _dev, _tensor_gate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _split_mode_restored():
    lib = PC.host_lib()
    prev = lib.dc_get_gemm_split()
    try:
        yield
    finally:
        lib.dc_set_gemm_split(prev)


def _ws(nbytes):
    return _Guarded((int(nbytes) + 3) // 4 + 4)


def _launch(case, inp, fold="case", want=0, nparts=None):
    """One launch of `case` on the fp32 inputs `inp`.  fold: "case" (what the case asks for), "null" (bn == NULL), "empty" (a fold
    with every pointer NULL).  Asserts the return code `want` and the guards.  Returns {"out": CPU tensor, "part": CPU (M, nparts, 2)
    or None}; after a refusal, additionally that nothing between the guards was written."""
    from depthcore import _lib
    from depthcore._lib import ptr
    L = _lib.lib()
    B, Ci, Co, H, W = a = case[2:7]
    x3 = case.family == "x3"
    if x3:
        L.dc_set_gemm_split(1)
    d = {k: _dev(v) for k, v in inp.items()}
    d["w"] = d["w"].view(Co, Ci)
    st = _lib.stream(d["w"])
    f = _lib.BnFold()
    f.groups = case.groups
    fp = None if fold == "null" else ctypes.byref(f)
    on = fold == "case"
    part, bufs = None, []
    if case.kind == "wgrad":
        out, shape = _Guarded(Co * Ci), (Co, Ci, 1, 1)
        if on:
            f.in_scale, f.in_shift = ptr(d["s"]), ptr(d["t"])
        if x3:
            ws = _ws(L.dc_pointwise_workspace(_lib.PASS_WGRAD, fp, *a, 1))
            rc = L.dc_pointwise_wgrad(ptr(d["x"]), ptr(d["gy"]), out.body.data_ptr(), ws.body.data_ptr(), *a, 1, fp, st)
        else:
            ws = _ws(L.dc_conv1x1_wgrad_workspace(*a, 1))
            rc = L.dc_conv1x1_wgrad_bn(ptr(d["x"]), ptr(d["gy"]), out.body.data_ptr(), ws.body.data_ptr(), *a, 1, fp, st)
    else:
        if nparts is None:
            nparts = PC.parts_query(case)[0]
        M = PC.dims(case)[0]
        if case.kind == "fwd":
            out, shape = _Guarded(B * Co * H * W), (B, Co, H, W)
            if on and case.loader:
                f.in_scale, f.in_shift = ptr(d["s"]), ptr(d["t"])
            if on and case.stats:
                part = _Guarded(M * nparts * 2)
                f.stat_part = part.body.data_ptr()
            if x3:
                ws = _ws(L.dc_pointwise_workspace(_lib.PASS_FWD, fp, *a, 1))
                rc = L.dc_pointwise_fwd(ptr(d["x"]), ptr(d["w"]), None, out.body.data_ptr(), ws.body.data_ptr(), *a, 1, 0, fp, st)
            else:
                ws = _ws(16)
                rc = L.dc_conv1x1_fwd_bn(ptr(d["x"]), ptr(d["w"]), out.body.data_ptr(), *a, 1, fp, st)
        else:
            out, shape = _Guarded(B * Ci * H * W), (B, Ci, H, W)
            part = _Guarded(M * nparts * 2)
            f.bn_x, f.bn_mean, f.bwd_part = ptr(d["bn_x"]), ptr(d["mean"]), part.body.data_ptr()
            if case.mode == 2:
                f.in_scale, f.in_shift = ptr(d["s"]), ptr(d["t"])
            else:
                # the decision can only come from the bits: no scale / shift in the fold.  The mask is dc_bn_apply's own.
                nbytes = L.dc_bn_mask_bytes(B, Ci, H * W)
                assert nbytes > 0
                mask, ybn = _Guarded(nbytes // 4), _Guarded(B * Ci * H * W)
                assert L.dc_bn_apply(ptr(d["bn_x"]), ptr(d["res"]), ptr(d["s"]), ptr(d["t"]), ybn.body.data_ptr(), mask.body.data_ptr(),
                                     B, Ci, H * W, 1, case.groups, st) == 0
                torch.cuda.synchronize()
                assert mask.intact() and ybn.intact()
                f.bn_mask = mask.body.data_ptr()
                bufs += [mask, ybn]
            if x3:
                ws = _ws(L.dc_pointwise_workspace(_lib.PASS_DGRAD, fp, *a, 1))
                rc = L.dc_pointwise_dgrad(ptr(d["gy"]), ptr(d["w"]), out.body.data_ptr(), ws.body.data_ptr(), ptr(d["addend"]), None, *a, 1, fp, st)
            else:
                ws = _ws(16)
                rc = L.dc_conv1x1_dgrad_bn(ptr(d["gy"]), ptr(d["w"]), out.body.data_ptr(), ptr(d["addend"]), *a, 1, fp, st)
    assert rc == want, rc
    torch.cuda.synchronize()
    assert out.intact() and ws.intact() and (part is None or part.intact()), "a write outside the buffer"
    if want != 0:
        assert bool(torch.isnan(out.body).all()) and (part is None or bool(torch.isnan(part.body).all())), "a refused call wrote"
    res = {"out": out.body.cpu().view(shape), "part": None}
    if part is not None:
        res["part"] = part.body.cpu().view(shape[1], -1, 2)
    return res


def _flat(t):
    """(B, M, H, W) -> (M, N): the flattened pixel order n = b P + p of both families."""
    return t.permute(1, 0, 2, 3).reshape(t.shape[1], -1)


def _partials_gate(case, got, part, inp, r64):
    """The `own` and `ref` gates.  Returns the largest share of each bound that was used: (own slot, own image, own group, ref sum,
    ref second); own image is nan where an image owns no whole slots."""
    m = PC.mech(case)
    B, groups, npg, P, N, cover = case.B, case.groups, m["npg"], m["P"], m["N"], m["cover"]
    nparts, ppg = part.shape[1], m["ppg"]
    assert (nparts, ppg) == PC.parts_query(case) == (m["nparts"], m["ppg"])
    assert not bool(torch.isnan(part).any()), "a partial slot was not written"
    live = PC.ceil_div(N, cover)
    assert bool((_bits(part[:, live:].contiguous()) == 0).all()), "the slot of an empty wave column is not +0.0"
    assert m["empty_column"] == (live < nparts)
    o = got.double()
    if case.kind == "fwd":
        terms, names = (o, o * o), ("S", "Q")
    else:
        gi = torch.arange(B) // npg
        xm = inp["bn_x"].double() - inp["mean"].double()[gi][:, :, None, None]
        terms, names = (o, o * xm), ("P0", "P1")
    flat = [_flat(t) for t in terms]
    pad = live * cover - N
    slots = [torch.nn.functional.pad(t, (0, pad)).view(t.shape[0], live, cover) for t in flat]
    share = [0.0, float("nan"), 0.0, 0.0, 0.0]
    p64 = part.double()

    def gate(k, what, lo, hi, q, n, total, mag):
        bound = PC.sum_bound(n, mag)
        diff = (p64[:, lo:hi, q].sum(1) - total).abs()
        share[k] = max(share[k] if share[k] == share[k] else 0.0, float((diff / bound.clamp_min(1e-300)).max()))
        assert bool((diff <= bound).all()), (what, names[q], float(diff.max()), float(bound.min()))

    nslot = torch.full((live,), float(cover), dtype=torch.float64)
    nslot[-1] = N - (live - 1) * cover
    for q in range(2):
        bound = PC.sum_bound(nslot, slots[q].abs().sum(2))
        diff = (p64[:, :live, q] - slots[q].sum(2)).abs()
        share[0] = max(share[0], float((diff / bound.clamp_min(1e-300)).max()))
        assert bool((diff <= bound).all()), ("slot", names[q], int((diff > bound).nonzero()[0][1]), float(diff.max()))
        if P % cover == 0:
            ppi = P // cover
            for b in range(B):
                gate(1, ("image", b), b * ppi, (b + 1) * ppi, q, P, terms[q][b].sum((1, 2)), terms[q][b].abs().sum((1, 2)))
    delta = PC.TENSOR_TOL * float(r64[PC.TENSORS[case.kind]].abs().max())
    n = npg * P
    for g in range(groups):
        lo, hi = g * ppg, (nparts if g == groups - 1 else (g + 1) * ppg)
        rows = slice(g * npg, (g + 1) * npg)
        for q in range(2):
            gate(2, ("group", g), lo, hi, q, n, terms[q][rows].sum((0, 2, 3)), terms[q][rows].abs().sum((0, 2, 3)))
        s = p64[:, lo:hi].sum(1)
        if case.kind == "fwd":
            yabs = r64["y"].abs()[rows].sum((0, 2, 3))
            b0, b1 = PC.stat_bounds(n, delta, yabs)
            b0 = torch.full_like(yabs, b0)
        else:
            b0 = torch.full((s.shape[0],), n * delta, dtype=torch.float64)
            b1 = delta * xm.abs()[rows].sum((0, 2, 3))
        for q, bound in ((0, b0), (1, b1)):
            diff = (s[:, q] - r64[names[q]][g]).abs()
            share[3 + q] = max(share[3 + q], float((diff / bound.clamp_min(1e-300)).max()))
            assert bool((diff <= bound).all()), ("statement", g, names[q], float(diff.max()), float(bound.min()))
    return share


def _check(case):
    inp, r64, r32 = PC.reference(case)
    name = PC.TENSORS[case.kind]
    res = _launch(case, inp)
    e32 = PC.rel_err(r32[name], r64[name])
    err = _tensor_gate(case, res["out"], r64[name], r64.get("keep"))
    line = "pointwise_bn_parity %-40s %s rel_err %.2e (%.0f%% of %.0e; torch fp32 %.1e)" % (
        PC.case_id(case), name, err, 100 * err / PC.TENSOR_TOL, PC.TENSOR_TOL, e32)
    if res["part"] is not None and err <= PC.TENSOR_TOL:
        print(line, end="")
        share = _partials_gate(case, res["out"], res["part"], inp, r64)
        pct = ["-" if v != v else "%.*f%%" % (0 if k < 3 else 1, 100 * v) for k, v in enumerate(share)]
        line = "  partials: own slot %s image %s group %s, statement sum %s second %s" % tuple(pct)
    print(line)
    assert err <= PC.TENSOR_TOL, (name, err)
    return res


@pytest.mark.parametrize("case", PC.params(PC.FWD))
def test_forward(case):
    _check(case)


@pytest.mark.parametrize("case", PC.params(PC.DGRAD))
def test_data_gradient(case):
    _check(case)


@pytest.mark.parametrize("case", PC.params(PC.WGRAD))
def test_weight_gradient(case):
    _check(case)


@pytest.mark.parametrize("case", PC.params(PC.DETERMINISM))
def test_two_launches_are_bitwise_equal(case):
    inp = PC.reference(case)[0]
    a, b = _launch(case, inp), _launch(case, inp)
    assert torch.equal(_bits(a["out"]), _bits(b["out"]))
    if case.kind != "wgrad":
        assert torch.equal(_bits(a["part"]), _bits(b["part"]))


@pytest.mark.parametrize("case", PC.params(PC.PLAIN_WGRAD))
def test_wgrad_without_a_fold_is_the_plain_weight_gradient(case):
    """bn == NULL, or a fold whose in_scale is NULL, is the family's plain entry (dc_conv1x1_wgrad / dc_gemm1x1x3_wgrad) on the RAW
    input, bitwise -- and not the folded statement's."""
    from depthcore import _lib
    from depthcore._lib import ptr
    L = _lib.lib()
    inp, r64, _ = PC.reference(case)
    null, empty = _launch(case, inp, "null")["out"], _launch(case, inp, "empty")["out"]
    assert torch.equal(_bits(null), _bits(empty))
    a = case[2:7]
    x, gy, out = _dev(inp["x"]), _dev(inp["gy"]), _Guarded(case.Co * case.Ci)
    if case.family == "x3":
        assert L.dc_gemm1x1x3_wgrad_ok(*a, 1)
        ws = _ws(L.dc_gemm1x1x3_wgrad_workspace(*a, 1))
        rc = L.dc_gemm1x1x3_wgrad(ptr(x), ptr(gy), out.body.data_ptr(), ws.body.data_ptr(), *a, 1, _lib.stream(x))
    else:
        ws = _ws(L.dc_conv1x1_wgrad_workspace(*a, 1))
        rc = L.dc_conv1x1_wgrad(ptr(x), ptr(gy), out.body.data_ptr(), ws.body.data_ptr(), *a, 1, _lib.stream(x))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert out.intact() and ws.intact()
    assert torch.equal(_bits(out.body.cpu().view(null.shape)), _bits(null))
    ref = torch.nn.grad.conv2d_weight(inp["x"].double(), null.shape, inp["gy"].double())
    assert PC.rel_err(null, ref) <= PC.TENSOR_TOL
    assert PC.rel_err(null, r64["dW"]) > 100 * PC.TENSOR_TOL


# ---- refusals: by return code, and nothing between the guards is written ----------------------------------------------------------
@pytest.mark.parametrize("case", PC.params(PC.NO_GROUP_LAYOUT))
def test_a_group_boundary_inside_a_wave_column_is_refused(case):
    """(The x3 case goes through the dispatcher: the split family has no partial layout here, so the pass falls to the fp32-MFMA
    entry and THAT one returns DC_EINVAL -- the split kernels' own refusal in g1x3_launch is not what this reaches.)"""
    assert PC.parts_query(case)[0] == 0
    _launch(case, PC.reference(case)[0], want=PC.EINVAL, nparts=8)
    dg = PC._dgrad(case.family, case.B, case.Co, case.Ci, case.H, case.W, case.groups, 2, 0)
    _launch(dg, PC.reference(dg)[0], want=PC.EINVAL, nparts=8)


def test_a_ragged_reduction_has_no_epilogue_and_no_folded_weight_gradient():
    c = PC.NO_DGRAD
    assert PC.parts_query(c)[0] == 0
    _launch(c, PC.reference(c)[0], want=PC.EINVAL, nparts=8)
    for c in PC.NO_WGRAD:
        _launch(c, PC.reference(c)[0], want=PC.EINVAL)


@pytest.mark.parametrize("case", PC.params(PC.MODE2_ADDEND))
def test_the_rederived_decision_refuses_an_addend(case):
    assert PC.parts_query(case)[0] > 0
    _launch(case, PC.reference(case)[0], want=PC.EINVAL)


# ---- module level: the shape whose partial count used to come with ppg = 0 --------------------------------------------------------
def test_module_level_fold_below_one_wave_column():
    """bnfold.conv1x1 -> bnfold.bn_apply at (2, 32, 64, 4, 4), one group, under the default split mode: N = 32 pixels are half a wave
    column of the split family's 64 x 128 tile.  Against the fp64 chain, to the output bound of
    tests/test_bnfold_gpu.py::test_conv_bn_relu_conv_chain_vs_torch."""
    from depthcore import bnfold
    from helpers import close
    B, Ci, Co, H, W = PC.MODULE_SHAPE
    g = torch.Generator().manual_seed(41)
    x = torch.randn(B, Ci, H, W, generator=g)
    w = torch.randn(Co, Ci, 1, 1, generator=g) / Ci ** 0.5
    gamma, beta = torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g) * 0.3
    bn = torch.nn.BatchNorm2d(Co)
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
    bn = bn.to(DEV)
    y64 = torch.nn.functional.conv2d(x.double(), w.double())
    mean, var = y64.mean((0, 2, 3), keepdim=True), y64.var((0, 2, 3), unbiased=False, keepdim=True)
    want = torch.relu((y64 - mean) / (var + bn.eps).sqrt() * gamma.double()[None, :, None, None] + beta.double()[None, :, None, None])
    ya, sa = bnfold.conv1x1(x.to(DEV), w.to(DEV), 1, 1)
    assert sa is not None and sa.nparts > 0 and sa.ppg >= 1, "no statistics epilogue on a tiled shape"
    yh = bnfold.bn_apply(ya, bn, sa, groups=1)
    torch.cuda.synchronize()
    err = float((yh.detach().cpu().double() - want).abs().max())
    print("pointwise_bn_parity module-2x32to64x4x4-g1 y max abs err %.2e (max |y| %.2f; nparts %d ppg %d)" % (err, float(want.abs().max()), sa.nparts, sa.ppg))
    close(yh.detach(), want.float(), rtol=2e-4, atol=2e-5)


# ---- the stride-2 data gradient with 0, 1 and 2 addends ------------------------------------------------------------------------------
STRIDE2 = [pytest.param(s, f, id="%s-%s" % (f, "x".join(map(str, s)))) for s in PC.STRIDE2 for f in ("g1", "x3") if PC.pass_ok(f, "dgrad", *s, 2)]


@pytest.mark.parametrize("naddends", [0, 1, 2])
@pytest.mark.parametrize("shape,family", STRIDE2)
def test_stride2_data_gradient_vs_fp64(shape, family, naddends):
    """g1_dgrad_kernel SD 2 / 3 and g1x3_kernel MODE 4: every cell of dx is written once; the cells the stride skips hold the fp32 sum
    of the addends (+0.0 without any); the tensor gate on the whole of dx.  (The split kernels take P % 16 == 0 only: the first shape
    is the fp32-MFMA family's alone.)"""
    from depthcore import _lib
    from depthcore._lib import ptr
    L = _lib.lib()
    B, Ci, Co, Hi, Wi = shape
    g =torch.Generator().manual_seed(sum(shape) + 7)
    gy = torch.randn(B, Co, Hi // 2, Wi // 2, generator=g)
    w = torch.randn(Co, Ci, 1, 1, generator=g) / Co ** 0.5
    adds = [torch.randn(B, Ci, Hi, Wi, generator=g) for _ in range(naddends)]
    ref = torch.nn.grad.conv2d_input((B, Ci, Hi, Wi), w.double(), gy.double(), stride=2)
    for t in adds:
        ref = ref + t.double()
    r32 = torch.nn.grad.conv2d_input((B, Ci, Hi, Wi), w, gy, stride=2)
    for t in adds:
        r32 = r32 + t
    dadds = [_dev(t) for t in adds] + [None, None]
    out, gyd, wd = _Guarded(B * Ci * Hi * Wi), _dev(gy), _dev(w.view(Co, Ci))
    st = _lib.stream(gyd)
    if family == "x3":
        L.dc_set_gemm_split(1)
        assert L.dc_gemm1x1x3_dgrad_ok(B, Ci, Co, Hi, Wi, 2)
        ws = _ws(L.dc_pointwise_workspace(_lib.PASS_DGRAD, None, B, Ci, Co, Hi, Wi, 2))
        rc = L.dc_pointwise_dgrad(ptr(gyd), ptr(wd), out.body.data_ptr(), ws.body.data_ptr(), ptr(dadds[0]), ptr(dadds[1]), B, Ci, Co, Hi, Wi, 2, None, st)
    else:
        ws = _ws(16)
        rc = L.dc_conv1x1_dgrad_add2(ptr(gyd), ptr(wd), out.body.data_ptr(), ptr(dadds[0]), ptr(dadds[1]), B, Ci, Co, Hi, Wi, 2, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert out.intact() and ws.intact(), "a write outside the buffer"
    got = out.body.cpu().view(B, Ci, Hi, Wi)
    assert bool(torch.isfinite(got).all()), "a cell of dx was not written"
    err, e32 = PC.rel_err(got, ref), PC.rel_err(r32, ref)
    print("pointwise_bn_parity %s-dgrad-s2-%s-add%d dx rel_err %.2e (%.0f%% of %.0e; torch fp32 %.1e)" % (
        family, "x".join(map(str, shape)), naddends, err, 100 * err / PC.TENSOR_TOL, PC.TENSOR_TOL, e32))
    skipped = torch.ones(Hi, Wi, dtype=torch.bool)
    skipped[::2, ::2] = False
    want = torch.zeros(B, Ci, Hi, Wi)
    for t in adds:
        want = want + t
    assert torch.equal(_bits(got[:, :, skipped].contiguous()), _bits(want[:, :, skipped].contiguous())), "a skipped cell is not the addends' sum"
    assert err <= PC.TENSOR_TOL, err
