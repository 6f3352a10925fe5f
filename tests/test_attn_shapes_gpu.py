"""The AttentionConv kernels (csrc/attn.hip) through the C ABI, one dc_attnconv_fwd and one dc_attnconv_bwd per case, against
the fp64 statement of tests/attn_cases.py at the kernels' tile, padding and reduction edges: maps that fill a forward or a
backward tile exactly and maps one pixel past it, a 1 x 1 map, two and three passes of the parameter reduction, pixel-shuffled
channels in x, res, dx and dres, batch chunks and a batch stride beyond C*H*W, the whole flag matrix, ReLU masks at +-0.0, logit
spreads that underflow the softmax, and the refusals.  The fitness of the cases is the subject of tests/test_attn_cases_cpu.py.

The case table with its reasons, the gate with the derivation of its exponential term, and the measured error of every case
next to its bound are in DESIGN.md, "AttentionConv at its tile, padding and reduction edges"; every test here prints its figures
(`attn_parity ...`) before it asserts.

Every output (y, each dx and dres source, dparams, the workspace of exactly dc_attnconv_bwd_workspace bytes) lives inside a larger
buffer: sentinel guard bands on both sides that must come back bit-identical (nothing is written outside the output), and a NaN
body that must come back without a NaN (every element is written, ragged last tiles and all four pixel-shuffle planes included).

Out of scope: the fp32 accumulation error of the 25k partial rows at the training shape (B=36, 192x640) is a property of that
workload, not of an edge; no case here is larger than about 340k elements.
"""
import ctypes
import math

import pytest
import torch

import attn_cases as AC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256                      # floats on either side of an output
SENTINEL = -7.0312e28
DC_EINVAL = -1
NAN = float("nan")


def _bits(t):
    return t.view(torch.int32)


class _Guarded:
    """`n` floats between two guard bands of sentinels.  The body starts as NaN; `hold` marks a part of the body that no launch
    may write either (the other chunk of a chunked tensor, the outer channels of a 6-channel one)."""

    def __init__(self, n):
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
        self.body = self.buf[GUARD:GUARD + n]
        self.body.fill_(NAN)
        self.held = [self.buf[:GUARD], self.buf[GUARD + n:]]

    def hold(self, view):
        view.fill_(SENTINEL)
        self.held.append(view)

    def intact(self):
        want = int(_bits(torch.tensor([SENTINEL]))[0])
        return all(bool((_bits(v) == want).all()) for v in self.held)


def _place(layout, values, B, H, W):
    """Device tensors of a layout's sources, each inside guards; `values`: fp64 masters to copy in, or None for an output (NaN).
    Returns (tensors, guarded buffers)."""
    tensors, bufs, chunked, nchunk = [], [], None, 0
    for i, k in enumerate(layout):
        shape = AC.source_shape(k, B, H, W)
        if k == "c1":
            if chunked is None:
                g = _Guarded(3 * B * H * W)
                chunked = g.body.view(3 * B, 1, H, W)
                g.hold(chunked[:B])
                bufs.append(g)
            nchunk += 1
            t = chunked[nchunk * B:(nchunk + 1) * B]
        elif k == "w4":
            g = _Guarded(B * 6 * H * W)
            full = g.body.view(B, 6, H, W)
            g.hold(full[:, 0]); g.hold(full[:, 5])
            bufs.append(g)
            t = full[:, 1:5]
        else:
            g = _Guarded(math.prod(shape))
            bufs.append(g)
            t = g.body.view(shape)
        if values is not None:
            t.copy_(values[i].float())
        tensors.append(t)
    return tensors, bufs


def _map(layout, tensors, H, W):
    """dc_attn_map of a layout: ops._attn_map per source; the 6-channel source is addressed by hand (batch stride 6 H W)."""
    from depthcore import _lib, ops
    m, c = _lib.AttnMap(), 0
    for k, t in zip(layout, tensors):
        if k == "w4":
            assert t.shape[1] == 4 and t.stride() == (6 * H * W, H * W, W, 1)
            for ch in range(4):
                m.ptr[c], m.batch_stride[c], m.mode[c] = t.data_ptr() + ch * H * W * 4, 6 * H * W, _lib.ATTN_PLAIN
                c += 1
        else:
            sub, n = ops._attn_map([t], [ops.PIXEL_SHUFFLE2 if k == "ps2" else ops.PLAIN], H, W)
            for j in range(n):
                m.ptr[c], m.batch_stride[c], m.mode[c] = sub.ptr[j], sub.batch_stride[j], sub.mode[j]
                c += 1
    return m


def _launch(case, inp):
    """One forward and one backward launch of `case` on the masters `inp`.  Returns {name: CPU fp32 tensor} named as the
    statement's results, plus "dparams" (the raw vector); asserts the guards and the absence of NaN."""
    from depthcore import _lib, ops
    L = _lib.lib()
    B, C, H, W = case[:4]
    keep = []
    xs, _ = _place(case.x_layout, inp["x"], B, H, W)
    xm = _map(case.x_layout, xs, H, W)
    rl = AC.res_layout(case)
    if case.res_layout == AC.SAME:
        rm = xm
    elif rl:
        rs, _ = _place(rl, inp["res"], B, H, W)
        keep.append(rs)
        rm = _map(rl, rs, H, W)
    else:
        rm = None
    ps = [inp["params"][k].float().to(DEV).contiguous() for k in AC.PARAM_KEYS]
    ap = ops._attn_params(ps)
    gy = inp["gy"].float().to(DEV).contiguous()
    add = None if inp["dx_add"] is None else inp["dx_add"].float().to(DEV).contiguous()
    st = _lib.stream(gy)
    ref = lambda m: None if m is None else ctypes.byref(m)
    outs = {}
    guards = []
    yg = _Guarded(B * C * H * W)
    guards.append(yg)
    _lib.check(L.dc_attnconv_fwd(ref(xm), ctypes.byref(ap), ref(rm), _lib.ptr(yg.body), B, C, H, W, case.relu_in, case.relu_res, st),
               "dc_attnconv_fwd")
    outs["y"] = yg.body.view(B, C, H, W)
    dxs, g = _place(case.x_layout, None, B, H, W)
    guards += g
    dxm = _map(case.x_layout, dxs, H, W)
    dresm, drs = None, []
    if case.dres:
        drs, g = _place(AC.dres_layout(case), None, B, H, W)
        guards += g
        dresm = _map(AC.dres_layout(case), drs, H, W)
    npar, nws = L.dc_attnconv_param_count(C), L.dc_attnconv_bwd_workspace(B, C, H, W)
    assert npar == AC.param_count(C) and nws == AC.bwd_blocks(case) * npar * 4
    dpg, wsg = _Guarded(npar), _Guarded(nws // 4)
    guards += [dpg, wsg]
    _lib.check(L.dc_attnconv_bwd(ref(xm), ctypes.byref(ap), ref(rm), _lib.ptr(gy), ref(dxm), _lib.ptr(add), ref(dresm), _lib.ptr(dpg.body),
                                 wsg.body.data_ptr(), B, C, H, W, case.relu_in, case.relu_res, st), "dc_attnconv_bwd")
    torch.cuda.synchronize()
    for i, t in enumerate(dxs):
        outs["dx.%d" % i] = t
    for i, t in enumerate(drs):
        outs["dres.%d" % i] = t
    for k, t in zip(AC.PARAM_KEYS, ops._attn_param_grads(dpg.body, C, ps)):
        outs[k] = t
    outs["dparams"] = dpg.body
    assert all(g.intact() for g in guards), (AC.case_id(case), "a launch wrote outside its output")
    assert not bool(torch.isnan(wsg.body).any()), (AC.case_id(case), "a partial row of the workspace was never written")
    outs = {k: v.cpu().contiguous() for k, v in outs.items()}
    for k, v in outs.items():
        assert not bool(torch.isnan(v).any()), (AC.case_id(case), k, "an element was never written")
    return outs


def _gate(case, got, r64, r32, info):
    failures = []
    for name in AC.compared(case, r64):
        assert got[name].shape == r64[name].shape and got[name].dtype == torch.float32, (name, got[name].shape)
        e_hip, e32 = AC.rel_err(got[name], r64[name]), AC.rel_err(r32[name], r64[name])
        b = AC.bound(e32, info["L"])
        print("attn_parity %-78s %-18s e_hip=%.3e e32=%.3e L=%8.2f bound=%.3e" % (AC.case_id(case), name, e_hip, e32, info["L"], b))
        if not e_hip <= b:
            failures.append((name, e_hip, e32, info["L"], b))
    kb = float(got[AC.KEY_BIAS].abs().max())
    print("attn_parity %-78s %-18s max|.|=%.3e limit=%.3e" % (AC.case_id(case), AC.KEY_BIAS, kb, AC.KEY_BIAS_TOL * info["scale"]))
    if not AC.key_bias_ok(got[AC.KEY_BIAS], info):
        failures.append((AC.KEY_BIAS, kb, AC.KEY_BIAS_TOL * info["scale"]))
    assert not failures, (AC.case_id(case), failures)


def _planted(case, shift):
    m = torch.zeros(case.B, case.C, case.H, case.W, dtype=torch.bool)
    for c, y, x, _ in AC.kink_positions(case):
        m[:, (c + shift) % case.C, y, x] = True
    return m


@pytest.mark.parametrize("case", AC.params())
def test_attention_conv_vs_fp64_statement(case):
    inp, r64, r32, info = AC.reference(case)
    got = _launch(case, inp)
    assert got.keys() - {"dparams"} == r64.keys()
    _gate(case, got, r64, r32, info)
    if case.dres and case.res_layout is None:          # no residual, no mask: dres is gy itself
        assert torch.equal(got["dres.0"], inp["gy"].float())
    if case.param_style == "kink":                      # relu'(+-0.0) = 0, for the input mask and for the residual mask
        assert bool(((got["dx.0"] - inp["dx_add"].float())[_planted(case, 0)] == 0).all())
        assert bool((got["dres.0"][_planted(case, 1)] == 0).all())
    if case.param_style == "uniform":                   # q = 0: the plain mean of the 9 value taps, bk / bv of the padding included
        mean = AC.uniform_mean(case, inp)
        assert AC.rel_err(got["y"], mean) <= AC.bound(AC.rel_err(r32["y"], mean), 0.0)
        for k in ("key_conv.weight", "rel_h", "rel_w"):
            assert bool((got[k] == 0).all()), k


def test_backward_is_reproducible_and_batch_decomposition_agrees():
    """A self-consistency check, not the reference comparison (that is test_attention_conv_vs_fp64_statement on the same case):
    two backward runs into fresh buffers agree bit for bit, and the B-image call agrees with B single-image calls -- bit for
    bit in y and dx, and in dparams (the single-image vectors summed in fp64) within gate_bound(0) * sqrt(nblocks) of the largest
    entry: the same partial rows, reached through another decomposition of the flat block index and summed in another order."""
    case = AC.DETERMINISM
    inp = AC.reference(case)[0]
    a, b = _launch(case, inp), _launch(case, inp)
    for k in a:
        assert torch.equal(a[k], b[k]), (k, "differs between two runs")
    one = case._replace(B=1)
    total = torch.zeros(AC.param_count(case.C), dtype=torch.float64)
    for i in range(case.B):
        sl = {"x": [t[i:i + 1] for t in inp["x"]], "res": [], "params": inp["params"], "gy": inp["gy"][i:i + 1],
              "dx_add": inp["dx_add"][i:i + 1]}
        s = _launch(one, sl)
        assert torch.equal(s["y"], a["y"][i:i + 1]) and torch.equal(s["dx.0"], a["dx.0"][i:i + 1]), i
        total += s["dparams"].double()
    err = float((a["dparams"].double() - total).abs().max()) / float(total.abs().max())
    lim = AC.LC.gate_bound(0.0) * math.sqrt(AC.bwd_blocks(case))
    print("attn_parity batch decomposition: dparams differ by %.3e of the largest entry (limit %.3e)" % (err, lim))
    assert err <= lim, (err, lim)


def _refusal_setup(C=4, H=6, W=8, B=1):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, C, H, W, generator=g).to(DEV)
    xp = torch.randn(B, 4, H // 2, W // 2, generator=g).to(DEV)          # a pixel-shuffled channel of the same map size
    ps = [t.to(DEV) for t in (torch.randn(3, generator=g), torch.randn(3, generator=g), torch.randn(C, C, generator=g),
                              torch.randn(C, generator=g), torch.randn(C, C, generator=g), torch.randn(C, generator=g),
                              torch.randn(C, C, generator=g), torch.randn(C, generator=g))]
    t = {"x": x, "xp": xp, "ps": ps, "gy": torch.randn(B, C, H, W, generator=g).to(DEV)}
    for name, n in (("y", x.numel()), ("dx", x.numel()), ("dxp", xp.numel()), ("dres", x.numel()),
                    ("dp", AC.param_count(C)), ("ws", AC.ceil_div(W, 30) * AC.ceil_div(H, 6) * B * AC.param_count(C))):
        t[name] = _Guarded(n)
    return t


def _untouched(t):
    torch.cuda.synchronize()
    for name in ("y", "dx", "dxp", "dres", "dp", "ws"):
        assert t[name].intact() and bool(torch.isnan(t[name].body).all()), name
    return True


def test_refusals_return_einval_and_write_nothing():
    from depthcore import _lib, ops
    L = _lib.lib()
    B, C, H, W = 1, 4, 6, 8
    t = _refusal_setup(C, H, W, B)
    st = _lib.stream(t["x"])
    ap = ops._attn_params(t["ps"])
    plain = lambda v: _map(("p4",), [v.view(B, C, H, W)], H, W)
    xm, dxm, dresm = plain(t["x"]), plain(t["dx"].body), plain(t["dres"].body)
    # channel 0 read through PixelShuffle(2), channels 1..3 plain (views of the same buffers: channel 0 of `dx` stays unused)
    hw = H * W
    mixed = lambda shuf, flat: _map(("ps2", "p1", "p2"), [shuf.view(B, 4, H // 2, W // 2), flat[hw:2 * hw].view(B, 1, H, W),
                                                        flat[2 * hw:].view(B, 2, H, W)], H, W)
    xpm, dxpm = mixed(t["xp"], t["x"].view(-1)), mixed(t["dxp"].body, t["dx"].body)
    y, gy, dp, ws = _lib.ptr(t["y"].body), _lib.ptr(t["gy"]), _lib.ptr(t["dp"].body), t["ws"].body.data_ptr()
    r = ctypes.byref

    def fwd(xm_=xm, ap_=ap, y_=y, B_=B, C_=C, H_=H, W_=W):
        return L.dc_attnconv_fwd(r(xm_), r(ap_) if ap_ is not None else None, None, y_, B_, C_, H_, W_, 1, 0, st)

    def bwd(xm_=xm, ap_=ap, dxm_=dxm, dresm_=None, relu_res=0, B_=B, C_=C, H_=H, W_=W):
        return L.dc_attnconv_bwd(r(xm_), r(ap_) if ap_ is not None else None, None, gy, r(dxm_), None,
                                 None if dresm_ is None else r(dresm_), dp, ws, B_, C_, H_, W_, 1, relu_res, st)

    assert fwd(C_=3) == DC_EINVAL and bwd(C_=3) == DC_EINVAL and _untouched(t)
    # an odd H or W with a pixel-shuffled channel (the tensors are those of the even map: a launch would stay inside them)
    assert fwd(xm_=xpm, H_=H - 1) == DC_EINVAL and fwd(xm_=xpm, W_=W - 1) == DC_EINVAL and _untouched(t)
    assert bwd(xm_=xpm, H_=H - 1) == DC_EINVAL and bwd(dxm_=dxpm, H_=H - 1) == DC_EINVAL and bwd(dxm_=dxpm, W_=W - 1) == DC_EINVAL
    assert _untouched(t)
    for name in ("wq", "bq", "wk", "bk", "wv", "bv", "rel_h", "rel_w"):
        bad = ops._attn_params(t["ps"])
        setattr(bad, name, None)
        assert fwd(ap_=bad) == DC_EINVAL and bwd(ap_=bad) == DC_EINVAL, name
    assert fwd(ap_=None) == DC_EINVAL and bwd(ap_=None) == DC_EINVAL and _untouched(t)
    assert fwd(y_=None) == DC_EINVAL and _untouched(t)
    assert bwd(dresm_=dresm, relu_res=1) == DC_EINVAL and _untouched(t)          # a ReLU mask of a residual that is not there
    # B*C*H*W = 2^31: refused before any launch, so the small tensors behind the pointers are never dereferenced
    assert 2 * 4 * 16384 * 16384 == 2 ** 31
    assert fwd(B_=2, H_=16384, W_=16384) == DC_EINVAL and bwd(B_=2, H_=16384, W_=16384) == DC_EINVAL and _untouched(t)
    # the same pointers are accepted when nothing is wrong (the refusals above are not a broken set-up)
    assert fwd(xm_=xpm) == 0 and bwd(xm_=xpm, dxm_=dxpm, dresm_=dresm) == 0
    torch.cuda.synchronize()
    for name in ("y", "dx", "dxp", "dres", "dp", "ws"):
        body = t[name].body[hw:] if name == "dx" else t[name].body
        assert t[name].intact() and not bool(torch.isnan(body).any()), name
    assert bool(torch.isnan(t["dx"].body[:hw]).all())


def test_param_count_and_workspace_size():
    from depthcore import _lib
    L = _lib.lib()
    for C in range(-1, 9):
        assert L.dc_attnconv_param_count(C) == (3 * (C * C + C) + 6 if C in (2, 4) else 0), C
    for bad in ((0, 4, 8, 8), (-1, 4, 8, 8), (1, 3, 8, 8), (1, 1, 8, 8), (1, 8, 8, 8), (1, 4, 0, 8), (1, 4, 8, 0), (1, 4, -6, 30)):
        assert L.dc_attnconv_bwd_workspace(*bad) == 0, bad
    for B, C, H, W in [(1, 2, 1, 1), (1, 4, 6, 30), (1, 4, 7, 31), (2, 2, 12, 60), (5, 2, 43, 391), (36, 4, 192, 640)]:
        assert L.dc_attnconv_bwd_workspace(B, C, H, W) == AC.ceil_div(W, 30) * AC.ceil_div(H, 6) * B * (3 * (C * C + C) + 6) * 4


def test_residual_attention_unit_with_a_pixel_shuffled_first_source():
    """ops.residual_attention_unit with kinds = [PIXEL_SHUFFLE2, PLAIN]: the only caller-visible path through the unit's
    derivation of H, W from a pixel-shuffled first source.  Checked as tests/test_fusion_gpu.py checks its unit cases."""
    from depthcore import ops
    from helpers import close, rel_l2
    from oracle import fusion_ref as FR
    from test_fusion_gpu import _order
    from test_fusion_oracle import attn_state
    g = torch.Generator().manual_seed(6)
    B, C, H, W = 2, 2, 20, 34
    srcs = [torch.randn(B, 4, H // 2, W // 2, generator=g), torch.randn(B, 1, H, W, generator=g)]
    kinds = [ops.PIXEL_SHUFFLE2, ops.PLAIN]
    st = {}
    for a in ("atten1.", "atten2."):
        for k, v in attn_state(C, seed=11 + len(st)).items():
            st[a + k] = v
    cot = torch.randn(B, C, H, W, generator=g)
    so = [t.clone().requires_grad_() for t in srcs]
    po = {k: v.clone().requires_grad_() for k, v in st.items()}
    yo = FR.residual_attention_unit(torch.cat([FR.upscale_ps_shuffle_only(so[0]), so[1]], 1), po, "")
    go = torch.autograd.grad((yo * cot).sum(), so + list(po.values()))
    sh = [t.to(DEV).contiguous().requires_grad_() for t in srcs]
    ph = {k: v.to(DEV).requires_grad_() for k, v in st.items()}
    yh = ops.residual_attention_unit(sh, kinds, _order(ph, "atten1."), _order(ph, "atten2."))
    assert yh.shape == (B, C, H, W)
    gh = torch.autograd.grad((yh * cot.to(DEV)).sum(), sh + list(ph.values()))
    close(yh, yo, rtol=1e-4, atol=1e-5)
    scale = max(float(b.abs().max()) for b in go)
    for n, a, b in zip(["src0", "src1"] + list(st), gh, go):
        assert a.shape == b.shape, n
        if "key_conv.bias" in n:
            assert float(a.abs().max()) <= 1e-5 * scale and float(b.abs().max()) <= 1e-5 * scale, n
            continue
        assert rel_l2(a, b) < 2e-4, (n, rel_l2(a, b))
