"""The 7x7 local self-attention kernels (csrc/sasa.hip) through the C ABI, one dc_sasa_fwd and one dc_sasa_bwd per case, against
the fp64 statement of tests/sasa_ref.py (pinned to the reference module by tests/test_sasa_cpu.py) at the kernels' edges: maps
smaller than the window, maps that fill a tile exactly and maps one past it, ragged widths, blocks that take several channel
planes with the rel_h / rel_w split inside them, batch-strided q / k / v, two and three passes of the rel-gradient reduction,
logit spreads beyond fp32's exp range, q = 0, and the refusals.

Every output (y, lse, dq, dk, dv, drel_h, drel_w, the workspace of exactly dc_sasa_bwd_workspace bytes) lives between sentinel
guard bands that must come back bit-identical, with a NaN body that must come back without a NaN.

Gate: the project's attention gate, attn_cases.bound(e32, L) = layer_ops_cases.gate_bound(e32) + 2 L 2^-24, where e32 is the error
of torch's fp32 CPU evaluation of the statement on the same inputs and L the largest logit spread; errors are max-abs relative to
the largest reference entry (attn_cases.rel_err).  Every test prints its figures (`sasa_parity ...`) before it asserts; DESIGN.md,
"Self-attention encoder", has the table.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import attn_cases as AC
import sasa_ref as SR
from test_attn_shapes_gpu import _Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DC_EINVAL = -1
OUTS = ("y", "lse", "dq", "dk", "dv", "rel_h", "rel_w")

# (B, C, H, W, input scale).  The launch geometry (dc_sasa_plan): balanced tiles of at most 16 x 32, np planes per block.
CASES = {
    "golden and small maps": SR.GOLDEN_CASES + [(2, 4, 3, 4, 1.0), (2, 8, 7, 7, 1.0)],      # 7x7: every pixel sees padding on all sides
    "tile edges": [(1, 2, 16, 32, 1.0), (1, 2, 17, 32, 1.0), (1, 2, 16, 33, 1.0), (2, 4, 17, 33, 1.0), (1, 2, 32, 64, 1.0)],
    "tail widths": [(1, 2, 5, 13, 1.0), (1, 4, 9, 41, 1.0)],
    # C/2 odd: the rel_h / rel_w split falls inside a block; 10 planes in blocks of 3: a ragged last block; 12 planes in blocks of 4
    # that straddle the two images
    "multi-plane blocks": [(1, 10, 12, 40, 1.0), (2, 6, 6, 20, 1.0), (3, 6, 1, 1, 1.0)],
    # 3 x 12 tiles: 108 rows per channel at B = 3 (two passes of 64), 144 at B = 4 (three)
    "reduction passes": [(3, 2, 33, 353, 1.0), (4, 2, 33, 353, 1.0)],
}
ALL = [c for v in CASES.values() for c in v]
DETERMINISM = (3, 10, 19, 45, 1.0)       # 2 x 2 tiles of 10 x 23, 3 planes per block: the block of planes 9..11 straddles two images


def _id(case):
    return SR.case_tag(case) + ("" if case[4] == 1.0 else "-x%g" % case[4])


@functools.lru_cache(maxsize=None)
def reference(case, q_zero=False):
    """(inputs, fp64 results, fp32 results, L): q, k, v = the three 1x1 convolutions of the seeded x of the case, rounded to fp32
    (so the device sees the same numbers); results by CPU autograd of the statement.  Shared and read-only."""
    x, st, gy = SR.golden_inputs(case)
    q, k, v = (F.conv2d(x, st[n + "_conv.weight"]).float().double() for n in ("query", "key", "value"))
    if q_zero:
        q = torch.zeros_like(q)
    inp = {"q": q, "k": k, "v": v, "rel_h": st["rel_h"], "rel_w": st["rel_w"], "gy": gy}
    res = {}
    for dt in (torch.float64, torch.float32):
        leaves = [inp[n].to(dt).clone().requires_grad_() for n in ("q", "k", "v", "rel_h", "rel_w")]
        y, lse = SR.attention(*leaves)
        grads = torch.autograd.grad((y * inp["gy"].to(dt)).sum(), leaves)
        res[dt] = dict(zip(OUTS, [y.detach(), lse.detach()] + [g.reshape(-1, 7) if i > 2 else g for i, g in enumerate(grads)]))
    lg = SR.logits(q, k, st["rel_h"], st["rel_w"])
    return inp, res[torch.float64], res[torch.float32], float((lg.max(0).values - lg.min(0).values).max())


def _launch(case, inp, strided=False, save_lse=True, backward=True):
    """One forward (and one backward) launch.  -> {name: CPU fp32 tensor}; asserts the guards and the absence of NaN."""
    from depthcore import _lib
    L = _lib.lib()
    B, C, H, W = case[:4]
    n = B * C * H * W
    if strided:         # q, k, v as channel slices of one (B,3C,H,W) tensor: batch stride 3 C H W
        qkv = torch.cat([inp[k].float() for k in ("q", "k", "v")], 1).to(DEV).contiguous()
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        bs = 3 * C * H * W
    else:
        q, k, v = (inp[k].float().to(DEV).contiguous() for k in ("q", "k", "v"))
        bs = C * H * W
    rh, rw = (inp[k].float().reshape(-1, 7).to(DEV).contiguous() for k in ("rel_h", "rel_w"))
    gy = inp["gy"].float().to(DEV).contiguous()
    st = _lib.stream(gy)
    g = {"y": _Guarded(n), "lse": _Guarded(n)}
    _lib.check(L.dc_sasa_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), bs, bs, bs, _lib.ptr(rh), _lib.ptr(rw), _lib.ptr(g["y"].body),
                             _lib.ptr(g["lse"].body) if save_lse else None, B, C, H, W, st), "dc_sasa_fwd")
    if not save_lse:
        torch.cuda.synchronize()
        assert g["lse"].intact() and bool(torch.isnan(g["lse"].body).all()), "the inference path wrote lse"
        del g["lse"]
    if backward:
        nws = L.dc_sasa_bwd_workspace(B, C, H, W)
        plan = (ctypes.c_int * 5)()
        assert L.dc_sasa_plan(B, C, H, W, plan) == 0
        th, tw, nx, ny, npl = plan
        assert nws == nx * ny * -(-B * C // npl) * npl * 7 * 4 and th <= 16 and tw <= 32
        g.update({k_: _Guarded(n) for k_ in ("dq", "dk", "dv")})
        g.update({"rel_h": _Guarded(C // 2 * 7), "rel_w": _Guarded(C // 2 * 7), "ws": _Guarded(nws // 4)})
        _lib.check(L.dc_sasa_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), bs, bs, bs, _lib.ptr(rh), _lib.ptr(rw), _lib.ptr(g["y"].body),
                                 _lib.ptr(g["lse"].body), _lib.ptr(gy), _lib.ptr(g["dq"].body), _lib.ptr(g["dk"].body),
                                 _lib.ptr(g["dv"].body), _lib.ptr(g["rel_h"].body), _lib.ptr(g["rel_w"].body), g["ws"].body.data_ptr(),
                                 B, C, H, W, st), "dc_sasa_bwd")
    torch.cuda.synchronize()
    assert all(b.intact() for b in g.values()), (_id(case), "a launch wrote outside its output")
    out = {}
    for name, b in g.items():
        assert not bool(torch.isnan(b.body).any()), (_id(case), name, "an element was never written")
        if name != "ws":
            out[name] = b.body.cpu().view(-1, 7) if name.startswith("rel") else b.body.cpu().view(B, C, H, W)
    return out


def _gate(case, got, r64, r32, L, what=""):
    failures = []
    for name in got:
        assert got[name].shape == r64[name].shape and got[name].dtype == torch.float32, (name, got[name].shape)
        e_hip, e32 = AC.rel_err(got[name], r64[name]), AC.rel_err(r32[name], r64[name])
        b = AC.bound(e32, L)
        print("sasa_parity %-24s %-6s e_hip=%.3e e32=%.3e L=%7.2f bound=%.3e" % (_id(case) + what, name, e_hip, e32, L, b))
        if not e_hip <= b:
            failures.append((name, e_hip, e32, L, b))
    assert not failures, (_id(case), failures)


@pytest.mark.parametrize("case", ALL, ids=_id)
def test_kernels_vs_fp64_statement(case):
    inp, r64, r32, L = reference(case)
    _gate(case, _launch(case, inp), r64, r32, L)


def test_the_wide_case_is_wide():
    _, _, r32, L = reference(SR.WIDE)
    assert L > 200 and bool(torch.isfinite(r32["y"]).all())


@pytest.mark.parametrize("case", [(2, 6, 6, 20, 1.0), (2, 4, 17, 33, 1.0)], ids=_id)
def test_batch_strided_inputs_are_read_in_place(case):
    """q, k, v as slices of one (B,3C,H,W) tensor, batch stride 3CHW: the same bits as from three dense tensors."""
    inp, r64, r32, L = reference(case)
    got = _launch(case, inp, strided=True)
    _gate(case, got, r64, r32, L, " strided")
    dense = _launch(case, inp)
    for k in got:
        assert torch.equal(got[k], dense[k]), k


@pytest.mark.parametrize("case", [(2, 4, 5, 9, 1.0), (1, 6, 17, 33, 1.0)], ids=_id)
def test_zero_query_gives_the_plain_mean(case):
    """q = 0: every logit is 0, so y = (sum of the in-image v taps) / 49 -- the padded taps count in the softmax and carry v = 0 --
    dk and both rel gradients are exactly 0, and dv matches the statement."""
    inp, r64, r32, L = reference(case, True)
    assert L == 0.0
    got = _launch(case, inp)
    mean = sum(SR._shift(inp["v"], dy, dx) for dy in range(7) for dx in range(7)) / 49
    e, e32 = AC.rel_err(got["y"], mean), AC.rel_err(r32["y"], mean)
    print("sasa_parity %-24s y vs the mean of the taps: e_hip=%.3e e32=%.3e" % (_id(case) + " q=0", e, e32))
    assert e <= AC.bound(e32, 0.0)
    for k in ("dk", "rel_h", "rel_w"):
        assert bool((got[k] == 0).all()), k
    _gate(case, got, r64, r32, L, " q=0")


def test_two_runs_are_bitwise_equal_and_the_batch_decomposes():
    """Two runs into fresh buffers agree bit for bit in everything; the B-image call equals B single-image calls bit for bit in
    y, lse, dq, dk, dv (the block decomposition changes -- 10 planes per image in blocks of 3 that straddle images -- the
    per-pixel arithmetic does not)."""
    case = DETERMINISM
    inp = reference(case)[0]
    a, b = _launch(case, inp), _launch(case, inp)
    for k in a:
        assert torch.equal(a[k], b[k]), (k, "differs between two runs")
    for i in range(case[0]):
        sl = {k: (t[i:i + 1] if k in ("q", "k", "v", "gy") else t) for k, t in inp.items()}
        s = _launch((1,) + case[1:], sl)
        for k in ("y", "lse", "dq", "dk", "dv"):
            assert torch.equal(s[k], a[k][i:i + 1]), (k, i)


@pytest.mark.parametrize("case", [(2, 6, 6, 20, 1.0), (1, 2, 17, 33, 1.0)], ids=_id)
def test_inference_forward_saves_nothing_and_equals_the_saving_forward(case):
    inp = reference(case)[0]
    full, inf = _launch(case, inp, backward=False), _launch(case, inp, save_lse=False, backward=False)
    assert set(inf) == {"y"} and torch.equal(full["y"], inf["y"])


def test_refusals_return_einval_and_write_nothing():
    from depthcore import _lib
    L = _lib.lib()
    B, C, H, W = 2, 4, 6, 8
    n = B * C * H * W
    gen = torch.Generator().manual_seed(5)
    t = {k: torch.randn(B, C, H, W, generator=gen).to(DEV) for k in ("q", "k", "v", "y", "lse", "gy")}
    t["rel_h"], t["rel_w"] = torch.randn(C // 2, 7, generator=gen).to(DEV), torch.randn(C // 2, 7, generator=gen).to(DEV)
    g = {k: _Guarded(n) for k in ("oy", "olse", "dq", "dk", "dv")}
    g.update({"drh": _Guarded(C // 2 * 7), "drw": _Guarded(C // 2 * 7), "ws": _Guarded(L.dc_sasa_bwd_workspace(B, C, H, W) // 4)})
    st = _lib.stream(t["q"])
    p = lambda x: None if x is None else x.data_ptr()
    chw = C * H * W

    def fwd(B_=B, C_=C, H_=H, W_=W, bs=(chw, chw, chw), **null):
        a = {k: (None if k in null else t[k]) for k in ("q", "k", "v", "rel_h", "rel_w")}
        return L.dc_sasa_fwd(p(a["q"]), p(a["k"]), p(a["v"]), *bs, p(a["rel_h"]), p(a["rel_w"]),
                             None if "oy" in null else p(g["oy"].body), p(g["olse"].body), B_, C_, H_, W_, st)

    def bwd(B_=B, C_=C, H_=H, W_=W, bs=(chw, chw, chw), **null):
        a = {k: (None if k in null else t[k]) for k in ("q", "k", "v", "rel_h", "rel_w", "y", "lse", "gy")}
        o = {k: (None if k in null else g[k].body) for k in ("dq", "dk", "dv", "drh", "drw", "ws")}
        return L.dc_sasa_bwd(p(a["q"]), p(a["k"]), p(a["v"]), *bs, p(a["rel_h"]), p(a["rel_w"]), p(a["y"]), p(a["lse"]), p(a["gy"]),
                             p(o["dq"]), p(o["dk"]), p(o["dv"]), p(o["drh"]), p(o["drw"]), p(o["ws"]), B_, C_, H_, W_, st)

    def untouched():
        torch.cuda.synchronize()
        return all(b.intact() and bool(torch.isnan(b.body).all()) for b in g.values())

    for kw in (dict(C_=3), dict(C_=1), dict(C_=0), dict(B_=0), dict(B_=-1), dict(H_=0), dict(W_=0), dict(H_=-6),
               dict(B_=2, H_=16384, W_=16384),                 # B*C*H*W = 2^31: refused before any pointer is dereferenced
               dict(bs=(chw - 1, chw, chw)), dict(bs=(chw, chw - 1, chw)), dict(bs=(chw, chw, -chw))):
        assert fwd(**kw) == DC_EINVAL and bwd(**kw) == DC_EINVAL, kw
    assert 2 * 4 * 16384 * 16384 == 2 ** 31 and untouched()
    for name in ("q", "k", "v", "rel_h", "rel_w"):
        assert fwd(**{name: 1}) == DC_EINVAL and bwd(**{name: 1}) == DC_EINVAL, name
    assert fwd(oy=1) == DC_EINVAL
    for name in ("y", "lse", "gy", "dq", "dk", "dv", "drh", "drw", "ws"):
        assert bwd(**{name: 1}) == DC_EINVAL, name
    assert untouched()
    # the same pointers are accepted when nothing is wrong (the refusals above are not a broken set-up)
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert all(b.intact() and not bool(torch.isnan(b.body).any()) for b in g.values())


def test_autograd_op_matches_the_statement_and_passes_no_lse_under_no_grad():
    """ops.local_attention7: gradients of all five inputs through autograd (rel in the reference's 5-d parameter shapes, q / k / v
    slices of one tensor), the same bits under no_grad."""
    from depthcore import ops
    case = (2, 6, 6, 20, 1.0)
    inp, r64, r32, L = reference(case)
    C = case[1]
    qkv = torch.cat([inp[k].float() for k in ("q", "k", "v")], 1).to(DEV).requires_grad_()
    rh, rw = inp["rel_h"].float().to(DEV).requires_grad_(), inp["rel_w"].float().to(DEV).requires_grad_()
    assert rh.shape == (C // 2, 1, 1, 7, 1) and rw.shape == (C // 2, 1, 1, 1, 7)
    y = ops.local_attention7(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], rh, rw)
    gqkv, grh, grw = torch.autograd.grad((y * inp["gy"].float().to(DEV)).sum(), [qkv, rh, rw])
    assert grh.shape == rh.shape and grw.shape == rw.shape
    got = {"y": y.detach().cpu(), "dq": gqkv[:, :C].cpu(), "dk": gqkv[:, C:2 * C].cpu(), "dv": gqkv[:, 2 * C:].cpu(),
           "rel_h": grh.cpu().view(-1, 7), "rel_w": grw.cpu().view(-1, 7)}
    _gate(case, got, r64, r32, L, " autograd")
    with torch.no_grad():
        y0 = ops.local_attention7(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], rh, rw)
    assert not y0.requires_grad and torch.equal(y0, y.detach())
