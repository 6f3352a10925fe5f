"""The hand-over item walk (csrc/c2f_dev.h) through its six raw entries -- dc_lstm_handover_fwd / _bwd, dc_gru_handover_fwd / _bwd,
dc_lstm_infer_step, dc_gru_c2f_infer_step -- where the per-kernel tests do not go:

  * the four TRAINING entries on pointers 4 bytes past a 16-byte boundary (the two inference entries have this test in
    test_lstm_infer_gpu.py / test_gru_c2f_infer_gpu.py): judged by test_lstm_gpu._judge against the fp64 statement, and equal to
    the aligned call bit for bit;
  * the second trip of the grid-stride loop.  The grid is capped at 4096 blocks of dc_lstm_block() = 256 threads, so a thread
    takes a second item only above 1,048,576 items.  The kernels are separable by batch row, and one row of either shape below
    stays under the cap: a B = 2 call must equal two B = 1 calls on its rows, bit for bit -- no CPU oracle is needed.

`lstm_train`, `gru_train`, `lstm_step` and `gru_step` run an entry pair on device tensors that the caller placed; every output
starts as NaN (a sentinel for the steps' state rows), so an element that no thread wrote shows."""
import pytest
import torch

import test_gru_c2f_gpu as TG
import test_lstm_gpu as TL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRID_CAP = 4096
# (B, C, h, w) of the second-trip test: float4 items / scalar elements
BIG_VEC, BIG_SCALAR = (2, 64, 192, 704), (2, 4, 363, 363)


def _nan(shape, prep):
    return prep(torch.full(tuple(shape), float("nan"), device=DEV))


def lstm_train(d, prep=lambda x: x):
    """dc_lstm_handover_fwd, then _bwd on its pre.  d: a, h_prev, h_new, g_pre, g_up."""
    from depthcore import _lib
    L, ptr = _lib.lib(), _lib.ptr
    B, C, h, w = d["a"].shape
    pre, up = _nan(d["a"].shape, prep), _nan((B, C // 4, 2 * h, 2 * w), prep)
    _lib.check(L.dc_lstm_handover_fwd(ptr(d["a"]), ptr(d["h_prev"]), ptr(d["h_new"]), ptr(pre), ptr(up), B, C, h, w, _lib.stream(pre)),
               "dc_lstm_handover_fwd")
    g = [_nan(d["a"].shape, prep) for _ in range(3)]
    _lib.check(L.dc_lstm_handover_bwd(ptr(pre), ptr(d["g_pre"]), ptr(d["g_up"]), ptr(g[0]), ptr(g[1]), ptr(g[2]), B, C, h, w,
                                      _lib.stream(pre)), "dc_lstm_handover_bwd")
    return dict(pre=pre, up=up, d_a=g[0], d_h_prev=g[1], d_h_new=g[2])


def gru_train(d, prep=lambda x: x):
    """dc_gru_handover_fwd, then _bwd on its pre.  d: gates, h_prev, cnm, a, g_h_new, g_pre, g_up."""
    from depthcore import _lib
    L, ptr = _lib.lib(), _lib.ptr
    B, C, h, w = d["a"].shape
    h_new, pre, up = _nan(d["a"].shape, prep), _nan(d["a"].shape, prep), _nan((B, C // 4, 2 * h, 2 * w), prep)
    _lib.check(L.dc_gru_handover_fwd(ptr(d["gates"]), ptr(d["h_prev"]), ptr(d["cnm"]), ptr(d["a"]), ptr(h_new), ptr(pre), ptr(up), B, C, h,
                                     w, _lib.stream(pre)), "dc_gru_handover_fwd")
    g = [_nan(d["gates"].shape, prep)] + [_nan(d["a"].shape, prep) for _ in range(3)]
    _lib.check(L.dc_gru_handover_bwd(ptr(d["gates"]), ptr(d["h_prev"]), ptr(d["cnm"]), ptr(pre), ptr(d["g_h_new"]), ptr(d["g_pre"]),
                                     ptr(d["g_up"]), ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(g[3]), B, C, h, w, _lib.stream(pre)),
               "dc_gru_handover_bwd")
    return dict(h_new=h_new, pre=pre, up=up, d_gates=g[0], d_h_prev=g[1], d_cnm=g[2], d_a=g[3])


def lstm_step(d):
    """dc_lstm_infer_step on copies of the states.  d: cc, h, c, y, r."""
    from depthcore import ops
    B, C, hh, w = d["h"].shape
    h, c = d["h"].clone(), d["c"].clone()
    pre, up = _nan(h.shape, lambda x: x), _nan((B, C // 4, 2 * hh, 2 * w), lambda x: x)
    ops.lstm_infer_step(d["cc"], h, c, d["y"], d["r"], pre, up)
    return dict(h=h, c=c, pre=pre, up=up)


def gru_step(d):
    """dc_gru_c2f_infer_step on a copy of the state.  d: gates, cnm, h, y, r."""
    from depthcore import ops
    B, C, hh, w = d["h"].shape
    h = d["h"].clone()
    pre, up = _nan(h.shape, lambda x: x), _nan((B, C // 4, 2 * hh, 2 * w), lambda x: x)
    ops.gru_c2f_infer_step(d["gates"], d["cnm"], h, d["y"], d["r"], pre, up)
    return dict(h=h, pre=pre, up=up)


# ---- unaligned pointers, training entries --------------------------------------------------------------------------------------
def shifted(x):
    """test_lstm_infer_gpu.py's: the same values 4 bytes past a 16-byte boundary."""
    flat = torch.empty(x.numel() + 1, device=DEV)
    flat[1:].copy_(x.reshape(-1))
    v = flat[1:].view(x.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def test_unaligned_lstm_training_entries_take_the_scalar_form():
    """(2, 8, 2, 4) allows float4, but every tensor, the gradients included, starts 4 bytes past a 16-byte boundary."""
    shape = (2, 8, 2, 4)
    a, hp, hn, g_pre, g_up = TL._hand_inputs(*shape, False, 2100)
    ref = TL._hand_oracle(a, hp, hn, g_pre, g_up, torch.float64)
    base = TL._hand_oracle(a, hp, hn, g_pre, g_up, torch.float32)
    d = {k: v.to(DEV) for k, v in dict(a=a, h_prev=hp, h_new=hn, g_pre=g_pre, g_up=g_up).items()}
    got = lstm_train({k: shifted(v) for k, v in d.items()}, prep=shifted)
    assert all(v.data_ptr() % 16 == 4 for v in got.values())
    TL._judge("lstm hand-over shifted %s" % (shape,), got, base, ref)
    aligned = lstm_train(d)
    assert all(v.data_ptr() % 16 == 0 for v in list(d.values()) + list(aligned.values()))
    for k in ref:
        assert torch.equal(got[k], aligned[k]), k                            # the two forms agree bit for bit


def test_unaligned_gru_training_entries_take_the_scalar_form():
    shape = (2, 8, 2, 4)
    t, cots = TG._inputs(*shape, False, 2200)
    ref, base = TG._oracle(t, cots), TG._composition(t, cots)               # test_gru_c2f_gpu.py's rule: the launches it replaces
    d = {k: v.to(DEV) for k, v in t.items()}
    d.update({"g_" + k: v.to(DEV) for k, v in cots.items()})
    got = gru_train({k: shifted(v) for k, v in d.items()}, prep=shifted)
    assert all(v.data_ptr() % 16 == 4 for v in got.values())
    TL._judge("gru hand-over shifted %s" % (shape,), got, base, ref)
    aligned = gru_train(d)
    assert all(v.data_ptr() % 16 == 0 for v in list(d.values()) + list(aligned.values()))
    for k in TG.OUTS:
        assert torch.equal(got[k], aligned[k]), k


# ---- the second trip of the grid-stride loop ------------------------------------------------------------------------------------
def test_big_shapes_are_what_the_comment_says():
    cap = GRID_CAP * TL._block()
    assert cap == 1048576
    B, C, h, w = BIG_VEC
    assert C % 4 == 0 and w % 4 == 0 and B * (C // 4) * h * (w // 4) == 1081344 > cap > 540672 == (C // 4) * h * (w // 4)
    B, C, h, w = BIG_SCALAR
    assert C % 4 == 0 and w % 4 and B * C * h * w == 1054152 > cap > 527076 == C * h * w


def big_inputs(shape, seed):
    """Random device inputs of the six entries at one shape -> (lstm training, gru training, lstm step, gru step) dicts."""
    B, C, h, w = shape
    g = torch.Generator(device=DEV).manual_seed(seed)

    def rn(*s):
        return torch.randn(*s, device=DEV, generator=g)
    state, up = (B, C, h, w), (B, C // 4, 2 * h, 2 * w)
    gates = torch.sigmoid(2.0 * rn(B, 2 * C, h, w))
    cnm = torch.tanh(rn(*state))
    lt = dict(a=rn(*state), h_prev=rn(*state), h_new=rn(*state), g_pre=rn(*state), g_up=rn(*up))
    gt = dict(gates=gates, h_prev=lt["h_prev"], cnm=cnm, a=lt["a"], g_h_new=rn(*state), g_pre=lt["g_pre"], g_up=lt["g_up"])
    ls = dict(cc=2.0 * rn(B, 4 * C, h, w), h=lt["h_prev"], c=rn(*state), y=lt["a"], r=lt["h_new"])
    gs = dict(gates=gates, cnm=cnm, h=lt["h_prev"], y=lt["a"], r=lt["h_new"])
    return lt, gt, ls, gs


@pytest.mark.parametrize("shape", [BIG_VEC, BIG_SCALAR], ids=["float4", "scalar"])
def test_second_trip_of_the_grid_stride_loop(shape):
    """All six entries: one B = 2 call (threads take a second item) against two B = 1 calls on its rows (they do not)."""
    for run, d in zip((lstm_train, gru_train, lstm_step, gru_step), big_inputs(shape, 2300 + shape[1])):
        both = run(d)
        for i in range(shape[0]):
            row = run({k: v[i:i + 1] for k, v in d.items()})
            for k, v in row.items():
                assert not bool(torch.isnan(v).any()), (run.__name__, k, i)
                assert torch.equal(both[k][i:i + 1], v), (run.__name__, k, i)
            del row
        del both
