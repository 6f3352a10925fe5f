"""The inference form of a ConvLSTM v8 frame (dc_lstm_infer_step: cell update + `+ r` + hand-over in one launch, states in
place) and the window predictor built on it (depthcore.evaluate.WindowPredictor / window_groups).

Kernel: against tests/lstm_ref.py (`lstm_cell`, then `handover` on a = y + r) in fp64 under tests/test_lstm_gpu.py's rule -- per
output tensor the Euclidean norm of the error is at most FACTOR = 4 times that of the same statement in fp32 torch on the CPU;
each ratio is printed before it is judged.
Predictor: against lstm_ref.v8_forward / v8_sequence in fp64; the max-abs error may be at most 2 times that of the composition
that existed before it (ConvGRUBlocks_v8.forward / run_sequence), the bound test_gru_infer_gpu.py::test_lockstep_vs_oracle gives
the v5 path: a batch changes the convolutions' tiling, not their precision."""
import numpy as np
import pytest
import torch

import lstm_ref as LR
from test_lstm_gpu import FACTOR, _judge

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENT = -7.0
# (B, C, hh, w): scalar with an odd w; float4; one pixel; float4 with 306 items = one full block of dc_lstm_block() threads and a
# ragged second; scalar with 468 elements = one full block and a ragged second
SHAPES = [(2, 4, 3, 5), (1, 8, 2, 4), (2, 4, 1, 1), (1, 8, 9, 68), (1, 4, 9, 13)]


def test_ragged_shapes_are_what_the_comment_says():
    from depthcore import _lib
    blk = _lib.lib().dc_lstm_block()
    assert FACTOR == 4.0
    assert 68 % 4 == 0 and 8 % 4 == 0 and 1 * (8 // 4) * 9 * (68 // 4) == 306 and blk < 306 < 2 * blk and 306 % blk
    assert 13 % 4 and 1 * 4 * 9 * 13 == 468 and blk < 468 < 2 * blk and 468 % blk
    assert 5 % 4 and 4 % 4 == 0 and 1 % 4                                   # (2,4,3,5) and (2,4,1,1) scalar, (1,8,2,4) float4


def _inputs(B, C, hh, w, seed):
    g = torch.Generator().manual_seed(seed)
    t = dict(cc=2.0 * torch.randn(B, 4 * C, hh, w, generator=g))            # N(0, 2^2): saturated and unsaturated gates
    for k in ("h", "c", "y", "r"):
        t[k] = torch.randn(B, C, hh, w, generator=g)
    return t


def _oracle(t, dtype):
    cc, h, c, y, r = (t[k].to(dtype) for k in ("cc", "h", "c", "y", "r"))
    hn, cn = LR.lstm_cell(cc, c)
    pre, up = LR.handover(y + r, h, hn)
    return dict(h=hn, c=cn, pre=pre, up=up)


def _run(t, S=None, y=True, pre=True, up=True, prep=lambda x: x):
    """One call on device copies (state buffers of S rows; `prep` places every tensor) -> dict(h, c, pre, up) of the buffers."""
    from depthcore import ops
    B, C, hh, w = t["h"].shape
    S = S or B
    dev = {k: prep(v.to(DEV)) for k, v in t.items() if k in ("cc", "y", "r")}
    for k in ("h", "c"):
        full = torch.full((S, C, hh, w), SENT, device=DEV)
        full[:B] = t[k].to(DEV)
        dev[k] = prep(full)
    out_pre = prep(torch.full((S, C, hh, w), SENT, device=DEV)) if pre else None
    out_up = prep(torch.full((S, C // 4, 2 * hh, 2 * w), SENT, device=DEV)) if up else None
    ops.lstm_infer_step(dev["cc"], dev["h"], dev["c"], dev["y"] if y else None, dev["r"] if y else None, out_pre, out_up, B)
    torch.cuda.synchronize()
    return dict(h=dev["h"], c=dev["c"], pre=out_pre, up=out_up)


def _rows(got, B):
    return {k: (None if v is None else v[:B]) for k, v in got.items()}


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_vs_fp64(shape):
    B, C, hh, w = shape
    t = _inputs(B, C, hh, w, 500 + B + 7 * C + hh * w)
    ref, base = _oracle(t, torch.float64), _oracle(t, torch.float32)
    if ref["pre"].numel() > 16:
        assert 0.2 < float((ref["pre"] == 0).double().mean()) < 0.8          # both sides of the ReLU occur
    a, b = _run(t), _run(t)
    assert a["up"].shape == (B, C // 4, 2 * hh, 2 * w)
    _judge("infer %s" % (shape,), a, base, ref)
    for k in ref:
        assert torch.equal(a[k], b[k]), k                                    # two runs from the same inputs: the same bits


def test_the_step_is_the_training_launches_bit_for_bit():
    """The same expressions in the same order: h', c', pre and up of the step are those of ops.lstm_cell followed by
    ops.lstm_handover on a = y + r."""
    from depthcore import ops
    for shape in ((1, 8, 9, 68), (2, 4, 3, 5)):
        t = _inputs(*shape, 550)
        got = _run(t)
        d = {k: v.to(DEV) for k, v in t.items()}
        hn, cn = ops.lstm_cell(d["cc"], d["c"])
        pre, up = ops.lstm_handover(d["y"] + d["r"], d["h"], hn)
        assert torch.equal(got["h"], hn) and torch.equal(got["c"], cn)
        assert torch.equal(got["pre"], pre) and torch.equal(got["up"], up)


@pytest.mark.parametrize("shape", [(2, 8, 2, 4), (2, 4, 3, 5)])             # float4, scalar
def test_rows_behind_B_are_not_touched(shape):
    B, C, hh, w = shape
    t = _inputs(B, C, hh, w, 600 + C)
    ref, base = _oracle(t, torch.float64), _oracle(t, torch.float32)
    got = _run(t, S=3)
    _judge("prefix %s" % (shape,), _rows(got, B), base, ref)
    for k in ("h", "c", "pre", "up"):
        assert bool((got[k][B:] == SENT).all()), k                           # bitwise the sentinel
    assert torch.equal(_rows(got, B)["h"], _run(t)["h"]) and torch.equal(_rows(got, B)["c"], _run(t)["c"])


def test_unaligned_pointers_take_the_scalar_form():
    """(2, 8, 2, 4) allows float4, but every tensor starts 4 bytes past a 16-byte boundary: a float4 access there would be
    misaligned, so the call must fall back to scalar accesses."""
    def shifted(x):
        flat = torch.empty(x.numel() + 1, device=DEV)
        flat[1:].copy_(x.reshape(-1))
        v = flat[1:].view(x.shape)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v
    t = _inputs(2, 8, 2, 4, 700)
    ref, base = _oracle(t, torch.float64), _oracle(t, torch.float32)
    got = _run(t, prep=shifted)
    _judge("shifted (2, 8, 2, 4)", got, base, ref)


@pytest.mark.parametrize("shape", [(2, 8, 2, 4), (2, 4, 3, 5)])             # float4, scalar
def test_up_lands_in_the_upper_channel_half(shape):
    """up_bstride = 2 C hh w: the launch writes into the upper channel half of a (B, 2 C/4, 2hh, 2w) buffer -- the next finer
    scale's cat(dec, up) -- and leaves the lower half alone."""
    from depthcore import ops
    B, C, hh, w = shape
    t = _inputs(B, C, hh, w, 800 + C)
    plain = _run(t)
    dev = {k: v.to(DEV) for k, v in t.items()}
    wide = torch.full((B, 2 * (C // 4), 2 * hh, 2 * w), SENT, device=DEV)
    up = wide[:, C // 4:]
    assert up.stride(0) == 2 * C * hh * w and not up.is_contiguous()
    ops.lstm_infer_step(dev["cc"], dev["h"], dev["c"], dev["y"], dev["r"], None, up)
    torch.cuda.synchronize()
    assert bool((wide[:, :C // 4] == SENT).all())
    assert torch.equal(wide[:, C // 4:], plain["up"])
    assert torch.equal(dev["h"], plain["h"]) and torch.equal(dev["c"], plain["c"])


@pytest.mark.parametrize("shape", [(1, 8, 9, 68), (2, 4, 3, 5)])            # float4, scalar
def test_null_outputs_leave_the_state_update_alone(shape):
    """State-only call (y = r = pre = up = NULL: scale 0 on every frame but a window's last) and pre without up (scale 0 on the
    last): h and c are the full call's, bit for bit."""
    B, C, hh, w = shape
    t = _inputs(B, C, hh, w, 900 + C)
    full = _run(t)
    state_only = _run(t, y=False, pre=False, up=False)
    no_up = _run(t, up=False)
    for got in (state_only, no_up):
        assert torch.equal(got["h"], full["h"]) and torch.equal(got["c"], full["c"])
    assert torch.equal(no_up["pre"], full["pre"]) and no_up["up"] is None and state_only["pre"] is None


def test_refusals():
    from depthcore import _lib
    L = _lib.lib()
    B, C, hh, w = 2, 8, 2, 4
    names = ("cc", "y", "r", "h", "c", "pre", "up")
    hold = {k: torch.zeros(B, 4 * C, hh, w, device=DEV) for k in names}      # real memory behind every pointer that is passed
    ok = dict({k: v.data_ptr() for k, v in hold.items()}, stride=C * hh * w, B=B, C=C, hh=hh, w=w)

    def call(**kw):
        a = dict(ok, **kw)
        return L.dc_lstm_infer_step(a["cc"], a["y"], a["r"], a["h"], a["c"], a["pre"], a["up"], a["stride"], a["B"], a["C"], a["hh"],
                                    a["w"], None)
    assert call() == 0
    for kw in (dict(B=0), dict(C=0), dict(hh=0), dict(w=0), dict(B=-1), dict(cc=None), dict(h=None), dict(c=None),
               dict(y=None), dict(r=None),                                   # exactly one of y / r
               dict(y=None, r=None), dict(y=None, r=None, up=None), dict(y=None, r=None, pre=None),      # pre or up without y
               dict(C=6, hh=1, w=1), dict(stride=C * hh * w - 1),            # up with C % 4 != 0 / a stride below a row
               dict(B=1 << 9, C=1 << 8, hh=1 << 6, w=1 << 6, up=None, pre=None)):        # cc: 4 B C hh w = 2^31 elements
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()                                                 # nothing was launched, nothing is pending
    assert all(bool(torch.isfinite(v).all()) for v in hold.values())


# ---- the predictor ------------------------------------------------------------------------------------------------------------
H, W = 32, 64                                                                # scale 3 is 4 x 8


def _v8(seed=5, height=H, width=W):
    import networks
    torch.manual_seed(seed)
    blk = networks.ConvGRUBlocks_v8((3, 3), True, "cpu", height=height, width=width).to(DEV)
    for p in blk.parameters():                                               # the learned initial states too: h0 and c0 count
        p.data.normal_(0, 0.05)
    return blk


def _maps(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, LR.NUM_CH_DEC[s], H >> s, W >> s, generator=g).to(DEV) for s in range(4)]


def _state64(blk):
    return {k: v.detach().cpu().double() for k, v in blk.state_dict().items()}


def test_advance_vs_oracle_and_existing_forward():
    """One advance_maps at B = 3 on a predictor of 4 streams: the new (h, c) of every scale against lstm_ref.v8_forward in fp64,
    at most 2 x the max-abs error of ConvGRUBlocks_v8.forward on the same batch; stream 3 stays at (h0, c0), bit for bit."""
    from depthcore import evaluate as E
    blk, B = _v8(), 3
    dec = _maps(B, 7)
    st = _state64(blk)
    states = [(st["cgru_%d.h0_layer1" % s], st["cgru_%d.c0_layer1" % s]) for s in range(4)]
    want, _ = LR.v8_forward([d.cpu().double() for d in dec], states, st)
    with torch.no_grad():
        mod, _ = blk({("disp", s): dec[s] for s in range(4)}, blk.initial_states())
    wp = E.WindowPredictor(None, None, blk, streams=4)
    assert wp.advance_maps(dec) is None
    torch.cuda.synchronize()
    for s in range(4):
        for k, name in enumerate("hc"):
            buf = (wp.h, wp.c)[k][s]
            e_wp = float((buf[:B].cpu().double() - want[s][k]).abs().max())
            e_mod = float((mod[s][k].cpu().double() - want[s][k]).abs().max())
            print("scale %d %s: predictor %.3e  forward %.3e" % (s, name, e_wp, e_mod))
            assert e_wp <= 2 * e_mod, (s, name, e_wp, e_mod)
            init = getattr(blk.cells()[s], "%s0_layer1" % name).detach()
            assert torch.equal(buf[B:], init)                                # stream 3 did not move
            assert not buf.requires_grad


def _windows(blk, wins, streams, wp=None):
    """Every window's final scale-0 disparity through advance_maps / step_maps on window_groups' schedule -> list in input order."""
    from depthcore import evaluate as E
    lengths = [w[0].shape[0] for w in wins]
    wp = wp or E.WindowPredictor(None, None, blk, streams=streams)
    got = [None] * len(wins)
    for ids, widths in E.window_groups(lengths, streams):
        wp.reset()
        L = len(widths)
        for j, B in enumerate(widths):
            at = [j - (L - lengths[c]) for c in ids[:B]]
            batch = [torch.cat([wins[c][s][t:t + 1] for c, t in zip(ids[:B], at)]) for s in range(4)]
            if j < L - 1:
                wp.advance_maps(batch)
            else:
                disp = wp.step_maps(batch).clone()
        assert disp.shape == (len(ids), 1, H, W) and not disp.requires_grad
        for b, c in enumerate(ids):
            got[c] = disp[b]
    return got, wp


@pytest.fixture(scope="module")
def window_case():
    """Windows of lengths [3, 1, 2] (unsorted), and per window the fp64 oracle's and today's run_sequence's last scale-0 disparity."""
    blk = _v8()
    st = _state64(blk)
    wins = [_maps(n, 30 + i) for i, n in enumerate((3, 1, 2))]
    want = [LR.v8_sequence([d.cpu().double() for d in w], st)[0][-1] for w in wins]
    with torch.no_grad():
        seq = [blk.run_sequence({("disp", s): w[s] for s in range(4)})[("disp", 0)][-1].clone() for w in wins]
    return blk, wins, want, seq


def test_windows_vs_oracle(window_case):
    """Per window: max-abs error of the lockstep path against the fp64 oracle <= 2 x that of run_sequence at batch 1, and within
    rtol = atol = 1e-3.  Measured values: DESIGN 4s."""
    blk, wins, want, seq = window_case
    got, wp = _windows(blk, wins, streams=3)
    for c in range(len(wins)):
        e_lock = float((got[c].cpu().double() - want[c]).abs().max())
        e_seq = float((seq[c].cpu().double() - want[c]).abs().max())
        print("window %d (%d frames): lockstep %.3e  run_sequence %.3e" % (c, wins[c][0].shape[0], e_lock, e_seq))
        assert e_lock <= 2 * e_seq, (c, e_lock, e_seq)
        np.testing.assert_allclose(got[c].cpu().numpy(), want[c].float().numpy(), rtol=1e-3, atol=1e-3)
    # a second round on the same predictor (every group starts with reset()): the same bits
    again, _ = _windows(blk, wins, streams=3, wp=wp)
    assert all(torch.equal(a, b) for a, b in zip(again, got))
    # three consecutive groups of one window each are the same evaluation
    narrow, _ = _windows(blk, wins, streams=1)
    for a, b in zip(narrow, got):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-3, atol=1e-3)


def test_hygiene_and_public_methods():
    """With real networks at 64 x 128 (the decoder's coarsest map needs two rows): training flags and every state_dict entry
    unchanged, outputs without grad, flags restored when batch_fn raises; advance / step are what predict_disparities_windows runs."""
    import networks
    from depthcore import evaluate as E
    Hn, Wn = 64, 128
    torch.manual_seed(6)
    enc = networks.ResnetEncoder(18, False).to(DEV)
    dec = networks.DepthDecoder(enc.num_ch_enc).to(DEV)
    blk = _v8(7, Hn, Wn)
    enc.train()
    dec.eval()
    blk.train()
    enc.encoder.layer2.train(False)
    nets = (enc, dec, blk)
    flags = [m.training for net in nets for m in net.modules()]
    state = {(i, k): v.clone() for i, net in enumerate(nets) for k, v in net.state_dict().items()}
    assert sum(1 for (_, k) in state if k.endswith("c0_layer1")) == 4 and any(k.endswith("running_var") for (_, k) in state)
    g = torch.Generator().manual_seed(8)
    lengths = [2, 1, 3]
    wins = [torch.rand(n, 3, Hn, Wn, generator=g).to(DEV) for n in lengths]
    calls = []

    def batch_fn(j, ids, frame_of):
        calls.append((j, list(ids), list(frame_of)))
        return torch.cat([wins[c][t:t + 1] for c, t in zip(ids, frame_of)])
    wide = E.predict_disparities_windows(enc, dec, blk, lengths, batch_fn, streams=3)
    assert calls == [(0, [2], [0]), (1, [2, 0], [1, 0]), (2, [2, 0, 1], [2, 1, 0])]
    narrow = E.predict_disparities_windows(enc, dec, blk, lengths, batch_fn, streams=2)             # two groups
    torch.cuda.synchronize()
    assert [m.training for net in nets for m in net.modules()] == flags
    for (i, k), v in state.items():
        assert torch.equal(nets[i].state_dict()[k], v), k
    assert wide.shape == narrow.shape == (3, 1, Hn, Wn) and not wide.requires_grad and not narrow.requires_grad
    np.testing.assert_allclose(narrow.cpu().numpy(), wide.cpu().numpy(), rtol=1e-3, atol=1e-3)
    # the public methods on the same schedule: the same bits; the streams behind B stay
    wp = E.WindowPredictor(enc, dec, blk, streams=3)
    assert wp.advance(wins[2][0:1]) is None
    assert torch.equal(wp.h[0][1:], blk.cgru_0.h0_layer1.detach().expand(2, -1, -1, -1))
    wp.advance(torch.cat([wins[2][1:2], wins[0][0:1]]))
    disp = wp.step(torch.cat([wins[2][2:3], wins[0][1:2], wins[1][0:1]]))
    assert not disp.requires_grad and torch.equal(disp, wide[[2, 0, 1]])
    assert [m.training for net in nets for m in net.modules()] == flags

    class Boom(RuntimeError):
        pass

    def bad(j, ids, frame_of):
        if j == 1:
            raise Boom()
        return batch_fn(j, ids, frame_of)
    with pytest.raises(Boom):
        E.predict_disparities_windows(enc, dec, blk, lengths, bad, streams=3)
    assert [m.training for net in nets for m in net.modules()] == flags
    for (i, k), v in state.items():
        assert torch.equal(nets[i].state_dict()[k], v), k
    with pytest.raises(ValueError):
        E.predict_disparities_windows(enc, dec, blk, [], batch_fn, streams=2)
