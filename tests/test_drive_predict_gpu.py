"""Drive inference (depthcore.evaluate.predict_disparities_drive) for the three recurrent front-ends, with a seeded resnet18 at
64 x 96, non-zero learned initial states and synthetic frames.

v8 / v10.  The drive path against predict_disparities_windows on the explicit windows (frame t: frames max(0, t - n_prev) .. t),
both against the project's fp64 statements (tests/lstm_ref.py, tests/gru_c2f_ref.py) of every window, evaluated in fp64 on the
decoder maps of ONE encoder / decoder pass over the drive.  With e_win the window path's error against fp64 and e_drive the drive
path's (max-abs, relative to the largest reference entry: layer_ops_cases.rel_err), the gate is

    e_drive <= 2 e_win + 4 * 2^-23.

The two paths run the same kernels on the same values and differ only in which batch a frame is convolved in, so a different
tile route (another summation order) can be selected: a factor 2 covers that, and four units of fp32 roundoff keep the gate
meaningful where e_win is itself a few ulps.  A wrong row -- an off-by-one in the ring or in the plan -- shows at 1e-2 and cannot
pass.  The statements are plain torch and run in fp64 on the device (all windows of one length as one batch); both figures are
printed before they are judged and recorded in DESIGN 4u.

v5.  The chunked drive path against SequencePredictor(streams=1) stepped frame by frame, under the same gate; the fp64 figure is
oracle/gru_ref.run_gru_v5 (the statement tests/test_gru_infer_gpu.py uses) on the encoder features of one pass over the drive,
decoded by the decoder at the drive's batch (the decoder has no fp64 statement; both paths see the same one)."""
import pytest
import torch

import gru_c2f_ref as GR
import lstm_ref as LR
from layer_ops_cases import rel_err
from oracle import gru_ref as G

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
H, W = 64, 96
MIN_DEPTH, MAX_DEPTH = 0.1, 100.0
ULP4 = 4 * 2.0 ** -23


def _gate(what, e_drive, e_win):
    print("\n%s: drive %.3e  window path %.3e  (gate %.3e)" % (what, e_drive, e_win, 2 * e_win + ULP4))
    assert e_drive <= 2 * e_win + ULP4, (what, e_drive, e_win)


def _scaled(disp):
    """disp_to_depth's scaled disparity, in the tensor's own precision."""
    lo, hi = 1.0 / MAX_DEPTH, 1.0 / MIN_DEPTH
    return lo + (hi - lo) * disp


def _front(kind, seed):
    import networks
    torch.manual_seed(seed)
    if kind == "v8":
        blk = networks.ConvGRUBlocks_v8((3, 3), True, "cpu", height=H, width=W)
    elif kind == "v10":
        blk = networks.ConvGRUBlocks_v9((3, 3), True, "cpu", attention=False, height=H, width=W)
    else:
        blk = networks.ConvGRUBlocks_v5(kernel_size=(3, 3), bias=True, device="cpu", height=H, width=W)
    blk = blk.to(DEV)
    for p in blk.parameters():                                   # the learned initial states too: they are not zero
        p.data.normal_(0, 0.05)
    return blk


@pytest.fixture(scope="module")
def nets():
    import networks
    torch.manual_seed(11)
    enc = networks.ResnetEncoder(18, False).to(DEV)
    dec = networks.DepthDecoder(enc.num_ch_enc).to(DEV)
    g = torch.Generator().manual_seed(12)
    frames = torch.rand(40, 3, H, W, generator=g).to(DEV)
    return enc, dec, {k: _front(k, 13 + i) for i, k in enumerate(("v8", "v10", "v5"))}, frames


def _batch_fn(frames, calls=None):
    def fn(lo, hi):
        if calls is not None:
            calls.append((lo, hi))
        return frames[lo:hi]
    return fn


def _windows(n, n_prev):
    return [list(range(max(0, t - n_prev), t + 1)) for t in range(n)]


def _window_path(enc, dec, front, frames, n_prev, streams):
    from depthcore import evaluate as E
    wins = _windows(frames.shape[0], n_prev)

    def batch(j, ids, frame_of):
        idx = torch.tensor([wins[c][f] for c, f in zip(ids, frame_of)], device=DEV)
        return frames.index_select(0, idx)
    return E.predict_disparities_windows(enc, dec, front, [len(w) for w in wins], batch, MIN_DEPTH, MAX_DEPTH, streams)


def _reference(enc, dec, front, frames, n_prev):
    """The fp64 statement of every window of the drive -> (n,1,H,W) scaled disparities (fp64, on the device).  The decoder maps
    are those of one pass over all frames; windows of one length advance as one batch of the statement."""
    from depthcore import evaluate as E
    forward = LR.v8_forward if hasattr(front.cells()[0], "clstm_1") else GR.v10_forward
    st = {k: v.detach().double() for k, v in front.state_dict().items()}
    with E._EvalMode(enc, dec):
        out = dec(enc(frames), True)
    maps = [out[("disp", s)].double() for s in range(4)]
    n = frames.shape[0]
    want = torch.empty(n, 1, H, W, dtype=torch.float64, device=DEV)
    by_length = {}
    for t in range(n):
        by_length.setdefault(min(t, n_prev) + 1, []).append(t)
    for L, targets in by_length.items():
        if forward is LR.v8_forward:
            states = [(st["cgru_%d.h0_layer1" % s], st["cgru_%d.c0_layer1" % s]) for s in range(4)]
        else:
            states = [st["cgru_%d.h0_layer1" % s] for s in range(4)]
        for j in range(L):
            idx = torch.tensor([t - (L - 1) + j for t in targets], device=DEV)
            states, disp = forward([m.index_select(0, idx) for m in maps], states, st)
        want[torch.tensor(targets, device=DEV)] = disp[0]
    return _scaled(want)


@pytest.fixture(scope="module")
def window_refs(nets):
    """Per front-end: the fp64 reference and the window path's prediction of the 14-frame and of the 40-frame drive (n_prev = 3,
    streams = 4), computed once and left unchanged."""
    enc, dec, fronts, frames = nets
    refs = {}
    for kind in ("v8", "v10"):
        for n in (14, 40) if kind == "v8" else (14,):
            refs[(kind, n)] = (_reference(enc, dec, fronts[kind], frames[:n], 3), _window_path(enc, dec, fronts[kind], frames[:n], 3, 4))
    return refs


@pytest.mark.parametrize("chunk", [5, 16])
@pytest.mark.parametrize("kind", ["v8", "v10"])
def test_drive_vs_windows(nets, window_refs, kind, chunk):
    """14 frames, n_prev = 3, streams = 4: groups (0,3) ragged, (3,7), (7,11), (11,14); chunks of 5 cut through the groups."""
    from depthcore import evaluate as E
    enc, dec, fronts, frames = nets
    want, win = window_refs[(kind, 14)]
    calls = []
    got = E.predict_disparities_drive(enc, dec, fronts[kind], 14, _batch_fn(frames[:14], calls), n_prev=3, streams=4, chunk=chunk,
                                      min_depth=MIN_DEPTH, max_depth=MAX_DEPTH)
    assert got.shape == (14, 1, H, W) and got.dtype == torch.float32 and got.is_cuda and not got.requires_grad
    assert calls == [(lo, min(lo + chunk, 14)) for lo in range(0, 14, chunk)]          # every frame asked for once, in order
    e_win = rel_err(win, want.cpu())
    _gate("%s chunk %d" % (kind, chunk), rel_err(got, want.cpu()), e_win)
    # the windows matter: frame 5 predicted from its own frame alone is another picture, far outside the gate
    alone = E.predict_disparities_drive(enc, dec, fronts[kind], 14, _batch_fn(frames[:14]), n_prev=0, streams=4, chunk=chunk)
    e_alone = rel_err(alone[5:6], want[5:6].cpu())
    print("frame 5 without its window: %.3e" % e_alone)
    assert e_alone > 8 * (2 * e_win + ULP4)


@pytest.mark.parametrize("kind", ["v8", "v10"])
def test_drive_shorter_than_a_window(nets, kind):
    """n_frames = 3 < n_prev = 6: one ragged group, a ring of three frames."""
    from depthcore import evaluate as E
    enc, dec, fronts, frames = nets
    want = _reference(enc, dec, fronts[kind], frames[:3], 6)
    win = _window_path(enc, dec, fronts[kind], frames[:3], 6, 16)
    got = E.predict_disparities_drive(enc, dec, fronts[kind], 3, _batch_fn(frames[:3]), n_prev=6, streams=16, chunk=16)
    assert got.shape == (3, 1, H, W)
    _gate("%s 3 frames" % kind, rel_err(got, want.cpu()), rel_err(win, want.cpu()))


def test_every_frame_is_encoded_once(nets):
    """A forward hook on the encoder counts input frames: 14 for the drive, 1 + 2 + 3 + 11 * 4 = 50 for the window path."""
    from depthcore import evaluate as E
    enc, dec, fronts, frames = nets
    seen = []
    hook = enc.register_forward_hook(lambda m, inp, out: seen.append(inp[0].shape[0]))
    try:
        for kind in ("v8", "v10"):
            for chunk in (5, 16):
                del seen[:]
                E.predict_disparities_drive(enc, dec, fronts[kind], 14, _batch_fn(frames[:14]), n_prev=3, streams=4, chunk=chunk)
                assert sum(seen) == 14 and len(seen) == -(-14 // chunk), (kind, chunk, seen)
            del seen[:]
            _window_path(enc, dec, fronts[kind], frames[:14], 3, 4)
            assert sum(seen) == 50, (kind, seen)
        del seen[:]
        E.predict_disparities_drive(enc, dec, fronts["v5"], 14, _batch_fn(frames[:14]), chunk=5)
        assert seen == [5, 5, 4]
    finally:
        hook.remove()


def test_ring_reuse(nets, window_refs):
    """40 frames, streams = 4, chunk = 4, n_prev = 3: a ring of 11 frames is written more than three times over."""
    from depthcore import evaluate as E
    enc, dec, fronts, frames = nets
    want, win = window_refs[("v8", 40)]
    got = E.predict_disparities_drive(enc, dec, fronts["v8"], 40, _batch_fn(frames), n_prev=3, streams=4, chunk=4)
    _gate("v8 40 frames", rel_err(got, want.cpu()), rel_err(win, want.cpu()))
    # other cuts of the same drive: chunks longer than the groups, and groups longer than the chunks
    for streams, chunk in ((4, 7), (3, 2)):
        other = E.predict_disparities_drive(enc, dec, fronts["v8"], 40, _batch_fn(frames), n_prev=3, streams=streams, chunk=chunk)
        _gate("v8 40 frames, streams %d chunk %d" % (streams, chunk), rel_err(other, want.cpu()), rel_err(win, want.cpu()))


def test_map_ring_slices():
    """The ring on its own: any run of up to `mirror + 1` consecutive frames is one slice that holds those frames, also across
    the ring's end and after several rounds; gathered rows are the same frames."""
    from depthcore import evaluate as E
    like = [torch.zeros(1, 2, 3, 4, device=DEV), torch.zeros(1, 1, 2, 2, device=DEV)]
    ring = E._MapRing(like, 7, 2)

    def frame(f):
        return [torch.full((1,) + tuple(m.shape[1:]), float(f), device=DEV) for m in like]
    hi = 0
    for n in (3, 4, 5, 2, 7, 1, 6):                                          # chunks of every size up to the ring's
        ring.store(hi, [torch.cat(x) for x in zip(*[frame(f) for f in range(hi, hi + n)])])
        hi += n
        for first in range(max(0, hi - 7), hi):
            for B in range(1, min(3, hi - first) + 1):
                for m in ring.run(first, B):
                    assert m.is_contiguous() and m.shape[0] == B
                    assert [float(v) for v in m.reshape(B, -1)[:, 0]] == list(range(first, first + B)), (hi, first, B)
                    assert bool((m.reshape(B, -1) == m.reshape(B, -1)[:, :1]).all())
        rows = list(range(max(0, hi - 7), hi))[::-1]
        assert [float(v) for v in ring.rows(rows)[0].reshape(len(rows), -1)[:, 0]] == rows


@pytest.fixture(scope="module")
def v5_refs(nets):
    """The fp64 figure of the 14-frame drive and SequencePredictor(streams=1) stepped frame by frame."""
    from depthcore import evaluate as E
    enc, dec, fronts, frames = nets
    blk, x = fronts["v5"], frames[:14]
    st = {k: v.detach().double() for k, v in blk.state_dict().items()}
    with E._EvalMode(enc, dec):
        fused = G.run_gru_v5([f.double() for f in enc(x)], st)
        want = _scaled(dec([f.float() for f in fused])[("disp", 0)].double())
    sp = E.SequencePredictor(enc, blk, dec, streams=1, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH)
    seq = torch.cat([sp.step(x[t:t + 1]) for t in range(14)])
    return want.cpu(), seq


@pytest.mark.parametrize("chunk", [1, 5, 14, 16])
def test_v5_drive_vs_sequence_predictor(nets, v5_refs, chunk):
    from depthcore import evaluate as E
    enc, dec, fronts, frames = nets
    want, seq = v5_refs
    got = E.predict_disparities_drive(enc, dec, fronts["v5"], 14, _batch_fn(frames[:14]), chunk=chunk, min_depth=MIN_DEPTH,
                                      max_depth=MAX_DEPTH)
    assert got.shape == (14, 1, H, W) and not got.requires_grad
    _gate("v5 chunk %d" % chunk, rel_err(got, want), rel_err(seq, want))


def test_v5_state_crosses_chunk_edges(nets, v5_refs):
    """chunk = 5 against chunk = 14 (one chunk): equal within the gate; a state that restarted at a chunk edge would not be --
    frame 5 run from the learned h0 is another picture."""
    from depthcore import evaluate as E
    enc, dec, fronts, frames = nets
    want, seq = v5_refs
    a = E.predict_disparities_drive(enc, dec, fronts["v5"], 14, _batch_fn(frames[:14]), chunk=5)
    b = E.predict_disparities_drive(enc, dec, fronts["v5"], 14, _batch_fn(frames[:14]), chunk=14)
    _gate("v5 chunk 5 vs 14", rel_err(a, want), rel_err(b, want))
    _gate("v5 chunk 14 vs 5", rel_err(b, want), rel_err(a, want))
    restarted = E.predict_disparities_drive(enc, dec, fronts["v5"], 9, _batch_fn(frames[5:14]), chunk=9)
    e_restart = rel_err(restarted[0:1], want[5:6])
    print("frame 5 from a restarted state: %.3e" % e_restart)
    assert e_restart > 8 * (2 * rel_err(b, want) + ULP4)


@pytest.mark.parametrize("kind", ["v5", "v8", "v10"])
def test_networks_are_left_as_they_were(nets, kind):
    from depthcore import evaluate as E
    enc, dec, fronts, frames = nets
    blk = fronts[kind]
    three = (enc, dec, blk)
    before = [[m.training for m in net.modules()] for net in three]
    try:
        enc.train()
        dec.eval()
        blk.train()
        enc.encoder.layer2.train(False)
        flags = [m.training for net in three for m in net.modules()]
        state = {(i, k): v.clone() for i, net in enumerate(three) for k, v in net.state_dict().items()}
        assert any(k.endswith("h0_layer1") for (_, k) in state) and any(k.endswith("running_var") for (_, k) in state)
        grad = torch.is_grad_enabled()
        pred = E.predict_disparities_drive(enc, dec, blk, 6, _batch_fn(frames[:6]), n_prev=2, streams=2, chunk=4)
        torch.cuda.synchronize()
        assert not pred.requires_grad and torch.is_grad_enabled() == grad
        assert [m.training for net in three for m in net.modules()] == flags
        for (i, k), v in state.items():
            assert torch.equal(three[i].state_dict()[k], v), k

        class Boom(RuntimeError):
            pass

        def broken(lo, hi):
            if lo:
                raise Boom()
            return frames[lo:hi]
        with pytest.raises(Boom):
            E.predict_disparities_drive(enc, dec, blk, 6, broken, n_prev=2, streams=2, chunk=2)
        assert [m.training for net in three for m in net.modules()] == flags and torch.is_grad_enabled() == grad
        with pytest.raises(Exception, match="returned 1 frames"):
            E.predict_disparities_drive(enc, dec, blk, 6, lambda lo, hi: frames[lo:lo + 1], n_prev=2, streams=2, chunk=2)
    finally:
        for net, flags in zip(three, before):
            for m, t in zip(net.modules(), flags):
                m.training = t
