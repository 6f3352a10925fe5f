"""The inference form of a ConvGRU v10 frame (dc_gru_c2f_infer_step: the GRU's tail + `+ r` + hand-over in one launch, the state
in place), the window predictor built on it (depthcore.evaluate.GruWindowPredictor) and evaluate_depth_gru.py --gru_version v10.

Kernel: against tests/gru_c2f_ref.py (`gru_handover` on a = y + r) in fp64 under tests/test_lstm_gpu.py's rule -- per output
tensor the Euclidean norm of the error is at most FACTOR = 4 times that of the same statement in fp32 torch on the CPU; each
ratio is printed before it is judged.
Predictor: against gru_c2f_ref.v10_sequence in fp64; a window's max-abs error may be at most 2 times that of the module's own
run_sequence at batch 1 (the bound tests/test_lstm_infer_gpu.py gives the v8 path: a batch changes the convolutions' tiling, not
their precision), and within rtol = atol = 1e-3.
Script: against the module's frame-by-frame forward per test file, with tests/test_eval_v8_gpu.py's tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

import gru_c2f_ref as GR
import kitti_tree as KT
from test_lstm_gpu import FACTOR, _judge

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "self-supervised-depth-estimation_amd")
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


def _inputs(B, C, hh, w, seed):
    g = torch.Generator().manual_seed(seed)
    t = dict(gates=torch.sigmoid(2.0 * torch.randn(B, 2 * C, hh, w, generator=g)), cnm=torch.tanh(torch.randn(B, C, hh, w, generator=g)))
    for k in ("h", "y", "r"):
        t[k] = torch.randn(B, C, hh, w, generator=g)
    return t


def _oracle(t, dtype):
    gates, cnm, h, y, r = (t[k].to(dtype) for k in ("gates", "cnm", "h", "y", "r"))
    hn, pre, up = GR.gru_handover(gates, h, cnm, y + r)
    return dict(h=hn, pre=pre, up=up)


def _run(t, S=None, y=True, pre=True, up=True, prep=lambda x: x):
    """One call on device copies (a state buffer of S rows; `prep` places every tensor) -> dict(h, pre, up) of the buffers."""
    from depthcore import ops
    B, C, hh, w = t["h"].shape
    S = S or B
    dev = {k: prep(v.to(DEV)) for k, v in t.items() if k in ("gates", "cnm", "y", "r")}
    full = torch.full((S, C, hh, w), SENT, device=DEV)
    full[:B] = t["h"].to(DEV)
    dev["h"] = prep(full)
    out_pre = prep(torch.full((S, C, hh, w), SENT, device=DEV)) if pre else None
    out_up = prep(torch.full((S, C // 4, 2 * hh, 2 * w), SENT, device=DEV)) if up else None
    ops.gru_c2f_infer_step(dev["gates"], dev["cnm"], dev["h"], dev["y"] if y else None, dev["r"] if y else None, out_pre, out_up, B)
    torch.cuda.synchronize()
    return dict(h=dev["h"], pre=out_pre, up=out_up)


def _rows(got, B):
    return {k: (None if v is None else v[:B]) for k, v in got.items()}


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_vs_fp64(shape):
    B, C, hh, w = shape
    t = _inputs(B, C, hh, w, 1500 + B + 7 * C + hh * w)
    ref, base = _oracle(t, torch.float64), _oracle(t, torch.float32)
    if ref["pre"].numel() > 16:
        assert 0.2 < float((ref["pre"] == 0).double().mean()) < 0.8          # both sides of the ReLU occur
    a, b = _run(t), _run(t)
    assert a["up"].shape == (B, C // 4, 2 * hh, 2 * w)
    _judge("gru infer %s" % (shape,), a, base, ref)
    for k in ref:
        assert torch.equal(a[k], b[k]), k                                    # two runs from the same inputs: the same bits


def test_the_step_is_the_training_launch_bit_for_bit():
    """The same expressions in the same order: h', pre and up of the step are those of ops.gru_handover on a = y + r."""
    from depthcore import ops
    for shape in ((1, 8, 9, 68), (2, 4, 3, 5)):
        t = _inputs(*shape, 1550)
        got = _run(t)
        d = {k: v.to(DEV) for k, v in t.items()}
        hn, pre, up = ops.gru_handover(d["gates"], d["h"], d["cnm"], d["y"] + d["r"])
        assert torch.equal(got["h"], hn) and torch.equal(got["pre"], pre) and torch.equal(got["up"], up)


@pytest.mark.parametrize("shape", [(2, 8, 2, 4), (2, 4, 3, 5)])             # float4, scalar
def test_rows_behind_B_are_not_touched(shape):
    B, C, hh, w = shape
    t = _inputs(B, C, hh, w, 1600 + C)
    ref, base = _oracle(t, torch.float64), _oracle(t, torch.float32)
    got = _run(t, S=3)
    _judge("gru prefix %s" % (shape,), _rows(got, B), base, ref)
    for k in ("h", "pre", "up"):
        assert bool((got[k][B:] == SENT).all()), k                           # bitwise the sentinel
    assert torch.equal(_rows(got, B)["h"], _run(t)["h"])


def test_unaligned_pointers_take_the_scalar_form():
    """(2, 8, 2, 4) allows float4, but every tensor starts 4 bytes past a 16-byte boundary: a float4 access there would be
    misaligned, so the call must fall back to scalar accesses."""
    def shifted(x):
        flat = torch.empty(x.numel() + 1, device=DEV)
        flat[1:].copy_(x.reshape(-1))
        v = flat[1:].view(x.shape)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v
    t = _inputs(2, 8, 2, 4, 1700)
    ref, base = _oracle(t, torch.float64), _oracle(t, torch.float32)
    got = _run(t, prep=shifted)
    _judge("gru shifted (2, 8, 2, 4)", got, base, ref)
    assert all(torch.equal(got[k], _run(t)[k]) for k in ref)                 # and the two forms agree bit for bit


@pytest.mark.parametrize("shape", [(2, 8, 2, 4), (2, 4, 3, 5)])             # float4, scalar
def test_up_lands_in_the_upper_channel_half(shape):
    """up_bstride = 2 C hh w: the launch writes into the upper channel half of a (B, 2 C/4, 2hh, 2w) buffer -- the next finer
    scale's cat(dec, up) -- and leaves the lower half alone."""
    from depthcore import ops
    B, C, hh, w = shape
    t = _inputs(B, C, hh, w, 1800 + C)
    plain = _run(t)
    dev = {k: v.to(DEV) for k, v in t.items()}
    wide = torch.full((B, 2 * (C // 4), 2 * hh, 2 * w), SENT, device=DEV)
    up = wide[:, C // 4:]
    assert up.stride(0) == 2 * C * hh * w and not up.is_contiguous()
    ops.gru_c2f_infer_step(dev["gates"], dev["cnm"], dev["h"], dev["y"], dev["r"], None, up)
    torch.cuda.synchronize()
    assert bool((wide[:, :C // 4] == SENT).all())
    assert torch.equal(wide[:, C // 4:], plain["up"])
    assert torch.equal(dev["h"], plain["h"])


@pytest.mark.parametrize("shape", [(1, 8, 9, 68), (2, 4, 3, 5)])            # float4, scalar
def test_null_outputs_leave_the_state_update_alone(shape):
    """State-only call (y = r = pre = up = NULL: scale 0 on every frame but a window's last) and pre without up (scale 0 on the
    last): h is the full call's, bit for bit."""
    B, C, hh, w = shape
    t = _inputs(B, C, hh, w, 1900 + C)
    full = _run(t)
    state_only = _run(t, y=False, pre=False, up=False)
    no_up = _run(t, up=False)
    for got in (state_only, no_up):
        assert torch.equal(got["h"], full["h"])
    assert torch.equal(no_up["pre"], full["pre"]) and no_up["up"] is None and state_only["pre"] is None


# ---- the predictor ------------------------------------------------------------------------------------------------------------
H, W = 32, 64                                                                # scale 3 is 4 x 8


def _v10(seed=5, height=H, width=W):
    import networks
    torch.manual_seed(seed)
    blk = networks.ConvGRUBlocks_v9((3, 3), True, "cpu", attention=False, height=height, width=width).to(DEV)
    for p in blk.parameters():                                               # the learned initial states too: h0 counts
        p.data.normal_(0, 0.05)
    return blk


def _maps(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, GR.NUM_CH_DEC[s], H >> s, W >> s, generator=g).to(DEV) for s in range(4)]


def _windows(blk, wins, streams, wp=None):
    """Every window's final scale-0 disparity through advance_maps / step_maps on window_groups' schedule -> list in input order."""
    from depthcore import evaluate as E
    lengths = [w[0].shape[0] for w in wins]
    wp = wp or E.GruWindowPredictor(None, None, blk, streams=streams)
    got = [None] * len(wins)
    for ids, widths in E.window_groups(lengths, streams):
        wp.reset()
        L = len(widths)
        for j, B in enumerate(widths):
            at = [j - (L - lengths[c]) for c in ids[:B]]
            batch = [torch.cat([wins[c][s][t:t + 1] for c, t in zip(ids[:B], at)]) for s in range(4)]
            if j < L - 1:
                assert wp.advance_maps(batch) is None
            else:
                disp = wp.step_maps(batch).clone()
        assert disp.shape == (len(ids), 1, H, W) and not disp.requires_grad
        for b, c in enumerate(ids):
            got[c] = disp[b]
    return got, wp


@pytest.fixture(scope="module")
def window_case():
    """Four windows of lengths [3, 1, 2, 2] (unsorted), and per window the last scale-0 disparity of the fp64 statement, of
    run_sequence and of the module's frame-by-frame forward."""
    blk = _v10()
    st = {k: v.detach().cpu().double() for k, v in blk.state_dict().items()}
    wins = [_maps(n, 40 + i) for i, n in enumerate((3, 1, 2, 2))]
    want = [GR.v10_sequence([d.cpu().double() for d in w], st)[0][-1] for w in wins]
    seq, loop = [], []
    with torch.no_grad():
        for w in wins:
            seq.append(blk.run_sequence({("disp", s): w[s] for s in range(4)})[("disp", 0)][-1].clone())
            states = blk.initial_states()
            for i in range(w[0].shape[0]):
                states, disp = blk({("disp", s): w[s][i:i + 1] for s in range(4)}, states)
            loop.append(disp[("disp", 0)][0].clone())
    return blk, wins, want, seq, loop


@pytest.mark.parametrize("streams", [1, 3])
def test_windows_vs_oracle(window_case, streams):
    """Per window: max-abs error of the lockstep path against the fp64 statement <= 2 x that of run_sequence at batch 1, within
    rtol = atol = 1e-3 of the statement and of the module's frame-by-frame forward."""
    blk, wins, want, seq, loop = window_case
    got, wp = _windows(blk, wins, streams=streams)
    for c in range(len(wins)):
        assert torch.equal(seq[c], loop[c])                                   # run_sequence is the frame loop
        e_lock = float((got[c].cpu().double() - want[c]).abs().max())
        e_seq = float((seq[c].cpu().double() - want[c]).abs().max())
        print("streams %d window %d (%d frames): lockstep %.3e  run_sequence %.3e" % (streams, c, wins[c][0].shape[0], e_lock, e_seq))
        assert e_lock <= 2 * e_seq, (c, e_lock, e_seq)
        np.testing.assert_allclose(got[c].cpu().numpy(), want[c].float().numpy(), rtol=1e-3, atol=1e-3)
        np.testing.assert_allclose(got[c].cpu().numpy(), loop[c].cpu().numpy(), rtol=1e-3, atol=1e-3)
    # a second round on the same predictor (every group starts with reset()): the same bits; h0 itself was never written
    again, _ = _windows(blk, wins, streams=streams, wp=wp)
    assert all(torch.equal(a, b) for a, b in zip(again, got))
    assert not wp.h[0].requires_grad and not hasattr(wp, "c")


def test_streams_behind_B_stay_at_h0():
    from depthcore import evaluate as E
    blk = _v10()
    wp = E.GruWindowPredictor(None, None, blk, streams=4)
    wp.advance_maps(_maps(3, 7))
    torch.cuda.synchronize()
    for s in range(4):
        init = blk.cells()[s].h0_layer1.detach()
        assert torch.equal(wp.h[s][3:], init) and not torch.equal(wp.h[s][:1], init)
    with pytest.raises(Exception, match="ConvGRUBlocks_v8"):
        E.WindowPredictor(None, None, blk, streams=2)                        # the ConvLSTM predictor refuses ConvGRU cells


# ---- the script ---------------------------------------------------------------------------------------------------------------
HN, WN = 64, 128
A, B_ = sorted(KT.DRIVES)
# shuffled; drive A at frames 0 (a window of one frame), 1 (two) and 8 (nine with --n_prev_images 10, seven by default), drive B at 3
LINES = ["%s 3 l" % B_, "%s 1 l" % A, "%s 8 l" % A, "%s 0 l" % A]
TOL = dict(rtol=1e-3, atol=1e-3)                        # the bound test_eval_v8_gpu.py uses


def test_v10_script(tmp_path):
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import evaluate_depth_gru as EG
    import trainer as T
    from depthcore import evaluate as E
    from depthcore import ops
    from depthcore.data import GpuPreprocessor
    from depthcore.synthetic import synthetic_depth_gt
    from options import MonodepthOptions
    root = str(tmp_path)
    data, splits = os.path.join(root, "kitti"), os.path.join(root, "splits")
    KT.write_raw_tree(data, frames=9)
    os.makedirs(os.path.join(splits, "eigen"))
    with open(os.path.join(splits, "eigen", "test_files.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
    gts = [synthetic_depth_gt(1, "cpu", seed=i, height=60 + 4 * (i % 2), width=200, density=0.3)[0, 0].numpy() for i in range(len(LINES))]
    arr = np.empty(len(gts), dtype=object)
    for i, g in enumerate(gts):
        arr[i] = g
    np.savez(os.path.join(splits, "eigen", "gt_depths.npz"), data=arr)
    torch.manual_seed(3)
    tr = T.Trainer(T.default_options(height=HN, width=WN, batch_size=1, gru="v10", len_sequence=3), device=DEV)
    with torch.no_grad():
        for p in tr.models["gru"].parameters():                   # the learned h0 start at zero: make them count
            p.normal_(0, 0.05)
    weights = tr.save_model(os.path.join(root, "weights"))
    common = ["--load_weights_folder", weights, "--data_path", data, "--splits_dir", splits, "--png", "--eval_mono", "--gru_version", "v10"]
    res = EG.evaluate(MonodepthOptions().parse(common + ["--batch_size", "2", "--save_pred_disps", "--n_prev_images", "10"]))
    saved = np.load(os.path.join(weights, "disps_eigen_split.npy"))
    assert saved.shape == (len(LINES), HN, WN) and saved.dtype == np.float32

    # file by file, batch 1, through the module's frame-by-frame forward
    enc, gru, dec, h, w = EG.load_networks(MonodepthOptions().parse(common), DEV)
    assert (h, w) == (HN, WN) and type(gru).__name__ == "ConvGRUBlocks_v9"
    for k, v in tr.models["gru"].state_dict().items():
        assert torch.equal(gru.state_dict()[k], v), k
    prep = GpuPreprocessor(h, w, num_scales=1, frame_idxs=(0,), device=DEV)
    for net in (enc, gru, dec):
        net.eval()

    def composition(n_prev):
        want = torch.empty(len(LINES), 1, h, w, device=DEV)
        with torch.no_grad():
            for i, line in enumerate(LINES):
                states = gru.initial_states()
                for p in EG.window_paths(data, line, ".png", n_prev):
                    states, disp = gru(dec(enc(EG.frame_batch(prep, [p], DEV)), True), states)
                want[i] = ops.disp_to_depth(disp[("disp", 0)], 0.1, 100.0)[0][0]
        return want
    assert [len(EG.window_paths(data, line, ".png", 10)) for line in LINES] == [4, 2, 9, 1]
    want = composition(10)
    err = float(np.abs(saved - want[:, 0].cpu().numpy()).max())
    print("max |script - composition| = %.3e" % err)
    np.testing.assert_allclose(saved, want[:, 0].cpu().numpy(), **TOL)                              # file order
    ref = E.evaluate_depth(want, gts, "eigen")
    np.testing.assert_allclose(res["errors"], ref["errors"], **TOL)
    np.testing.assert_allclose(res["ratio_median"], ref["ratio_median"], rtol=1e-3)
    # the windows matter: the prediction of a test file differs from that of its frame alone
    assert float(np.abs(saved[2] - composition(0)[2, 0].cpu().numpy()).max()) > 0
    # the option's default stays 6 previous frames, at another lockstep width
    res6 = EG.evaluate(MonodepthOptions().parse(common + ["--batch_size", "1"]))
    ref6 = E.evaluate_depth(composition(6), gts, "eigen")
    np.testing.assert_allclose(res6["errors"], ref6["errors"], **TOL)
    tr.close()
