"""The inference form of the ConvGRU v5 step (dc_gru_infer_*: B streams, every level in one launch) and the lockstep
evaluation built on it (depthcore.evaluate.SequencePredictor / predict_disparities_sequences), against the torch expression,
the existing cell and the fp64 CPU oracle."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import gru_ref as G

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RTOL, ATOL = 1e-6, 1e-7                     # what tests/test_gru_gpu.py holds dc_gru_rh / dc_gru_blend / the residual to
H, W = 64, 96


def _close(a, b, msg=""):
    np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=RTOL, atol=ATOL, err_msg=msg)


def _level_tensors(shapes, S, seed):
    """One level per (C, h, w): gates in (0,1), state / candidate / features random, rh / out filled with a sentinel."""
    g = torch.Generator().manual_seed(seed)
    lv = {k: [] for k in ("gates", "h", "cnm", "f", "rh", "out")}
    for C, h, w in shapes:
        lv["gates"].append(torch.rand(S, 2 * C, h, w, generator=g).to(DEV))
        for k in ("h", "cnm", "f"):
            lv[k].append(torch.randn(S, C, h, w, generator=g).to(DEV))
        for k in ("rh", "out"):
            lv[k].append(torch.full((S, C, h, w), -7.0, device=DEV))
    return lv


def _expected(lv, k, B):
    gates, h, cnm, f = (lv[n][k][:B] for n in ("gates", "h", "cnm", "f"))
    C = h.shape[1]
    rh = gates[:, :C] * h
    u = gates[:, C:]
    h_next = (1 - u) * h + u * cnm
    return rh, h_next, f + (h_next + h) / 2


# (C, P) = (3, 15), (4, 6), (8, 64), (2, 4 * 4097), (64, 48 * 160): C * P = 45 of the first is no multiple of 4 (scalar path, rows
# 1.. start unaligned) next to aligned levels, the fourth has an odd row length; the grid is sized for the last and the small
# levels' blocks idle.  ("one_level" is a second scalar case: C * P = 315.)
FIVE = [(3, 3, 5), (4, 2, 3), (8, 8, 8), (2, 4, 4097), (64, 48, 160)]


@pytest.mark.parametrize("name,shapes,S,B", [
    ("five_levels", FIVE, 3, 3),
    ("one_level", [(5, 7, 9)], 2, 2),
    ("one_stream", FIVE[:4], 1, 1),
    ("prefix", FIVE[:4] + [(16, 12, 40)], 4, 2),
    ("grid_wraps", [(64, 48, 160), (3, 3, 5)], 9, 9),           # 9 * 64 * 48 * 160 > 4096 * 256 * 4
])
def test_grouped_kernels_vs_torch(name, shapes, S, B):
    from depthcore import ops
    lv = _level_tensors(shapes, S, seed=len(shapes) + S)
    if name == "grid_wraps":
        assert B * 64 * 48 * 160 > 4096 * 256 * 4
    want = [_expected(lv, k, B) for k in range(len(shapes))]
    h_before = [t.clone() for t in lv["h"]]
    ops.gru_infer_rh(lv["gates"], lv["h"], lv["rh"], B)
    for k in range(len(shapes)):
        assert torch.equal(lv["h"][k], h_before[k])             # rh only reads the state
    ops.gru_infer_tail(lv["gates"], lv["cnm"], [f[:B] for f in lv["f"]], lv["h"], lv["out"], B)
    torch.cuda.synchronize()
    for k in range(len(shapes)):
        _close(lv["rh"][k][:B], want[k][0], "rh level %d" % k)
        _close(lv["h"][k][:B], want[k][1], "h level %d" % k)
        _close(lv["out"][k][:B], want[k][2], "out level %d" % k)
        # the rows behind the prefix: bitwise untouched
        assert torch.equal(lv["h"][k][B:], h_before[k][B:])
        assert bool((lv["rh"][k][B:] == -7.0).all()) and bool((lv["out"][k][B:] == -7.0).all())


def test_unaligned_pointers_take_the_scalar_path():
    """C * P = 32 allows float4, but every tensor starts 4 bytes past a 16-byte boundary: the level must fall back to scalar
    accesses (a float4 access there would be misaligned) next to a level that is aligned."""
    from depthcore import ops
    S, B = 3, 3
    lv = _level_tensors([(4, 2, 4), (4, 2, 4)], S, seed=11)

    def shifted(t):
        flat = torch.empty(t.numel() + 1, device=DEV)
        flat[1:].copy_(t.reshape(-1))
        v = flat[1:].view(t.shape)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v
    for name in lv:
        lv[name][0] = shifted(lv[name][0])
    want = [_expected(lv, k, B) for k in range(2)]
    ops.gru_infer_rh(lv["gates"], lv["h"], lv["rh"], B)
    ops.gru_infer_tail(lv["gates"], lv["cnm"], lv["f"], lv["h"], lv["out"], B)
    state = [torch.full((S, 4, 2, 4), -7.0, device=DEV) for _ in range(2)]
    state[0] = shifted(state[0])
    h0 = [shifted(torch.randn(1, 4, 2, 4).to(DEV)), torch.randn(1, 4, 2, 4).to(DEV)]
    ops.gru_infer_init(h0, state, B)
    torch.cuda.synchronize()
    for k in range(2):
        _close(lv["rh"][k], want[k][0]); _close(lv["h"][k], want[k][1]); _close(lv["out"][k], want[k][2])
        assert torch.equal(state[k], h0[k].expand(S, -1, -1, -1))


def test_init_broadcasts_and_leaves_h0_alone():
    from depthcore import ops
    g = torch.Generator().manual_seed(1)
    shapes = [(3, 3, 5), (4, 2, 3), (8, 8, 8), (2, 4, 4097), (64, 12, 40)]
    h0 = [torch.nn.Parameter(torch.randn(1, C, h, w, generator=g).to(DEV)) for C, h, w in shapes]
    keep = [p.detach().clone() for p in h0]
    for S, B in ((4, 4), (4, 2), (1, 1)):
        state = [torch.full((S, C, h, w), -7.0, device=DEV) for C, h, w in shapes]
        ops.gru_infer_init(h0, state, B)
        for p, k0, s in zip(h0, keep, state):
            assert torch.equal(p.detach(), k0)
            assert all(torch.equal(s[b], k0[0]) for b in range(B))
            assert bool((s[B:] == -7.0).all())
            assert not s.requires_grad


def test_refusals():
    from depthcore import _lib
    L = _lib.lib()
    t = torch.zeros(2, 4, 3, 3, device=DEV)
    gt = torch.zeros(2, 8, 3, 3, device=DEV)

    def levels(n, h=t):
        lv = (_lib.GruInferLevel * max(n, 1))()
        for k in range(max(n, 1)):
            lv[k].gates, lv[k].cnm, lv[k].f, lv[k].rh, lv[k].out = (x.data_ptr() for x in (gt, t, t, t, t))
            lv[k].h = h.data_ptr() if h is not None else None
            lv[k].C, lv[k].P = 4, 9
        return lv
    for fn in (L.dc_gru_infer_rh, L.dc_gru_infer_tail):
        assert fn(levels(1), 0, 2, None) == -1
        assert fn(levels(9), 9, 2, None) == -1
        assert fn(levels(1), 1, 0, None) == -1
        assert fn(levels(1, None), 1, 2, None) == -1
        assert fn(None, 1, 2, None) == -1
    big = levels(1)
    big[0].C, big[0].P = 1 << 15, 1 << 15                      # 2 * C * P = 2^31 elements of gates: refused before any launch
    assert L.dc_gru_infer_rh(big, 1, 1, None) == -1
    ptrs = (ctypes.c_void_p * 1)(t.data_ptr())
    for nlev, B, h0, M in ((0, 2, ptrs, 36), (9, 2, ptrs, 36), (1, 0, ptrs, 36), (1, 2, None, 36), (1, 2, ptrs, 0), (1, 2, ptrs, 1 << 31)):
        assert L.dc_gru_infer_init(h0, ptrs, (ctypes.c_size_t * 1)(M), nlev, B, None) == -1
    torch.cuda.synchronize()


# ---- the step, the lockstep schedule and the predictor ------------------------------------------------------------------------
def _gru(seed=5):
    import networks
    torch.manual_seed(seed)
    blk = networks.ConvGRUBlocks_v5(kernel_size=(3, 3), bias=True, device="cpu", height=H, width=W).to(DEV)
    for p in blk.parameters():                                  # the learned initial states too: non-zero h0
        p.data.normal_(0, 0.05)
    return blk


def _features(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, c, H >> (k + 1), W >> (k + 1), generator=g).to(DEV) for k, c in enumerate((64, 64, 128, 256, 512))]


class _Identity(torch.nn.Module):
    def forward(self, x):
        return x


def test_step_vs_existing_cell():
    """One cell step at B = 3 from the learned initial states: fused features and new state against ConvGRUBlocks_v5.forward on
    the same batch -- the convolutions are the same calls, the gate arithmetic differs by its rounding only."""
    from depthcore import evaluate as E
    blk = _gru()
    B = 3
    feats = _features(B, 7)
    sp = E.SequencePredictor(_Identity(), blk, _Identity(), streams=4)
    fused = [o.clone() for o in sp.fuse(feats)]
    with torch.no_grad():
        h0 = [c.h0_layer1.expand(B, -1, -1, -1).contiguous() for c in blk.cells()]
        h1 = blk(feats, h0)
    for k in range(5):
        _close(sp.state[k][:B], h1[k], "state level %d" % k)
        _close(fused[k], feats[k] + (h1[k] + h0[k]) / 2, "fused level %d" % k)
        assert torch.equal(sp.state[k][B:], blk.cells()[k].h0_layer1.detach().expand(1, -1, -1, -1))      # stream 3 did not move


def _lockstep_fused(blk, scene_feats, streams):
    """The fused features of every scene, run through SequencePredictor.fuse on lockstep_groups' schedule."""
    from depthcore import evaluate as E
    lengths = [f[0].shape[0] for f in scene_feats]
    outs = [[torch.empty_like(f) for f in feats] for feats in scene_feats]
    sp = E.SequencePredictor(_Identity(), blk, _Identity(), streams=streams)
    for ids, widths in E.lockstep_groups(lengths, streams):
        sp.reset()
        for t, B in enumerate(widths):
            batch = [torch.cat([scene_feats[c][k][t:t + 1] for c in ids[:B]]) for k in range(5)]
            fused = sp.fuse(batch)
            for b, c in enumerate(ids[:B]):
                for k in range(5):
                    outs[c][k][t] = fused[k][b]
    return outs


@pytest.fixture(scope="module")
def oracle_case():
    """Scenes of lengths [2, 3, 1] (unsorted), their fp32 features, and per scene the fp64 oracle and today's run_sequence."""
    blk = _gru()
    st = {k: v.detach().cpu().double() for k, v in blk.state_dict().items()}
    scenes = [_features(n, 20 + i) for i, n in enumerate((2, 3, 1))]
    want = [G.run_gru_v5([f.cpu().double() for f in feats], st) for feats in scenes]
    with torch.no_grad():
        seq = [[o.clone() for o in blk.run_sequence(feats)] for feats in scenes]
    return blk, scenes, want, seq


def test_lockstep_vs_oracle(oracle_case):
    """Per scene and level: max-abs error of the lockstep path against the fp64 oracle <= 2 x that of run_sequence (a batch
    changes the convolution's tiling and reduction order, not its precision), and within rtol = atol = 1e-3.
    Measured on an MI355X (fp32 policy), worst scene per level 0..4: lockstep 6.7e-7, 4.7e-7, 9.9e-7, 1.8e-6, 4.0e-6 against
    run_sequence 6.4e-7, 4.7e-7, 9.9e-7, 1.8e-6, 4.0e-6."""
    blk, scenes, want, seq = oracle_case
    got = _lockstep_fused(blk, scenes, streams=3)
    for c in range(len(scenes)):                                # scene 2 has one frame, scene 1 is the longest
        for k in range(5):
            e_lock = float((got[c][k].cpu().double() - want[c][k]).abs().max())
            e_seq = float((seq[c][k].cpu().double() - want[c][k]).abs().max())
            print("scene %d level %d: lockstep %.3e  run_sequence %.3e" % (c, k, e_lock, e_seq))
            assert e_lock <= 2 * e_seq, (c, k, e_lock, e_seq)
            np.testing.assert_allclose(got[c][k].cpu().numpy(), want[c][k].float().numpy(), rtol=1e-3, atol=1e-3)


def _nets(seed=2):
    import networks
    torch.manual_seed(seed)
    enc = networks.ResnetEncoder(18, False).to(DEV)
    dec = networks.DepthDecoder(enc.num_ch_enc).to(DEV)
    return enc, _gru(seed + 1), dec


def _scenes(lengths, seed=4):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(n, 3, H, W, generator=g).to(DEV) for n in lengths]


def test_streaming_equals_lockstep():
    from depthcore import evaluate as E
    enc, blk, dec = _nets()
    scenes = _scenes([2, 3, 1])
    pred = E.predict_disparities_sequences(enc, blk, dec, scenes, streams=3)
    assert [tuple(p.shape) for p in pred] == [(2, 1, H, W), (3, 1, H, W), (1, 1, H, W)]             # input order
    assert not any(p.requires_grad for p in pred)
    (ids, widths), = E.lockstep_groups([2, 3, 1], 3)
    assert ids == [1, 0, 2] and widths == [3, 2, 1]
    sp = E.SequencePredictor(enc, blk, dec, streams=3)
    for rnd in range(2):                                        # the second round after reset(): the same bits
        for t, B in enumerate(widths):
            disp = sp.step(torch.cat([scenes[c][t:t + 1] for c in ids[:B]]))
            for b, c in enumerate(ids[:B]):
                assert torch.equal(disp[b], pred[c][t]), (rnd, t, c)
        sp.reset()
    # iterables of (1,3,h,w) frames are the same scenes
    again = E.predict_disparities_sequences(enc, blk, dec, [[s[i:i + 1] for i in range(s.shape[0])] for s in scenes], streams=3)
    assert all(torch.equal(a, b) for a, b in zip(again, pred))
    # a scene's prediction depends on its own frames only: scene 1 alone at width 1 agrees to the convolutions' rounding
    alone = E.predict_disparities_sequences(enc, blk, dec, scenes[1:2], streams=1)[0]
    np.testing.assert_allclose(alone.cpu().numpy(), pred[1].cpu().numpy(), rtol=1e-3, atol=1e-3)


def test_hygiene_and_groups():
    from depthcore import evaluate as E
    enc, blk, dec = _nets(6)
    enc.train()
    dec.eval()
    blk.train()
    enc.encoder.layer2.train(False)
    nets = (enc, blk, dec)
    flags = [m.training for net in nets for m in net.modules()]
    state = {(i, k): v.clone() for i, net in enumerate(nets) for k, v in net.state_dict().items()}
    assert sum(1 for (_, k) in state if k.endswith("h0_layer1")) == 5 and any(k.endswith("running_var") for (_, k) in state)
    scenes = _scenes([2, 1, 3, 2, 1], seed=8)
    wide = E.predict_disparities_sequences(enc, blk, dec, scenes, streams=5)
    narrow = E.predict_disparities_sequences(enc, blk, dec, scenes, streams=2)          # three consecutive groups
    torch.cuda.synchronize()
    assert [m.training for net in nets for m in net.modules()] == flags
    for (i, k), v in state.items():
        assert torch.equal(nets[i].state_dict()[k], v), k
    for a, b in zip(wide, narrow):
        assert a.shape == b.shape and not a.requires_grad and not b.requires_grad
        np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), rtol=1e-3, atol=1e-3)

    class Boom(RuntimeError):
        pass

    def frames():
        yield scenes[0][0:1]
        raise Boom()
    with pytest.raises(Boom):
        E.predict_disparities_sequences(enc, blk, dec, [scenes[2], _Sized(frames(), 2)], streams=2)
    assert [m.training for net in nets for m in net.modules()] == flags
    for (i, k), v in state.items():
        assert torch.equal(nets[i].state_dict()[k], v), k
    with pytest.raises(ValueError):
        E.predict_disparities_sequences(enc, blk, dec, [], streams=2)


class _Sized:
    def __init__(self, it, n):
        self.it, self.n = it, n

    def __len__(self):
        return self.n

    def __iter__(self):
        return self.it
