"""The coarse-to-fine ConvGRU front-end (gru_version v10) on the HIP path.

Kernels (dc_gru_handover_fwd / _bwd) against tests/gru_c2f_ref.py evaluated in fp64.  The bound is not a constant: per output
tensor the fused launch's error (Euclidean norm of the difference to the oracle, tests/test_lstm_gpu.py's `_err`) is judged by
that file's `_judge` -- its margin, FACTOR = 4 -- against the error of the composition the launch replaces, run on the device on
the same inputs: ops.gru_blend (dc_gru_blend_*) followed by ops.lstm_handover (dc_lstm_handover_*).  The kernel is never compared
with itself.  Each ratio is printed before it is judged.

Module (networks.ConvGRUBlocks_v9(attention=False)) against the reference's outputs and gradients
(tests/golden/convgru_v10.npz) with test_lstm_gpu.py's `_check` tolerances, run_sequence against the frame loop, and the trainer
with gru="v10"."""
import os

import numpy as np
import pytest
import torch

import gru_c2f_ref as GR
import make_golden as MG
import make_golden_gru_c2f as MC
import test_lstm_gpu as TL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convgru_v10.npz")
# test_lstm_gpu.py's hand-over shapes (the same item walk): scalar forms with odd w / one pixel, float4 forms, then (1, 8, 9, 68):
# 306 float4 items = one full block + 50 threads, and (1, 4, 9, 13): 468 elements = one full block + 212 threads
SHAPES = TL.HAND_SHAPES
OUTS = ("h_new", "pre", "up", "d_gates", "d_h_prev", "d_cnm", "d_a")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD, allow_pickle=False)


def test_shapes_cover_both_forms_and_a_ragged_second_block():
    assert TL.FACTOR == 4.0
    assert (2, 4, 3, 5) in SHAPES and (1, 8, 2, 4) in SHAPES and (1, 8, 9, 68) in SHAPES and (1, 4, 9, 13) in SHAPES
    blk = TL._block()
    assert blk < 1 * 2 * 9 * 17 < 2 * blk and blk < 4 * 9 * 13 < 2 * blk


def _inputs(B, C, h, w, bcast, seed):
    """gates (post-sigmoid, in (0, 1)), h_prev (one row with bcast), cnm (post-tanh), a, then the cotangents of h_new, pre, up."""
    g = torch.Generator().manual_seed(seed)
    t = dict(gates=torch.sigmoid(2.0 * torch.randn(B, 2 * C, h, w, generator=g)), h_prev=torch.randn(1 if bcast else B, C, h, w, generator=g),
             cnm=torch.tanh(torch.randn(B, C, h, w, generator=g)), a=torch.randn(B, C, h, w, generator=g))
    cots = dict(h_new=torch.randn(B, C, h, w, generator=g), pre=torch.randn(B, C, h, w, generator=g),
                up=torch.randn(B, C // 4, 2 * h, 2 * w, generator=g))
    return t, cots


def _total(outs, cots):
    tot = 0
    for k, o in zip(("h_new", "pre", "up"), outs):
        if cots.get(k) is not None and o is not None:
            tot = tot + (o * cots[k].to(device=o.device, dtype=o.dtype)).sum()
    return tot


def _result(leaves, outs, cots):
    # (an input that no read output depends on -- `a` when only h_new is read -- has a zero gradient)
    d = torch.autograd.grad(_total(outs, cots), leaves, allow_unused=True)
    d = [torch.zeros_like(x) if g is None else g for g, x in zip(d, leaves)]
    return dict(h_new=outs[0].detach(), pre=outs[1].detach(), up=None if outs[2] is None else outs[2].detach(),
                d_gates=d[0], d_h_prev=d[1], d_cnm=d[2], d_a=d[3])


def _oracle(t, cots, need_up=True):
    leaves = [t[k].double().requires_grad_() for k in ("gates", "h_prev", "cnm", "a")]
    gt, hp, cn, a = leaves
    return _result(leaves, GR.gru_handover(gt, hp.expand_as(a), cn, a, need_up), cots)


def _composition(t, cots, need_up=True):
    """What exists without the fused launch: dc_gru_blend_*, then dc_lstm_handover_*, chained by autograd, on the device."""
    from depthcore import ops
    leaves = [t[k].to(DEV).requires_grad_() for k in ("gates", "h_prev", "cnm", "a")]
    gt, hp, cn, a = leaves
    hpe = hp.expand_as(a)
    h_new = ops.gru_blend(gt, hpe, cn)
    pre, up = ops.lstm_handover(a, hpe, h_new, need_up=need_up)
    return _result(leaves, (h_new, pre, up), cots)


def _fused(t, cots, need_up=True):
    from depthcore import ops
    leaves = [t[k].to(DEV).requires_grad_() for k in ("gates", "h_prev", "cnm", "a")]
    return _result(leaves, ops.gru_handover(*leaves, need_up=need_up), cots)


@pytest.mark.parametrize("bcast", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_handover_vs_fp64_and_the_composition(shape, bcast):
    B, C, h, w = shape
    t, cots = _inputs(B, C, h, w, bcast, 1000 + B + 7 * C + h * w)
    ref = _oracle(t, cots)
    assert 0.2 < float((ref["pre"] == 0).double().mean()) < 0.8 or ref["pre"].numel() <= 16      # both sides of the ReLU occur
    base = _composition(t, cots)
    runs = [_fused(t, cots), _fused(t, cots)]
    assert runs[0]["up"].shape == (B, C // 4, 2 * h, 2 * w) and runs[0]["d_h_prev"].shape == t["h_prev"].shape
    assert runs[0]["d_gates"].shape == t["gates"].shape and float(runs[0]["d_gates"][:, :C].abs().max()) == 0      # reset half: zero
    TL._judge("gru hand-over %s%s" % (shape, " bcast" if bcast else ""), runs[0], base, ref)
    for k in OUTS:
        assert torch.equal(runs[0][k], runs[1][k]), k


def _raw(t, cots, need_up):
    """The raw entries on NaN-filled outputs; cots' entries may be None -> NULL."""
    from depthcore import _lib
    L, ptr = _lib.lib(), _lib.ptr
    d = {k: v.to(DEV) for k, v in t.items()}
    g = {k: (None if v is None else v.to(DEV)) for k, v in cots.items()}
    B, C, h, w = d["a"].shape
    nan = lambda like: torch.full_like(like, float("nan"))
    h_new, pre = nan(d["a"]), nan(d["a"])
    up = torch.full((B, C // 4, 2 * h, 2 * w), float("nan"), device=DEV) if need_up else None
    _lib.check(L.dc_gru_handover_fwd(ptr(d["gates"]), ptr(d["h_prev"]), ptr(d["cnm"]), ptr(d["a"]), ptr(h_new), ptr(pre), ptr(up), B, C, h, w,
                                     _lib.stream(pre)), "dc_gru_handover_fwd")
    outs = [nan(d["gates"]), nan(d["a"]), nan(d["a"]), nan(d["a"])]
    _lib.check(L.dc_gru_handover_bwd(ptr(d["gates"]), ptr(d["h_prev"]), ptr(d["cnm"]), ptr(pre), ptr(g["h_new"]), ptr(g["pre"]), ptr(g["up"]),
                                     ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), B, C, h, w, _lib.stream(pre)),
               "dc_gru_handover_bwd")
    return dict(h_new=h_new, pre=pre, up=up, d_gates=outs[0], d_h_prev=outs[1], d_cnm=outs[2], d_a=outs[3])


@pytest.mark.parametrize("null", ["up", "g_h_new", "g_pre", "g_up", "only_g_h_new", "only_g_up"])
@pytest.mark.parametrize("shape", [(2, 4, 3, 5), (1, 8, 9, 68)])            # scalar, float4
def test_null_arguments(shape, null):
    """Each NULL-able argument alone through the raw entries: up (scale 0: only h_new and pre are written), each of the three
    incoming gradients, and two of them at once (the last frame's state has no consumer; a frame whose disparity alone is read)."""
    B, C, h, w = shape
    t, cots = _inputs(B, C, h, w, False, 1100 + C)
    need_up = null != "up"
    drop = {"up": ("up",), "g_h_new": ("h_new",), "g_pre": ("pre",), "g_up": ("up",), "only_g_h_new": ("pre", "up"),
            "only_g_up": ("h_new", "pre")}[null]
    cots = {k: (None if k in drop else v) for k, v in cots.items()}
    ref, base = _oracle(t, cots, need_up), _composition(t, cots, need_up)
    runs = [_raw(t, cots, need_up), _raw(t, cots, need_up)]
    TL._judge("gru hand-over %s %s=NULL" % (shape, null), runs[0], base, ref)
    for k in OUTS:
        assert (runs[0][k] is None and runs[1][k] is None) or torch.equal(runs[0][k], runs[1][k]), k


def test_unread_outputs_reach_the_kernel_as_null():
    """Through autograd: only `up` is read -> g_h_new and g_pre arrive as None, not as zero tensors; and the C % 4 rule holds only where a
    shuffle is written."""
    from depthcore import ops
    t, cots = _inputs(2, 8, 2, 4, False, 1200)
    only = dict(h_new=None, pre=None, up=cots["up"])
    TL._judge("only up read", _fused(t, only), _composition(t, only), _oracle(t, only))
    with pytest.raises(Exception, match="multiple of 4|C % 4"):
        ops.gru_handover(torch.rand(1, 12, 2, 2, device=DEV), torch.rand(1, 6, 2, 2, device=DEV), torch.rand(1, 6, 2, 2, device=DEV),
                         torch.rand(1, 6, 2, 2, device=DEV))
    h_new, pre, up = ops.gru_handover(torch.rand(1, 12, 2, 2, device=DEV), torch.rand(1, 6, 2, 2, device=DEV),
                                      torch.rand(1, 6, 2, 2, device=DEV), torch.rand(1, 6, 2, 2, device=DEV), need_up=False)
    assert up is None and pre.shape == (1, 6, 2, 2)                          # without a shuffle C need not be a multiple of 4


# ---- the module against the reference's fixture ----------------------------------------------------------------------------
def test_blocks_v10_forward_chain_vs_reference_fixture(gold):
    """ConvGRUBlocks_v9.forward chained over the two frames of the fixture from the seeded initial states that are passed in."""
    import networks
    c = MC.V10
    v10 = networks.ConvGRUBlocks_v9(kernel_size=(3, 3), bias=True, device="cpu", attention=False)
    assert list(v10.state_dict().keys()) == list(gold["v10_keys"])
    MG.seeded_state(v10, c["wseed"], c["wscale"])
    v10 = v10.to(DEV)
    dec, states, cots = MC.v10_inputs()
    dec = [d.to(DEV).requires_grad_() for d in dec]
    states = [h.to(DEV).requires_grad_() for h in states]
    cur, tot = states, 0
    for i in range(c["n"]):
        cur, disp = v10({("disp", s): dec[s][i:i + 1] for s in range(4)}, cur)
        for s in range(4):
            TL._check("v10_disp%d_%d" % (s, i), disp[("disp", s)], gold["v10_disp%d_%d" % (s, i)], **TL.OUT_TOL)
            tot = tot + (disp[("disp", s)] * cots[s][i:i + 1].to(DEV)).sum()
    ps = {k: p for k, p in v10.named_parameters() if not k.endswith("h0_layer1")}
    gr = torch.autograd.grad(tot, dec + list(ps.values()) + states)
    for s in range(4):
        TL._check("v10_gdec%d" % s, MG.summ(gr[s]), gold["v10_gdec%d" % s], **TL.GIN_TOL)
        TL._check("v10_gh%d" % s, MG.summ(gr[4 + len(ps) + s]), gold["v10_gh%d" % s], **TL.GIN_TOL)
    for j, k in enumerate(ps):
        TL._check("v10_g_" + k, MG.summ(gr[4 + j]), gold["v10_g_" + k], **TL.GPAR_TOL)


def test_run_sequence_is_the_frame_loop():
    import networks
    torch.manual_seed(7)
    H, W, n = 32, 64, 3
    v10 = networks.ConvGRUBlocks_v9((3, 3), True, "cpu", attention=False, height=H, width=W).to(DEV)
    dec = {("disp", s): torch.randn(n, GR.NUM_CH_DEC[s], H >> s, W >> s, device=DEV).requires_grad_() for s in range(4)}
    out = v10.run_sequence(dec)
    states = v10.initial_states()
    for i in range(n):
        states, disp = v10({k: v[i:i + 1] for k, v in dec.items()}, states)
        for s in range(4):
            assert torch.equal(out[("disp", s)][i:i + 1], disp[("disp", s)]), (s, i)
    assert [tuple(out[("disp", s)].shape) for s in range(4)] == [(n, 1, H >> s, W >> s) for s in range(4)]
    sum(o.sum() for o in out.values()).backward()
    for cell in v10.cells():
        assert cell.h0_layer1.grad is not None and float(cell.h0_layer1.grad.abs().sum()) > 0
    assert all(d.grad is not None and float(d.grad.abs().sum()) > 0 for d in dec.values())


def test_trainer_v10(tmp_path):
    """gru="v10" at 64x96 on a synthetic 2-frame sequence: a finite loss, the dispconvs left alone, a checkpoint round trip, and
    the freeze of h0 at h_s_epoch."""
    import trainer as T_
    from depthcore.synthetic import synthetic_sequence_batch
    H, W, n = 64, 96, 2
    kw = dict(batch_size=1, height=H, width=W, gru="v10", len_sequence=n, log_dir=str(tmp_path), model_name="v10", h_s_epoch=2)
    tr = T_.Trainer(T_.default_options(**kw), device=DEV, seed=0)
    assert type(tr.models["gru"]).__name__ == "ConvGRUBlocks_v9"
    tr.set_train()
    inputs = synthetic_sequence_batch(n, H, W, torch.device(DEV))
    dispconv0 = {k: v.clone() for k, v in tr.models["depth"].state_dict().items() if k.startswith(("decoder.1",)) and
                 int(k.split(".")[1]) >= 10}
    assert len(dispconv0) == 8                                      # four dispconvs, weight and bias
    ls = []
    for _ in range(2):
        outputs, l = tr.train_step(dict(inputs))
        ls.append(float(l["loss"]))
    assert all(np.isfinite(ls))
    assert [tuple(outputs[("disp", s)].shape) for s in range(4)] == [(n, 1, H >> s, W >> s) for s in range(4)]
    cells = tr.models["gru"].cells()
    for cell in cells:
        assert float(cell.h0_layer1.detach().abs().sum()) > 0       # moved away from its zero initialisation
    sd = tr.models["depth"].state_dict()
    for k, v in dispconv0.items():
        assert torch.equal(sd[k], v), k                             # no gradient, and Adam leaves them untouched
    # checkpoint: a fresh trainer that loads it takes the same next step (the tie-break noise is seeded by the step count)
    folder = tr.save_model(str(tmp_path / "w"))
    saved = torch.load(os.path.join(folder, "gru.pth"), map_location="cpu")
    assert "cgru_3.h0_layer1" in saved and "cgru_0.cgru_1.conv_can.weight" in saved and not any("c0_layer1" in k for k in saved)
    other = T_.Trainer(T_.default_options(**kw), device=DEV, seed=5)
    other.load_model(folder)
    other.set_train()
    other.step = tr.step
    _, la = tr.train_step(dict(inputs))
    _, lb = other.train_step(dict(inputs))
    assert float(la["loss"]) == float(lb["loss"]) and torch.equal(la["loss"], lb["loss"])
    other.close()
    # from h_s_epoch on the learned initial states stop training (trainer_gru.py:295-301): epoch 0 leaves them, epoch 1 freezes
    tr.start_epoch(0)
    assert all(c.h0_layer1.requires_grad for c in cells)
    tr.start_epoch(1)
    frozen = [c.h0_layer1.detach().clone() for c in cells]
    w0 = cells[3].cgru_1.conv_gates.weight.detach().clone()
    _, l = tr.train_step(dict(inputs))
    assert np.isfinite(float(l["loss"]))
    for c, q in zip(cells, frozen):
        assert torch.equal(c.h0_layer1.detach(), q) and c.h0_layer1.grad is None
    assert not torch.equal(cells[3].cgru_1.conv_gates.weight.detach(), w0)              # the rest keeps training
    tr.close()
