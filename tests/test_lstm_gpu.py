"""f3: the ConvLSTM v8 front-end on the HIP path.

Kernels (dc_lstm_cell_*, dc_lstm_handover_*) against tests/lstm_ref.py evaluated in fp64.  The tolerance is not a constant: a
kernel's error may be at most 4 times the error that the stock fp32 torch statement of the same formula (lstm_ref in float32,
on the CPU, same inputs) has against the same fp64 oracle -- the factor covers device exp / tanh differing in the last bits.
"Error" is the Euclidean norm of the difference to the oracle over a whole output tensor: the sum over the elements is what a
last-bit difference of single elements averages out in (the 1x1 shapes have 8 elements), and it is not divided by anything, so
the ratio of two errors is what is compared.  Each ratio is printed before it is judged.

Modules (networks.ConvLSTMCell_v1, FeatureFusionBlock_v2, ConvGRUBlocks_v8) against the reference's outputs and gradients
(tests/golden/convlstm_v8.npz), run_sequence against the frame loop, and the trainer with gru="v8"."""
import os

import numpy as np
import pytest
import torch

import lstm_ref as LR
import make_golden as MG
import make_golden_lstm as ML
from helpers import T, close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 4.0
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convlstm_v8.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD, allow_pickle=False)


def _err(x, ref64):
    return float((x.detach().cpu().double() - ref64).norm())


def _judge(tag, got, base32, ref64):
    """got: device tensors; base32: the fp32 CPU statement's; ref64: the oracle's -- tensor by tensor."""
    for name in ref64:
        if ref64[name] is None:
            assert got[name] is None
            continue
        e, b = _err(got[name], ref64[name]), _err(base32[name], ref64[name])
        print("%s %-8s device %.3e  fp32-torch %.3e  ratio %.2f" % (tag, name, e, b, e / max(b, 1e-300)))
        assert e <= FACTOR * b, "%s %s: error %.3e exceeds %g x the fp32 torch statement's %.3e" % (tag, name, e, FACTOR, b)


def _block():
    from depthcore import _lib
    return _lib.lib().dc_lstm_block()


# ---- the cell ------------------------------------------------------------------------------------------------------------
# (B, C, h, w): the issue's three, then two whose plane spans more than one block of the launch with a ragged last block --
# the launch has dc_lstm_block() = 256 threads per block and blockIdx.y = the batch item, so per item:
#   (1, 4, 9, 37): C * P = 1332 is a multiple of 4 -> the float4 body, 333 groups = one full block + 77 threads of a second;
#   (2, 3, 7, 43): C * P = 903 is odd -> the scalar loop, three full blocks + 135 threads of a fourth.
CELL_SHAPES = [(2, 1, 3, 5), (1, 3, 2, 4), (2, 4, 1, 1), (1, 4, 9, 37), (2, 3, 7, 43)]


def test_ragged_shapes_are_what_the_comment_says():
    blk = _block()
    assert (4 * 9 * 37) % 4 == 0 and blk < 4 * 9 * 37 // 4 < 2 * blk and (4 * 9 * 37 // 4) % blk
    assert (3 * 7 * 43) % 4 and 3 * 7 * 43 > blk and (3 * 7 * 43) % blk
    assert 2 * 9 * (68 // 4) > blk and (2 * 9 * (68 // 4)) % blk and 68 % 4 == 0      # hand-over, float4 form: items
    assert (4 * 9 * 13) > blk and (4 * 9 * 13) % blk and 13 % 4                       # hand-over, scalar form: elements


def _cell_inputs(B, C, h, w, bcast, seed):
    g = torch.Generator().manual_seed(seed)
    cc = 2.0 * torch.randn(B, 4 * C, h, w, generator=g)                 # N(0, 2^2): saturated and unsaturated gates
    c = torch.randn(1 if bcast else B, C, h, w, generator=g)
    return cc, c, torch.randn(B, C, h, w, generator=g), torch.randn(B, C, h, w, generator=g)


def _cell_oracle(cc, c, g_h, g_c, dtype):
    cc, c = cc.to(dtype).requires_grad_(), c.to(dtype).requires_grad_()
    hn, cn = LR.lstm_cell(cc, c.expand(cc.shape[0], -1, -1, -1))
    tot = 0
    if g_h is not None:
        tot = tot + (hn * g_h.to(dtype)).sum()
    if g_c is not None:
        tot = tot + (cn * g_c.to(dtype)).sum()
    d_cc, d_c = torch.autograd.grad(tot, [cc, c])
    return dict(h_next=hn.detach(), c_next=cn.detach(), d_cc=d_cc, d_c_cur=d_c)


@pytest.mark.parametrize("bcast", [False, True])
@pytest.mark.parametrize("shape", CELL_SHAPES)
def test_cell_kernels_vs_fp64(shape, bcast):
    from depthcore import ops
    B, C, h, w = shape
    cc, c, g_h, g_c = _cell_inputs(B, C, h, w, bcast, 100 + B + 7 * C + h * w)
    ref, base = _cell_oracle(cc, c, g_h, g_c, torch.float64), _cell_oracle(cc, c, g_h, g_c, torch.float32)
    runs = []
    for _ in range(2):
        a, b = cc.to(DEV).requires_grad_(), c.to(DEV).requires_grad_()
        hn, cn = ops.lstm_cell(a, b)
        d_cc, d_c = torch.autograd.grad((hn * g_h.to(DEV)).sum() + (cn * g_c.to(DEV)).sum(), [a, b])
        runs.append(dict(h_next=hn.detach(), c_next=cn.detach(), d_cc=d_cc, d_c_cur=d_c))
    assert runs[0]["d_c_cur"].shape == c.shape
    _judge("cell %s%s" % (shape, " bcast" if bcast else ""), runs[0], base, ref)
    for k in ref:
        assert torch.equal(runs[0][k], runs[1][k]), k


@pytest.mark.parametrize("null", ["g_h", "g_c"])
@pytest.mark.parametrize("shape", [(2, 1, 3, 5), (1, 4, 9, 37)])
def test_cell_bwd_null_gradient(shape, null):
    """The raw entry with g_h or g_c NULL: the gradient of that output is zero (the last frame's cell state has no consumer)."""
    from depthcore import _lib
    L = _lib.lib()
    B, C, h, w = shape
    cc, c, g_h, g_c = _cell_inputs(B, C, h, w, False, 200 + C)
    if null == "g_h":
        g_h = None
    else:
        g_c = None
    ref, base = _cell_oracle(cc, c, g_h, g_c, torch.float64), _cell_oracle(cc, c, g_h, g_c, torch.float32)
    a, b = cc.to(DEV), c.to(DEV)
    gh, gc = (None if g_h is None else g_h.to(DEV)), (None if g_c is None else g_c.to(DEV))
    runs = []
    for _ in range(2):
        d_cc, d_c = torch.full_like(a, float("nan")), torch.full_like(b, float("nan"))
        _lib.check(L.dc_lstm_cell_bwd(_lib.ptr(a), _lib.ptr(b), _lib.ptr(gh), _lib.ptr(gc), _lib.ptr(d_cc), _lib.ptr(d_c), B, C, h * w,
                                      _lib.stream(a)), "dc_lstm_cell_bwd")
        runs.append(dict(d_cc=d_cc, d_c_cur=d_c))
    _judge("cell %s %s=NULL" % (shape, null), runs[0], {k: base[k] for k in runs[0]}, {k: ref[k] for k in runs[0]})
    assert torch.equal(runs[0]["d_cc"], runs[1]["d_cc"]) and torch.equal(runs[0]["d_c_cur"], runs[1]["d_c_cur"])


# ---- the hand-over ------------------------------------------------------------------------------------------------------
# the cell's (B, h, w) with C in {4, 8}; then (1, 8, 9, 68): w % 4 == 0 -> the float4 form, 306 items = one full block + 50
# threads; (1, 4, 9, 13): the scalar form, 468 elements = one full block + 212 threads
HAND_SHAPES = [(2, C, 3, 5) for C in (4, 8)] + [(1, C, 2, 4) for C in (4, 8)] + [(2, C, 1, 1) for C in (4, 8)] + \
    [(1, 8, 9, 68), (1, 4, 9, 13)]


def _hand_inputs(B, C, h, w, bcast, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, C, h, w, generator=g), torch.randn(1 if bcast else B, C, h, w, generator=g),
            torch.randn(B, C, h, w, generator=g), torch.randn(B, C, h, w, generator=g),
            torch.randn(B, C // 4, 2 * h, 2 * w, generator=g))


def _hand_oracle(a, hp, hn, g_pre, g_up, dtype, need_up=True):
    a, hp, hn = [t.to(dtype).requires_grad_() for t in (a, hp, hn)]
    pre, up = LR.handover(a, hp.expand_as(a), hn, need_up)
    tot = 0
    if g_pre is not None:
        tot = tot + (pre * g_pre.to(dtype)).sum()
    if g_up is not None and need_up:
        tot = tot + (up * g_up.to(dtype)).sum()
    d = torch.autograd.grad(tot, [a, hp, hn])
    return dict(pre=pre.detach(), up=None if up is None else up.detach(), d_a=d[0], d_h_prev=d[1], d_h_new=d[2])


@pytest.mark.parametrize("bcast", [False, True])
@pytest.mark.parametrize("shape", HAND_SHAPES)
def test_handover_kernels_vs_fp64(shape, bcast):
    from depthcore import ops
    B, C, h, w = shape
    a, hp, hn, g_pre, g_up = _hand_inputs(B, C, h, w, bcast, 300 + B + 7 * C + h * w)
    ref = _hand_oracle(a, hp, hn, g_pre, g_up, torch.float64)
    base = _hand_oracle(a, hp, hn, g_pre, g_up, torch.float32)
    assert 0.2 < float((ref["pre"] == 0).double().mean()) < 0.8 or ref["pre"].numel() <= 16      # both sides of the ReLU occur
    runs = []
    for _ in range(2):
        x = [t.to(DEV).requires_grad_() for t in (a, hp, hn)]
        pre, up = ops.lstm_handover(*x)
        d = torch.autograd.grad((pre * g_pre.to(DEV)).sum() + (up * g_up.to(DEV)).sum(), x)
        runs.append(dict(pre=pre.detach(), up=up.detach(), d_a=d[0], d_h_prev=d[1], d_h_new=d[2]))
    assert runs[0]["up"].shape == (B, C // 4, 2 * h, 2 * w) and runs[0]["d_h_prev"].shape == hp.shape
    _judge("hand-over %s%s" % (shape, " bcast" if bcast else ""), runs[0], base, ref)
    for k in ref:
        assert torch.equal(runs[0][k], runs[1][k]), k


@pytest.mark.parametrize("null", ["up", "g_pre", "g_up"])
@pytest.mark.parametrize("shape", [(2, 4, 3, 5), (1, 8, 9, 68)])
def test_handover_null_arguments(shape, null):
    """up NULL (the finest block has no hand-over: only pre is written), g_pre NULL, g_up NULL -- through the raw entries."""
    from depthcore import _lib
    L = _lib.lib()
    B, C, h, w = shape
    a, hp, hn, g_pre, g_up = _hand_inputs(B, C, h, w, False, 400 + C)
    need_up = null != "up"
    if null == "g_pre":
        g_pre = None
    if null in ("g_up", "up"):
        g_up = None
    ref = _hand_oracle(a, hp, hn, g_pre, g_up, torch.float64, need_up)
    base = _hand_oracle(a, hp, hn, g_pre, g_up, torch.float32, need_up)
    da, dhp, dhn = a.to(DEV), hp.to(DEV), hn.to(DEV)
    gp, gu = (None if g_pre is None else g_pre.to(DEV)), (None if g_up is None else g_up.to(DEV))
    runs = []
    for _ in range(2):
        pre = torch.full_like(da, float("nan"))
        up = torch.full((B, C // 4, 2 * h, 2 * w), float("nan"), device=DEV) if need_up else None
        _lib.check(L.dc_lstm_handover_fwd(_lib.ptr(da), _lib.ptr(dhp), _lib.ptr(dhn), _lib.ptr(pre), _lib.ptr(up), B, C, h, w,
                                          _lib.stream(da)), "dc_lstm_handover_fwd")
        d = [torch.full_like(da, float("nan")) for _ in range(3)]
        _lib.check(L.dc_lstm_handover_bwd(_lib.ptr(pre), _lib.ptr(gp), _lib.ptr(gu), _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]),
                                          B, C, h, w, _lib.stream(da)), "dc_lstm_handover_bwd")
        runs.append(dict(pre=pre, up=up, d_a=d[0], d_h_prev=d[1], d_h_new=d[2]))
    _judge("hand-over %s %s=NULL" % (shape, null), runs[0], base, ref)
    for k in ref:
        assert (runs[0][k] is None and runs[1][k] is None) or torch.equal(runs[0][k], runs[1][k]), k


# ---- modules against the reference's fixtures --------------------------------------------------------------------------
# the tolerances of test_gru_gpu.py's v5 block (the same convolution kernels over 2 frames)
OUT_TOL = dict(rtol=1e-3, atol=1e-3)
GIN_TOL = dict(rtol=2e-3, atol=2e-5)
GPAR_TOL = dict(rtol=5e-3, atol=5e-5)


def _check(name, got, want, rtol, atol):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    worst = float(np.max(np.abs(got - want) / (atol + rtol * np.abs(want))))
    print("%-44s worst |diff| / (atol + rtol |want|) = %.3f" % (name, worst))
    close(got, want, rtol=rtol, atol=atol, msg=name)


def test_cell_module_vs_reference_fixture(gold):
    import networks
    c = ML.CELL
    cell = networks.ConvLSTMCell_v1(c["Cin"], c["Chid"], (3, 3), True)
    MG.seeded_state(cell, c["wseed"], c["wscale"])
    cell = cell.to(DEV)
    x, h, cc, cot_h, cot_c = [t.to(DEV) for t in ML.cell_inputs()]
    leaves = [t.requires_grad_() for t in (x, h, cc)]
    hn, cn = cell(leaves[0], (leaves[1], leaves[2]))
    _check("cell_h", hn, gold["cell_h"], **OUT_TOL)
    _check("cell_c", cn, gold["cell_c"], **OUT_TOL)
    ps = dict(cell.named_parameters())
    gr = torch.autograd.grad((hn * cot_h).sum() + (cn * cot_c).sum(), leaves + list(ps.values()))
    for got, k in zip(gr[:3], ("cell_gx", "cell_gh", "cell_gc")):
        _check(k, got, gold[k], **GIN_TOL)
    for got, k in zip(gr[3:], ps):
        _check("cell_g_" + k, got, gold["cell_g_" + k], **GPAR_TOL)


def test_fusion_block_module_vs_reference_fixture(gold):
    import networks
    c = ML.FUS
    blk = networks.FeatureFusionBlock_v2(c["C"], up=True, attention=False)
    MG.seeded_state(blk, c["wseed"], c["wscale"])
    blk = blk.to(DEV)
    i1, i2, cot_o, cot_u = [t.to(DEV) for t in ML.fus_inputs()]
    i1.requires_grad_(); i2.requires_grad_()
    o, u = blk(i1, i2)
    _check("fus_out", o, gold["fus_out"], **OUT_TOL)
    _check("fus_up", u, gold["fus_up"], **OUT_TOL)
    assert float(u.detach().min()) == 0.0                      # tanh(relu(.)): the in-place ReLU of the reference
    ps = dict(blk.named_parameters())
    gr = torch.autograd.grad((o * cot_o).sum() + (u * cot_u).sum(), [i1, i2] + list(ps.values()))
    _check("fus_g1", gr[0], gold["fus_g1"], **GIN_TOL)
    _check("fus_g2", gr[1], gold["fus_g2"], **GIN_TOL)
    for got, k in zip(gr[2:], ps):
        _check("fus_g_" + k, got, gold["fus_g_" + k], **GPAR_TOL)


def test_blocks_v8_forward_chain_vs_reference_fixture(gold):
    """ConvGRUBlocks_v8.forward chained over the two frames of fixture (c) from the seeded initial states that are passed in."""
    import networks
    c = ML.V8
    v8 = networks.ConvGRUBlocks_v8(kernel_size=(3, 3), bias=True, device="cpu", attention=False)
    assert list(v8.state_dict().keys()) == list(gold["v8_keys"])
    MG.seeded_state(v8, c["wseed"], c["wscale"])
    v8 = v8.to(DEV)
    dec, states, cots = ML.v8_inputs()
    dec = [d.to(DEV).requires_grad_() for d in dec]
    states = [(h.to(DEV).requires_grad_(), cc.to(DEV).requires_grad_()) for h, cc in states]
    cur, tot = states, 0
    for i in range(c["n"]):
        cur, disp = v8({("disp", s): dec[s][i:i + 1] for s in range(4)}, cur)
        for s in range(4):
            _check("v8_disp%d_%d" % (s, i), disp[("disp", s)], gold["v8_disp%d_%d" % (s, i)], **OUT_TOL)
            tot = tot + (disp[("disp", s)] * cots[s][i:i + 1].to(DEV)).sum()
    ps = {k: p for k, p in v8.named_parameters() if not k.endswith(("h0_layer1", "c0_layer1"))}
    flat = [t for hc in states for t in hc]
    gr = torch.autograd.grad(tot, dec + list(ps.values()) + flat)
    for s in range(4):
        _check("v8_gdec%d" % s, MG.summ(gr[s]), gold["v8_gdec%d" % s], **GIN_TOL)
        _check("v8_gh%d" % s, MG.summ(gr[4 + len(ps) + 2 * s]), gold["v8_gh%d" % s], **GIN_TOL)
        _check("v8_gc%d" % s, MG.summ(gr[4 + len(ps) + 2 * s + 1]), gold["v8_gc%d" % s], **GIN_TOL)
    for j, k in enumerate(ps):
        _check("v8_g_" + k, MG.summ(gr[4 + j]), gold["v8_g_" + k], **GPAR_TOL)


def test_run_sequence_is_the_frame_loop():
    import networks
    torch.manual_seed(7)
    H, W, n = 32, 64, 3
    v8 = networks.ConvGRUBlocks_v8((3, 3), True, "cpu", height=H, width=W).to(DEV)
    dec = {("disp", s): torch.randn(n, LR.NUM_CH_DEC[s], H >> s, W >> s, device=DEV).requires_grad_() for s in range(4)}
    out = v8.run_sequence(dec)
    states = v8.initial_states()
    for i in range(n):
        states, disp = v8({k: v[i:i + 1] for k, v in dec.items()}, states)
        for s in range(4):
            assert torch.equal(out[("disp", s)][i:i + 1], disp[("disp", s)]), (s, i)
    assert [tuple(out[("disp", s)].shape) for s in range(4)] == [(n, 1, H >> s, W >> s) for s in range(4)]
    sum(o.sum() for o in out.values()).backward()
    for cell in v8.cells():
        for p in (cell.h0_layer1, cell.c0_layer1):
            assert p.grad is not None and float(p.grad.abs().sum()) > 0
    assert all(d.grad is not None and float(d.grad.abs().sum()) > 0 for d in dec.values())


def test_trainer_v8(tmp_path):
    """gru="v8" at 64x96 on a synthetic 2-frame sequence: training, the dispconvs left alone, the freeze of h0 and c0,
    val_sequence, and a checkpoint round trip."""
    import trainer as T_
    from depthcore.synthetic import synthetic_depth_gt, synthetic_sequence_batch
    H, W, n = 64, 96, 2
    kw = dict(batch_size=1, height=H, width=W, gru="v8", len_sequence=n, log_dir=str(tmp_path), model_name="v8")
    tr = T_.Trainer(T_.default_options(**kw), device=DEV, seed=0)
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
        for p in (cell.h0_layer1, cell.c0_layer1):
            assert float(p.detach().abs().sum()) > 0                # moved away from its zero initialisation
    sd = tr.models["depth"].state_dict()
    for k, v in dispconv0.items():
        assert torch.equal(sd[k], v), k                             # no gradient, and Adam leaves them untouched
    # val_sequence: the four disparities; parameters, buffers, the step count and the training mode are left where they were
    before = {name: {k: v.clone() for k, v in m.state_dict().items()} for name, m in tr.models.items()}
    step0 = tr.step
    vin = dict(inputs)
    vin["depth_gt"] = synthetic_depth_gt(n, torch.device(DEV), 3)
    vout, vl = tr.val_sequence(vin)
    assert all(tuple(vout[("disp", s)].shape) == (n, 1, H >> s, W >> s) for s in range(4))
    assert np.isfinite(float(vl["loss"])) and all(np.isfinite(vl[m]) for m in tr.depth_metric_names)
    assert tr.step == step0 and all(m.training for m in tr.models.values())
    for name, m in tr.models.items():
        for k, v in m.state_dict().items():
            assert torch.equal(v, before[name][k]), (name, k)
    # checkpoint: a fresh trainer that loads it takes the same next step (the tie-break noise is seeded by the step count)
    folder = tr.save_model(str(tmp_path / "w"))
    assert "cgru_3.c0_layer1" in torch.load(os.path.join(folder, "gru.pth"), map_location="cpu")
    other = T_.Trainer(T_.default_options(**kw), device=DEV, seed=5)
    other.load_model(folder)
    other.set_train()
    other.step = tr.step
    _, la = tr.train_step(dict(inputs))
    _, lb = other.train_step(dict(inputs))
    assert float(la["loss"]) == float(lb["loss"]) and torch.equal(la["loss"], lb["loss"])
    other.close()
    # from h_s_epoch on the learned initial states, h0 and c0, stop training (trainer_gru.py:303-307)
    tr.freeze_hidden_states()
    frozen = [p.detach().clone() for cell in cells for p in (cell.h0_layer1, cell.c0_layer1)]
    w0 = cells[3].clstm_1.conv.weight.detach().clone()
    _, l = tr.train_step(dict(inputs))
    assert np.isfinite(float(l["loss"]))
    for p, q in zip([p for cell in cells for p in (cell.h0_layer1, cell.c0_layer1)], frozen):
        assert torch.equal(p.detach(), q) and p.grad is None
    assert not torch.equal(cells[3].clstm_1.conv.weight.detach(), w0)          # the rest keeps training
    tr.close()
