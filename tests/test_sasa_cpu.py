"""No-GPU checks of the self-attention encoder: the project's statement of the 7x7 local attention (tests/sasa_ref.py) against
the reference module's fp64 results (tests/golden/sasa.npz, written by tests/golden/make_golden_sasa.py), the facade's names,
shapes and parameter count, the Trainer's `model` switch with a checkpoint round trip, and the library's new entry points."""
import ctypes
import os

import numpy as np
import pytest
import torch

import sasa_ref as SR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(REPO, "tests", "golden", "sasa.npz"), allow_pickle=False)


def _rel(a, b):
    b = torch.as_tensor(b)
    den = float(b.abs().max())
    return float((a.detach() - b).abs().max()) / (den if den > 0 else 1.0)


@pytest.mark.parametrize("case", SR.GOLDEN_CASES, ids=SR.case_tag)
def test_statement_reproduces_the_reference_module(case, gold):
    """attention_conv and its autograd gradients, and the gather-form gradients stated directly, within 1e-12 relative of the
    reference module in fp64."""
    x, st, gy = SR.golden_inputs(case)
    tag = SR.case_tag(case)
    xr = x.clone().requires_grad_()
    sr = {k: v.clone().requires_grad_() for k, v in st.items()}
    y = SR.attention_conv(xr, sr)
    grads = torch.autograd.grad((y * gy).sum(), [xr] + [sr[k] for k in SR.PARAM_KEYS])
    errs = {"y": _rel(y, gold[tag + "_y"]), "gx": _rel(grads[0], gold[tag + "_gx"])}
    for k, g in zip(SR.PARAM_KEYS, grads[1:]):
        assert g.shape == gold[tag + "_g_" + k].shape
        errs[k] = _rel(g, gold[tag + "_g_" + k])
    # the formulas of the kernels' backward: same numbers without autograd
    F = torch.nn.functional
    q, k, v = (F.conv2d(x, st[n + "_conv.weight"]) for n in ("query", "key", "value"))
    yy, lse = SR.attention(q, k, v, st["rel_h"], st["rel_w"])
    dq, dk, dv, drh, drw = SR.attention_grads(q, k, v, st["rel_h"], st["rel_w"], yy, lse, gy)
    C = x.shape[1]
    w = lambda n: st[n + "_conv.weight"].view(C, C)
    gx = sum(torch.einsum("oi,bohw->bihw", w(n), d) for n, d in (("query", dq), ("key", dk), ("value", dv)))
    errs["formula gx"] = _rel(gx, gold[tag + "_gx"])
    errs["formula rel_h"] = _rel(drh, gold[tag + "_g_rel_h"])
    errs["formula rel_w"] = _rel(drw, gold[tag + "_g_rel_w"])
    for n, d in (("query", dq), ("key", dk), ("value", dv)):
        errs["formula " + n] = _rel(torch.einsum("bohw,bihw->oi", d, x).view(C, C, 1, 1), gold[tag + "_g_" + n + "_conv.weight"])
    print("sasa statement %s: %s" % (tag, " ".join("%s=%.1e" % kv for kv in errs.items())))
    assert max(errs.values()) <= TOL, errs


def test_wide_case_is_beyond_fp32_exp_range_and_fp32_stays_finite(gold):
    x, st, _ = SR.golden_inputs(SR.WIDE)
    L, amax = SR.logit_spread(x, st)
    assert L > 200 and amax > 100, (L, amax)            # exp(-L) underflows fp32; exp(amax) overflows it
    y32 = SR.attention_conv(x.float(), {k: v.float() for k, v in st.items()})
    assert bool(torch.isfinite(y32).all())
    assert _rel(y32.double(), gold[SR.case_tag(SR.WIDE) + "_y"]) < 1e-5


def test_groups_change_nothing(gold):
    """The reference module built with groups = 3 and with groups = 1 on the same 6-channel inputs: bit-identical output and
    input gradient -- the facade keeps `groups` for the constructor signature only."""
    tag = SR.case_tag(SR.GROUPS_CASE)
    g = tag + "_groups%d" % SR.GROUPS
    for k in ["_y", "_gx"] + ["_g_" + p for p in SR.PARAM_KEYS]:
        assert np.array_equal(gold[tag + k], gold[g + k]), k
    from networks.resnet_encoder_attention import AttentionConv
    a, b = AttentionConv(16, 16, 7, padding=3, groups=8), AttentionConv(16, 16, 7, padding=3, groups=1)
    assert [(k, v.shape) for k, v in a.state_dict().items()] == [(k, v.shape) for k, v in b.state_dict().items()]


def test_facade_names_shapes_and_parameter_count():
    import networks
    from networks.resnet_encoder_attention import AttentionConv
    enc = networks.ResnetEncoderAttention(18, False)
    plain = networks.ResnetEncoder(18, False)
    n = lambda m: sum(p.numel() for p in m.parameters())
    assert n(enc) - n(plain) == 1051200 == sum(3 * c * c + 2 * (c // 2) * 7 for c in (64, 128, 256, 512))
    keys = list(enc.state_dict())
    assert keys[:len(plain.state_dict())] == list(plain.state_dict())
    extra = keys[len(plain.state_dict()):]
    assert extra == ["atten%d.%s" % (i, k) for i in range(1, 5) for k in SR.PARAM_KEYS]
    sd = enc.state_dict()
    for i, c in enumerate((64, 128, 256, 512), start=1):
        assert sd["atten%d.rel_h" % i].shape == (c // 2, 1, 1, 7, 1) and sd["atten%d.rel_w" % i].shape == (c // 2, 1, 1, 1, 7)
        for k in ("key", "query", "value"):
            assert sd["atten%d.%s_conv.weight" % (i, k)].shape == (c, c, 1, 1)
    assert list(enc.num_ch_enc) == [64, 64, 128, 256, 512]
    assert isinstance(networks.ResnetEncoderAttention(34, False), networks.ResnetEncoder)
    for bad in (50, 101, 152):
        with pytest.raises(ValueError):
            networks.ResnetEncoderAttention(bad, False)
    with pytest.raises(ValueError):
        networks.ResnetEncoderAttention(19, False)
    for kw in (dict(kernel_size=3, padding=1), dict(kernel_size=7, padding=3, stride=2), dict(kernel_size=7, padding=2),
               dict(kernel_size=7, padding=3, bias=True)):
        with pytest.raises(NotImplementedError):
            AttentionConv(8, 8, **kw)
    with pytest.raises(NotImplementedError):
        AttentionConv(8, 16, kernel_size=7, padding=3)
    # the reference's init: rel ~ N(0, 1), the 1x1 weights kaiming (fan_out, relu): std sqrt(2 / C)
    torch.manual_seed(0)
    a = AttentionConv(256, 256, 7, padding=3, groups=8)
    assert abs(float(a.rel_h.detach().std()) - 1.0) < 0.1 and abs(float(a.key_conv.weight.detach().std()) - (2.0 / 256) ** 0.5) < 0.002


def test_local_attention_refuses_cpu_tensors():
    from depthcore import ops, _lib
    t = torch.rand(1, 4, 5, 5)
    with pytest.raises(_lib.DepthcoreError):
        ops.local_attention7(t, t, t, torch.rand(2, 7), torch.rand(2, 7))
    import networks
    with pytest.raises(_lib.DepthcoreError):
        networks.ResnetEncoderAttention(18, False).atten1(torch.rand(1, 64, 4, 4))


def test_trainer_builds_the_attention_encoder_and_round_trips_a_checkpoint(tmp_path):
    import networks
    import trainer as T
    kw = dict(batch_size=1, height=64, width=96, log_dir=str(tmp_path), model_name="run")
    for model in ("rn_encoder_with_attention",):
        a = T.Trainer(T.default_options(model=model, **kw), device="cpu", seed=1)
        assert type(a.models["encoder"]) is networks.ResnetEncoderAttention
        assert type(a.models["pose_encoder"]) is networks.ResnetEncoder           # the pose networks are unchanged
        folder = a.save_model(str(tmp_path / "w"))
        saved = torch.load(os.path.join(folder, "encoder.pth"), map_location="cpu")
        assert "atten4.value_conv.weight" in saved and saved["height"] == 64 and saved["width"] == 96
        b = T.Trainer(T.default_options(model=model, **kw), device="cpu", seed=2)
        sa, sb = a.models["encoder"].state_dict(), b.models["encoder"].state_dict()
        assert not torch.equal(sa["atten2.rel_h"], sb["atten2.rel_h"])
        b.load_model(folder, ["encoder", "depth", "pose_encoder", "pose"])
        sb = b.models["encoder"].state_dict()
        assert set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
        # the parameters reach the optimiser and the gradient buckets
        ids = {id(p) for p in b.parameters_to_train}
        assert all(id(p) in ids for p in b.models["encoder"].parameters())
    f = T.Trainer(T.default_options(model="rn_fusion", fusion="v3", frame_ids=[0, -2, -1, 1], **kw), device="cpu", seed=1)
    assert type(f.models["encoder"]) is networks.ResnetEncoderAttention and "fusion" in f.models


def test_other_model_strings_build_the_plain_encoder(tmp_path):
    import networks
    import trainer as T
    kw = dict(batch_size=1, height=64, width=96, log_dir=str(tmp_path), model_name="run")
    assert T.default_options(**kw).model == "dpt_gru"
    for o in (T.default_options(**kw), T.default_options(model="dpt", **kw), T.default_options(model="anything", **kw)):
        assert type(T.Trainer(o, device="cpu", seed=1).models["encoder"]) is networks.ResnetEncoder
    assert networks.depth_encoder_class(None) is networks.ResnetEncoder
    with pytest.raises(ValueError):
        T.Trainer(T.default_options(model="rn_fusion", **kw), device="cpu", seed=1)


def test_scripts_build_the_encoder_from_model(tmp_path):
    import argparse
    import evaluate_depth as ED
    import networks
    import trainer as T
    kw = dict(batch_size=1, height=64, width=96, log_dir=str(tmp_path), model_name="run")
    att = T.Trainer(T.default_options(model="rn_encoder_with_attention", **kw), device="cpu", seed=1).save_model(str(tmp_path / "w"))
    plain = T.Trainer(T.default_options(**kw), device="cpu", seed=1).save_model(str(tmp_path / "p"))
    ns = lambda folder, **k: argparse.Namespace(load_weights_folder=folder, num_layers=18, **k)
    saved = torch.load(os.path.join(att, "encoder.pth"), map_location="cpu")
    for model in ("rn_encoder_with_attention", "rn_fusion"):
        enc, _, h, w = ED.load_networks(ns(att, model=model), "cpu")
        assert type(enc) is networks.ResnetEncoderAttention and (h, w) == (64, 96)
        assert torch.equal(enc.state_dict()["atten1.rel_w"], saved["atten1.rel_w"])
    assert type(ED.load_networks(ns(plain, model="dpt_gru"), "cpu")[0]) is networks.ResnetEncoder
    # weights of the other class are refused, in both directions: no attention layer is dropped or left at its init silently
    for folder, model in ((att, "dpt_gru"), (plain, "rn_encoder_with_attention")):
        with pytest.raises(ValueError):
            ED.load_networks(ns(folder, model=model), "cpu")
    # a caller without a `model` option (test_simple.py's predict_folder) gets the class the checkpoint was saved from
    enc = ED.load_networks(ns(att), "cpu")[0]
    assert type(enc) is networks.ResnetEncoderAttention and torch.equal(enc.state_dict()["atten4.rel_h"], saved["atten4.rel_h"])
    assert type(ED.load_networks(ns(plain), "cpu")[0]) is networks.ResnetEncoder


def test_library_exports_and_workspace_query():
    from depthcore import _lib
    L = _lib.lib()
    for n in ("dc_sasa_plan", "dc_sasa_fwd", "dc_sasa_bwd_workspace", "dc_sasa_bwd"):
        assert hasattr(L, n) and n in _lib.EXPORTS, n
    plan = (ctypes.c_int * 5)()
    for bad in ((0, 4, 8, 8), (-1, 4, 8, 8), (1, 3, 8, 8), (1, 1, 8, 8), (1, 0, 8, 8), (1, 4, 0, 8), (1, 4, 8, 0), (1, 4, -6, 30),
                (2, 4, 16384, 16384), (1, 2, 2 ** 30, 1), (2 ** 16, 2 ** 15, 1, 1)):
        assert L.dc_sasa_bwd_workspace(*bad) == 0, bad
        assert L.dc_sasa_plan(*bad, plan) == -1, bad
    assert L.dc_sasa_plan(1, 4, 8, 8, None) == -1
    # balanced tiles of at most 16 x 32; small planes share a block (at most 768 pixels, 1536 staged elements per array)
    for shape, want in [((12, 64, 48, 160), (16, 32, 5, 3, 1)), ((12, 128, 24, 80), (12, 27, 3, 2, 2)),
                        ((12, 256, 12, 40), (12, 20, 2, 1, 3)), ((12, 512, 6, 20), (6, 20, 1, 1, 4)),
                        ((1, 2, 1, 1), (1, 1, 1, 1, 2)), ((1, 64, 1, 1), (1, 1, 1, 1, 31)), ((2, 4, 17, 33), (9, 17, 2, 2, 4))]:
        assert L.dc_sasa_plan(*shape, plan) == 0 and tuple(plan) == want, (shape, tuple(plan))
        th, tw, nx, ny, np_ = want
        assert th * tw * np_ <= 768 and (th + 6) * (tw + 6) * np_ <= 1536
        B, C = shape[:2]
        assert L.dc_sasa_bwd_workspace(*shape) == nx * ny * -(-B * C // np_) * np_ * 7 * 4
