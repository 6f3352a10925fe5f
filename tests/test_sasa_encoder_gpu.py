"""networks.ResnetEncoderAttention on the HIP path: forward and every parameter gradient against the fp64 encoder statement of
tests/sasa_ref.py with the procedure and the gate of tests/test_encoder_gpu.py (KinkTape: the HIP forward's ReLU / max-pool
decisions are imposed on the oracle, legitimate only on near-ties; every tensor within max(2 x the fp32 oracle's own error, 2.5e-5));
eval mode under no_grad, module by module and without a framework kernel; and the Trainer with model="rn_encoder_with_attention"
(steps, SkipSum bookkeeping, bf16 networks, a captured step, the Fusion_v3 front-end, validation and prediction)."""
import os

import numpy as np
import pytest
import torch

import sasa_ref as SR
from helpers import rel_l2
from kink_tape import KinkTape

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODEL = "rn_encoder_with_attention"


def _oracle(state, x, cots, num_layers, dtype, tape):
    from oracle.kinks import ForcedKinks
    st = {k: (v.to(dtype).requires_grad_() if v.is_floating_point() and "running" not in k else
              (v.to(dtype) if v.is_floating_point() else v)) for k, v in state.items()}
    kn = ForcedKinks(tape, keep_pre=True)
    feats = SR.encoder_forward(st, x.to(dtype), num_layers, training=True, kinks=kn)
    kn.done()
    loss = sum((f * c.to(dtype)).sum() for f, c in zip(feats, cots))
    names = [k for k, v in st.items() if v.requires_grad and ".fc." not in k]
    return feats, dict(zip(names, torch.autograd.grad(loss, [st[k] for k in names]))), kn


@pytest.mark.parametrize("num_layers,B,H,W", [(18, 2, 64, 96), (18, 4, 64, 128), (34, 2, 64, 128)])
def test_attention_encoder_forward_and_all_gradients_vs_fp64_statement(num_layers, B, H, W):
    """The layer-4 map is 2 x 3 / 2 x 4: almost every tap of its attention is padding."""
    import networks
    from oracle.kinks import uncalibrated_disagreements
    torch.manual_seed(0)
    enc = networks.ResnetEncoderAttention(num_layers, False).to(DEV)
    enc.train()
    state = {k: v.detach().cpu().clone() for k, v in enc.state_dict().items()}
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 3, H, W, generator=g)
    with KinkTape() as tape:
        got = enc(x.to(DEV))
    assert [tuple(f.shape) for f in got] == [(B, c, H >> (i + 1), W >> (i + 1)) for i, c in enumerate((64, 64, 128, 256, 512))]
    cots = [torch.randn(f.shape, generator=g) / f[0].numel() ** 0.5 for f in got]
    loss = sum((f * c.to(DEV)).sum() for f, c in zip(got, cots))
    params = {n: p for n, p in enc.named_parameters() if not n.startswith("encoder.fc.")}
    gh_p = dict(zip(params.keys(), torch.autograd.grad(loss, list(params.values()))))
    assert sum(n.startswith("atten") for n in gh_p) == 20

    f64, g64, kn64 = _oracle(state, x, cots, num_layers, torch.float64, tape.entries)
    f32, g32, kn32 = _oracle(state, x, cots, num_layers, torch.float32, tape.entries)
    assert sum(1 for k, _ in tape.entries if k == "relu") == {18: 17, 34: 33}[num_layers]
    far = uncalibrated_disagreements(kn64, kn32)
    assert not far, ("a HIP ReLU / max-pool decision differs from fp64 away from a tie (kind, entry, count, margin, fp32 error)", far)

    bound = lambda e32: max(2.0 * e32, 2.5e-5)
    bad, used, worst_att = [], 0.0, 0.0
    rows = [("feature %d" % i, got[i], f64[i], f32[i]) for i in range(5)]
    assert set(g64) == set(gh_p)
    rows += [(k, gh_p[k], g64[k], g32[k]) for k in g64]
    for name, a, r64, r32 in rows:
        e, e32 = rel_l2(a, r64), rel_l2(r32, r64)
        used = max(used, e / bound(e32))
        if name.startswith("atten") or name.startswith("feature"):
            worst_att = max(worst_att, e)
            print("sasa_encoder resnet%d %dx%dx%d %-28s e_hip=%.3e e32=%.3e bound=%.3e" % (num_layers, B, H, W, name, e, e32, bound(e32)))
        if e > bound(e32):
            bad.append((name, e, e32))
    print("sasa_encoder resnet%d %dx%dx%d: %d decisions differ from fp64; worst feature / attention-gradient error %.2e; largest "
          "fraction of max(2 x e32, 2.5e-5) used by any tensor: %.2f" % (num_layers, B, H, W, sum(d[2] for d in kn64.disagree), worst_att, used))
    assert not bad, sorted(bad, key=lambda t: -t[1])[:8]


def test_eval_forward_is_the_modules_one_by_one_and_enters_no_framework_kernel():
    import networks
    from networks.resnet_encoder import _bn_act, _conv
    from depthcore import ops
    from test_val_gpu import _Census
    torch.manual_seed(0)
    enc = networks.ResnetEncoderAttention(18, False).to(DEV)
    enc.eval()
    x = torch.rand(2, 3, 64, 128, generator=torch.Generator().manual_seed(2)).to(DEV)
    with torch.no_grad():
        feats = [f.clone() for f in enc(x)]
        torch.cuda.synchronize()
        with _Census() as cen:
            again = enc(x)
            torch.cuda.synchronize()
        assert dict(cen.count) == {}, dict(cen.count)
        assert all(torch.equal(a, b) for a, b in zip(feats, again))
        e = enc.encoder
        t = _bn_act(ops.stem_conv((x,), e.conv1.weight) if ops.stem_supported((x,), e.conv1.weight) else _conv(e.conv1, (x - 0.45) / 0.225),
                    e.bn1)
        assert torch.equal(t, feats[0])
        t = ops.maxpool3x3s2(t)
        for i in range(1, 5):
            t = getattr(e, "layer%d" % i)(t)
            a = getattr(enc, "atten%d" % i)
            q, k, v = (ops.conv1x1(t, c.weight) for c in (a.query_conv, a.key_conv, a.value_conv))
            t = ops.local_attention7(q, k, v, a.rel_h, a.rel_w)
            assert torch.equal(t, feats[i]), i


def _trainer(seed=5, **kw):
    import trainer as T
    o = T.default_options(batch_size=kw.pop("batch_size", 2), height=64, width=128, model=kw.pop("model", MODEL), **kw)
    tr = T.Trainer(o, device=DEV, seed=seed)
    tr.set_train()
    return tr


def _batch(seed=2, **kw):
    from depthcore.synthetic import synthetic_batch
    return synthetic_batch(2, 64, 128, torch.device(DEV), seed=seed, **kw)


def test_three_training_steps_with_the_attention_encoder():
    import networks
    from depthcore import ops
    tr = _trainer()
    assert type(tr.models["encoder"]) is networks.ResnetEncoderAttention
    inputs = _batch()
    ls = []
    for _ in range(3):
        _, l = tr.train_step(dict(inputs))
        ops.assert_no_dangling_sums()
        ls.append(float(l["loss"].detach()))
    print("sasa_encoder trainer losses", ls)
    assert all(np.isfinite(ls)) and ls[1] <= ls[0] and ls[2] <= ls[1], ls
    for n, p in tr.models["encoder"].named_parameters():
        assert (p.grad is not None) or n.startswith("encoder.fc."), n
        assert p.grad is None or bool(torch.isfinite(p.grad).all()), n


def test_gradient_sums_in_kernel_epilogues_change_nothing_with_the_attention_encoder(monkeypatch):
    """The tagged feature map is now the attention output; its SkipSum is collected by the next stage's first block as before.
    Bound as in tests/test_train_gpu.py::test_gradient_sums_in_kernel_epilogues_change_nothing: every parameter gradient equals the
    autograd-summed one to fp32 summation order, rel_l2 < 1e-5, the loss bit for bit."""
    from networks import resnet_encoder as RE
    from depthcore import ops
    res = {}
    for on in (True, False):
        monkeypatch.setattr(RE, "SKIP_SUMS", on)
        tr = _trainer(seed=3, cpu_tiebreak_noise=True)
        torch.manual_seed(1234)
        tr.buckets.zero()
        _, losses = tr.process_batch(dict(_batch()))
        losses["loss"].backward()
        ops.assert_no_dangling_sums()
        res[on] = {(k, n): p.grad.detach().clone() for k, m in tr.models.items() for n, p in m.named_parameters() if p.grad is not None}
        res[on]["loss"] = losses["loss"].detach().clone()
    assert torch.equal(res[True]["loss"], res[False]["loss"]) and set(res[True]) == set(res[False])
    assert any(k[1].startswith("atten") for k in res[True] if k != "loss")
    worst = max((rel_l2(res[True][k], res[False][k]), k) for k in res[True])
    print("sasa_encoder SkipSum on / off: worst rel_l2", worst)
    assert worst[0] < 1e-5, worst


def test_bf16_networks_run_one_finite_step():
    tr = _trainer(nets_dtype="bf16")
    _, l = tr.train_step(dict(_batch()))
    assert bool(torch.isfinite(l["loss"]))
    assert all(bool(torch.isfinite(p.grad).all()) for p in tr.models["encoder"].parameters() if p.grad is not None)


def test_hip_graph_replays_like_eager_steps():
    """As tests/test_train_gpu.py::test_hip_graph_replays_train_like_eager_steps, with the attention encoder in the captured step."""
    def run(graph, n=6):
        tr = _trainer(hip_graph=graph)
        batches = [_batch(s) for s in (2, 3)]
        losses = [float(tr.train_step(dict(batches[i % 2]))[1]["loss"].detach()) for i in range(n)]
        captured = tr._graph is not None
        tr.wino_cache.close()
        return losses, captured

    le, ce = run(False)
    lg, cg = run(True)
    assert cg and not ce
    assert np.allclose(le[:3], lg[:3], rtol=1e-5), (le, lg)
    assert np.allclose(le, lg, rtol=5e-4), (le, lg)
    assert len(set(round(v, 7) for v in lg[3:])) == len(lg[3:])


def test_rn_fusion_runs_one_finite_step():
    import networks
    tr = _trainer(model="rn_fusion", fusion="v3", frame_ids=[0, -2, -1, 1])
    assert type(tr.models["encoder"]) is networks.ResnetEncoderAttention and "fusion" in tr.models
    _, l = tr.train_step(_batch(frame_ids=(0, -2, -1, 1)))
    assert bool(torch.isfinite(l["loss"]))
    import trainer as T
    with pytest.raises(ValueError):
        T.Trainer(T.default_options(batch_size=2, height=64, width=128, model="rn_fusion"), device=DEV)


def test_val_and_predict_disparities_with_the_attention_encoder():
    from depthcore import evaluate as E
    from depthcore.synthetic import synthetic_depth_gt
    tr = _trainer()
    inputs = _batch()
    inputs["depth_gt"] = synthetic_depth_gt(2, torch.device(DEV), seed=2)
    outputs, losses = tr.val(dict(inputs))
    assert "de/abs_rel" in losses and all(np.isfinite(float(v)) for v in losses.values()), losses
    assert bool(torch.isfinite(outputs[("disp", 0)]).all())
    assert tr.models["encoder"].training                      # val leaves the trainer in training mode
    disp = E.predict_disparities(tr.models["encoder"], tr.models["depth"], inputs[("color", 0, 0)])
    assert disp.shape == (2, 1, 64, 128) and bool(torch.isfinite(disp).all())


def test_single_image_script_runs_an_attention_checkpoint(tmp_path):
    """test_simple.py has no --model option: evaluate_depth.load_networks takes the encoder class from the checkpoint, so the saved
    disparity is the attention encoder's -- bitwise what the API gives with the same weights -- and not a plain encoder's with the
    attention layers dropped."""
    import argparse
    from PIL import Image
    import evaluate_depth as ED
    import networks
    import test_simple as TS
    from depthcore import evaluate as E
    tr = _trainer()
    weights = tr.save_model(str(tmp_path / "weights"))
    yy, xx = np.mgrid[0:100, 0:330]
    img = np.stack([255.0 * xx / 330, 255.0 * yy / 100, 127 + 120 * np.sin(xx / 9.0 + yy / 5.0)], -1)
    photo = str(tmp_path / "a.jpg")
    Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(photo, quality=95)
    rec = TS.predict_folder(TS.parse_args(["--image_path", photo, "--load_weights_folder", weights]))
    assert len(rec) == 1 and os.path.isfile(rec[0]["jpeg"])
    enc, dec, h, w = ED.load_networks(argparse.Namespace(load_weights_folder=weights, num_layers=18, model=MODEL), DEV)
    assert type(enc) is networks.ResnetEncoderAttention and (h, w) == (64, 128)
    pred = E.predict_disparities(enc, dec, ED.image_batches([photo], h, w, 1, torch.device(DEV)), 0.1, 100.0)
    assert np.array_equal(np.load(rec[0]["npy"]), pred.cpu().numpy())
