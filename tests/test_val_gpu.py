"""Trainer.val / compute_depth_losses (trainer.py:444-463, 624-652): the metrics equal an eval-mode process_batch plus the
restated trainer protocol; val leaves training exactly where it was (eager and captured steps); no ATen compute op."""
import collections

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode
from torch.utils._pytree import tree_flatten

import depth_metrics_ref as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B, H, W = 2, 64, 96


def _trainer(**kw):
    import trainer as T
    o = T.default_options(batch_size=kw.pop("batch_size", B), height=kw.pop("height", H), width=kw.pop("width", W), **kw)
    tr = T.Trainer(o, device=DEV)
    tr.set_train()
    return tr


def _batch(seed=0, gt=True, b=B, h=H, w=W, **kw):
    from depthcore.synthetic import synthetic_batch, synthetic_depth_gt
    inputs = synthetic_batch(b, h, w, DEV, seed=seed, **kw)
    if gt:
        inputs["depth_gt"] = synthetic_depth_gt(b, DEV, seed=seed)
    return inputs


def _snapshot(tr):
    s = {"params": [p.detach().clone() for p in tr.parameters_to_train],
         "buffers": {(k, n): b.clone() for k, m in tr.models.items() for n, b in m.named_buffers()},
         "step": tr.step}
    opt = tr.model_optimizer.state_dict()
    s["adam"] = [(k, {n: (v.clone() if torch.is_tensor(v) else v) for n, v in st.items()}) for k, st in opt["state"].items()]
    s["seed"] = tr._seed_dev.clone() if tr._seed_dev is not None else None
    return s


def _same(a, b):
    assert a["step"] == b["step"]
    assert all(torch.equal(x, y) for x, y in zip(a["params"], b["params"]))
    assert a["buffers"].keys() == b["buffers"].keys()
    for k in a["buffers"]:
        assert torch.equal(a["buffers"][k], b["buffers"][k]), k
    assert len(a["adam"]) == len(b["adam"])
    for (ka, sa), (kb, sb) in zip(a["adam"], b["adam"]):
        assert ka == kb and sa.keys() == sb.keys()
        for n in sa:
            assert (torch.equal(sa[n], sb[n]) if torch.is_tensor(sa[n]) else sa[n] == sb[n]), (ka, n)
    assert (a["seed"] is None) == (b["seed"] is None) and (a["seed"] is None or torch.equal(a["seed"], b["seed"]))


@pytest.mark.parametrize("materialize", [False, True])
def test_val_equals_eval_process_batch_plus_trainer_protocol(materialize):
    from depthcore import ops
    tr = _trainer(materialize_logs=materialize)
    inputs = _batch(1)
    tr.train_step({k: v for k, v in inputs.items() if k != "depth_gt"})
    outputs, losses = tr.val(dict(inputs))
    assert all(m.training for m in tr.models.values())
    assert tr.depth_metric_names == ["de/abs_rel", "de/sq_rel", "de/rms", "de/log_rms", "da/a1", "da/a2", "da/a3"]
    tr.set_eval()
    with torch.no_grad():
        out2, loss2 = tr.process_batch({k: v for k, v in inputs.items() if k != "depth_gt"})
    tr.set_train()
    assert torch.equal(losses["loss"], loss2["loss"])
    if materialize:         # the fused loss's own depth (trainer.py:495), which compute_depth_losses reads when present
        depth = out2[("depth", 0, 0)]
        assert torch.equal(outputs[("depth", 0, 0)], depth)
    else:                   # what generate_images_pred would have stored
        _, depth = ops.disp_to_depth(out2[("disp", 0)], tr.opt.min_depth, tr.opt.max_depth)
    up = ops.upsample_bilinear(depth, 375, 1242).cpu()
    _, _, _, want, counts, n = M.trainer_protocol(up, inputs["depth_gt"].cpu())
    got = np.array([float(losses[k]) for k in tr.depth_metric_names])
    for k in tr.depth_metric_names:
        assert isinstance(losses[k], np.ndarray) and losses[k].shape == ()
    np.testing.assert_allclose(got[:4], want[:4], rtol=1e-5)
    assert [np.float32(got[4 + i]) for i in range(3)] == [np.float32(c / n) for c in counts]


def test_val_without_depth_gt_and_state_untouched():
    tr = _trainer()
    inputs = _batch(2, gt=False)
    tr.train_step(inputs)
    before = _snapshot(tr)
    outputs, losses = tr.val(dict(inputs))
    assert "de/abs_rel" not in losses and torch.isfinite(losses["loss"])
    _same(before, _snapshot(tr))


@pytest.mark.parametrize("graph", [False, True])
def test_train_val_train_is_bitwise_train_train(graph):
    kw = dict(hip_graph=True) if graph else {}
    steps = 5 if graph else 2           # graph mode: 3 eager warm-up steps, the capture, a replay -- then val, then replays
    a, b = _trainer(**kw), _trainer(**kw)
    inputs = _batch(3, gt=False)
    val_in = _batch(4)
    la, lb = [], []
    for i in range(steps):
        la.append(a.train_step(inputs)[1]["loss"].clone())
        lb.append(b.train_step(inputs)[1]["loss"].clone())
    graphs = dict(a._graphs)
    before = _snapshot(a)
    a.val(dict(val_in))
    _same(before, _snapshot(a))
    assert a._graphs == graphs
    for i in range(2):
        la.append(a.train_step(inputs)[1]["loss"].clone())
        lb.append(b.train_step(inputs)[1]["loss"].clone())
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(la, lb))
    _same(_snapshot(a), _snapshot(b))
    if graph:
        assert a._graph is not None and len(a._graphs) == 1


def test_val_cpu_noise_draws_like_reference():
    tr = _trainer(cpu_tiebreak_noise=True)
    inputs = _batch(5)
    torch.manual_seed(123)
    tr.val(dict(inputs))
    after_val = torch.randn(4)
    torch.manual_seed(123)
    tr.set_eval()
    with torch.no_grad():
        tr.process_batch({k: v for k, v in inputs.items() if k != "depth_gt"})
    tr.set_train()
    assert torch.equal(after_val, torch.randn(4))


@pytest.mark.parametrize("pose", ["separate_resnet", "shared", "posecnn"])
def test_val_every_pose_model_type(pose):
    tr = _trainer(pose_model_type=pose)
    inputs = _batch(6)
    _, losses = tr.val(dict(inputs))
    assert torch.isfinite(losses["loss"])
    assert all(np.isfinite(losses[k]) for k in tr.depth_metric_names)


def test_val_fusion_raises():
    tr = _trainer(fusion="v3", frame_ids=[0, -2, -1, 1])
    with pytest.raises(NotImplementedError, match="Fusion_v3"):
        tr.val(_batch(7, frame_ids=(0, -2, -1, 1)))


def test_val_gru_raises():
    from depthcore.synthetic import synthetic_sequence_batch
    tr = _trainer(batch_size=1, gru="v5", len_sequence=3)
    with pytest.raises(NotImplementedError, match="ConvGRU"):
        tr.val(synthetic_sequence_batch(3, H, W, DEV))


# memory ops the census tolerates, each with its reason; everything else that reaches ATen with a device tensor is a failure
ALLOWED = {
    "_to_copy": "the one device-to-host copy of the metrics (ops._depth_errors)",
    "copy_": "the device-to-host copy's destination write",
}
SKIP = {"view", "reshape", "slice", "select", "expand", "permute", "transpose", "t", "unsqueeze", "squeeze", "alias", "detach",
        "as_strided", "empty", "empty_like", "empty_strided", "new_empty", "unbind", "split", "split_with_sizes", "narrow",
        "_unsafe_view", "_local_scalar_dense", "lift_fresh", "record_stream", "resize_", "set_", "is_pinned", "is_same_size",
        "_reshape_alias", "view_as", "expand_as", "flatten", "unflatten", "movedim", "_has_compatible_shallow_copy_type"}


class _Census(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.count = collections.Counter()

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        name = str(func).split(".")[1]
        if name not in SKIP and any(isinstance(a, torch.Tensor) and a.is_cuda for a in tree_flatten((args, kwargs or {}, out))[0]):
            self.count[name] += 1
        return out


def test_val_aten_census():
    tr = _trainer(batch_size=2, height=192, width=640)
    inputs = _batch(8, b=2, h=192, w=640)
    tr.val(dict(inputs))
    torch.cuda.synchronize()
    with _Census() as cen:
        tr.val(dict(inputs))
        torch.cuda.synchronize()
    found = dict(cen.count)
    for banned in ("native_batch_norm", "_native_batch_norm_legit_no_training", "median", "sort", "index", "batch_norm"):
        assert banned not in found, found
    assert set(found) <= set(ALLOWED), found
