"""Trainer.train() end to end on a tmp KITTI-shaped tree: loader -> ragged data step -> train_step, validation at the log
steps, scalars.jsonl, checkpoints, the learning-rate schedule -- and the logged losses are those of a hand-written
train_step loop over the same loader."""
import json
import os

import numpy as np
import pytest
import torch

from kitti_tree import DRIVES, write_raw_tree, write_splits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kitti"))
    write_raw_tree(root, frames=6)                                    # 2 drives x 6 frames, native (47, 155) and (45, 150)
    a, b = sorted(DRIVES)
    train = ["%s 0 l" % a] + ["%s %d l" % (a, i) for i in (2, 3, 4)] + ["%s %d l" % (b, i) for i in (1, 2, 3, 4)]   # frame 0: no frame -1
    val = ["%s 1 l" % a, "%s 3 l" % a, "%s 2 l" % b, "%s 4 l" % b]
    splits = os.path.join(root, "splits")
    write_splits(splits, "eigen_zhou", train, val)
    return root, splits


def _options(tree, log_dir, **kw):
    import trainer as T
    root, splits = tree
    return T.default_options(data_path=root, splits_dir=splits, split="eigen_zhou", dataset="kitti", png=True, num_layers=18,
                             height=64, width=128, batch_size=2, num_epochs=2, scheduler_step_size=1, log_frequency=2,
                             num_workers=4, log_dir=str(log_dir), model_name="loop", **kw)


def _rows(log_dir, mode):
    path = os.path.join(str(log_dir), "loop", mode, "scalars.jsonl")
    if not os.path.isfile(path):
        return None
    with open(path) as f:
        return [json.loads(line) for line in f]


@pytest.mark.parametrize("variant", ["eager", "hip_graph", "fusion_v3"])
def test_train_runs_logs_checkpoints_and_matches_a_hand_written_loop(tree, tmp_path, variant):
    import trainer as T
    kw = {"hip_graph": dict(hip_graph=True), "fusion_v3": dict(fusion="v3", frame_ids=[0, -2, -1, 1])}.get(variant, {})
    tr = T.Trainer(_options(tree, tmp_path / "a", **kw), device=DEV, seed=4)
    lrs = []
    run_epoch = tr.run_epoch

    def recording_run_epoch():
        run_epoch()
        lrs.append(tr.model_optimizer.param_groups[0]["lr"])
    tr.run_epoch = recording_run_epoch
    tr.train()
    torch.cuda.synchronize()
    assert tr.step == 8 and tr.num_total_steps == 8
    assert np.allclose(lrs, [1e-5, 1e-6], rtol=1e-9, atol=0)          # ends epoch 0 at 1e-5 and epoch 1 at 1e-6
    models = os.path.join(str(tmp_path / "a"), "loop", "models")
    assert sorted(os.listdir(models)) == ["opt.json", "weights_0", "weights_1"]
    for w in ("weights_0", "weights_1"):
        assert {"encoder.pth", "depth.pth", "pose_encoder.pth", "pose.pth", "adam.pth"} <= set(os.listdir(os.path.join(models, w)))
    with open(os.path.join(models, "opt.json")) as f:
        assert json.load(f)["batch_size"] == 2
    log_steps = [s for s in range(8) if T.Trainer.is_log_step(s % 4, s, 2)]
    assert log_steps == [0, 2, 4, 6]
    train_rows, val_rows = _rows(tmp_path / "a", "train"), _rows(tmp_path / "a", "val")
    assert [r["step"] for r in train_rows] == log_steps
    for r in train_rows:
        assert set(r) == {"step", "loss", "loss/0", "loss/1", "loss/2", "loss/3"} and all(np.isfinite(v) for v in r.values())
    if variant == "fusion_v3":
        assert val_rows is None                                       # Trainer.val refuses that front-end: no validation
    else:
        assert [r["step"] for r in val_rows] == log_steps
        assert all(np.isfinite(v) for r in val_rows for v in r.values())
    captured = tr._graph is not None
    assert captured == (variant == "hip_graph")
    tr.close()

    # the same steps by hand in a second trainer with the same seed: same loader, same order, same draws
    tr2 = T.Trainer(_options(tree, tmp_path / "b", **kw), device=DEV, seed=4)
    loader, _ = tr2.build_loaders()
    tr2.set_train()
    want = {}
    for epoch in range(2):
        loader.set_epoch(epoch)
        for inputs in loader:
            _, losses = tr2.train_step(inputs)
            want[tr2.step - 1] = {k: float(v.detach()) for k, v in losses.items()}
        tr2.model_lr_scheduler.step()
    tr2.close()
    assert len(want) == 8
    for r in train_rows:
        for k, v in want[r["step"]].items():
            assert r[k] == v, (r["step"], k, r[k], v)                 # bitwise, as two runs of the same step are
