"""Sequence training on the GPU: SequenceLoader on a tmp KITTI-shaped tree against the chain reference evaluated with the
plan's draws ("depth_gt" included), one training step on the loader-shaped dict of views against the materialised per-position
dict, train_sequences() end to end, and val_sequence leaving training where it was."""
import json
import os

import numpy as np
import pytest
import torch

import seq_data_ref as R
from kitti_tree import DRIVES, write_raw_tree
from lidar_tree import write_scans

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DRIVE_A, DRIVE_B = sorted(DRIVES)                      # native 47 x 155 and 45 x 150
H, W = 64, 128                                         # the sizes of tests/test_train_gpu.py's loop tests


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kitti_seq"))
    pixels = write_raw_tree(root, frames=9)
    scans = write_scans(root, frames=9, points=400)
    splits = os.path.join(root, "splits", "mine")
    os.makedirs(splits)
    for mode, drives in (("train", [DRIVE_A, DRIVE_B]), ("val", [DRIVE_B])):
        with open(os.path.join(splits, "%s_sequences.txt" % mode), "w") as f:
            f.write("\n".join(drives) + "\n")
    return root, pixels, scans


def _dataset(root, n, is_train, h=32, w=96):
    import datasets
    items = [(DRIVE_A, range(1, n + 3)), (DRIVE_B, range(0, n + 2)), (DRIVE_A, range(4, n + 6)), (DRIVE_B, range(3, n + 5))]
    return datasets.KITTISequenceDataset(root, h, w, n, items, is_train, img_ext=".png")


def _epochs(ds, workers, epochs=(0, 1), seed=3):
    from depthcore.loader import SequenceLoader
    ld = SequenceLoader(ds, num_workers=workers, device=DEV, seed=seed)
    out = []
    for e in epochs:
        ld.set_epoch(e)
        out.append((ld.plan(), list(ld)))
    torch.cuda.synchronize()
    ld.close()
    return out


def test_loader_items_equal_the_chain_with_the_plan_s_draws(tree):
    from depthcore import lidar
    root, pixels, scans = tree
    n = 2
    ds = _dataset(root, n, True)
    runs = {workers: _epochs(ds, workers) for workers in (1, 4)}
    seen = set()
    for plan, batches in runs[4]:
        assert len(plan) == len(batches) == 4
        for (index, (flip, jitters)), batch in zip(plan, batches):
            seen.add((flip, jitters is not None))
            drive, frames = ds.sequences[index]
            native = np.stack([pixels[(drive, i, "l")] for i in frames])
            want = R.sequence_item(native, 32, 96, 4, flip, jitters)
            assert set(batch) == set(want) | {("color_aug", f, s) for f in (0, -1, 1) for s in range(4)} | \
                {(k, s) for k in ("K", "inv_K") for s in range(4)} | {"depth_gt"}
            for key, v in want.items():
                assert np.array_equal(batch[key].cpu().numpy(), v), (index, key)
                if key[0] == "color":
                    assert batch[("color_aug",) + key[1:]] is batch[key]
            P, size = lidar.velo_to_image(ds.calib_dir(index), 2)
            gt = R.depth_gt([scans[(drive, i)] for i in list(frames)[1:-1]], P, size, flip)
            assert gt.shape == (n, 1, 375, 1242) and np.array_equal(batch["depth_gt"].cpu().numpy(), gt), index
            if flip:                                                    # mirrored once: the unmirrored map, reversed
                plain = R.depth_gt([scans[(drive, i)] for i in list(frames)[1:-1]], P, size, False)
                assert np.array_equal(gt, plain[..., ::-1]) and gt.any()
            for s in range(4):
                K = ds.K.copy()
                K[0] *= 96 >> s
                K[1] *= 32 >> s
                assert batch[("K", s)].shape == (n, 4, 4) and np.array_equal(batch[("K", s)][1].cpu().numpy(), K)
                assert np.array_equal(batch[("inv_K", s)][0].cpu().numpy(), np.linalg.pinv(K))
    assert len(seen) >= 3                                               # flipped, jittered and plain items all occurred
    # the same items whatever the number of decode threads
    for (pa, ba), (pb, bb) in zip(runs[1], runs[4]):
        assert pa == pb
        for x, y in zip(ba, bb):
            assert x.keys() == y.keys() and all(torch.equal(x[k], y[k]) for k in x)


def test_validation_loader_draws_nothing_and_a_tree_without_scans_has_no_depth_gt(tree, tmp_path):
    from depthcore.loader import SequenceLoader
    root, pixels, _ = tree
    ds = _dataset(root, 2, False)
    ld = SequenceLoader(ds, num_workers=2, device=DEV, shuffle=False)
    first = next(iter(ld))
    torch.cuda.synchronize()
    ld.close()
    drive, frames = ds.sequences[0]
    want = R.sequence_item(np.stack([pixels[(drive, i, "l")] for i in frames]), 32, 96, 4, False, None)
    assert all(np.array_equal(first[k].cpu().numpy(), v) for k, v in want.items()) and "depth_gt" in first
    bare = str(tmp_path)
    write_raw_tree(bare, frames=5)
    import datasets
    ds2 = datasets.KITTISequenceDataset(bare, 32, 96, 2, [(DRIVE_A, range(0, 4))], False, img_ext=".png")
    ld = SequenceLoader(ds2, num_workers=2, device=DEV)
    (only,) = list(ld)
    torch.cuda.synchronize()
    ld.close()
    assert "depth_gt" not in only and only[("color", 0, 0)].shape == (2, 3, 32, 96)


def _trainer(seed=4, **kw):
    import trainer as T
    opt = T.default_options(height=H, width=W, batch_size=1, gru="v5", len_sequence=3, **kw)
    tr = T.Trainer(opt, device=DEV, seed=seed)
    tr.set_train()
    return tr


def _item(n=3, seed=0, gt=False):
    """A loader-shaped item: GpuPreprocessor.sequence on n + 2 frames of the target size (views of one pyramid), K / inv_K."""
    from depthcore.data import GpuPreprocessor
    from depthcore.synthetic import KITTI_K, synthetic_depth_gt
    from kitti_tree import frame_pixels
    pre = GpuPreprocessor(H, W, device=DEV)
    native = torch.from_numpy(np.stack([frame_pixels(H, W, 50 + seed + i) for i in range(n + 2)])).to(DEV)
    item = pre.sequence(native)
    item.update(pre.intrinsics(KITTI_K, n))
    if gt:
        item["depth_gt"] = synthetic_depth_gt(n, DEV, seed=seed)
    return item


def test_one_training_step_on_views_equals_the_materialised_sequence():
    """The loader's dict holds overlapping views of one (n + 2)-frame pyramid and skips _stack_sequence; the per-position dict
    of the same pixels is materialised and stacked by ops.stack_frames.  Losses, every gradient and every updated parameter
    are bitwise equal: no kernel of the step depends on an input's storage offset."""
    n = 3
    item = _item(n)
    assert item[("color", 0, 0)].data_ptr() != item[("color", 0, 0)].untyped_storage().data_ptr()      # a view at an offset
    per_j = {}
    for key, v in item.items():
        if key[0] in ("color", "K", "inv_K"):
            for j in range(n):
                per_j[key + (j,)] = v[j:j + 1].clone()
    a, b = _trainer(), _trainer()
    for k in range(5):                                   # h0 starts at zero: move it so that its path is exercised
        for tr in (a, b):
            with torch.no_grad():
                getattr(tr.models["gru"], "cgru_%d" % k).h0_layer1.normal_(0, 0.1, generator=torch.Generator(device=DEV).manual_seed(k))
    _, la = a.train_step(item)
    _, lb = b.train_step(per_j)
    torch.cuda.synchronize()
    assert la.keys() == lb.keys() and torch.isfinite(la["loss"])
    for k in la:
        assert torch.equal(la[k], lb[k]), k
    grads = 0
    for pa, pb in zip(a.parameters_to_train, b.parameters_to_train):
        assert (pa.grad is None) == (pb.grad is None)
        if pa.grad is not None:
            assert torch.equal(pa.grad, pb.grad)
            grads += int(pa.grad.abs().sum() > 0)
        assert torch.equal(pa, pb)
    assert grads > 50
    a.close()
    b.close()


def _rows(log_dir, mode):
    with open(os.path.join(str(log_dir), "seq", mode, "scalars.jsonl")) as f:
        return [json.loads(line) for line in f]


def test_train_sequences_end_to_end(tree, tmp_path):
    import trainer as T
    root, _, _ = tree
    opt = T.default_options(data_path=root, splits_dir=os.path.join(root, "splits"), split="mine", png=True, num_layers=18, height=H,
                            width=W, batch_size=1, gru="v5", len_sequence=3, train_n_tuples=1, test_n_tuples=1, h_s_epoch=2,
                            num_epochs=2, log_frequency=2, num_workers=4, log_dir=str(tmp_path), model_name="seq")
    tr = T.Trainer(opt, device=DEV, seed=4)
    lr0 = tr.model_optimizer.param_groups[0]["lr"]
    h0 = [c.h0_layer1 for c in tr.models["gru"].cells()]
    seen, run = [], tr.run_sequence_epoch

    def recording():
        seen.append((tr.epoch, [p.requires_grad for p in h0]))
        run()
    tr.run_sequence_epoch = recording
    tr.train_sequences()
    torch.cuda.synchronize()
    # 9 frames per drive, n = 3: max(9 // 3, 1) = 3 items per drive, two drives for training and one for validation
    assert len(tr.train_loader) == 6 and len(tr.val_loader) == 3 and tr.step == 12 and tr.num_total_steps == 12
    assert seen == [(0, [True] * 5), (1, [False] * 5)]                  # frozen from epoch h_s_epoch - 1 on
    assert tr.model_optimizer.param_groups[0]["lr"] == lr0 == opt.learning_rate      # the scheduler is never stepped
    log_steps = [s for s in range(12) if T.Trainer.is_sequence_log_step(s % 6, s, 2)]
    assert log_steps == [0, 2, 4, 6, 8, 10]
    names = {"step", "loss", "loss/0", "loss/1", "loss/2", "loss/3", "de/abs_rel", "de/sq_rel", "de/rms", "de/log_rms", "da/a1", "da/a2", "da/a3"}
    for mode in ("train", "val"):
        rows = _rows(tmp_path, mode)
        assert [r["step"] for r in rows] == log_steps
        for r in rows:                                                  # the tree has scans: every item carries "depth_gt"
            assert set(r) == names and all(np.isfinite(v) for v in r.values()), r
    models = os.path.join(str(tmp_path), "seq", "models")
    assert sorted(os.listdir(models)) == ["opt.json", "weights_0", "weights_1"]
    for w in ("weights_0", "weights_1"):
        assert {"encoder.pth", "depth.pth", "gru.pth", "pose_encoder.pth", "pose.pth", "adam.pth"} <= set(os.listdir(os.path.join(models, w)))
    with open(os.path.join(models, "opt.json")) as f:
        saved = json.load(f)
    assert saved["gru"] == "v5" and saved["len_sequence"] == 3 and saved["batch_size"] == 1
    with pytest.raises(NotImplementedError):
        tr.train()
    tr.close()


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


def test_val_sequence_leaves_training_where_it_was():
    import depth_metrics_ref as M
    from depthcore import ops
    from depthcore.synthetic import synthetic_sequence_batch
    tr = _trainer()
    tr.train_step(_item(seed=1))
    tr.train_step(_item(seed=2))                                        # Adam has state, BatchNorm has moved
    torch.cuda.synchronize()
    before = _snapshot(tr)
    inputs = _item(seed=3, gt=True)
    outputs, losses = tr.val_sequence(inputs)
    torch.cuda.synchronize()
    _same(before, _snapshot(tr))
    assert all(m.training for m in tr.models.values())
    assert not losses["loss"].requires_grad and outputs[("disp", 0)].shape == (3, 1, H, W)
    # the metrics: the "trainer" protocol over the n stacked frames
    _, depth = ops.disp_to_depth(outputs[("disp", 0)], tr.opt.min_depth, tr.opt.max_depth)
    _, _, _, want, counts, npix = M.trainer_protocol(ops.upsample_bilinear(depth, 375, 1242).cpu(), inputs["depth_gt"].cpu())
    got = np.array([float(losses[k]) for k in tr.depth_metric_names])
    np.testing.assert_allclose(got[:4], want[:4], rtol=1e-5)
    assert [np.float32(got[4 + i]) for i in range(3)] == [np.float32(c / npix) for c in counts]
    # the same call twice: the same numbers (eval mode reads the running statistics, nothing moved)
    _, again = tr.val_sequence(_item(seed=3, gt=True))
    assert torch.equal(again["loss"], losses["loss"]) and all(again[m] == losses[m] for m in tr.depth_metric_names)
    # an item without ground truth has no metrics; the per-position dict is taken too
    _, plain = tr.val_sequence(synthetic_sequence_batch(3, H, W, DEV, seed=5))
    assert "de/abs_rel" not in plain and torch.isfinite(plain["loss"])
    _same(before, _snapshot(tr))
    with pytest.raises(NotImplementedError, match="ConvGRU"):
        tr.val(_item(seed=3))
    tr.close()
