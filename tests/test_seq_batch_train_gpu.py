"""Training the ConvGRU front-end on several sequence items per step (`seq_batch`): one whole training step against the same
step with the recurrence run item by item, the loader's stacked steps against its single items, and train_sequences() end to
end on a small KITTI-shaped tree.

The networks run at 64 x 128, the size of tests/test_seq_train_gpu.py: at 32 x 96 the encoder's last level is one row high, and
the depth decoder's ReflectionPad2d has no second row to mirror there (in the reference as here), so no trainer exists at that
size.  The loader test keeps 32 x 96: the data step has no such limit."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import rel_l2
from kitti_tree import DRIVES, write_raw_tree
from lidar_tree import write_scans

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DRIVE_A, DRIVE_B = sorted(DRIVES)                      # native 47 x 155 and 45 x 150
H, W = 64, 128                                        # the networks' size (see above)


def _trainer(seq_batch, seed=4, **kw):
    import trainer as T
    opt = T.default_options(height=H, width=W, batch_size=1, gru="v5", len_sequence=3, num_layers=18, seq_batch=seq_batch, **kw)
    tr = T.Trainer(opt, device=DEV, seed=seed)
    tr.set_train()
    for k in range(5):                                   # h0 starts at zero: move it so that its path is exercised
        with torch.no_grad():
            getattr(tr.models["gru"], "cgru_%d" % k).h0_layer1.normal_(0, 0.1, generator=torch.Generator(device=DEV).manual_seed(k))
    return tr


@pytest.fixture(scope="module")
def step_pair():
    """One train_step at seq_batch = 2, n = 3 on a stacked synthetic batch, in two trainers with the same seed (the same
    BatchNorm batch, the same tie-break noise): the second one's run_sequence gathers each item's rows, runs the
    single-sequence path and scatters the results back.  -> (first trainer, second trainer, their outputs, their losses,
    the stream counts the second one's run_sequence was called with)."""
    from depthcore import ops
    from depthcore.synthetic import synthetic_sequence_batch
    S, n = 2, 3
    a, b = _trainer(S), _trainer(S)
    gru = b.models["gru"]
    original, calls = gru.run_sequence, []

    def item_by_item(features, streams=1):
        calls.append(streams)
        outs = []
        for s in range(streams):
            rows = ops.seq_item_rows(s, streams, n)
            outs.append(original([f[rows].contiguous() for f in features], streams=1))
        # (n, S, ...) -> (n * S, ...): frame j of item s back at row j * S + s
        return [torch.stack([o[k] for o in outs], 1).flatten(0, 1) for k in range(5)]
    gru.run_sequence = item_by_item
    batch = synthetic_sequence_batch(n, H, W, DEV, items=S)
    assert batch[("color", 0, 0)].shape == (n * S, 3, H, W) and batch[("K", 0)].shape == (n * S, 4, 4)
    assert batch[("color_packed", 0, 0)].shape == (n * S, H, W, 4)
    out_a, la = a.train_step(dict(batch))
    out_b, lb = b.train_step(dict(batch))
    torch.cuda.synchronize()
    yield a, b, out_a, out_b, la, lb, calls
    a.close()
    b.close()


def test_one_step_of_two_items_forward_equals_the_recurrence_run_item_by_item(step_pair):
    """The forward of the step: the loss, the disparities of every scale, the poses and the loss's per-pixel selections are
    those of the item-by-item composition BIT FOR BIT -- the lockstep launches order an image's sums as its single-sequence
    call does (dc_set_wino_plan_streams; without it the 64-channel levels' reductions were split differently at batch 2, the
    disparities differed in the last bits and 3 of 49152 selections of the loss came out differently); the shared initial
    states receive a gradient; and the trainer built for two items per step still validates one item."""
    from depthcore.synthetic import synthetic_sequence_batch
    a, b, out_a, out_b, la, lb, calls = step_pair
    S, n = 2, 3
    assert calls == [S] and out_a[("disp", 0)].shape == (n * S, 1, H, W)
    assert la.keys() == lb.keys() and torch.isfinite(la["loss"])
    for key in sorted((k for k in out_a if torch.is_tensor(out_a[k]) and k in out_b), key=str):
        d = out_a[key].detach() != out_b[key].detach()
        r = rel_l2(out_a[key].float(), out_b[key].float())
        print("  output %s: %d of %d elements differ, rel_l2 %.3e" % (key, int(d.sum()), d.numel(), r))
        assert r < 1e-5, (key, r)
        assert int(d.sum()) == 0, key
    for k in la:
        assert rel_l2(la[k].detach(), lb[k].detach()) < 1e-5, k
    for k in range(5):                                                          # the shared initial states got the sum over the items
        assert float(getattr(a.models["gru"], "cgru_%d" % k).h0_layer1.grad.abs().sum()) > 0
    _, val = a.val_sequence(synthetic_sequence_batch(n, H, W, DEV, seed=5))
    assert torch.isfinite(val["loss"])


def test_one_step_of_two_items_equals_the_recurrence_run_item_by_item(step_pair):
    """The loss and every parameter's gradient of the two trainers agree to rel_l2 < 1e-5.  With the forward and the data
    gradients of the recurrence ordered per stream as in the single-sequence call, everything outside the ConvGRU parameters is
    equal bit for bit; those sum n * S rows in one pass against S passes of n rows (measured: at most 1.4e-7)."""
    a, b, _, _, la, lb, _ = step_pair
    loss_rel = abs(float(la["loss"].detach()) - float(lb["loss"].detach())) / abs(float(lb["loss"].detach()))
    names = [("%s.%s" % (k, name)) for k, m in a.models.items() for name, _ in m.named_parameters()]
    assert len(names) == len(a.parameters_to_train)
    rels, grads = [], 0
    for name, pa, pb in zip(names, a.parameters_to_train, b.parameters_to_train):
        assert (pa.grad is None) == (pb.grad is None)
        if pa.grad is not None:
            rels.append((rel_l2(pa.grad, pb.grad), name, float(pb.grad.norm())))
            grads += int(pa.grad.abs().sum() > 0)
    rels.sort(reverse=True)
    print("loss rel %.3e; %d gradients; the largest rel_l2 (name, norm of the gradient):" % (loss_rel, grads))
    for r, name, norm in rels[:12]:
        print("  %.3e  %s  %.3e" % (r, name, norm))
    assert grads > 50
    assert loss_rel < 1e-5
    assert rels[0][0] < 1e-5, rels[0]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kitti_seq_batch"))
    pixels = write_raw_tree(root, frames=9)
    scans = write_scans(root, frames=9, points=400)
    splits = os.path.join(root, "splits", "mine")
    os.makedirs(splits)
    for mode, drives in (("train", [DRIVE_A, DRIVE_B]), ("val", [DRIVE_B])):
        with open(os.path.join(splits, "%s_sequences.txt" % mode), "w") as f:
            f.write("\n".join(drives) + "\n")
    return root, pixels, scans


def test_loader_steps_are_its_single_items_stacked_time_major(tree):
    """items_per_step = 2 over drives of two native sizes: every step's rows of item s are, bit for bit, the dict the
    single-item loader delivers for that item with the same draws -- colours, RGBx, intrinsics and "depth_gt"."""
    import datasets
    from depthcore.data import seq_item_rows
    from depthcore.loader import SequenceLoader
    root, _, _ = tree
    n, S = 2, 2
    items = [(DRIVE_A, range(1, n + 3)), (DRIVE_B, range(0, n + 2)), (DRIVE_A, range(4, n + 6)), (DRIVE_B, range(3, n + 5)),
             (DRIVE_A, range(2, n + 4))]
    ds = datasets.KITTISequenceDataset(root, 32, 96, n, items, True, img_ext=".png")
    one = SequenceLoader(ds, num_workers=4, device=DEV, seed=3)
    two = SequenceLoader(ds, num_workers=4, device=DEV, seed=3, items_per_step=S)
    mixed = 0
    for epoch in (0, 1):
        one.set_epoch(epoch)
        two.set_epoch(epoch)
        singles, steps, plan = list(one), list(two), two.plan()
        torch.cuda.synchronize()
        assert len(steps) == len(two) == 2 and len(singles) == 5
        for k, step in enumerate(steps):
            mixed += int(len({ds.sequences[i][0] for i in plan[k][0]}) == 2)
            assert step["depth_gt"].shape == (n * S, 1, 375, 1242) and step[("K", 0)].shape == (n * S, 4, 4)
            for s in range(S):
                single = singles[k * S + s]
                assert step.keys() == single.keys()
                for key, v in single.items():
                    assert torch.equal(step[key][seq_item_rows(s, S, n)], v), (epoch, k, s, key)
    assert mixed > 0                                                            # a step held both native sizes
    one.close()
    two.close()


def _rows(log_dir, mode):
    with open(os.path.join(str(log_dir), "seq2", mode, "scalars.jsonl")) as f:
        return [json.loads(line) for line in f]


def test_train_sequences_with_two_items_per_step(tree, tmp_path):
    import trainer as T
    root, _, _ = tree
    opt = T.default_options(data_path=root, splits_dir=os.path.join(root, "splits"), split="mine", png=True, num_layers=18, height=H,
                            width=W, batch_size=1, gru="v5", len_sequence=3, seq_batch=2, train_n_tuples=1, test_n_tuples=1,
                            h_s_epoch=2, num_epochs=2, log_frequency=2, num_workers=4, log_dir=str(tmp_path), model_name="seq2")
    tr = T.Trainer(opt, device=DEV, seed=4)
    val_rows, trained_rows = [], []
    val, step = tr.val_sequence, tr.train_step

    def recording_val(inputs):
        val_rows.append(inputs[("color", 0, 0)].shape[0])
        return val(inputs)

    def recording_step(inputs):
        trained_rows.append((inputs[("color", 0, 0)].shape[0], inputs["depth_gt"].shape[0]))
        return step(inputs)
    tr.val_sequence, tr.train_step = recording_val, recording_step
    tr.train_sequences()
    torch.cuda.synchronize()
    # 9 frames per drive, n = 3: 3 items per drive, two drives for training: 6 items = 3 steps of 2 per epoch; validation one by one
    assert len(tr.train_loader) == 3 and tr.train_loader.items_per_step == 2
    assert len(tr.val_loader) == 3 and tr.val_loader.items_per_step == 1
    assert tr.step == 6 and tr.num_total_steps == 6 and trained_rows == [(6, 6)] * 6
    log_steps = [s for s in range(6) if T.Trainer.is_sequence_log_step(s % 3, s, 2)]
    assert log_steps == [0, 2, 3, 5] and val_rows == [3] * len(log_steps)          # one validation item per log step
    names = {"step", "loss", "loss/0", "loss/1", "loss/2", "loss/3", "de/abs_rel", "de/sq_rel", "de/rms", "de/log_rms", "da/a1", "da/a2", "da/a3"}
    for mode in ("train", "val"):
        rows = _rows(tmp_path, mode)
        assert [r["step"] for r in rows] == log_steps
        for r in rows:
            assert set(r) == names and all(np.isfinite(v) for v in r.values()), r
    models = os.path.join(str(tmp_path), "seq2", "models")
    assert sorted(os.listdir(models)) == ["opt.json", "weights_0", "weights_1"]
    for w in ("weights_0", "weights_1"):
        assert {"encoder.pth", "depth.pth", "gru.pth", "pose_encoder.pth", "pose.pth", "adam.pth"} <= set(os.listdir(os.path.join(models, w)))
    with open(os.path.join(models, "opt.json")) as f:
        saved = json.load(f)
    assert saved["seq_batch"] == 2 and saved["batch_size"] == 1 and saved["gru"] == "v5" and saved["len_sequence"] == 3
    tr.close()
