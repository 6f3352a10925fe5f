"""Sequence training without a GPU: the tuples of generate_sequences, the files of a KITTISequenceDataset item, the plan of a
SequenceLoader, and train_sequences() / run_sequence_epoch() on a stub trainer -- the GRU trainer's log rule, the cycling
validation item, the scheduler that is never stepped, the freeze epoch, the checkpoints."""
import json
import os
import random
import time
import types

import numpy as np
import pytest
import torch

from kitti_tree import DRIVES, write_raw_tree

DRIVE_A, DRIVE_B = sorted(DRIVES)


def test_generate_sequences_counts_bounds_and_seed(tmp_path):
    from datasets import generate_sequences
    root = str(tmp_path)
    write_raw_tree(root, frames=14, drives={DRIVE_A: (4, 6)})
    write_raw_tree(root, frames=9, drives={DRIVE_B: (4, 6)})
    n = 2
    items = generate_sequences(root, [DRIVE_B, DRIVE_A], n, 3, random.Random(5))
    # per drive max(n_frames // n, n_tuples) items, the drives in the order of the list
    assert [d for d, _ in items] == [DRIVE_B] * 4 + [DRIVE_A] * 7
    for drive, frames in items:
        n_frames = 9 if drive == DRIVE_B else 14
        assert isinstance(frames, range) and len(frames) == n + 2 and frames.step == 1
        assert 0 <= frames.start < n_frames - 1 - n - 2
    assert len({(d, f.start) for d, f in items}) == len(items)                    # sampled without replacement
    # n_tuples wins where it is larger than n_frames // n
    assert len(generate_sequences(root, [DRIVE_A], 2, 8, random.Random(0))) == 8
    assert len(generate_sequences(root, [DRIVE_B], 4, 1, random.Random(0))) == 2
    # deterministic under a seed, and the draws are random.sample's
    again = generate_sequences(root, [DRIVE_B, DRIVE_A], n, 3, random.Random(5))
    assert [(d, f.start) for d, f in again] == [(d, f.start) for d, f in items]
    twin = random.Random(5)
    want = twin.sample(range(9 - 1 - n - 2), 4) + twin.sample(range(14 - 1 - n - 2), 7)
    assert [f.start for _, f in items] == want
    assert [f.start for _, f in generate_sequences(root, [DRIVE_B, DRIVE_A], n, 3, random.Random(6))] != want


def test_a_short_drive_is_a_value_error_that_names_it(tmp_path):
    from datasets import generate_sequences
    root = str(tmp_path)
    write_raw_tree(root, frames=9, drives={DRIVE_B: (4, 6)})
    with pytest.raises(ValueError, match=DRIVE_B.split("/")[1]):
        generate_sequences(root, [DRIVE_B], 2, 5 + 1, random.Random(0))           # 4 start frames to draw 6 from
    with pytest.raises(ValueError, match="9 frames"):
        generate_sequences(root, [DRIVE_B], 7, 1, random.Random(0))               # no start frame at all
    with pytest.raises(ValueError):
        generate_sequences(root, [DRIVE_B], 0, 1, random.Random(0))


def test_dataset_paths_scans_and_calibration(tmp_path):
    import datasets
    from lidar_tree import write_scans
    root = str(tmp_path)
    write_raw_tree(root, frames=8)
    items = [(DRIVE_A, range(2, 6)), (DRIVE_B, range(0, 4))]
    ds = datasets.KITTIDataset_v1(root, 32, 96, 2, items, True, img_ext=".png")
    assert datasets.KITTIDataset_v1 is datasets.KITTISequenceDataset
    assert len(ds) == 2 and ds.n == 2 and ds.is_train and ds.frame_idxs == [0, -1, 1] and ds.num_scales == 4
    assert ds.full_res_shape == (1242, 375) and ds.K.dtype == np.float32 and ds.K[0, 0] == np.float32(0.58) and ds.K[1, 1] == np.float32(1.92)
    base = os.path.join(root, DRIVE_A)
    assert ds.frame_paths(0) == [os.path.join(base, "image_02", "data", "%010d.png" % i) for i in (2, 3, 4, 5)]
    assert all(os.path.isfile(p) for p in ds.frame_paths(0) + ds.frame_paths(1))
    assert ds.scan_paths(0) == [os.path.join(base, "velodyne_points/data", "%010d.bin" % i) for i in (3, 4)]
    assert ds.calib_dir(1) == os.path.join(root, DRIVE_B.split("/")[0])
    assert ds.check_depth() is False and ds.load_depth is False                   # no scans in the tree yet
    assert datasets.KITTISequenceDataset(root, 32, 96, 2, items, False).frame_paths(1)[0].endswith("0000000000.jpg")
    scans = write_scans(root, frames=8)
    ds = datasets.KITTISequenceDataset(root, 32, 96, 2, items, False, img_ext=".png")
    assert ds.check_depth() is True and ds.load_depth is True and ds.device_depth is True
    # the host path of "depth_gt": camera 2, resized to 375 x 1242, mirrored with the flip
    import lidar_ref
    from depthcore import lidar
    P, size = lidar.velo_to_image(ds.calib_dir(0), 2)
    want = lidar_ref.resize_flip(lidar_ref.depth_map(scans[(DRIVE_A, 3)], P, size), (375, 1242), True)
    assert np.array_equal(ds.get_depth(3, DRIVE_A, True), want) and want.shape == (375, 1242)
    with pytest.raises(ValueError, match="4 frames"):
        datasets.KITTISequenceDataset(root, 32, 96, 2, [(DRIVE_A, range(0, 5))], False)


def test_loader_plan_is_a_function_of_seed_and_epoch(tmp_path):
    import datasets
    from depthcore.data import sample_sequence
    from depthcore.loader import SequenceLoader, epoch_rng
    items = [(DRIVE_A, range(i, i + 4)) for i in range(5)]
    ds = datasets.KITTISequenceDataset(str(tmp_path), 32, 96, 2, items, True, img_ext=".png")
    ld = SequenceLoader(ds, num_workers=64, device="cpu", seed=3, prefetch=7)
    assert len(ld) == 5 and ld.threads == 16 and ld.prefetch == 2 and ld.batch_size == 1 and ld.cache is None
    p0, p1 = ld.plan(0), ld.plan(1)
    assert sorted(i for i, _ in p0) == list(range(5)) and p0 != p1 and ld.plan(0) == p0
    ld.set_epoch(1)
    assert ld.plan() == p1
    assert SequenceLoader(ds, device="cpu", seed=4).plan(0) != p0
    rng = epoch_rng(3, 0)
    order = list(range(5))
    rng.shuffle(order)
    assert p0 == [(i, sample_sequence(True, rng, 2, 4)) for i in order]           # the permutation, then the draws in item order
    # the validation loader: in order, nothing drawn
    val = SequenceLoader(datasets.KITTISequenceDataset(str(tmp_path), 32, 96, 2, items, False), device="cpu", seed=1, shuffle=False)
    assert val.plan(0) == val.plan(9) == [(i, (False, None)) for i in range(5)]


def test_frames_of_an_item_share_one_size(tmp_path):
    import datasets
    from depthcore.loader import SequenceLoader
    root = str(tmp_path)
    write_raw_tree(root, frames=4, drives={DRIVE_A: (8, 12)})
    from PIL import Image
    Image.fromarray(np.zeros((8, 10, 3), np.uint8)).save(os.path.join(root, DRIVE_A, "image_02", "data", "%010d.png" % 2))
    ds = datasets.KITTISequenceDataset(root, 8, 16, 2, [(DRIVE_A, range(0, 4))], False, img_ext=".png")
    ld = SequenceLoader(ds, num_workers=2, device="cpu")
    with pytest.raises(ValueError, match="share one size"):
        ld.decode_item(0)
    ld.close()
    write_raw_tree(root, frames=4, drives={DRIVE_A: (8, 12)})
    frames, flip, jitters = ld.decode_item(0, (True, None))
    assert frames.shape == (4, 8, 12, 3) and frames.dtype == np.uint8 and flip is True and jitters is None
    from kitti_tree import frame_pixels
    assert np.array_equal(frames[3], frame_pixels(8, 12, 30))                     # decoded, not mirrored: the device mirrors
    ld.close()


# ------------------------------------------------------------------------------------------------------ the loop on a stub
class _StubLoader:
    def __init__(self, n):
        self.n, self.epoch, self.epochs_seen = n, 0, []

    def __len__(self):
        return self.n

    def set_epoch(self, epoch):
        self.epoch = epoch
        self.epochs_seen.append(epoch)

    def __iter__(self):
        return iter([{"x": torch.full((1,), float(10 * self.epoch + i))} for i in range(self.n)])


class _CountingScheduler:
    calls = 0

    def step(self):
        self.calls += 1


def _stub(tmp_path, **kw):
    import trainer as T
    tr = T.Trainer.__new__(T.Trainer)
    opt = dict(num_epochs=3, save_frequency=2, log_frequency=2, batch_size=1, scheduler_step_size=1, learning_rate=1e-4,
               log_dir=str(tmp_path), model_name="stub", fusion=None, gru="v5", h_s_epoch=2)
    opt.update(kw)
    tr.opt = types.SimpleNamespace(**opt)
    tr.device = torch.device("cpu")
    tr.step = tr.epoch = 0
    tr.models = {}
    tr.train_loader, tr.val_loader, tr._val_iter = _StubLoader(4), _StubLoader(3), None
    tr.model_optimizer = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], tr.opt.learning_rate)
    tr.model_lr_scheduler = _CountingScheduler()
    tr.calls = []

    def train_step(inputs):
        tr.calls.append(("step", tr.epoch, float(inputs["x"])))
        tr.step += 1
        return {}, {"loss": torch.tensor(0.5 + tr.step)}

    def val_sequence(inputs):
        tr.calls.append(("val", float(inputs["x"])))
        return {}, {"loss": torch.tensor(2.0)}

    def val(inputs):
        raise AssertionError("the sequence loop validates through val_sequence")
    tr.train_step, tr.val_sequence, tr.val = train_step, val_sequence, val
    tr.save_model = lambda: tr.calls.append(("save", tr.epoch))
    tr.freeze_hidden_states = lambda: tr.calls.append(("freeze", tr.epoch))
    return tr


def _rows(tmp_path, mode):
    with open(os.path.join(str(tmp_path), "stub", mode, "scalars.jsonl")) as f:
        return [json.loads(line) for line in f]


def test_sequence_log_rule_has_no_early_phase_limit():
    from trainer import Trainer
    f = Trainer.is_sequence_log_step
    assert [b for b in range(8) if f(b, 100 + b, 2)] == [0, 2, 4, 6]
    assert f(250, 2251, 250) and f(0, 123457, 250)                                # past step 2000, where Trainer.is_log_step is silent
    assert not Trainer.is_log_step(250, 2251, 250)
    assert f(17, 4000, 250) and f(17, 0, 250) and not f(17, 4001, 250)


def test_train_sequences_on_a_stub(tmp_path, capsys):
    tr = _stub(tmp_path)
    tr.train_sequences()
    steps = [c for c in tr.calls if c[0] == "step"]
    assert len(steps) == 12 and tr.step == 12 and tr.num_total_steps == 12 and tr.train_loader.epochs_seen == [0, 1, 2]
    # the scheduler is never stepped, the rate never moves
    assert tr.model_lr_scheduler.calls == 0 and tr.model_optimizer.param_groups[0]["lr"] == 1e-4
    # the freeze: at epoch h_s_epoch - 1 only, before that epoch's first step
    freezes = [i for i, c in enumerate(tr.calls) if c[0] == "freeze"]
    assert [tr.calls[i] for i in freezes] == [("freeze", 1)]
    assert sum(1 for c in tr.calls[:freezes[0]] if c[0] == "step") == 4
    # checkpoints when (epoch + 1) % save_frequency == 0
    saves = [i for i, c in enumerate(tr.calls) if c[0] == "save"]
    assert [tr.calls[i] for i in saves] == [("save", 1)] and sum(1 for c in tr.calls[:saves[0]] if c[0] == "step") == 8
    assert os.path.isfile(os.path.join(str(tmp_path), "stub", "models", "opt.json"))
    # log steps: items 0 and 2 of every epoch; one validation item each, the 3-item loader cycling into its next epoch
    train_rows, val_rows = _rows(tmp_path, "train"), _rows(tmp_path, "val")
    assert [r["step"] for r in train_rows] == [r["step"] for r in val_rows] == [0, 2, 4, 6, 8, 10]
    assert train_rows[1] == {"step": 2, "loss": 3.5} and val_rows[0] == {"step": 0, "loss": 2.0}
    assert [c[1] for c in tr.calls if c[0] == "val"] == [0.0, 1.0, 2.0, 10.0, 11.0, 12.0]
    assert [c[0] for c in tr.calls[:5]] == ["step", "val", "step", "step", "val"]
    assert len(capsys.readouterr().out.splitlines()) == 6


def test_the_log_rule_holds_after_step_2000(tmp_path):
    """The counter preset beyond 2000: Trainer.train would log only every 2000th step there, this loop keeps logging at
    every log_frequency-th item and at the multiples of 2000 in between."""
    tr = _stub(tmp_path, num_epochs=1, h_s_epoch=99)
    tr.train_loader = _StubLoader(7)

    tr.start_time, tr.num_total_steps = time.time(), 7                        # what train_sequences sets before its first epoch
    tr.step = 3995
    tr.start_epoch(0)
    tr.run_sequence_epoch()
    # items 0, 2, 4, 6 are steps 3995, 3997, 3999, 4001; step 4000 (item 5) is a multiple of 2000
    assert [r["step"] for r in _rows(tmp_path, "train")] == [3995, 3997, 3999, 4000, 4001]
    assert len([c for c in tr.calls if c[0] == "val"]) == 5 and tr.model_lr_scheduler.calls == 0


def test_item_batch_entry_points_still_refuse_gru(tmp_path):
    import trainer as T
    tr = _stub(tmp_path)
    with pytest.raises(NotImplementedError):
        tr.train()
    with pytest.raises(NotImplementedError):
        tr.build_loaders()
    with pytest.raises(NotImplementedError, match="ConvGRU"):
        T.Trainer.val(tr, {})
    plain = _stub(tmp_path, gru=None)
    with pytest.raises(ValueError):
        plain.train_sequences()
    with pytest.raises(ValueError):
        T.Trainer.val_sequence(plain, {})
    with pytest.raises(ValueError):
        plain.build_sequence_loaders()


def test_build_sequence_loaders_reads_the_drive_lists(tmp_path):
    import trainer as T
    root = str(tmp_path)
    write_raw_tree(root, frames=12)
    os.makedirs(os.path.join(root, "splits", "mine"))
    for mode, drives in (("train", [DRIVE_A, DRIVE_B]), ("val", [DRIVE_B])):
        with open(os.path.join(root, "splits", "mine", "%s_sequences.txt" % mode), "w") as f:
            f.write("\n".join(drives) + "\n")
    tr = T.Trainer.__new__(T.Trainer)
    tr.opt = types.SimpleNamespace(gru="v5", batch_size=1, frame_ids=[0, -1, 1], png=True, splits_dir=os.path.join(root, "splits"),
                                   split="mine", data_path=root, height=32, width=96, num_workers=2, len_sequence=2, train_n_tuples=3,
                                   test_n_tuples=7)
    tr.device, tr.rank, tr.world_size = torch.device("cpu"), 0, 1
    train, val = tr.build_sequence_loaders()
    assert len(train) == 12 and len(val) == 7 and tr.train_loader is train and tr.val_loader is val     # 2 x max(12 // 2, 3); max(6, 7)
    assert train.is_train and train.shuffle and not val.is_train and not val.shuffle
    assert train.dataset.n == 2 and train.dataset.img_ext == ".png" and val.dataset.sequences[0][0] == DRIVE_B
    assert all(draw == (False, None) for _, draw in val.plan(0))
    again = tr.build_sequence_loaders()[0]
    assert [(d, f.start) for d, f in again.dataset.sequences] == [(d, f.start) for d, f in train.dataset.sequences]
    tr.opt.batch_size = 2
    with pytest.raises(ValueError, match="batch_size 1"):
        tr.build_sequence_loaders()
    tr.opt.batch_size, tr.opt.split = 1, "other"
    with pytest.raises(FileNotFoundError, match="train_sequences.txt"):
        tr.build_sequence_loaders()


def test_train_gru_py_refuses_stereo_and_sets_the_front_end(monkeypatch):
    import train_gru
    with pytest.raises(SystemExit) as e:
        train_gru.main(["--use_stereo"])
    assert "stereo" in str(e.value)
    import trainer as T
    seen = {}

    class Fake:
        def __init__(self, opts):
            seen["gru"], seen["batch_size"] = opts.gru, opts.batch_size

        def train_sequences(self):
            seen["trained"] = True

        def close(self):
            seen["closed"] = True
    monkeypatch.setattr(T, "Trainer", Fake)
    train_gru.main(["--batch_size", "4"])
    assert seen == {"gru": "v5", "batch_size": 1, "trained": True, "closed": True}
