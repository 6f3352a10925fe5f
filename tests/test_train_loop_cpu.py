"""Trainer.train() / run_epoch() / log() on a stub trainer (no GPU, no networks): the log-step predicate, where the
learning-rate scheduler steps, which checkpoints are written, what lands in scalars.jsonl."""
import json
import os
import types

import torch


def test_log_step_predicate_is_the_reference_s():
    from trainer import Trainer
    f = Trainer.is_log_step
    # early phase: every log_frequency-th batch of an epoch while fewer than 2000 steps have been taken
    assert [b for b in range(8) if f(b, 100 + b, 2)] == [0, 2, 4, 6]
    assert f(0, 1999, 250) and f(250, 1999, 250) and not f(249, 1999, 250)
    # late phase: every 2000th step, whatever the batch index
    assert not f(0, 2001, 250) and not f(250, 3999, 250)
    assert f(17, 2000, 250) and f(17, 4000, 250) and f(17, 0, 250)
    assert [s for s in range(1990, 6001) if f(s % 7 + 1, s, 1)] == list(range(1990, 2000)) + [2000, 4000, 6000]


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


def _stub(tmp_path, **kw):
    """A Trainer without __init__: the loop's own state and recording stand-ins for the step, validation and checkpoint."""
    import trainer as T
    tr = T.Trainer.__new__(T.Trainer)
    opt = dict(num_epochs=3, save_frequency=2, log_frequency=2, batch_size=2, scheduler_step_size=1, learning_rate=1e-4,
               log_dir=str(tmp_path), model_name="stub", fusion=None, gru=None, h_s_epoch=10)
    opt.update(kw)
    tr.opt = types.SimpleNamespace(**opt)
    tr.device = torch.device("cpu")
    tr.step = tr.epoch = 0
    tr.models = {}
    tr.train_loader, tr.val_loader, tr._val_iter = _StubLoader(4), _StubLoader(3), None
    w = torch.nn.Parameter(torch.zeros(1))
    tr.model_optimizer = torch.optim.SGD([w], tr.opt.learning_rate)
    tr.model_lr_scheduler = torch.optim.lr_scheduler.StepLR(tr.model_optimizer, tr.opt.scheduler_step_size, 0.1)
    tr.calls = []

    def train_step(inputs):
        tr.calls.append(("step", tr.epoch, float(inputs["x"]), tr.model_optimizer.param_groups[0]["lr"]))
        tr.step += 1
        return {}, {"loss": torch.tensor(0.5 + tr.step), "loss/0": torch.tensor(1.0)}

    def val(inputs):
        tr.calls.append(("val", float(inputs["x"])))
        return {}, {"loss": torch.tensor(2.0)}
    tr.train_step, tr.val = train_step, val
    tr.save_model = lambda: tr.calls.append(("save", tr.epoch))
    return tr


def _rows(tmp_path, mode):
    with open(os.path.join(str(tmp_path), "stub", mode, "scalars.jsonl")) as f:
        return [json.loads(line) for line in f]


def test_train_loop_order_scheduler_and_logs(tmp_path, capsys):
    tr = _stub(tmp_path)
    tr.train()
    steps = [c for c in tr.calls if c[0] == "step"]
    assert len(steps) == 12 and tr.step == 12 and tr.num_total_steps == 12
    assert tr.train_loader.epochs_seen == [0, 1, 2]
    # the scheduler steps at the END of an epoch: every step of epoch 0 runs at the initial rate
    lrs = [round(c[3] / 1e-4, 6) for c in steps]
    assert lrs == [1.0] * 4 + [0.1] * 4 + [0.01] * 4
    assert abs(tr.model_optimizer.param_groups[0]["lr"] - 1e-7) < 1e-12
    # checkpoints when (epoch + 1) % save_frequency == 0, after that epoch's last step; opt.json once
    saves = [i for i, c in enumerate(tr.calls) if c[0] == "save"]
    assert [tr.calls[i] for i in saves] == [("save", 1)]
    assert sum(1 for c in tr.calls[:saves[0]] if c[0] == "step") == 8
    assert os.path.isfile(os.path.join(str(tmp_path), "stub", "models", "opt.json"))
    # log steps: batches 0 and 2 of every epoch -> steps 0, 2, 4, 6, 8, 10; one validation batch each, the 3-batch
    # validation loader cycling into its next epoch
    train_rows, val_rows = _rows(tmp_path, "train"), _rows(tmp_path, "val")
    assert [r["step"] for r in train_rows] == [r["step"] for r in val_rows] == [0, 2, 4, 6, 8, 10]
    assert train_rows[1] == {"step": 2, "loss": 3.5, "loss/0": 1.0} and val_rows[0] == {"step": 0, "loss": 2.0}
    assert [c[1] for c in tr.calls if c[0] == "val"] == [0.0, 1.0, 2.0, 10.0, 11.0, 12.0]
    # validation follows the step it belongs to
    assert [c[0] for c in tr.calls[:5]] == ["step", "val", "step", "step", "val"]
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 6 and out[0].startswith("epoch   0 | batch      0 | examples/s:") and "| loss: 1.50000 | time elapsed: 00h00m00s" in out[0]


def test_fusion_front_end_skips_val_and_gru_is_refused(tmp_path):
    import pytest
    tr = _stub(tmp_path, fusion="v3", num_epochs=1)
    tr.train()
    assert not [c for c in tr.calls if c[0] == "val"]
    assert [r["step"] for r in _rows(tmp_path, "train")] == [0, 2]
    assert not os.path.exists(os.path.join(str(tmp_path), "stub", "val"))
    with pytest.raises(NotImplementedError):
        _stub(tmp_path, gru="v5").train()


def test_train_py_refuses_stereo():
    import pytest
    import train
    with pytest.raises(SystemExit) as e:
        train.main(["--use_stereo"])
    assert "stereo" in str(e.value)
