"""Several sequence items per step (`--seq_batch S`) without a GPU: the time-major row rule, the loader's plan cut into runs of
S, the option and the trainer's refusals, and the host-side checks of dc_data_seq_batch_plan / dc_data_seq_batch_levels /
dc_gru_state_bwd (no HIP call is made before they answer)."""
import ctypes

import numpy as np
import pytest

from kitti_tree import DRIVES

DRIVE_A, DRIVE_B = sorted(DRIVES)


def test_row_rule_is_time_major():
    from depthcore import ops
    from depthcore.data import seq_item_rows, seq_rows
    assert ops.seq_rows is seq_rows and ops.seq_item_rows is seq_item_rows
    n, S = 4, 3
    rows = np.arange((n + 2) * S)
    for j in range(n + 2):
        assert rows[seq_rows(j, S)].tolist() == [j * S + s for s in range(S)]              # frame j of every item: one slab
    assert rows[seq_rows(1, S, n)].tolist() == list(range(S, (n + 1) * S))                 # the centre window [S : (n+1)S]
    assert rows[seq_rows(0, S, n)].tolist() == list(range(0, n * S))                       # left  [0 : nS]
    assert rows[seq_rows(2, S, n)].tolist() == list(range(2 * S, (n + 2) * S))             # right [2S : (n+2)S]
    for s in range(S):
        assert rows[:n * S][seq_item_rows(s, S, n)].tolist() == [j * S + s for j in range(n)]
    # the items partition the rows, and S = 1 is the single sequence
    assert sorted(r for s in range(S) for r in rows[:n * S][seq_item_rows(s, S, n)]) == list(range(n * S))
    assert seq_rows(2, 1) == slice(2, 3) and rows[:n][seq_item_rows(0, 1, n)].tolist() == list(range(n))


def test_loader_plan_is_the_single_item_plan_cut_into_runs(tmp_path):
    import datasets
    from depthcore.loader import SequenceLoader
    items = [(DRIVE_A, range(i, i + 4)) for i in range(11)]
    ds = datasets.KITTISequenceDataset(str(tmp_path), 32, 96, 2, items, True, img_ext=".png")
    one = SequenceLoader(ds, device="cpu", seed=3)
    three = SequenceLoader(ds, device="cpu", seed=3, items_per_step=3)
    assert len(one) == 11 and len(three) == 11 // 3 and three.items_per_step == 3 and one.items_per_step == 1
    for epoch in (0, 1, 5):
        flat, steps = one.plan(epoch), three.plan(epoch)
        assert len(steps) == 3                                                           # the partial step of 2 items is dropped
        for k, (indices, draws) in enumerate(steps):
            assert len(indices) == len(draws) == 3
            assert list(zip(indices, draws)) == flat[3 * k:3 * k + 3]                    # the same items, the same draws
    assert three.plan(0) == three.plan(0) != three.plan(1)
    assert SequenceLoader(ds, device="cpu", seed=3, items_per_step=3).plan(1) == three.plan(1)    # (seed, epoch) alone
    assert SequenceLoader(ds, device="cpu", seed=4, items_per_step=3).plan(1) != three.plan(1)
    three.set_epoch(1)
    assert three.plan() == three.plan(1)
    assert any(d[1] is not None for _, draws in three.plan(0) for d in draws)            # jittered items among them
    assert SequenceLoader(ds, device="cpu", items_per_step=1).plan(0) == SequenceLoader(ds, device="cpu").plan(0)
    with pytest.raises(ValueError):
        SequenceLoader(ds, device="cpu", items_per_step=0)


def test_option_default_and_trainer_refusals():
    import trainer as T
    from options import MonodepthOptions
    assert T.default_options().seq_batch == 1
    assert MonodepthOptions().parse(["--seq_batch", "4"]).seq_batch == 4 and MonodepthOptions().parse([]).seq_batch == 1
    kw = dict(batch_size=1, height=32, width=96, len_sequence=3)
    with pytest.raises(ValueError, match="seq_batch"):
        T.Trainer(T.default_options(gru="v5", seq_batch=0, **kw), device="cpu", seed=1)
    with pytest.raises(ValueError, match="seq_batch"):
        T.Trainer(T.default_options(gru="v5", seq_batch=-2, **kw), device="cpu", seed=1)
    with pytest.raises(ValueError, match="ConvGRU"):
        T.Trainer(T.default_options(seq_batch=2, **kw), device="cpu", seed=1)             # no gru front-end
    with pytest.raises(NotImplementedError, match="hip_graph"):
        T.Trainer(T.default_options(gru="v5", seq_batch=2, hip_graph=1, **kw), device="cpu", seed=1)
    with pytest.raises(ValueError, match="batch_size"):
        T.Trainer(T.default_options(gru="v5", seq_batch=2, height=32, width=96, len_sequence=3, batch_size=2), device="cpu", seed=1)
    tr = T.Trainer(T.default_options(gru="v5", seq_batch=2, **kw), device="cpu", seed=1)
    assert tr.seq_batch == 2 and tr.opt.batch_size == 1 and tr.loss_batch == 6
    assert T.Trainer(T.default_options(gru="v5", **kw), device="cpu", seed=1).seq_batch == 1


def test_train_gru_script_sets_the_option(monkeypatch):
    import train_gru
    import trainer as T
    seen = {}

    class Stub:
        def __init__(self, opts):
            seen["opts"] = opts

        def train_sequences(self):
            seen["ran"] = True

        def close(self):
            pass
    monkeypatch.setattr(T, "Trainer", Stub)
    train_gru.main(["--seq_batch", "4", "--batch_size", "12"])
    assert seen["ran"] and seen["opts"].seq_batch == 4 and seen["opts"].batch_size == 1 and seen["opts"].gru == "v5"
    train_gru.main([])
    assert seen["opts"].seq_batch == 1 and seen["opts"].batch_size == 1


def test_synthetic_items_argument():
    import torch
    from depthcore.synthetic import synthetic_sequence_batch
    cpu = torch.device("cpu")
    per_j = synthetic_sequence_batch(3, 32, 96, cpu)
    assert ("color", 0, 0, 2) in per_j and ("color", 0, 0) not in per_j                  # the default keeps today's schema
    with pytest.raises(ValueError):
        synthetic_sequence_batch(3, 32, 96, cpu, items=0)


def test_batch_plan_scales_with_the_items():
    from depthcore import _lib
    L = _lib.lib()

    def plan(items, n, h, w, S, jitter=0, budget=0):
        p = _lib.SeqPlan()
        assert L.dc_data_seq_batch_plan(items, n, h, w, S, jitter, budget, p) == 0
        return p

    def single(n, h, w, S, jitter=0, budget=0):
        p = _lib.SeqPlan()
        assert L.dc_data_seq_plan(n, h, w, S, jitter, budget, p) == 0
        return p
    fields = ("lds_bytes", "table_len", "scratch_bytes", "n_img", "tail_start")
    for args in ((3, 32, 96, 4, 0, 0), (3, 32, 96, 4, 1, 0), (10, 192, 640, 4, 1, 160 * 1024), (1, 64, 192, 4, 0, 64)):
        a, b = plan(1, *args), single(*args)
        assert all(getattr(a, f) == getattr(b, f) for f in fields), args                # one item IS the single-item plan
    # the split honours the budget with the single item's rule: it does not move with the number of items
    for budget in (0, 1, 2048, 8192, 160 * 1024):
        for jitter in (0, 1):
            one, many = single(3, 32, 96, 4, jitter, budget), plan(3, 3, 32, 96, 4, jitter, budget)
            assert (many.tail_start, many.lds_bytes, many.table_len) == (one.tail_start, one.lds_bytes, one.table_len)
            assert many.n_img == 3 * one.n_img
    assert plan(3, 3, 32, 96, 4).n_img == 15 and plan(3, 3, 32, 96, 4, 1).n_img == 27
    p = plan(4, 10, 192, 640, 4, 1)
    levels = [120 * (192 >> s) * (640 >> s) * 3 for s in range(4)]
    assert p.scratch_bytes == 120 * 4 * 8 + sum(levels[:3]) + 120 * 192 * 320 * 3 + levels[1]
    q = _lib.SeqPlan()
    for bad in ((0, 3, 32, 96, 4), (-1, 3, 32, 96, 4), (65, 3, 32, 96, 4), (2, 0, 32, 96, 4), (2, 3, 36, 96, 4), (2, 3, 32, 96, 5)):
        assert L.dc_data_seq_batch_plan(*bad, 0, 0, q) == -1, bad
    assert L.dc_data_seq_batch_plan(64, 400, 32, 96, 4, 1, 0, q) == -1                   # 76800 images: more than a grid holds
    assert L.dc_data_seq_batch_plan(2, 3, 32, 96, 4, 0, -1, q) == -1
    assert L.dc_data_seq_batch_plan(2, 3, 32, 96, 4, 0, 0, None) == -1


def test_batch_levels_refuses_bad_arguments_before_any_launch():
    """DC_EINVAL / DC_EWORKSPACE from the host-side check: no HIP call is made, so made-up device pointers are fine here."""
    from depthcore import _lib
    from depthcore.data import resample_table
    L = _lib.lib()
    fake = 4096                                                                   # never dereferenced
    h, w, S = 32, 96, 4
    parts = []
    for s in range(1, S):
        for size in (w, h):
            bounds, kk = resample_table(size >> (s - 1), size >> s)
            parts += [bounds.reshape(-1), kk.reshape(-1)]
    tab = np.concatenate(parts)
    plan = _lib.SeqPlan()
    assert L.dc_data_seq_batch_plan(3, 3, h, w, S, 1, 1, plan) == 0 and plan.table_len == tab.size

    def call(items=3, n=3, h=h, w=w, S=S, frames=fake, flips=True, color=True, color_null=None, packed=fake, steps=fake, params=fake,
             tab=tab, tab_host=True, tab_dev=fake, tab_len=None, scratch=fake, scratch_bytes=1 << 30):
        ptrs = (ctypes.c_void_p * 4)(*[fake] * max(min(S, 4), 0))
        if color_null is not None:
            ptrs[color_null] = None
        fl = (ctypes.c_int * max(items, 1))(*[1, 0, 1][:max(min(items, 3), 0)])
        return L.dc_data_seq_batch_levels(frames, items, n, h, w, S, fl if flips else None, ptrs if color else None, packed, steps,
                                          params, tab.ctypes.data if tab_host else None, tab_dev,
                                          tab.size if tab_len is None else tab_len, scratch, scratch_bytes, 1, None)
    worse = tab.copy()
    worse[0] = -1
    refused = {
        "no frames": call(frames=None),
        "no flips": call(flips=False),
        "items 0": call(items=0),
        "items negative": call(items=-3),
        "items 65": call(items=65),
        "no color": call(color=False),
        "a level without color": call(color_null=1),
        "no packed": call(packed=None),
        "packed not 16-byte aligned": call(packed=fake + 4),
        "no scratch": call(scratch=None),
        "scratch not 16-byte aligned": call(scratch=fake + 8),
        "steps without params": call(params=None),
        "params without steps": call(steps=None),
        "n 0": call(n=0),
        "height not divisible by 8": call(h=36),
        "num_scales 5": call(S=5),
        "no host tables": call(tab_host=False),
        "no device tables": call(tab_dev=None),
        "tables of another length": call(tab_len=tab.size + 1),
        "negative tap start": call(tab=worse),
    }
    assert all(rc == -1 for rc in refused.values()), refused
    assert call(scratch_bytes=plan.scratch_bytes - 1) == -3                      # DC_EWORKSPACE, still before any launch
    single = _lib.SeqPlan()
    assert L.dc_data_seq_plan(3, h, w, S, 1, 1, single) == 0
    assert call(scratch_bytes=single.scratch_bytes) == -3                        # one item's scratch does not serve three


def test_state_bwd_refuses_bad_arguments_and_the_symbols_are_exported():
    from depthcore import _lib
    L = _lib.lib()
    assert not _lib.MISSING
    for name in ("dc_data_seq_batch_plan", "dc_data_seq_batch_levels", "dc_gru_state_bwd"):
        assert name in _lib.EXPORTS
    fake = 4096
    assert L.dc_gru_state_bwd(None, fake, 2, 64, None) == -1
    assert L.dc_gru_state_bwd(fake, None, 2, 64, None) == -1
    assert L.dc_gru_state_bwd(fake, fake, 0, 64, None) == -1
    assert L.dc_gru_state_bwd(fake, fake, -1, 64, None) == -1
    assert L.dc_gru_state_bwd(fake, fake, 2, 0, None) == -1


def test_plan_streams_setting_is_per_thread_and_returns_the_previous_value():
    import threading
    from depthcore import _lib, ops
    L = _lib.lib()
    assert "dc_set_wino_plan_streams" in _lib.EXPORTS
    assert L.dc_set_wino_plan_streams(3) == 1 and L.dc_set_wino_plan_streams(1) == 3
    assert L.dc_set_wino_plan_streams(0) == -1 and L.dc_set_wino_plan_streams(-2) == -1 and L.dc_set_wino_plan_streams(1) == 1
    with ops._plan_streams(4):
        seen = []
        t = threading.Thread(target=lambda: seen.append(L.dc_set_wino_plan_streams(1)))      # another thread: its own default
        t.start()
        t.join()
        assert seen == [1] and L.dc_set_wino_plan_streams(4) == 4
    assert L.dc_set_wino_plan_streams(1) == 1                                   # restored on the way out
    with ops._plan_streams(1):                                                  # one stream touches nothing
        assert L.dc_set_wino_plan_streams(1) == 1
    # the workspace queries made under a setting cover its launches: never smaller than the plain query
    for B in (2, 4, 6):
        plain = L.dc_conv3x3_fwd_workspace(64, 64, B, 128, 32, 64), L.dc_conv3x3_bwd_workspace(64, 64, B, 128, 32, 64)
        with ops._plan_streams(2):
            under = L.dc_conv3x3_fwd_workspace(64, 64, B, 128, 32, 64), L.dc_conv3x3_bwd_workspace(64, 64, B, 128, 32, 64)
        assert under[0] >= plain[0] and under[1] >= plain[1]
