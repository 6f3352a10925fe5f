"""The sequence data step without a GPU: the chain reference of the sequence tests pinned against the installed Pillow, the
order of `sample_sequence`'s draws, and the host-side plan and refusals of dc_data_seq_levels."""
import ctypes
import random

import numpy as np
import pytest

import seq_data_ref as R
from helpers import data_case_image
from oracle import data_ref as D


@pytest.mark.parametrize("sizes", [(47, 155, 32, 96), (375, 1242, 192, 640)])
@pytest.mark.parametrize("flip", [False, True])
def test_chain_reference_equals_pillow(sizes, flip):
    from depthcore.frame_cache import tables_mirror_symmetric
    hn, wn, h, w = sizes
    native = data_case_image(hn, wn, 11)
    got, want = R.frame_chain(native, h, w, 4, flip), R.pillow_chain(native, h, w, 4, flip)
    for s in range(4):
        assert got[s].shape == (h >> s, w >> s, 3) and np.array_equal(got[s], want[s]), (s, flip)
    # the cumulative mirror: where the tables are mirror-symmetric, levels 1 and 3 of the flipped chain are the unflipped
    # pyramid and levels 0 and 2 its mirror
    if flip:
        assert all(tables_mirror_symmetric(a, b) for a, b in [(wn, w)] + [(w >> s, w >> (s + 1)) for s in range(3)])
        plain = R.frame_chain(native, h, w, 4, False)
        for s in range(4):
            assert np.array_equal(got[s], plain[s] if s % 2 else plain[s][:, ::-1]), s


def test_chain_resizes_from_the_jittered_level():
    native = data_case_image(47, 155, 5)
    jit = [((1, 0, 2, 3), (0.9, 1.15, 0.85, 0.05)), ((3, 2, 0, 1), (1.1, 0.9, 1.2, -0.07))]
    u = R.frame_chain(native, 32, 96, 2, True, jit)
    l0 = D.color_jitter(np.ascontiguousarray(D.resize_lanczos(native, 32, 96)[:, ::-1]), *jit[0])
    l1 = D.color_jitter(np.ascontiguousarray(D.resize_lanczos(l0, 16, 48)[:, ::-1]), *jit[1])
    assert np.array_equal(u[0], l0) and np.array_equal(u[1], l1)
    item = R.sequence_item(np.stack([native] * 3), 32, 96, 2, False, None)
    assert item[("color", 0, 1)].shape == (1, 3, 16, 48) and item[("color_packed", -1, 0)].shape == (1, 32, 96, 4)
    assert np.array_equal(item[("color", 0, 0)], item[("color", 1, 0)])            # three equal frames, no jitter


class Tape:
    """A random.Random behind the three methods the sampler may use, recording every draw by kind."""

    def __init__(self, seed):
        self.inner, self.tape = random.Random(seed), []

    def random(self):
        self.tape.append("r")
        return self.inner.random()

    def uniform(self, a, b):
        self.tape.append(("u", a, b))
        return self.inner.uniform(a, b)

    def shuffle(self, x):
        self.tape.append("s")
        self.inner.shuffle(x)


def test_sample_sequence_draw_order():
    from depthcore.data import sample_sequence
    n, S = 3, 4
    seen = set()
    for seed in range(12):
        rng, twin = Tape(seed), random.Random(seed)
        flip, jitters = sample_sequence(True, rng, n, S)
        want_flip, want_aug = twin.random() > 0.5, twin.random() > 0.5          # the flip is drawn first
        assert flip == want_flip and (jitters is not None) == want_aug
        seen.add((flip, jitters is not None))
        one = [("u", 0.8, 1.2), ("u", 0.8, 1.2), ("u", 0.8, 1.2), ("u", -0.1, 0.1), "s"]
        assert rng.tape == ["r", "r"] + (one * (3 * n * S) if want_aug else [])
        if want_aug:
            assert len(jitters) == 3 and all(len(win) == n and all(len(lv) == S for lv in win) for win in jitters)
            for w in range(3):                                                    # window-major, then frame, then level
                for j in range(n):
                    for s in range(S):
                        factors = tuple(twin.uniform(*r) for r in ((0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.1, 0.1)))
                        order = [0, 1, 2, 3]
                        twin.shuffle(order)
                        assert jitters[w][j][s] == (tuple(order), factors)
        assert twin.random() == rng.inner.random()                        # and nothing else was drawn
    assert len(seen) == 4
    rng = Tape(0)
    assert sample_sequence(False, rng, n, S) == (False, None) and rng.tape == []


def test_plan_splits_by_the_lds_budget():
    from depthcore import _lib
    L = _lib.lib()

    def plan(n, h, w, S, jitter=0, budget=0):
        p = _lib.SeqPlan()
        assert L.dc_data_seq_plan(n, h, w, S, jitter, budget, p) == 0
        return p
    cap = 160 * 1024
    # the default budget (12 KiB) hands the tail small levels only: none at the training sizes
    assert plan(3, 16, 96, 4).tail_start == 0 and plan(3, 32, 96, 4).tail_start == 1 and plan(1, 64, 192, 4).tail_start == 2
    assert plan(10, 192, 640, 4).tail_start == 4 and plan(10, 320, 1024, 4, 1).tail_start == 4 and plan(10, 192, 640, 4).lds_bytes == 0
    assert plan(3, 32, 96, 4).n_img == 5 and plan(3, 32, 96, 4, 1).n_img == 9
    p = plan(10, 192, 640, 4, 1)
    levels = [30 * (192 >> s) * (640 >> s) * 3 for s in range(4)]
    assert p.scratch_bytes == 30 * 4 * 8 + sum(levels[:3]) + 30 * 192 * 320 * 3 + levels[1]     # sums, u[0..2], the two passes of level 1
    assert p.table_len == 15 * sum((192 >> s) + (640 >> s) for s in (1, 2, 3))
    # the whole LDS of a workgroup: a level-1 image of 192 x 640 and its pass buffer fit, level 1 of 320 x 1024 does not
    p = plan(10, 192, 640, 4, 1, budget=cap)
    assert p.tail_start == 1 and p.lds_bytes == 92160 + 46080 and p.lds_bytes <= cap
    assert p.scratch_bytes == 30 * 4 * 8 + levels[0]                                # sums and u[0]
    assert plan(10, 192, 640, 4, 1, budget=1 << 30).lds_bytes == p.lds_bytes      # larger budgets are clamped to the hardware's
    assert plan(1, 320, 1024, 4, budget=cap).tail_start == 2
    assert plan(3, 32, 96, 4, budget=cap).tail_start == 0
    assert plan(3, 32, 96, 4, budget=1).tail_start == 4                            # no level fits
    assert plan(3, 32, 96, 1).table_len == 0
    p = _lib.SeqPlan()
    for bad in ((0, 32, 96, 4), (3, 36, 96, 4), (3, 32, 100, 4), (3, 32, 96, 0), (3, 32, 96, 5)):
        assert L.dc_data_seq_plan(*bad, 0, 0, p) == -1, bad
    assert L.dc_data_seq_plan(3, 32, 96, 4, 0, 0, None) == -1


def test_seq_levels_refuses_bad_arguments_before_any_launch():
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
            assert kk.shape[1] == 13
            parts += [bounds.reshape(-1), kk.reshape(-1)]
    tab = np.concatenate(parts)
    plan = _lib.SeqPlan()
    assert L.dc_data_seq_plan(3, h, w, S, 1, 1, plan) == 0 and plan.table_len == tab.size

    def call(n=3, h=h, w=w, S=S, frames=fake, color=True, color_null=None, packed=fake, steps=fake, params=fake, tab=tab, tab_host=True,
             tab_dev=fake, tab_len=None, scratch=fake, scratch_bytes=1 << 30):
        ptrs = (ctypes.c_void_p * 4)(*[fake] * max(min(S, 4), 0))
        if color_null is not None:
            ptrs[color_null] = None
        return L.dc_data_seq_levels(frames, n, h, w, S, 1, ptrs if color else None, packed, steps, params,
                                    tab.ctypes.data if tab_host else None, tab_dev, tab.size if tab_len is None else tab_len,
                                    scratch, scratch_bytes, 1, None)
    worse = tab.copy()
    worse[0] = -1                                                                 # a tap in front of its row
    far = tab.copy()
    far[2 * 48 - 2] = 96                                                          # the last width tap window past the row
    refused = {
        "no frames": call(frames=None),
        "no color": call(color=False),
        "a level without color": call(color_null=2),
        "no packed": call(packed=None),
        "packed not 16-byte aligned": call(packed=fake + 4),
        "no scratch": call(scratch=None),
        "scratch not 16-byte aligned": call(scratch=fake + 8),
        "steps without params": call(params=None),
        "params without steps": call(steps=None),
        "n 0": call(n=0),
        "n negative": call(n=-2),
        "height not divisible by 8": call(h=36),
        "width not divisible by 8": call(w=100),
        "num_scales 0": call(S=0),
        "num_scales 5": call(S=5),
        "no host tables": call(tab_host=False),
        "no device tables": call(tab_dev=None),
        "tables of another length": call(tab_len=tab.size - 1),
        "negative tap start": call(tab=worse),
        "tap past the row": call(tab=far),
    }
    assert all(rc == -1 for rc in refused.values()), refused
    assert call(scratch_bytes=plan.scratch_bytes - 1) == -3                      # DC_EWORKSPACE, still before any launch
    assert call(S=1, tab_host=False, tab_dev=None, tab_len=0, scratch_bytes=0) == -3


def test_seq_symbols_are_part_of_the_abi():
    from depthcore import _lib
    _lib.lib()
    assert "dc_data_seq_levels" in _lib.EXPORTS and "dc_data_seq_plan" in _lib.EXPORTS and not _lib.MISSING
    assert ctypes.sizeof(_lib.SeqPlan) == 32


def test_jitter_rows_under_the_sequence_layout():
    """`GpuPreprocessor.sequence` hands jitters[w][j][s], flattened in that nesting, to the per-draw helper and reads the
    result as (3n, S, 4) tables, row w * n + j, level s: against a literal restatement, for 3 windows x n = 2 x 2 levels,
    a negative hue and shuffled orders."""
    from depthcore.data import HUE, hue_shift, jitter_rows
    n, S = 2, 2
    rng = random.Random(11)
    jitters = [[[(tuple(rng.sample(range(4), 4)), (rng.uniform(0.8, 1.2), rng.uniform(0.8, 1.2), rng.uniform(0.8, 1.2), rng.uniform(-0.1, 0.1)))
                 for _ in range(S)] for _ in range(n)] for _ in range(3)]
    jitters[1][0][1] = ((2, 3, 0, 1), (1.1, 0.9, 1.05, -0.07))
    assert any(order != (0, 1, 2, 3) for win in jitters for lv in win for order, _ in lv)
    steps, params = jitter_rows([draw for win in jitters for levels in win for draw in levels])
    assert steps.shape == params.shape == (3 * n * S, 4) and params.dtype == np.float32
    steps, params = steps.reshape(3 * n, S, 4), params.reshape(3 * n, S, 4)
    for w in range(3):
        for j in range(n):
            for s in range(S):
                order, factors = jitters[w][j][s]
                for k in range(4):
                    assert steps[w * n + j, s, k] == order[k]
                    want = float(hue_shift(factors[3])) if order[k] == HUE else factors[order[k]]
                    assert params[w * n + j, s, k] == np.float32(want)
    assert steps[1 * n + 0, 1].tolist() == [2, 3, 0, 1]
    assert params[1 * n + 0, 1].tolist() == [np.float32(1.05), 239.0, np.float32(1.1), np.float32(0.9)]
