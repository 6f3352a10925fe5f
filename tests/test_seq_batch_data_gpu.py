"""The data step of a STEP of several sequence items on the GPU (GpuPreprocessor.sequence_batch / dc_data_seq_batch_levels):
every item's rows of the time-major stack are BITWISE what the single-item entry (GpuPreprocessor.sequence /
dc_data_seq_levels) gives for that item with the same draws -- un-jittered and jittered, at every split between the HBM levels
and the on-chip tail, for one item, for n = 1, for items of two native sizes, and for a jittered step that holds an item
without a draw -- and one item is checked against the CPU restatement of the reference's chain (tests/seq_data_ref.py)."""
import functools
import random

import numpy as np
import pytest
import torch

import seq_data_ref as R
from helpers import data_case_image

pytestmark = pytest.mark.gpu

H, W, LEVELS = 32, 96, 4
FLIPS = (True, False, True)
NATIVE = (47, 155)
OTHER = (45, 150)


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def natives(sizes, n):
    """One (n + 2, Hn, Wn, 3) uint8 array per item, every frame its own picture."""
    return tuple(np.stack([data_case_image(hn, wn, 500 + 31 * it + 7 * i) for i in range(n + 2)]) for it, (hn, wn) in enumerate(sizes))


def draws(item, n):
    """jitters[w][j][s] of one item: every (window, frame, level) its own order and factors, different for every item."""
    rng = random.Random("seq-batch-test/%d" % item)
    return [[[(tuple(rng.sample(range(4), 4)), (rng.uniform(0.8, 1.2), rng.uniform(0.8, 1.2), rng.uniform(0.8, 1.2), rng.uniform(-0.1, 0.1)))
              for _ in range(LEVELS)] for _ in range(n)] for _ in range(3)]


def pack(frames):
    return torch.from_numpy(np.concatenate([f.reshape(-1) for f in frames])).to(_dev())


def run_batch(sizes, n, flips, jitters, budget=0):
    from depthcore.data import GpuPreprocessor
    pre = GpuPreprocessor(H, W, num_scales=LEVELS, device=_dev())
    pre.seq_lds_budget = budget
    out = pre.sequence_batch(pack(natives(tuple(sizes), n)), sizes, n, flips, jitters)
    return pre, out


def run_single(native, flip, jitters, budget=0):
    from depthcore.data import GpuPreprocessor
    pre = GpuPreprocessor(H, W, num_scales=LEVELS, device=_dev())
    pre.seq_lds_budget = budget
    return pre.sequence(torch.from_numpy(native).to(_dev()), flip, jitters)


def check_items(out, singles, n):
    """Every item's rows (frame j of item s is row j * S + s) equal that item's own dict, key by key, bit by bit."""
    from depthcore.data import seq_item_rows
    S = len(singles)
    keys = {(name, f, s) for name in ("color", "color_aug") for f in (0, -1, 1) for s in range(LEVELS)} | \
        {("color_packed", f, 0) for f in (0, -1, 1)}
    assert set(out) == keys
    for key in keys:
        got = out[key]
        assert got.shape[0] == n * S and got.dtype == torch.float32 and got.is_contiguous(), key
        if key[0] == "color":
            assert got.shape == (n * S, 3, H >> key[2], W >> key[2]) and out[("color_aug",) + key[1:]] is got
        else:
            assert key[0] == "color_aug" or (got.shape == (n * S, H, W, 4) and got.data_ptr() % 16 == 0)
        for s, one in enumerate(singles):
            assert torch.equal(got[seq_item_rows(s, S, n)], one[key]), (key, s)


def budgets(n, jitter):
    """LDS budgets that start the tail at level 0, at level 1 (the library's default at this size) and nowhere."""
    from depthcore.data import GpuPreprocessor
    pre = GpuPreprocessor(H, W, num_scales=LEVELS, device=_dev())
    first = {}
    for b in range(64, 16384, 64):
        pre.seq_lds_budget = b
        first.setdefault(pre.sequence_batch_plan(3, n, jitter).tail_start, b)
    pre.seq_lds_budget = 0
    assert pre.sequence_batch_plan(3, n, jitter).tail_start == 1
    return {0: first[0], 1: 0, 4: first[4]}


@pytest.mark.parametrize("tail", [1, 0, 4])
@pytest.mark.parametrize("jitter", [False, True])
def test_items_of_a_step_equal_the_single_item_entry(jitter, tail):
    n, S = 3, 3
    sizes = [NATIVE] * S
    budget = budgets(n, jitter)[tail]
    jit = [draws(it, n) if jitter else None for it in range(S)]
    pre, out = run_batch(sizes, n, FLIPS, jit, budget)
    plan = pre.sequence_batch_plan(S, n, jitter)
    assert plan.tail_start == tail and plan.n_img == S * (3 * n if jitter else n + 2)
    singles = [run_single(natives(tuple(sizes), n)[it], FLIPS[it], jit[it], budget) for it in range(S)]
    check_items(out, singles, n)


def test_unjittered_windows_are_slices_of_one_time_major_pyramid():
    n, S = 3, 3
    _, out = run_batch([NATIVE] * S, n, FLIPS, None)
    for s in range(LEVELS):
        slab = S * 3 * (H >> s) * (W >> s) * 4                                   # one time step of the S items
        c = out[("color", 0, s)]
        assert out[("color", -1, s)].data_ptr() == c.data_ptr() - slab and out[("color", 1, s)].data_ptr() == c.data_ptr() + slab
        assert c.untyped_storage().data_ptr() == out[("color", -1, s)].untyped_storage().data_ptr() == out[("color", 1, s)].untyped_storage().data_ptr()
    pk = out[("color_packed", 0, 0)]
    assert out[("color_packed", -1, 0)].data_ptr() == pk.data_ptr() - S * H * W * 16


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("S,n", [(1, 3), (3, 1), (2, 2)])
def test_one_item_and_one_frame(S, n, jitter):
    sizes = [NATIVE] * S
    jit = [draws(it, n) if jitter else None for it in range(S)]
    _, out = run_batch(sizes, n, FLIPS[:S], jit)
    singles = [run_single(natives(tuple(sizes), n)[it], FLIPS[it], jit[it]) for it in range(S)]
    check_items(out, singles, n)


@pytest.mark.parametrize("jitter", [False, True])
def test_one_item_of_a_step_against_the_cpu_chain(jitter):
    from depthcore.data import seq_item_rows
    n, S = 3, 3
    sizes = [NATIVE] * S
    jit = [draws(it, n) if jitter else None for it in range(S)]
    _, out = run_batch(sizes, n, FLIPS, jit)
    for it in (0, 1):                                                           # a mirrored item and a plain one
        want = R.sequence_item(natives(tuple(sizes), n)[it], H, W, LEVELS, FLIPS[it], jit[it])
        for key, v in want.items():
            assert np.array_equal(out[key][seq_item_rows(it, S, n)].cpu().numpy(), v), (it, key)


@pytest.mark.parametrize("jitter", [False, True])
def test_two_native_sizes_in_one_step(jitter):
    """Drives of different native sizes in one step: level 0 comes from the ragged resize passes."""
    n = 3
    sizes = [NATIVE, OTHER, NATIVE]
    jit = [draws(it, n) if jitter else None for it in range(3)]
    _, out = run_batch(sizes, n, FLIPS, jit)
    singles = [run_single(natives(tuple(sizes), n)[it], FLIPS[it], jit[it]) for it in range(3)]
    check_items(out, singles, n)
    # and a step whose items already have the target's size: no resize at all
    sizes = [(H, W), (H, W)]
    _, out = run_batch(sizes, 2, (False, True), None)
    check_items(out, [run_single(natives(tuple(sizes), 2)[it], (False, True)[it], None) for it in range(2)], 2)


def test_an_item_without_a_draw_in_a_jittered_step():
    """A step is jittered as a whole: the item without a draw carries no-op steps, and its windows hold the bytes of its plain
    pyramid (what `sequence` hands out as slices for that item)."""
    n, S = 3, 3
    sizes = [NATIVE] * S
    jit = [draws(0, n), None, draws(2, n)]
    _, out = run_batch(sizes, n, FLIPS, jit)
    singles = [run_single(natives(tuple(sizes), n)[it], FLIPS[it], jit[it]) for it in range(S)]
    check_items(out, singles, n)


def test_two_calls_give_the_same_bits_and_bad_steps_are_refused():
    from depthcore import _lib
    from depthcore.data import GpuPreprocessor
    n, S = 3, 3
    jit = [draws(it, n) for it in range(S)]
    _, a = run_batch([NATIVE] * S, n, FLIPS, jit)
    _, b = run_batch([NATIVE] * S, n, FLIPS, jit)
    assert all(torch.equal(a[k], b[k]) for k in a)
    pre = GpuPreprocessor(H, W, device=_dev())
    packed = pack(natives((NATIVE,) * S, n))
    with pytest.raises(_lib.DepthcoreError):
        pre.sequence_batch(packed, [NATIVE] * S, n, FLIPS[:2])                   # one flip short
    with pytest.raises(_lib.DepthcoreError):
        pre.sequence_batch(packed[:-3], [NATIVE] * S, n, FLIPS)                  # not n + 2 frames per item
    with pytest.raises(_lib.DepthcoreError):
        pre.sequence_batch(packed, [NATIVE] * S, n, FLIPS, [draws(0, n + 1), None, None])   # jitters of another n
    with pytest.raises(_lib.DepthcoreError):
        pre.sequence_batch(packed.float(), [NATIVE] * S, n, FLIPS)
