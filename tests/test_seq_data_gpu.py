"""The sequence data step on the GPU: GpuPreprocessor.sequence / dc_data_seq_levels, BITWISE against the reference's chain
restated on the CPU (tests/seq_data_ref.py) and against the per-level composition of the entry points that existed before it
(dc_data_resize_axis x2, dc_data_flip, dc_data_jitter, dc_data_to_tensor, dc_data_to_rgbx).

Cases (native -> target, n, S) and where the on-chip tail starts with the library's default LDS budget (12 KiB):
  A0 47 x 155   -> 16 x 96,    n = 3, S = 4   every level in the tail (tail_start 0), odd native sizes
  A  47 x 155   -> 32 x 96,    n = 3, S = 4   level 0 through HBM, the tail starts at level 1
  F  47 x 155   -> 64 x 192,   n = 1, S = 4   two levels through HBM, the tail starts at level 2
  B  375 x 1242 -> 192 x 640,  n = 1, S = 4   a training size: no level fits the default budget, every level through HBM
  C  375 x 1242 -> 320 x 1024, n = 1, S = 4   the other training size, likewise
  D  32 x 96    -> 32 x 96,    n = 2, S = 4   native == target: no level-0 resize
  E  A's sizes,                n = 3, S = 1   a single level
B and C again with the budget raised to the hardware's 160 KiB (the tail then starts at level 1 and 2: level 1 of 320 x 1024
does not fit), and A with the budget set so that the tail starts at level 0, 1, 2, 3 and nowhere."""
import functools

import numpy as np
import pytest
import torch

import seq_data_ref as R
from helpers import data_case_image

pytestmark = pytest.mark.gpu

CASES = {"A0": (47, 155, 16, 96, 3, 4, 0), "A": (47, 155, 32, 96, 3, 4, 1), "F": (47, 155, 64, 192, 1, 4, 2),
         "B": (375, 1242, 192, 640, 1, 4, 4), "C": (375, 1242, 320, 1024, 1, 4, 4), "D": (32, 96, 32, 96, 2, 4, 1),
         "E": (47, 155, 32, 96, 3, 1, 0)}
LDS_CAP = 160 * 1024
ORDERS = ((1, 0, 2, 3), (0, 2, 3, 1), (3, 1, 0, 2), (2, 3, 1, 0), (1, 3, 2, 0), (2, 0, 3, 1))   # contrast first and last among them


def _dev():
    return torch.device("cuda:0")


def make_jitters(n, S):
    """jitters[w][j][s]: every (window, frame, level) its own order and factors; both hue signs; contrast first / last."""
    out, k = [], 0
    for w in range(3):
        win = []
        for j in range(n):
            levels = []
            for s in range(S):
                t = (k * 0.37) % 1.0
                factors = (0.8 + 0.4 * t, 1.2 - 0.4 * ((t + 0.31) % 1.0), 0.8 + 0.4 * ((t + 0.63) % 1.0), (0.1 - 0.2 * t) * (1 if k % 2 else -1))
                levels.append((ORDERS[k % len(ORDERS)], factors))
                k += 1
            win.append(levels)
        out.append(win)
    flat = [lv for win in out for fr in win for lv in fr]
    assert any(o[0] == 1 for o, _ in flat) and any(o[3] == 1 for o, _ in flat)
    assert any(f[3] > 0.01 for _, f in flat) and any(f[3] < -0.01 for _, f in flat)
    assert len({(o, f) for o, f in flat}) == len(flat)
    return out


@functools.lru_cache(maxsize=None)
def native_frames(case):
    hn, wn, _, _, n, _, _ = CASES[case]
    return np.stack([data_case_image(hn, wn, 300 + 7 * i + sum(map(ord, case))) for i in range(n + 2)])


@functools.lru_cache(maxsize=None)
def reference(case, flip, jitter):
    _, _, h, w, n, S, _ = CASES[case]
    return R.sequence_item(native_frames(case), h, w, S, flip, make_jitters(n, S) if jitter else None)


def run(case, flip, jitter, budget=0):
    from depthcore.data import GpuPreprocessor
    _, _, h, w, n, S, _ = CASES[case]
    pre = GpuPreprocessor(h, w, num_scales=S, device=_dev())
    pre.seq_lds_budget = budget
    out = pre.sequence(torch.from_numpy(native_frames(case)).to(_dev()), flip, make_jitters(n, S) if jitter else None)
    return pre, out


def check_against(out, want, n, S, h, w, tag):
    assert set(out) == {(name, f, s) for name in ("color", "color_aug") for f in (0, -1, 1) for s in range(S)} | \
        {("color_packed", f, 0) for f in (0, -1, 1)}
    for f in (0, -1, 1):
        for s in range(S):
            got = out[("color", f, s)]
            assert got.shape == (n, 3, h >> s, w >> s) and got.dtype == torch.float32 and got.is_contiguous()
            assert out[("color_aug", f, s)] is got
            got = got.cpu().numpy()
            assert np.array_equal(got, want[("color", f, s)]), (tag, f, s, int((got != want[("color", f, s)]).sum()))
        pk = out[("color_packed", f, 0)]
        assert pk.shape == (n, h, w, 4) and pk.is_contiguous() and pk.data_ptr() % 16 == 0
        assert np.array_equal(pk.cpu().numpy(), want[("color_packed", f, 0)]), (tag, f, "packed")


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("case", sorted(CASES))
def test_sequence_equals_the_chain(case, flip, jitter):
    _, _, h, w, n, S, tail = CASES[case]
    pre, out = run(case, flip, jitter)
    plan = pre.sequence_plan(n, jitter)
    assert plan.tail_start == tail and plan.n_img == (3 * n if jitter else n + 2)
    check_against(out, reference(case, flip, jitter), n, S, h, w, (case, flip, jitter))


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("case,tail", [("B", 1), ("C", 2)])
def test_training_sizes_with_the_tail_on_the_whole_lds(case, tail, flip, jitter):
    """The budget raised to the hardware's: at 192 x 640 level 0 goes through HBM and the tail starts at level 1; at 320 x 1024
    level 1 does not fit either."""
    _, _, h, w, n, S, _ = CASES[case]
    pre, out = run(case, flip, jitter, LDS_CAP)
    assert pre.sequence_plan(n, jitter).tail_start == tail
    check_against(out, reference(case, flip, jitter), n, S, h, w, (case, flip, jitter, "tail"))


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("tail", [0, 1, 2, 3, 4])
def test_any_split_gives_the_same_bits(tail, jitter):
    """Case A with the LDS budget set so that the tail starts at `tail` (4: no level fits, every level goes through HBM)."""
    from depthcore.data import GpuPreprocessor
    _, _, h, w, n, S, _ = CASES["A"]
    pre = GpuPreprocessor(h, w, num_scales=S, device=_dev())
    budget = {}
    for b in range(64, 16384, 64):                      # the smallest budgets at which each start level fits
        pre.seq_lds_budget = b
        budget.setdefault(pre.sequence_plan(n, jitter).tail_start, b)
    assert sorted(budget) == [0, 1, 2, 3, 4]
    _, out = run("A", True, jitter, budget[tail])
    check_against(out, reference("A", True, jitter), n, S, h, w, ("A", tail, jitter))


def compose(native, h, w, S, flip, jitters):
    """The same item from the entry points that existed before dc_data_seq_levels, level after level, per image."""
    from depthcore import _lib
    from depthcore.data import HUE, GpuPreprocessor, hue_shift
    L, dev = _lib.lib(), native.device
    n = native.shape[0] - 2
    pre = GpuPreprocessor(h, w, num_scales=S, device=dev)
    frames = [1 + j for j in range(n)] + list(range(n)) + [2 + j for j in range(n)] if jitters is not None else list(range(n + 2))
    img = native[frames].contiguous()
    N = img.shape[0]
    ones = torch.ones(N, dtype=torch.uint8, device=dev)
    sums = torch.zeros(N, dtype=torch.int64, device=dev)
    color, packed = [], None
    for s in range(S):
        img = pre._resize(img, h >> s, w >> s, None)                                       # dc_data_resize_axis x 2
        if flip:
            dst = torch.empty_like(img)
            _lib.check(L.dc_data_flip(img.data_ptr(), dst.data_ptr(), N, h >> s, w >> s, ones.data_ptr(), _lib.stream(img)), "flip")
            img = dst
        if jitters is not None:
            st = np.zeros((N, 4), np.int32)
            pr = np.zeros((N, 4), np.float32)
            for i in range(N):
                order, factors = jitters[i // n][i % n][s]
                for k, op in enumerate(order):
                    st[i, k], pr[i, k] = op, float(hue_shift(factors[op])) if op == HUE else factors[op]
            img = img.clone()
            st_d, pr_d = torch.from_numpy(st).to(dev), torch.from_numpy(pr).to(dev)
            _lib.check(L.dc_data_jitter(img.data_ptr(), N, (h >> s) * (w >> s), st_d.data_ptr(), pr_d.data_ptr(), sums.data_ptr(),
                                        _lib.stream(img)), "jitter")
        color.append(pre._to_tensor(img))
        if s == 0:
            packed = torch.empty((N, h, w, 4), dtype=torch.float32, device=dev)
            _lib.check(L.dc_data_to_rgbx(img.data_ptr(), packed.data_ptr(), N, h * w, _lib.stream(img)), "rgbx")
    return color, packed


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("case", sorted(CASES))
def test_sequence_equals_the_composition_of_existing_entry_points(case, jitter):
    _, _, h, w, n, S, _ = CASES[case]
    jit = make_jitters(n, S) if jitter else None
    _, out = run(case, True, jitter)
    color, packed = compose(torch.from_numpy(native_frames(case)).to(_dev()), h, w, S, True, jit)
    for wi, (first, f) in enumerate(zip((1, 0, 2), (0, -1, 1))):
        lo = wi * n if jitter else first
        for s in range(S):
            assert torch.equal(out[("color", f, s)], color[s][lo:lo + n]), (case, f, s)
        assert torch.equal(out[("color_packed", f, 0)], packed[lo:lo + n]), (case, f)


@pytest.mark.parametrize("case", ["A", "B"])
def test_unjittered_windows_are_slices_of_one_pyramid(case):
    _, _, h, w, n, S, _ = CASES[case]
    _, out = run(case, False, False)
    for s in range(S):
        frame = 3 * (h >> s) * (w >> s) * 4
        c = out[("color", 0, s)]
        assert out[("color", -1, s)].data_ptr() == c.data_ptr() - frame and out[("color", 1, s)].data_ptr() == c.data_ptr() + frame
        assert c.untyped_storage().data_ptr() == out[("color", -1, s)].untyped_storage().data_ptr() == out[("color", 1, s)].untyped_storage().data_ptr()
        for f in (0, -1, 1):
            assert out[("color_aug", f, s)] is out[("color", f, s)]
        # the centre's frame j is the left window's frame j + 1 and the right window's frame j - 1: the same memory
        if n > 1:
            assert out[("color", 0, s)][0].data_ptr() == out[("color", -1, s)][1].data_ptr() == out[("color", 1, s)][0].data_ptr() - frame
    pk = out[("color_packed", 0, 0)]
    assert out[("color_packed", -1, 0)].data_ptr() == pk.data_ptr() - h * w * 16 and out[("color_packed", 1, 0)].data_ptr() == pk.data_ptr() + h * w * 16


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("case", ["A", "B"])
def test_two_calls_give_the_same_bits(case, jitter):
    _, a = run(case, True, jitter)
    _, b = run(case, True, jitter)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_bad_items_are_refused():
    from depthcore import _lib
    from depthcore.data import GpuPreprocessor
    pre = GpuPreprocessor(32, 96, device=_dev())
    frames = torch.zeros((5, 32, 96, 3), dtype=torch.uint8, device=_dev())
    with pytest.raises(_lib.DepthcoreError):
        pre.sequence(frames[:2])                                     # n = 0
    with pytest.raises(_lib.DepthcoreError):
        pre.sequence(frames.float())
    with pytest.raises(_lib.DepthcoreError):
        pre.sequence(frames, jitters=make_jitters(2, 4))             # jitters of another n
