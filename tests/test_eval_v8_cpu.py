"""The ConvLSTM v8 evaluation without a GPU: the right-aligned lockstep schedule, a test file's window, what
evaluate_depth_gru.py accepts and refuses, and the new entry's place in the header and the binding table."""
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "self-supervised-depth-estimation_amd")
A = "2011_09_26/2011_09_26_drive_0002_sync"


def _script():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import evaluate_depth_gru as EG
    return EG


def _frames(lengths, ids, widths):
    """{window: [its frame index at every step it is alive]} of one group, as predict_disparities_windows forms frame_of."""
    L = len(widths)
    seen = {c: [] for c in ids}
    for j, B in enumerate(widths):
        for c in ids[:B]:
            seen[c].append(j - (L - lengths[c]))
    return seen


def test_window_groups_are_growing_prefixes():
    from depthcore import evaluate as E
    lengths = [2, 3, 1, 3, 2]
    groups = E.window_groups(lengths, 2)
    assert groups == [([1, 3], [2, 2, 2]), ([0, 4], [2, 2]), ([2], [1])]       # descending, stable, consecutive groups
    (ids, widths), = E.window_groups([3, 1, 2], 16)
    assert ids == [0, 2, 1] and widths == [1, 2, 3]                            # the shorter windows join later
    assert _frames([3, 1, 2], ids, widths) == {0: [0, 1, 2], 2: [0, 1], 1: [0]}
    for lens, streams in ((lengths, 2), ([3, 1, 2], 16), ([3, 1, 2], 1), ([7, 1, 7, 2, 5], 3)):
        for ids, widths in E.window_groups(lens, streams):
            assert len(ids) <= streams and widths == sorted(widths) and widths[-1] == len(ids)      # all alive at the last step
            assert len(widths) == lens[ids[0]] == max(lens[c] for c in ids)
            for c, fr in _frames(lens, ids, widths).items():
                assert fr == list(range(lens[c])), (c, fr)                     # every frame once, in order, the last one last
        assert sorted(c for ids, _ in E.window_groups(lens, streams) for c in ids) == list(range(len(lens)))
    for bad in (([1, 0], 2), ([1], 0)):
        with pytest.raises(ValueError):
            E.window_groups(*bad)


def test_window_paths_clip_at_the_first_frame():
    EG = _script()
    name = lambda i, cam=2, ext=".jpg": os.path.join("/d", A, "image_0%d/data" % cam, "%010d%s" % (i, ext))
    assert EG.N_PREV_IMAGES == 6
    assert EG.window_paths("/d", "%s 8 l" % A) == [name(i) for i in range(2, 9)]
    assert EG.window_paths("/d", "%s 6 l" % A) == [name(i) for i in range(0, 7)]
    assert EG.window_paths("/d", "%s 2 r" % A, ".png") == [name(i, 3, ".png") for i in range(0, 3)]      # clipped at frame 0
    assert EG.window_paths("/d", "%s 0 l" % A) == [name(0)]
    assert EG.window_paths("/d", "%s 5 l" % A, ".jpg", 0) == [name(5)]
    assert EG.window_paths("/d", "%s 5 l" % A, ".jpg", 2) == [name(3), name(4), name(5)]


def test_check_options():
    from options import MonodepthOptions
    EG = _script()
    assert tuple(EG.VERSIONS) == ("v5", "v8")

    def check(opt):                                                             # the check evaluate() makes
        EG.check_options(opt, tuple(EG.VERSIONS))
    opt = MonodepthOptions().parse(["--eval_mono", "--gru_version", "v8"])
    check(opt)
    check(MonodepthOptions().parse(["--eval_mono"]))
    assert opt.n_prev_images == 6
    for n in (0, 1, 2):                                                         # an int, also at the values a flag would take
        got = MonodepthOptions().parse(["--eval_mono", "--gru_version", "v8", "--n_prev_images", str(n)]).n_prev_images
        assert got == n and type(got) is int
    with pytest.raises(NotImplementedError, match="post_process"):
        check(MonodepthOptions().parse(["--eval_mono", "--gru_version", "v8", "--post_process"]))
    with pytest.raises(NotImplementedError, match="v5") as e:
        check(MonodepthOptions().parse(["--eval_mono", "--gru_version", "v4"]))
    assert "v8" in str(e.value)
    with pytest.raises(ValueError, match="pose"):
        check(MonodepthOptions().parse(["--eval_mono", "--gru_version", "v8", "--eval_split", "odom_9"]))
    # the script itself: v8 gets past the version check (the next refusal in line is --post_process'), v4 does not
    with pytest.raises(NotImplementedError, match="post_process"):
        EG.evaluate(MonodepthOptions().parse(["--eval_mono", "--gru_version", "v8", "--post_process"]))
    with pytest.raises(NotImplementedError, match="v5"):
        EG.evaluate(MonodepthOptions().parse(["--eval_mono", "--gru_version", "v4", "--post_process"]))
    # the one-argument form is the v5 evaluation's check, as before
    with pytest.raises(NotImplementedError, match="v5"):
        EG.check_options(opt)


def test_entry_is_declared_and_bound_with_matching_arity():
    from depthcore import _lib, ops, recurrent
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "depthcore.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+dc_lstm_infer_step\s*\(([^)]*)\)\s*;", src)
    assert m, "include/depthcore.h does not declare dc_lstm_infer_step"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 13 and params[7].startswith("size_t") and params[-1].startswith("void*")
    L = _lib.lib()
    res, args = _lib.EXPORTS["dc_lstm_infer_step"]
    assert len(args) == len(params) and hasattr(L, "dc_lstm_infer_step")
    assert ops.lstm_infer_step is recurrent.lstm_infer_step


def test_abi_refuses_before_any_launch():
    """The refusals that need no device memory: the entry validates before any HIP call (pointers are never dereferenced)."""
    from depthcore import _lib
    L = _lib.lib()
    p = 1 << 20                                                                # a non-NULL, 16-byte aligned address
    ok = dict(cc=p, y=p, r=p, h=p, c=p, pre=p, up=p, stride=8 * 2 * 4, B=2, C=8, hh=2, w=4)

    def call(**kw):
        a = dict(ok, **kw)
        return L.dc_lstm_infer_step(a["cc"], a["y"], a["r"], a["h"], a["c"], a["pre"], a["up"], a["stride"], a["B"], a["C"], a["hh"], a["w"], None)
    for kw in (dict(B=0), dict(C=0), dict(hh=0), dict(w=-1), dict(cc=None), dict(h=None), dict(c=None), dict(y=None), dict(r=None),
               dict(y=None, r=None), dict(y=None, r=None, up=None), dict(y=None, r=None, pre=None), dict(C=6), dict(stride=8 * 2 * 4 - 1),
               dict(B=1 << 9, C=1 << 8, hh=1 << 6, w=1 << 6, up=None)):               # 4 B C hh w = 2^31
        assert call(**kw) == -1, kw
