"""evaluate_depth_gru.py / evaluate_depth_fusion_v3.py without a GPU: the order in which the recurrent evaluation visits the
test files, the lockstep schedule, and what the scripts refuse."""
import collections
import os
import sys

import numpy as np
import pytest

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "self-supervised-depth-estimation_amd")
A, B = "2011_09_26/2011_09_26_drive_0002_sync", "2011_09_28/2011_09_28_drive_0001_sync"
# two scenes interleaved and shuffled; "100" sorts before "20" as a string, which the reference's sorted() does too
LINES = ["%s 20 l" % B, "%s 5 l" % A, "%s 100 l" % B, "%s 0000000069 l" % A, "%s 7 r" % B, "%s 12 l" % A, "%s 3 l" % A]


def _scripts():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import evaluate_depth as ED
    import evaluate_depth_fusion_v3 as EF
    import evaluate_depth_gru as EG
    return ED, EG, EF


def _reference_order(lines):
    """evaluate_depth_gru_fusion.py:728-731, :505, :514 restated."""
    test_files = collections.defaultdict(list)
    for img in lines:
        test_files[img.split()[0]].append(img)
    return [img for scene in sorted(test_files) for img in sorted(test_files[scene])]


def test_sequence_order_is_the_references_grouping():
    _, EG, _ = _scripts()
    order = EG.sequence_order(LINES)
    assert sorted(order.tolist()) == list(range(len(LINES)))                   # a permutation
    assert [LINES[i] for i in order] == _reference_order(LINES)
    assert [LINES[i] for i in order][:2] == ["%s 0000000069 l" % A, "%s 12 l" % A]
    gt_file = np.arange(len(LINES)) * 10
    gt_seq = gt_file[order]                                                    # what export_gt_depth_seq.py would have written
    inverse = np.argsort(order)
    assert np.array_equal(gt_seq[inverse], gt_file)
    scenes = EG.scenes_of(LINES)
    assert [s for s, _ in scenes] == [A, B] and [len(ids) for _, ids in scenes] == [4, 3]


def test_lockstep_groups_are_prefixes():
    from depthcore import evaluate as E
    groups = E.lockstep_groups([2, 3, 1, 3, 2], 2)
    assert groups == [([1, 3], [2, 2, 2]), ([0, 4], [2, 2]), ([2], [1])]       # descending, stable, consecutive groups
    (ids, widths), = E.lockstep_groups([2, 3, 1], 16)
    assert ids == [1, 0, 2] and widths == [3, 2, 1]
    for bad in (([1, 0], 2), ([1], 0)):
        with pytest.raises(ValueError):
            E.lockstep_groups(*bad)


def test_refusals():
    from options import MonodepthOptions
    ED, EG, EF = _scripts()
    with pytest.raises(NotImplementedError, match="post_process"):
        EG.evaluate(MonodepthOptions().parse(["--eval_mono", "--post_process"]))
    with pytest.raises(NotImplementedError, match="v5"):
        EG.evaluate(MonodepthOptions().parse(["--eval_mono", "--gru_version", "v4"]))
    for mod in (EG, EF):
        with pytest.raises(ValueError, match="pose"):
            mod.evaluate(MonodepthOptions().parse(["--eval_mono", "--eval_split", "odom_9"]))
    # the drop-in for the plain model keeps refusing both front-ends, and says where to go
    for flag, name, script in ((["--fusion", "v3"], "Fusion_v3", "evaluate_depth_fusion_v3.py"), (["--gru", "v5"], "ConvGRU", "evaluate_depth_gru.py")):
        with pytest.raises(NotImplementedError, match=name) as e:
            ED.evaluate(MonodepthOptions().parse(["--eval_mono"] + flag))
        assert script in str(e.value)


def test_triplet_paths_replace_missing_neighbours(tmp_path):
    _, _, EF = _scripts()
    d = tmp_path / A / "image_02" / "data"
    d.mkdir(parents=True)
    for i in (0, 1, 2):
        (d / ("%010d.jpg" % i)).write_bytes(b"")
    name = lambda i: str(d / ("%010d.jpg" % i))
    assert EF.triplet_paths(str(tmp_path), "%s 2 l" % A) == [name(0), name(1), name(2)]
    assert EF.triplet_paths(str(tmp_path), "%s 1 l" % A) == [name(1), name(0), name(1)]     # frame -1 does not exist
    assert EF.triplet_paths(str(tmp_path), "%s 0 l" % A) == [name(0), name(0), name(0)]
