"""The evaluation restatements of tests/eval_ref.py against the reference's own results (tests/golden/depth_eval.npz, written by
tests/golden/make_golden_eval.py), and the drop-in evaluate_depth.py's options (no GPU needed)."""
import os
import sys

import numpy as np
import pytest

import eval_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_eval.npz")
CASES = {"mono_eigen": ("eigen", True, 1.0), "stereo_eigen": ("eigen", False, 5.4), "mono_benchmark": ("eigen_benchmark", True, 1.0)}


def _fixture():
    z = np.load(GOLDEN, allow_pickle=False)
    shapes = [tuple(int(v) for v in s) for s in z["gt_shapes"]]
    flat = np.zeros(sum(a * b for a, b in shapes), np.float32)
    flat[z["gt_idx"]] = z["gt_val"]
    gts, off = [], 0
    for a, b in shapes:
        gts.append(flat[off:off + a * b].reshape(a, b))
        off += a * b
    return z, gts


def test_fixture_loads_without_pickle_and_is_small():
    z, gts = _fixture()
    assert os.path.getsize(GOLDEN) < 100 * 1024
    assert len({g.shape for g in gts}) == 2
    assert z["post"].dtype == np.float64 and z["left"].dtype == np.float32


def test_post_process_restatement_matches_reference():
    z, _ = _fixture()
    got = R.post_process64(z["left"], z["right"][:, :, ::-1])
    assert got.dtype == np.float64
    assert got.tobytes() == z["post"].tobytes()


@pytest.mark.parametrize("w", [1, 2, 3, 40])
def test_post_process_masks_edge_widths(w):
    l = np.full((1, 2, w), 1.0, np.float32)
    r = np.full((1, 2, w), 3.0, np.float32)
    got = R.post_process64(l, r)
    # the left 5 % of the columns take the right image, the right 5 % the left one, the middle their mean
    assert got[0, 0, 0] == (3.0 if w > 1 else 2.0)          # w == 1: both masks are 1, 1 + 3 - 2
    if w >= 3:
        assert got[0, 0, -1] == 1.0 and got[0, 0, w // 2] == 2.0


@pytest.mark.parametrize("case", sorted(CASES))
def test_evaluate_restatement_matches_reference(case):
    z, gts = _fixture()
    split, scaling, sf = CASES[case]
    got = R.evaluate_loop(z["left"], gts, split, scaling, sf)
    assert got["errors"].tobytes() == z[case + "_errors"].tobytes()
    assert got["mean_errors"].tobytes() == z[case + "_mean"].tobytes()
    if scaling:
        assert got["ratios"].astype(np.float32).tobytes() == z[case + "_ratios"].tobytes()
        assert np.float64(got["ratio_median"]) == z[case + "_med"]
        assert np.float64(got["ratio_std"]) == z[case + "_std"]
    else:
        assert got["ratios"] is None and case + "_ratios" not in z.files


def test_two_masks_differ_on_the_fixture():
    z, gts = _fixture()
    eig = R.evaluate_loop(z["left"], gts, "eigen")["n"]
    pos = R.evaluate_loop(z["left"], gts, "eigen_benchmark")["n"]
    assert (pos > eig).all()


def _drop_in():
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "self-supervised-depth-estimation_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    import evaluate_depth
    return evaluate_depth


def test_drop_in_options():
    from options import MonodepthOptions, reference_option_names
    ED = _drop_in()
    opt = MonodepthOptions().parse(["--eval_mono", "--post_process", "--eval_split", "eigen_benchmark", "--splits_dir", "/s",
                                    "--eval_json", "/o.json", "--load_weights_folder", "/w"])
    assert opt.eval_mono and opt.post_process and opt.eval_split == "eigen_benchmark"
    assert opt.splits_dir == "/s" and opt.eval_json == "/o.json"
    default = MonodepthOptions().parse([])
    assert default.splits_dir == os.path.join(os.path.dirname(os.path.abspath(ED.__file__)), "splits")
    assert default.eval_json is None
    assert "splits_dir" not in reference_option_names() and "eval_json" not in reference_option_names()
    assert ED.image_path("/d", "2011_09_26/2011_09_26_drive_0002_sync 69 l") == \
        "/d/2011_09_26/2011_09_26_drive_0002_sync/image_02/data/0000000069.jpg"
    assert ED.image_path("/d", "x 3 r", ".png") == "/d/x/image_03/data/0000000003.png"


@pytest.mark.parametrize("split", ["odom_9", "odom_10"])
def test_drop_in_refuses_odometry(split):
    from options import MonodepthOptions
    ED = _drop_in()
    opt = MonodepthOptions().parse(["--eval_mono", "--eval_split", split])
    with pytest.raises(ValueError, match="pose"):
        ED.evaluate(opt)


def test_drop_in_refuses_sequence_front_ends():
    from options import MonodepthOptions
    ED = _drop_in()
    for flag, name in ((["--fusion", "v3"], "Fusion_v3"), (["--gru", "v5"], "ConvGRU")):
        opt = MonodepthOptions().parse(["--eval_mono"] + flag)
        with pytest.raises(NotImplementedError, match=name):
            ED.evaluate(opt)


def test_evaluate_depth_refuses_odometry():
    from depthcore import evaluate as E
    with pytest.raises(ValueError, match="pose"):
        E.evaluate_depth(np.zeros((1, 1, 4, 4), np.float32), [np.zeros((4, 4), np.float32)], "odom_9")
