"""The datasets/ package on a tmp tree of PIL-written PNGs: paths, line parsing, missing-neighbour substitution, K,
stereo_T, the depth benchmark's ground truth.  No GPU."""
import os

import numpy as np
import pytest
from PIL import Image

from kitti_tree import DRIVES, write_raw_tree

DRIVE_A, DRIVE_B = sorted(DRIVES)


def test_image_path_formats():
    import datasets
    raw = datasets.KITTIRAWDataset("/d", ["%s 7 l" % DRIVE_A], 32, 64, [0, -1, 1], 4, img_ext=".jpg")
    assert raw.get_image_path(DRIVE_A, 7, "l") == "/d/%s/image_02/data/0000000007.jpg" % DRIVE_A
    assert raw.get_image_path(DRIVE_A, 123, "r") == "/d/%s/image_03/data/0000000123.jpg" % DRIVE_A
    assert raw.get_image_path(DRIVE_A, 7, "3") == "/d/%s/image_03/data/0000000007.jpg" % DRIVE_A
    odom = datasets.KITTIOdomDataset("/d", ["9 7 l"], 32, 64, [0, -1, 1], 4, img_ext=".png")
    assert odom.get_image_path("9", 7, "l") == "/d/sequences/09/image_2/000007.png"
    assert odom.get_image_path("10", 1234, "r") == "/d/sequences/10/image_3/001234.png"
    dep = datasets.KITTIDepthDataset("/d", ["%s 7 r" % DRIVE_A], 32, 64, [0], 4, img_ext=".png")
    assert dep.get_image_path(DRIVE_A, 7, "r") == "/d/%s/image_03/data/0000000007.png" % DRIVE_A
    assert dep.depth_path(DRIVE_A, 7, "r") == "/d/%s/proj_depth/groundtruth/image_03/0000000007.png" % DRIVE_A
    for ds in (raw, odom, dep):
        assert ds.side_map == {"2": 2, "3": 3, "l": 2, "r": 3} and ds.full_res_shape == (1242, 375)
        assert isinstance(ds, datasets.KITTIDataset) and isinstance(ds, datasets.MonoDataset)


def test_line_parsing():
    from datasets import parse_line
    assert parse_line("a/b 12 r") == ("a/b", 12, "r")
    assert parse_line("a/b    0003   l\n") == ("a/b", 3, "l")
    assert parse_line("only_a_folder") == ("only_a_folder", 0, None)      # one token: frame 0, no side
    assert parse_line("a/b 5") == ("a/b", 0, None)                         # anything but three tokens, as the reference


def test_normalised_intrinsics():
    import datasets
    ds = datasets.KITTIRAWDataset("/d", ["x 0 l"], 32, 64, [0], 4)
    want = np.array([[0.58, 0, 0.5, 0], [0, 1.92, 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
    assert ds.K.dtype == np.float32 and np.array_equal(ds.K, want)
    assert ds.check_depth() is False and ds.load_depth is False


def test_items_and_missing_neighbours(tmp_path):
    """Frame 0 of a drive has no frame -1, the last one no frame +1: frame 0 of the item stands in; frames come back as
    decoded, unflipped uint8 arrays."""
    import datasets
    px = write_raw_tree(str(tmp_path), frames=4)
    lines = ["%s 0 l" % DRIVE_A, "%s 2 l" % DRIVE_B, "%s 3 l" % DRIVE_B]
    ds = datasets.KITTIRAWDataset(str(tmp_path), lines, 32, 64, [0, -1, 1], 4, is_train=True, img_ext=".png")
    assert len(ds) == 3
    first, mid, last = ds[0], ds[1], ds.get_item(2, do_flip=True)
    assert sorted(first, key=str) == sorted([("color", 0, -1), ("color", -1, -1), ("color", 1, -1)], key=str)
    assert np.array_equal(first[("color", -1, -1)], px[(DRIVE_A, 0, "l")])             # substituted
    assert np.array_equal(first[("color", 0, -1)], px[(DRIVE_A, 0, "l")])
    assert np.array_equal(first[("color", 1, -1)], px[(DRIVE_A, 1, "l")])
    for f in (-1, 0, 1):
        assert np.array_equal(mid[("color", f, -1)], px[(DRIVE_B, 2 + f, "l")])
        assert mid[("color", f, -1)].dtype == np.uint8 and mid[("color", f, -1)].shape == DRIVES[DRIVE_B] + (3,)
    assert np.array_equal(last[("color", 1, -1)], px[(DRIVE_B, 3, "l")])                # substituted, and not mirrored
    assert np.array_equal(last[("color", -1, -1)], px[(DRIVE_B, 2, "l")])
    paths = ds.frame_paths(0)
    assert paths[1] == paths[0] and paths[2].endswith("0000000001.png")


@pytest.mark.parametrize("side,flip,sign", [("l", False, -1), ("l", True, 1), ("r", False, 1), ("r", True, -1)])
def test_stereo_frame_and_stereo_T(tmp_path, side, flip, sign):
    import datasets
    px = write_raw_tree(str(tmp_path), frames=2, sides=("l", "r"))
    ds = datasets.KITTIRAWDataset(str(tmp_path), ["%s 1 %s" % (DRIVE_A, side)], 32, 64, [0, "s"], 4, is_train=True, img_ext=".png")
    item = ds.get_item(0, do_flip=flip)
    other = {"l": "r", "r": "l"}[side]
    assert np.array_equal(item[("color", 0, -1)], px[(DRIVE_A, 1, side)])
    assert np.array_equal(item[("color", "s", -1)], px[(DRIVE_A, 1, other)])
    want = np.eye(4, dtype=np.float32)
    want[0, 3] = sign * 0.1
    assert item["stereo_T"].dtype == np.float32 and np.array_equal(item["stereo_T"], want)
    assert "depth_gt" not in item


def test_depth_dataset_ground_truth(tmp_path):
    """uint16 PNG in 1/256 m -> NEAREST resize to full_res_shape, / 256, mirrored with the flip."""
    import datasets
    write_raw_tree(str(tmp_path), frames=2)
    h, w = DRIVES[DRIVE_A]
    rng = np.random.RandomState(3)
    gt = (rng.randint(0, 80 * 256, (h, w)) * (rng.rand(h, w) < 0.3)).astype(np.uint16)
    folder = tmp_path / DRIVE_A / "proj_depth" / "groundtruth" / "image_02"
    os.makedirs(folder)
    Image.fromarray(gt).save(str(folder / "0000000001.png"))
    ds = datasets.KITTIDepthDataset(str(tmp_path), ["%s 1 l" % DRIVE_A], 32, 64, [0, -1, 1], 4, img_ext=".png")
    assert ds.check_depth() is True and ds.load_depth
    want = np.array(Image.fromarray(gt).resize((1242, 375), Image.NEAREST)).astype(np.float32) / 256
    for flip in (False, True):
        got = ds.get_item(0, do_flip=flip)["depth_gt"]
        assert got.dtype == np.float32 and got.shape == (1, 375, 1242)
        assert np.array_equal(got[0], want[:, ::-1] if flip else want)
    assert want.max() > 1 and (want == 0).mean() > 0.5
    # no ground-truth file for the first line: the dataset carries no depth
    assert datasets.KITTIDepthDataset(str(tmp_path), ["%s 0 l" % DRIVE_A], 32, 64, [0], 4, img_ext=".png").load_depth is False
