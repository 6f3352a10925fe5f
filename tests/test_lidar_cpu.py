"""Velodyne depth maps without a GPU: the host path of depthcore/lidar.py and the loop restatement (lidar_ref) against the
maps the reference's generate_depth_map gave (tests/golden/lidar.npz), the calibration parser, KITTIRAWDataset's check_depth /
get_depth, the loader's host half, and export_gt_depth.py."""
import os

import numpy as np
import pytest
from PIL import Image

import lidar_ref
from kitti_tree import DRIVES, write_raw_tree
from lidar_tree import calibration, write_calibration, write_scans

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = {"a": (33, 17, 3001), "b": (64, 24, 6000), "c": (40, 20, 1)}
CASES = [(n, cam, vel) for n in "abc" for cam in (2, 3) for vel in (False, True)]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "lidar.npz"))


def fixture_calib(golden, name):
    return {k: golden["%s_%s" % (name, k)] for k in ("S_rect_02", "P_rect_02", "P_rect_03", "R_rect_00", "R", "T")}


def test_golden_fixtures_are_what_the_tests_assume(golden):
    for name, (W, H, n) in FIXTURES.items():
        pts = golden[name + "_points"]
        assert pts.shape == (n, 4) and pts.dtype == np.float32
        assert tuple(golden[name + "_S_rect_02"]) == (W, H)
        if n > 1:
            assert (pts[:, 0] < 0).any() and (pts[:, 0] == 0).any()
        for cam in (2, 3):
            assert golden["%s_map_cam%d_vel0" % (name, cam)].shape == (H, W)


@pytest.mark.parametrize("name,cam,vel", CASES)
def test_restatement_and_host_path_equal_the_reference_maps(golden, name, cam, vel):
    from depthcore import lidar
    W, H, _ = FIXTURES[name]
    P = lidar_ref.projection_matrix(fixture_calib(golden, name), cam)
    want = golden["%s_map_cam%d_vel%d" % (name, cam, vel)]
    assert want.dtype == np.float32
    got_ref = lidar_ref.depth_map(golden[name + "_points"], P, (W, H), vel)
    got = lidar.depth_map_host(golden[name + "_points"], P, (W, H), vel)
    assert got.dtype == np.float32 and got.shape == (H, W)
    assert np.array_equal(got_ref, want)
    assert np.array_equal(got, want)


def test_edge_rule_matters_in_the_fixtures(golden):
    """A per-pixel minimum alone differs from the reference in columns 0 and W-1, and nowhere else."""
    for name in "ab":
        W, H, _ = FIXTURES[name]
        P = lidar_ref.projection_matrix(fixture_calib(golden, name), 2)
        pts = golden[name + "_points"]
        pts = pts[pts[:, 0] >= 0].astype(np.float64)
        q = np.stack([((P[r, 0] * pts[:, 0] + P[r, 1] * pts[:, 1]) + P[r, 2] * pts[:, 2]) + P[r, 3] for r in range(3)], 1)
        px, py = np.rint(q[:, 0] / q[:, 2]) - 1, np.rint(q[:, 1] / q[:, 2]) - 1
        ok = (px >= 0) & (py >= 0) & (px < W) & (py < H)
        plain = np.full(W * H, np.inf, np.float32)
        np.minimum.at(plain, (py[ok] * W + px[ok]).astype(int), pts[ok, 0].astype(np.float32))
        plain = np.where(np.isinf(plain), 0, plain).reshape(H, W)
        diff = plain != golden["%s_map_cam2_vel1" % name]
        assert diff.any() and not diff[:, 1:W - 1].any()


def test_calibration_parser_and_projection_matrix(tmp_path, golden):
    from depthcore import lidar
    calib = fixture_calib(golden, "a")
    write_calibration(str(tmp_path), calib)
    parsed = lidar.read_calib(str(tmp_path / "calib_cam_to_cam.txt"))
    assert parsed["calib_time"] == "09-Jan-2012 13:57:47"                       # not numeric: stays a string
    assert parsed["corner_dist"].shape == (1,) and parsed["corner_dist"][0] == 9.95e-2
    assert parsed["P_rect_03"].dtype == np.float64 and np.array_equal(parsed["P_rect_03"], calib["P_rect_03"])
    for cam in (2, 3):
        P, size = lidar.velo_to_image(str(tmp_path), cam)
        assert size == (33, 17) and P.shape == (3, 4) and P.dtype == np.float64
        assert np.array_equal(P, lidar_ref.projection_matrix(calib, cam))
    assert lidar.velo_to_image(str(tmp_path), 2)[0] is lidar.velo_to_image(str(tmp_path), 2)[0]     # cached
    assert not np.array_equal(lidar.velo_to_image(str(tmp_path), 2)[0], lidar.velo_to_image(str(tmp_path), 3)[0])


def test_generate_depth_map_has_the_reference_signature_and_values(tmp_path, golden):
    from depthcore import lidar
    write_calibration(str(tmp_path), fixture_calib(golden, "b"))
    golden["b_points"].tofile(str(tmp_path / "scan.bin"))
    for cam, vel in ((2, False), (3, True)):
        got = lidar.generate_depth_map(str(tmp_path), str(tmp_path / "scan.bin"), cam, vel)
        assert got.dtype == np.float64 and got.shape == (24, 64)
        assert np.array_equal(got.astype(np.float32), golden["b_map_cam%d_vel%d" % (cam, vel)])
        assert np.array_equal(got.astype(np.float32).astype(np.float64), got)


def test_nearest_tables_are_pillows(golden):
    from depthcore import lidar
    for native, out in (((33, 17), (40, 20)), ((64, 24), (40, 20)), ((1224, 370), (1242, 375)), ((155, 47), (1242, 375))):
        rows, cols = lidar.nearest_tables(native, out)
        assert rows.dtype == cols.dtype == np.int32 and rows.shape == (out[1],) and cols.shape == (out[0],)
        img = np.random.RandomState(0).rand(native[1], native[0]).astype(np.float32)
        assert np.array_equal(img[rows][:, cols], lidar_ref.resize_flip(img, (out[1], out[0])))
    rows, cols = lidar.nearest_tables((1242, 375), (1242, 375))
    assert np.array_equal(rows, np.arange(375)) and np.array_equal(cols, np.arange(1242))
    assert lidar.nearest_tables((1224, 370), (1242, 375))[1][34] == 34 and lidar.nearest_tables((1224, 370), (1242, 375))[1][35] == 34


def test_layout_workspace_query_and_host_side_refusals():
    """sizeof(dc_lidar_img) as gcc sees it; the workspace query; DC_EINVAL for every bad argument before anything could be
    launched (the device pointers here are made-up addresses: a launch would fault, a refusal never touches them)."""
    import subprocess
    import tempfile
    import lidar_abi
    from depthcore import _lib
    from depthcore.lidar import LIDAR_IMG
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "sz.c"), "w") as f:
            f.write('#include <stdio.h>\n#include <stddef.h>\n#include "depthcore.h"\nint main(){printf("%zu %zu %zu\\n",'
                    'sizeof(dc_lidar_img), offsetof(dc_lidar_img, flip), offsetof(dc_lidar_img, P));return 0;}\n')
        subprocess.check_call(["gcc", "-I", os.path.join(os.path.dirname(HERE), "include"), os.path.join(tmp, "sz.c"), "-o",
                               os.path.join(tmp, "sz")])
        got = [int(x) for x in subprocess.check_output([os.path.join(tmp, "sz")]).split()]
    assert got == [LIDAR_IMG.itemsize, LIDAR_IMG.fields["flip"][1], LIDAR_IMG.fields["P"][1]] == [128, 24, 32]
    L = _lib.lib()
    # key planes (4 bytes a pixel, rounded to 8 per image) + two 8-byte side planes of 2 * max_h entries per image
    assert L.dc_lidar_workspace_bytes(3, 33, 17) == 3 * (8 * ((33 * 17 + 1) // 2) + 2 * 2 * 17 * 8)
    assert L.dc_lidar_workspace_bytes(12, 1242, 376) == 12 * (1242 * 376 * 4 + 2 * 2 * 376 * 8)
    assert L.dc_lidar_workspace_bytes(0, 33, 17) == 0 and L.dc_lidar_workspace_bytes(1, 1, 17) == 0 and L.dc_lidar_workspace_bytes(1, 33, 0) == 0
    fake = 0x7f0000000000
    for what in lidar_abi.BAD_ARGUMENTS:
        args = lidar_abi.arguments([5, 7], [(33, 17), (40, 20)], (20, 40))
        null = lidar_abi.spoil(args, what)
        assert lidar_abi.call(L, args, fake, fake, fake, fake, fake, fake, 1 << 20, null=null) == -1, what
    args = lidar_abi.arguments([5, 7], [(33, 17), (40, 20)], (20, 40))
    assert lidar_abi.call(L, args, fake + 4, fake, fake, fake, fake, fake, 1 << 20) == -1          # points not 16-byte aligned
    assert lidar_abi.call(L, args, fake, fake, fake, fake, fake, fake, 64) == -3                   # DC_EWORKSPACE


@pytest.fixture(scope="module")
def raw_tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kitti_scans"))
    write_raw_tree(root, frames=3, sides=("l", "r"))
    return root, write_scans(root, frames=3)


def test_check_depth_follows_the_first_lines_scan(raw_tree, tmp_path):
    import datasets
    root, _ = raw_tree
    drive = sorted(DRIVES)[0]
    assert datasets.KITTIRAWDataset.device_depth is True and datasets.KITTIDepthDataset.device_depth is False
    assert datasets.KITTIRAWDataset(root, ["%s 1 l" % drive], 32, 64, [0], 4, img_ext=".png").load_depth is True
    assert datasets.KITTIRAWDataset(root, ["%s 9 l" % drive], 32, 64, [0], 4, img_ext=".png").load_depth is False      # no such scan
    assert datasets.KITTIRAWDataset(root, [drive], 32, 64, [0], 4, img_ext=".png").load_depth is False                 # no side
    write_raw_tree(str(tmp_path), frames=2)
    assert datasets.KITTIRAWDataset(str(tmp_path), ["%s 1 l" % drive], 32, 64, [0], 4, img_ext=".png").load_depth is False


@pytest.mark.parametrize("side,flip", [("l", False), ("r", True)])
def test_get_depth_is_restatement_plus_pillow_nearest_plus_flip(raw_tree, side, flip):
    import datasets
    root, scans = raw_tree
    drive = sorted(DRIVES)[1]
    h, w = DRIVES[drive]
    ds = datasets.KITTIRAWDataset(root, ["%s 2 %s" % (drive, side)], 32, 64, [0], 4, img_ext=".png")
    path, calib_dir, cam = ds.depth_source(0)
    assert cam == {"l": 2, "r": 3}[side] and calib_dir == os.path.join(root, drive.split("/")[0])
    assert np.array_equal(np.fromfile(path, np.float32).reshape(-1, 4), scans[(drive, 2)])
    # drive index 1 of the sorted tree; the numbers as the calibration files hold them ("%e")
    P = lidar_ref.projection_matrix({k: np.array([float("%e" % x) for x in v]) for k, v in calibration(w, h, 1).items()}, cam)
    want = lidar_ref.resize_flip(lidar_ref.depth_map(scans[(drive, 2)], P, (w, h)), (375, 1242), flip)
    got = ds.get_depth(drive, 2, side, flip)
    assert got.shape == (375, 1242) and got.dtype == np.float32 and np.count_nonzero(got) > 375 * 1242 // 10
    assert np.array_equal(got, want)
    item = ds.get_item(0, do_flip=flip)
    assert item["depth_gt"].shape == (1, 375, 1242) and np.array_equal(item["depth_gt"][0], want)
    assert "depth_gt" not in ds.metadata(0, flip, device_depth=True) and "depth_gt" in ds.metadata(0, flip)


def test_decode_batch_returns_depth_gt_and_the_frames_only(raw_tree):
    import datasets
    from depthcore.loader import BatchLoader
    root, _ = raw_tree
    lines = ["%s %d l" % (d, i) for d in sorted(DRIVES) for i in range(3)]
    ds = datasets.KITTIRAWDataset(root, lines, 32, 64, [0, -1, 1], 4, is_train=True, img_ext=".png")
    ld = BatchLoader(ds, 2, num_workers=2, device="cpu")
    buf, sizes, flips, _, extras = ld.decode_batch([1, 4], [(True, None), (False, None)])
    assert buf.size == 3 * sum(h * w * 3 for h, w in sizes)                      # no scan bytes: those are the device path's
    assert extras["depth_gt"].shape == (2, 1, 375, 1242) and extras["depth_gt"].dtype == np.float32
    for b, (i, flip) in enumerate(((1, True), (4, False))):
        folder, frame, side = datasets.parse_line(lines[i])
        assert np.array_equal(extras["depth_gt"][b, 0], ds.get_depth(folder, frame, side, flip))
    # the device path's job: the scans behind the frames from a 16-byte boundary, no host-built depth_gt
    job = ld._submit([1, 4], [(True, None), (False, None)], lambda n: np.zeros(n, np.uint8))
    for f in job["futures"]:
        f.result()
    sc = job["scans"]
    assert sc["off"] % 16 == 0 and 0 <= sc["off"] - job["frame_bytes"] < 16 and sc["end"] % 16 == 0 and job["buf"].size == sc["total"]
    desc = sc["desc"]
    assert np.array_equal(job["buf"][sc["end"]:], desc.host) and (desc.Ho, desc.Wo) == (375, 1242)
    assert list(desc.desc["flip"]) == [1, 0] and list(desc.desc["vel_depth"]) == [0, 0]
    assert list(zip(desc.desc["W"], desc.desc["H"])) == [DRIVES[lines[i].split()[0]][::-1] for i in (1, 4)]
    got = job["buf"][sc["off"]:sc["end"]].view(np.float32).reshape(-1, 4)
    assert list(desc.desc["n_points"]) == [len(np.fromfile(ds.depth_source(i)[0], np.float32)) // 4 for i in (1, 4)]
    assert np.array_equal(got, np.concatenate([np.fromfile(ds.depth_source(i)[0], np.float32).reshape(-1, 4) for i in (1, 4)]))
    assert all("depth_gt" not in m for m in job["meta"].result())
    ld.close()


def _export(root, splits, split, lines):
    import export_gt_depth
    os.makedirs(os.path.join(splits, split), exist_ok=True)
    with open(os.path.join(splits, split, "test_files.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    path = export_gt_depth.export_gt_depths_kitti(["--data_path", root, "--split", split, "--splits_dir", splits])
    assert path == os.path.join(splits, split, "gt_depths.npz")
    return np.load(path, fix_imports=True, encoding="latin1", allow_pickle=True)["data"]        # as evaluate_depth.py loads it


def test_export_eigen_two_native_sizes_is_an_object_array(raw_tree, tmp_path, capsys):
    root, scans = raw_tree
    drives = sorted(DRIVES)
    lines = ["%s %d %s" % (drives[i % 2], i // 2, "lr"[i % 2]) for i in range(6)]           # sizes alternate line by line
    data = _export(root, str(tmp_path), "eigen", lines)
    assert capsys.readouterr().out.splitlines()[:2] == ["Exporting ground truth depths for eigen", "Saving to eigen"]
    assert data.dtype == object and data.shape == (6,)
    for i, m in enumerate(data):
        drive = drives[i % 2]
        h, w = DRIVES[drive]
        calib = {k: np.array([float("%e" % x) for x in v]) for k, v in calibration(w, h, i % 2).items()}
        want = lidar_ref.depth_map(scans[(drive, i // 2)], lidar_ref.projection_matrix(calib, 2), (w, h), True)     # camera 2 always
        assert m.dtype == np.float32 and m.shape == (h, w) and np.array_equal(m, want)
    # what depthcore.evaluate.evaluate_depth does with gt_depths on its way in: len, per-map shape, float32 view
    assert len(data) == 6 and [tuple(np.shape(data[i]))[:2] for i in range(6)] == [DRIVES[drives[i % 2]] for i in range(6)]


def test_export_eigen_one_native_size_is_a_dense_array(raw_tree, tmp_path):
    root, _ = raw_tree
    drive = sorted(DRIVES)[0]
    data = _export(root, str(tmp_path), "eigen", ["%s %d l" % (drive, i) for i in range(3)])
    assert data.dtype == np.float32 and data.shape == (3,) + DRIVES[drive] and (data > 0).any()


def test_export_eigen_benchmark_reads_the_pngs(tmp_path):
    drive = sorted(DRIVES)[0]
    folder = tmp_path / "data" / drive / "proj_depth" / "groundtruth" / "image_02"
    os.makedirs(str(folder))
    rng = np.random.RandomState(5)
    maps = [rng.randint(0, 65536, (12, 20)).astype(np.uint16) for _ in range(2)]
    for i, m in enumerate(maps):
        Image.fromarray(m).save(str(folder / ("%010d.png" % i)))
    data = _export(str(tmp_path / "data"), str(tmp_path / "splits"), "eigen_benchmark", ["%s %d l" % (drive, i) for i in range(2)])
    assert data.dtype == np.float32 and data.shape == (2, 12, 20)
    assert np.array_equal(data, np.stack(maps).astype(np.float32) / 256)
