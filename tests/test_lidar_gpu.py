"""ops.lidar_depth_maps / dc_lidar_depth_maps on the device: bitwise the maps the reference's generate_depth_map gave
(tests/golden/lidar.npz), batches with mixed native sizes, resize and flip against lidar_ref, the argument checks, and the
loader / Trainer.val / evaluate_depth paths that consume the maps."""
import os

import numpy as np
import pytest
import torch

import lidar_abi
import lidar_ref
from kitti_tree import write_raw_tree
from lidar_tree import calibration, scan, write_scans

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = {"a": (33, 17), "b": (64, 24), "c": (40, 20)}
TREE = {"2011_09_26/2011_09_26_drive_0001_sync": (70, 200), "2011_09_28/2011_09_28_drive_0002_sync": (66, 190)}     # (h, w)


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "lidar.npz"))
    out = {}
    for name in FIXTURES:
        calib = {k: g["%s_%s" % (name, k)] for k in ("P_rect_02", "P_rect_03", "R_rect_00", "R", "T")}
        out[name] = {"points": g[name + "_points"], "P": {cam: lidar_ref.projection_matrix(calib, cam) for cam in (2, 3)},
                     "maps": {(cam, vel): g["%s_map_cam%d_vel%d" % (name, cam, vel)] for cam in (2, 3) for vel in (0, 1)}}
    return out


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(got, want):
    """got: device tensor; want: numpy float32 of the same shape."""
    want = torch.from_numpy(np.ascontiguousarray(want, np.float32))
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == torch.float32
    assert torch.equal(_bits(got), want.view(torch.int32))


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_every_fixture_equals_the_reference_bitwise(golden, name):
    from depthcore import ops
    f = golden[name]
    W, H = FIXTURES[name]
    pts = torch.from_numpy(f["points"]).to(DEV)
    for (cam, vel), want in f["maps"].items():
        got = ops.lidar_depth_maps(pts, [len(f["points"])], f["P"][cam][None], [(W, H)], vel_depth=bool(vel))
        _same_bits(got, want[None, None])
        same = ops.lidar_depth_maps(pts, [len(f["points"])], f["P"][cam][None], [(W, H)], out_size=(H, W), vel_depth=bool(vel))
        _same_bits(same, want[None, None])


MIXED = (("a", 3, 1, True), ("b", 2, 0, False), ("c", 2, 1, True))        # fixture, camera, vel_depth, flip


@pytest.mark.parametrize("out_hw", [(17, 33), (20, 40), (375, 1242)])
def test_one_batch_of_mixed_sizes_cameras_depths_and_flips(golden, out_hw):
    """(20, 40) shrinks "b" (64 x 24) and enlarges "a" (33 x 17); (17, 33) is "a"'s native size."""
    from depthcore import ops
    pts = torch.from_numpy(np.concatenate([golden[n]["points"] for n, _, _, _ in MIXED])).to(DEV)
    got = ops.lidar_depth_maps(pts, [len(golden[n]["points"]) for n, _, _, _ in MIXED], np.stack([golden[n]["P"][c] for n, c, _, _ in MIXED]),
                               [FIXTURES[n] for n, _, _, _ in MIXED], out_size=out_hw, vel_depth=[bool(v) for _, _, v, _ in MIXED],
                               flips=[fl for _, _, _, fl in MIXED])
    want = np.stack([lidar_ref.resize_flip(golden[n]["maps"][(c, v)], out_hw, fl) for n, c, v, fl in MIXED])[:, None]
    _same_bits(got, want)


def test_out_size_none_needs_one_native_size(golden):
    from depthcore import ops
    pts = torch.from_numpy(np.concatenate([golden["a"]["points"], golden["b"]["points"]])).to(DEV)
    with pytest.raises(ops.DepthcoreError):
        ops.lidar_depth_maps(pts, [3001, 6000], np.stack([golden["a"]["P"][2], golden["b"]["P"][2]]), [(33, 17), (64, 24)])


def test_an_empty_scan_gives_zeros(golden):
    from depthcore import ops
    a = golden["a"]
    pts = torch.from_numpy(np.concatenate([a["points"], a["points"]])).to(DEV)
    got = ops.lidar_depth_maps(pts, [3001, 0, 3001], np.stack([a["P"][2]] * 3), [(33, 17)] * 3, vel_depth=[True, True, False])
    _same_bits(got[0:1], a["maps"][(2, 1)][None, None])
    assert torch.count_nonzero(got[1]) == 0
    _same_bits(got[2:3], a["maps"][(2, 0)][None, None])
    only = ops.lidar_depth_maps(torch.empty((0, 4), device=DEV), [0], a["P"][2][None], [(33, 17)])
    assert only.shape == (1, 1, 17, 33) and torch.count_nonzero(only) == 0


@pytest.fixture(scope="module")
def full_scan():
    """One scan of 120 001 points (no multiple of any block size) at 1242 x 375, and the restatement's maps, computed once."""
    calib = calibration(1242, 375, 3)
    pts = scan(calib, 1242, 375, 120001, 9)
    P = {cam: lidar_ref.projection_matrix(calib, cam) for cam in (2, 3)}
    return pts, P, {(2, False): lidar_ref.depth_map(pts, P[2], (1242, 375), False), (3, True): lidar_ref.depth_map(pts, P[3], (1242, 375), True)}


def test_a_full_size_scan_matches_the_restatement_and_repeats_bitwise(full_scan):
    from depthcore import ops
    pts, P, want = full_scan
    dev = torch.from_numpy(pts).to(DEV)
    for (cam, vel), w in want.items():
        assert np.count_nonzero(w) > 50000
        got = ops.lidar_depth_maps(dev, [len(pts)], P[cam][None], [(1242, 375)], vel_depth=vel)
        _same_bits(got, w[None, None])
        again = ops.lidar_depth_maps(dev, [len(pts)], P[cam][None], [(1242, 375)], vel_depth=vel)
        assert torch.equal(_bits(got), _bits(again))


def _device_arguments(args, points):
    L_bytes = np.concatenate([args["desc"].view(np.uint8), args["rows"].view(np.uint8).ravel(), args["cols"].view(np.uint8).ravel()])
    dev = torch.from_numpy(L_bytes).to(DEV)
    base, nd, nr = dev.data_ptr(), args["desc"].nbytes, args["rows"].nbytes
    return dev, (torch.from_numpy(points).to(DEV), base, base + nd, base + nd + nr)


def test_every_output_element_is_written_and_bad_arguments_write_nothing(golden):
    """The raw entry point on the test's own buffers: a NaN-filled output holds no NaN after a good call (no memset needed);
    every DC_EINVAL case returns before anything is launched and leaves a sentinel-filled output as it was."""
    from depthcore import _lib
    L = _lib.lib()
    a, c = golden["a"], golden["c"]
    points = np.concatenate([a["points"], c["points"]])
    sizes, out_hw = [(33, 17), (40, 20)], (20, 40)

    def fresh():
        args = lidar_abi.arguments([3001, 1], sizes, out_hw)
        args["desc"]["P"] = np.stack([a["P"][2].ravel(), c["P"][2].ravel()])
        return args
    ws_bytes = L.dc_lidar_workspace_bytes(2, 40, 20)
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=DEV)
    out = torch.full((2, 1) + out_hw, float("nan"), device=DEV)
    args = fresh()
    keep, (pts, desc_d, rows_d, cols_d) = _device_arguments(args, points)
    st = _lib.stream(out)
    assert lidar_abi.call(L, args, pts.data_ptr(), desc_d, rows_d, cols_d, out.data_ptr(), ws.data_ptr(), ws_bytes, st) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(out).any() and torch.count_nonzero(out[0]) > 100 and torch.count_nonzero(out[1]) >= 1
    want = [golden[n]["maps"][(2, 0)][args["rows"][i]][:, args["cols"][i]] for i, n in enumerate("ac")]
    _same_bits(out, np.stack(want)[:, None])
    sentinel = torch.full_like(out, -7.5)
    for what in lidar_abi.BAD_ARGUMENTS:
        bad = fresh()
        null = lidar_abi.spoil(bad, what)
        keep_bad, (_, desc_b, rows_b, cols_b) = _device_arguments(bad, points)
        out.copy_(sentinel)
        assert lidar_abi.call(L, bad, pts.data_ptr(), desc_b, rows_b, cols_b, out.data_ptr(), ws.data_ptr(), ws_bytes, st, null=null) == -1, what
        torch.cuda.synchronize()
        assert torch.equal(out, sentinel), what
    assert lidar_abi.call(L, fresh(), pts.data_ptr(), desc_d, rows_d, cols_d, out.data_ptr(), ws.data_ptr(), ws_bytes - 8, st) == -3
    torch.cuda.synchronize()
    assert torch.equal(out, sentinel)


# ------------------------------------------------------------------------------------------------ loader, trainer, export
@pytest.fixture(scope="module")
def scan_tree(tmp_path_factory):
    import datasets
    root = str(tmp_path_factory.mktemp("kitti_scans"))
    write_raw_tree(root, frames=4, sides=("l", "r"), drives=TREE)
    write_scans(root, frames=4, drives=TREE, points=4000)
    lines = ["%s %d %s" % (drive, i, "lr"[i % 2]) for drive in sorted(TREE) for i in range(4)]
    ds = datasets.KITTIRAWDataset(root, lines, 64, 96, [0, -1, 1], 4, is_train=True, img_ext=".png")
    assert ds.load_depth
    return root, ds


@pytest.mark.parametrize("cache_slots", [0, 8 * 3 + 6])
def test_loader_delivers_the_depth_gt_of_decode_batch(scan_tree, cache_slots):
    """Uncached, and with a frame cache that holds every frame: cold epoch 0, warm epoch 1 (nothing decoded, scans still read)."""
    from depthcore.data import slot_layout
    from depthcore.loader import BatchLoader
    _, ds = scan_tree
    ld = BatchLoader(ds, 2, num_workers=4, device=DEV, seed=5, prefetch=2, cache_bytes=cache_slots * slot_layout(64, 96, 4)[1])
    flipped = sizes = 0
    for epoch in range(2):
        ld.set_epoch(epoch)
        plan = ld.plan()
        batches = list(ld)
        torch.cuda.synchronize()
        assert len(batches) == len(plan) == 4
        for (indices, draws), batch in zip(plan, batches):
            want = ld.decode_batch(indices, draws)[4]["depth_gt"]
            assert batch["depth_gt"].shape == (2, 1, 375, 1242) and np.count_nonzero(want) > 2 * 375 * 1242 // 10
            _same_bits(batch["depth_gt"], want)
            flipped += sum(d[0] for d in draws)
            sizes += len({ds.filenames[i].split()[0] for i in indices}) == 2
    assert flipped and sizes                       # flipped items and batches that mix the two native sizes were among them
    if cache_slots:
        assert ld.cache.stats["hits"] >= 3 * 8 and ld.cache.stats["bypassed"] == 0
    ld.close()


def test_trainer_val_scores_a_loader_batch(scan_tree):
    import trainer as T
    from depthcore.loader import BatchLoader
    _, ds = scan_tree
    ld = BatchLoader(ds, 2, num_workers=2, device=DEV, seed=5)
    batch = next(iter(ld))
    ld.close()
    tr = T.Trainer(T.default_options(batch_size=2, height=64, width=96), device=DEV)
    tr.set_train()
    _, losses = tr.val(batch)
    assert tr.depth_metric_names == ["de/abs_rel", "de/sq_rel", "de/rms", "de/log_rms", "da/a1", "da/a2", "da/a3"]
    assert all(k in losses and np.isfinite(float(losses[k])) for k in tr.depth_metric_names)


def test_export_writes_what_evaluate_depth_accepts(scan_tree, tmp_path):
    import export_gt_depth
    from depthcore import evaluate as E
    from depthcore import lidar
    root, ds = scan_tree
    lines = [ds.filenames[i] for i in (0, 4, 1, 5, 2, 6)]                    # two native sizes, alternating
    os.makedirs(str(tmp_path / "eigen"))
    (tmp_path / "eigen" / "test_files.txt").write_text("\n".join(lines) + "\n")
    path = export_gt_depth.export_gt_depths_kitti(["--data_path", root, "--split", "eigen", "--splits_dir", str(tmp_path)])
    data = np.load(path, fix_imports=True, encoding="latin1", allow_pickle=True)["data"]
    assert data.dtype == object and data.shape == (6,)
    for line, m in zip(lines, data):
        folder, frame = line.split()[0], int(line.split()[1])
        P, size = lidar.velo_to_image(os.path.join(root, folder.split("/")[0]), 2)
        want = lidar_ref.depth_map(lidar.load_velodyne_points(ds.velo_path(folder, frame)), P, size, True)
        assert m.dtype == np.float32 and np.array_equal(m.view(np.int32), want.view(np.int32))
    pred = torch.rand(6, 1, 64, 96, generator=torch.Generator().manual_seed(0)) * 0.5 + 0.01
    res = E.evaluate_depth(pred, data, "eigen")
    assert res["errors"].shape == (6, 7) and np.isfinite(res["errors"]).all()
