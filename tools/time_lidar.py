#!/usr/bin/env python3
"""Times the velodyne "depth_gt" path on synthetic scans.  Prints one JSON line:

  batch_*                12 scans of 120 000 points, 1242 x 375 -> (12, 1, 375, 1242), medians by hipEvents:
                         `upload_ms` the pinned host-to-device copy of the 23 MB of points, `passes_ms` dc_lidar_depth_maps alone
                         (descriptors and tables already on the device), `op_ms` ops.lidar_depth_maps (with its small
                         descriptor copy and allocations); `host_12_threads_ms` the numpy path (depth_map_host + resize) of the
                         same 12 scans on 12 threads, wall clock
  scan_read_ms           the 12 scan files of a batch read into pinned memory on the decode thread count, wall clock, six runs
  loader_batches_per_s   BatchLoader on a tmp raw tree of JPEGs in the five native sizes, without scans (the tree as it is
                         before the scans are written: no "depth_gt", the loader's behaviour without this feature) and with a
                         120 000-point scan per frame; uncached, and on a warm frame cache
  train_ms_per_step      Trainer.train_step fed by each of the four loaders, alternating blocks

    python tools/time_lidar.py [--batch 12] [--height 192] [--width 640] [--num_workers 12] [--steps 30] [--frames 14]
"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "self-supervised-depth-estimation_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import datasets  # noqa: E402
import trainer as T  # noqa: E402
from depthcore import _lib, lidar, ops  # noqa: E402
from depthcore.data import slot_layout  # noqa: E402
from depthcore.loader import BatchLoader, _read_into  # noqa: E402
from time_loader import KITTI_SIZES, median_ms, write_tree  # noqa: E402

POINTS = 120000


def calibration(W, H):
    f = 0.58 * W
    c, s = np.cos(0.01), np.sin(0.01)
    return {"S_rect_02": [float(W), float(H)], "R_rect_00": [c, -s, 0, s, c, 0, 0, 0, 1.0],
            "P_rect_02": [f, 0, W / 2 + 0.3, 0.045 * f, 0, f, H / 2 - 0.2, -0.0003 * f, 0, 0, 1, 0.0027],
            "P_rect_03": [f, 0, W / 2 + 0.3, -0.47 * f, 0, f, H / 2 - 0.2, 0.0021 * f, 0, 0, 1, 0.0031],
            "R": [s, -c, 0, 0, 0, -1.0, c, s, 0], "T": [-0.004, -0.076, -0.27]}


def scan(calib, n, seed):
    """(n, 4) float32 around the sensor like a real sweep: about a fifth of the points fall inside camera 2's image."""
    rng = np.random.RandomState(seed)
    az, el, r = rng.uniform(-np.pi, np.pi, n), rng.uniform(-0.43, 0.04, n), rng.uniform(3, 80, n)
    pts = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el), rng.uniform(0, 1, n)], 1)
    return pts.astype(np.float32)


def write_scans(root, frames):
    for d, (h, w) in enumerate(KITTI_SIZES):
        date = "2011_09_%02d" % (26 + d)
        calib = calibration(w, h)
        with open(os.path.join(root, date, "calib_cam_to_cam.txt"), "w") as f:
            for k in ("S_rect_02", "R_rect_00", "P_rect_02", "P_rect_03"):
                f.write("%s: %s\n" % (k, " ".join("%e" % v for v in calib[k])))
        with open(os.path.join(root, date, "calib_velo_to_cam.txt"), "w") as f:
            for k in ("R", "T"):
                f.write("%s: %s\n" % (k, " ".join("%e" % v for v in calib[k])))
        folder = os.path.join(root, date, "%s_drive_%04d_sync" % (date, d + 1), "velodyne_points", "data")
        os.makedirs(folder)
        for i in range(frames):
            scan(calib, POINTS, 100 * d + i).tofile(os.path.join(folder, "%010d.bin" % i))


def batch_times(dev, B, res):
    calib = calibration(1242, 375)
    v2c = np.vstack((np.hstack((np.array(calib["R"]).reshape(3, 3), np.array(calib["T"]).reshape(3, 1))), [0, 0, 0, 1.0]))
    R = np.eye(4)
    R[:3, :3] = np.array(calib["R_rect_00"]).reshape(3, 3)
    P = np.dot(np.dot(np.array(calib["P_rect_02"]).reshape(3, 4), R), v2c)
    scans = [scan(calib, POINTS, s) for s in range(B)]
    host = torch.from_numpy(np.concatenate(scans)).pin_memory()
    pts = torch.empty_like(host, device=dev)
    counts, Ps, sizes, flips = [POINTS] * B, np.stack([P] * B), [(1242, 375)] * B, [b % 2 == 1 for b in range(B)]

    def per_call(fn, calls=20):       # 20 calls between the two events: a single call is too short a window to time
        return round(median_ms(lambda: [fn() for _ in range(calls)], 15) / calls, 4)
    res["batch_upload_ms"] = per_call(lambda: pts.copy_(host, non_blocking=True))
    got = ops.lidar_depth_maps(pts, counts, Ps, sizes, out_size=(375, 1242), flips=flips)
    res["batch_hit_pixels_per_map"] = int(torch.count_nonzero(got)) // B
    res["batch_op_ms"] = per_call(lambda: ops.lidar_depth_maps(pts, counts, Ps, sizes, out_size=(375, 1242), flips=flips))
    # the entry point alone
    L = _lib.lib()
    desc = np.zeros(B, lidar.LIDAR_IMG)
    desc["n_points"], desc["point_off"], desc["W"], desc["H"], desc["flip"] = POINTS, np.arange(B) * POINTS, 1242, 375, flips
    desc["P"] = P.ravel()
    rows, cols = (np.ascontiguousarray(np.tile(t, (B, 1))) for t in lidar.nearest_tables((1242, 375), (1242, 375)))
    desc_d, rows_d, cols_d = (torch.from_numpy(x.view(np.uint8).reshape(-1)).to(dev) for x in (desc, rows, cols))
    ws_bytes = L.dc_lidar_workspace_bytes(B, 1242, 375)
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    out = torch.empty((B, 1, 375, 1242), device=dev)

    def passes():
        _lib.check(L.dc_lidar_depth_maps(pts.data_ptr(), B * POINTS, desc.ctypes.data, desc_d.data_ptr(), B, rows.ctypes.data,
                                         rows_d.data_ptr(), cols.ctypes.data, cols_d.data_ptr(), 375, 1242, out.data_ptr(), ws.data_ptr(),
                                         ws_bytes, _lib.stream(out)), "dc_lidar_depth_maps")
    res["batch_passes_ms"] = per_call(passes)
    assert torch.equal(out, got)
    with ThreadPoolExecutor(12) as pool:
        def one(b):
            return lidar.resize_flip(lidar.depth_map_host(scans[b], P, (1242, 375)), (1242, 375), flips[b])
        want = list(pool.map(one, range(B)))
        ms = []
        for _ in range(5):
            t0 = time.perf_counter()
            list(pool.map(one, range(B)))
            ms.append(1e3 * (time.perf_counter() - t0))
    assert np.array_equal(np.stack(want)[:, None], got.cpu().numpy()), "device and host maps differ"
    res["batch_host_12_threads_ms"] = round(sorted(ms)[len(ms) // 2], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--num_workers", type=int, default=12)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--frames", type=int, default=14)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    B = a.batch
    res = {"config": "resnet18 %d x %d x %d, %d decode threads, %d points per scan" % (B, a.height, a.width, min(a.num_workers, 16), POINTS)}
    batch_times(dev, B, res)
    with tempfile.TemporaryDirectory() as root:
        lines = write_tree(root, a.frames)
        make = lambda: datasets.KITTIRAWDataset(root, lines, a.height, a.width, [0, -1, 1], 4, is_train=True, img_ext=".jpg")  # noqa: E731
        plain = make()                  # before the scans exist: check_depth() is False, no "depth_gt"
        write_scans(root, a.frames)
        scans = make()
        assert not plain.load_depth and scans.load_depth
        # the host's share of a batch's scans: B files read into pinned memory on the loader's thread count
        paths = [scans.depth_source(i)[0] for i in range(B)]
        pinned = torch.empty(sum(os.path.getsize(p) for p in paths), dtype=torch.uint8).pin_memory().numpy()
        with ThreadPoolExecutor(min(a.num_workers, 16)) as pool:
            ms = []
            for _ in range(6):
                t0 = time.perf_counter()
                list(pool.map(lambda b: _read_into(paths[b], pinned[b * POINTS * 16:(b + 1) * POINTS * 16]), range(B)))
                ms.append(1e3 * (time.perf_counter() - t0))
        res["scan_read_ms"] = [round(v, 3) for v in ms]
        cache_bytes = (len(KITTI_SIZES) * a.frames + 3 * B + 1) * slot_layout(a.height, a.width, 4)[1]
        loaders = {"plain": BatchLoader(plain, B, a.num_workers, dev, seed=1), "scans": BatchLoader(scans, B, a.num_workers, dev, seed=1),
                   "plain_warm_cache": BatchLoader(plain, B, a.num_workers, dev, seed=1, cache_bytes=cache_bytes),
                   "scans_warm_cache": BatchLoader(scans, B, a.num_workers, dev, seed=1, cache_bytes=cache_bytes)}
        epoch = {k: 0 for k in loaders}

        def one_epoch(name):
            ld = loaders[name]
            ld.set_epoch(epoch[name])
            epoch[name] += 1
            it = iter(ld)
            first = next(it)
            assert ("depth_gt" in first) == name.startswith("scans")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            count = sum(1 for _ in it)
            torch.cuda.synchronize()
            return round(count / (time.perf_counter() - t0), 1)
        for name in loaders:            # the cached loaders' cold epoch (and everybody's first: page cache, tables) is not reported
            one_epoch(name)
        for _ in range(3):
            for name in loaders:
                res.setdefault("loader_batches_per_s", {}).setdefault(name, []).append(one_epoch(name))

        tr = T.Trainer(T.default_options(batch_size=B, height=a.height, width=a.width), device=dev)
        tr.set_train()

        def cycle(name):
            while True:
                loaders[name].set_epoch(epoch[name])
                epoch[name] += 1
                for batch in loaders[name]:
                    yield batch
        feeds = {name: cycle(name) for name in loaders}

        def steps_ms(feed):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                tr.train_step(next(feed))
            torch.cuda.synchronize()
            return round(1e3 * (time.perf_counter() - t0) / a.steps, 3)
        with tr.on_step_stream():
            for _ in range(4):
                for feed in feeds.values():
                    tr.train_step(next(feed))
            for _ in range(3):
                for name, feed in feeds.items():
                    res.setdefault("train_ms_per_step", {}).setdefault(name, []).append(steps_ms(feed))
        for feed in feeds.values():
            feed.close()
        for ld in loaders.values():
            ld.close()
        tr.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
