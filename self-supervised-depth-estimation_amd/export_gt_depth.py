"""Drop-in for the reference's export_gt_depth.py: writes <splits_dir>/<split>/gt_depths.npz, the ground truth that
evaluate_depth.py scores against.

    python export_gt_depth.py --data_path kitti_data --split eigen [--splits_dir splits]

  eigen            the velodyne scan of every line of test_files.txt projected into camera 2 with vel_depth=True
                   (export_gt_depth.py:45-49), at the drive's native size: ops.lidar_depth_maps, a batch of scans of one native
                   size per call; on a machine without a GPU the host path of depthcore.lidar (the same values);
  eigen_benchmark  proj_depth/groundtruth/image_02/<frame>.png / 256 (:50-53), on the host.

`data` in the file is what the reference's np.array(list of float32 maps) gave on the numpy it was written for: an (N, H, W)
float32 array when all maps share a shape, else a 1-D object array of (H, W) float32 maps (evaluate_depth.py loads it with
allow_pickle=True).  --splits_dir is an addition (the reference reads the splits next to the script; none ship here).
"""
import argparse
import os
import sys

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from depthcore import lidar  # noqa: E402

SCANS_PER_CALL = 32


def readlines(filename):
    with open(filename, "r") as f:
        return f.read().splitlines()


def velodyne_maps(sources):
    """sources: [(calib_dir, scan path)] -> the (H, W) float32 maps of camera 2 with vel_depth=True, in order."""
    maps = [None] * len(sources)
    if not torch.cuda.is_available():
        for i, (calib_dir, path) in enumerate(sources):
            P, size = lidar.velo_to_image(calib_dir, 2)
            maps[i] = lidar.depth_map_host(lidar.load_velodyne_points(path), P, size, vel_depth=True)
        return maps
    from depthcore import ops
    device = torch.device("cuda", torch.cuda.current_device())
    by_size = {}
    for i, (calib_dir, _) in enumerate(sources):
        by_size.setdefault(lidar.velo_to_image(calib_dir, 2)[1], []).append(i)
    for size, idx in by_size.items():
        for c0 in range(0, len(idx), SCANS_PER_CALL):
            ids = idx[c0:c0 + SCANS_PER_CALL]
            scans = [lidar.load_velodyne_points(sources[i][1]) for i in ids]
            P = np.stack([lidar.velo_to_image(sources[i][0], 2)[0] for i in ids])
            out = ops.lidar_depth_maps(torch.from_numpy(np.concatenate(scans)).to(device), [len(s) for s in scans], P,
                                       [size] * len(ids), vel_depth=True)
            for i, m in zip(ids, out[:, 0].cpu().numpy()):
                maps[i] = m
    return maps


def export_gt_depths_kitti(argv=None):
    parser = argparse.ArgumentParser(description="export_gt_depth")
    parser.add_argument("--data_path", type=str, help="path to the root of the KITTI data", required=True)
    parser.add_argument("--split", type=str, help="which split to export gt from", required=True, choices=["eigen", "eigen_benchmark"])
    parser.add_argument("--splits_dir", type=str, help="folder of the split files",
                        default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "splits"))
    opt = parser.parse_args(argv)

    split_folder = os.path.join(opt.splits_dir, opt.split)
    lines = readlines(os.path.join(split_folder, "test_files.txt"))
    print("Exporting ground truth depths for {}".format(opt.split))
    parsed = [(line.split()[0], int(line.split()[1])) for line in lines]
    if opt.split == "eigen":
        gt_depths = velodyne_maps([(os.path.join(opt.data_path, folder.split("/")[0]),
                                    os.path.join(opt.data_path, folder, "velodyne_points/data", "{:010d}.bin".format(frame_id)))
                                   for folder, frame_id in parsed])
    else:
        gt_depths = []
        for folder, frame_id in parsed:
            path = os.path.join(opt.data_path, folder, "proj_depth", "groundtruth", "image_02", "{:010d}.png".format(frame_id))
            with Image.open(path) as img:
                gt_depths.append(np.array(img).astype(np.float32) / 256)
    if len(set(m.shape for m in gt_depths)) == 1:
        data = np.stack(gt_depths).astype(np.float32)
    else:
        data = np.empty(len(gt_depths), dtype=object)
        for i, m in enumerate(gt_depths):
            data[i] = m.astype(np.float32)
    output_path = os.path.join(split_folder, "gt_depths.npz")
    print("Saving to {}".format(opt.split))
    np.savez_compressed(output_path, data=data)
    return output_path


if __name__ == "__main__":
    export_gt_depths_kitti()
