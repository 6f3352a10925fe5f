"""Velodyne scans and calibration files for a kitti_tree raw tree: KITTI-shaped numbers at the tree's small native sizes."""
import os

import numpy as np

from kitti_tree import DRIVES


def calibration(W, H, seed):
    """The numbers of one date folder: cameras 2 and 3 (the right camera half a metre to the side), the velodyne looking along
    +x and the cameras along +z, slightly rotated against each other."""
    rng = np.random.RandomState(seed)
    f = 0.6 * W
    cx, cy = W / 2 + 0.3, H / 2 - 0.2
    c, s = np.cos(0.01), np.sin(0.01)
    return {"S_rect_02": np.array([float(W), float(H)]),
            "R_rect_00": np.array([c, -s, 0, s, c, 0, 0, 0, 1.0]),
            "P_rect_02": np.array([f, 0, cx, 0.045 * f, 0, f, cy, -0.0003 * f, 0, 0, 1, 0.0027]),
            "P_rect_03": np.array([f, 0, cx, -0.47 * f, 0, f, cy, 0.0021 * f, 0, 0, 1, 0.0031]),
            "R": np.array([s, -c, 0, 0, 0, -1.0, c, s, 0]),
            "T": np.array([-0.004, -0.076, -0.27]) + 0.01 * rng.randn(3)}


def scan(calib, W, H, n, seed):
    """(n, 4) float32: points spread over camera 2's image and a little beyond, some behind the sensor (x < 0)."""
    rng = np.random.RandomState(seed)
    u, v, Z = rng.uniform(-2.5, W + 3.5, n), rng.uniform(-2.5, H + 3.5, n), rng.uniform(2, 70, n)
    P = calib["P_rect_02"].reshape(3, 4)
    q2 = Z + P[2, 3]
    cam = np.stack([(u * q2 - P[0, 2] * Z - P[0, 3]) / P[0, 0], (v * q2 - P[1, 2] * Z - P[1, 3]) / P[1, 1], Z], 1)
    velo = (cam @ calib["R_rect_00"].reshape(3, 3) - calib["T"]) @ calib["R"].reshape(3, 3)
    pts = np.concatenate([velo, rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)
    pts[::17, 0] *= -1
    return pts


def write_calibration(folder, calib):
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, "calib_cam_to_cam.txt"), "w") as f:
        f.write("calib_time: 09-Jan-2012 13:57:47\ncorner_dist: 9.950000e-02\n")
        for k in ("S_rect_02", "R_rect_00", "P_rect_02", "P_rect_03"):
            f.write("%s: %s\n" % (k, " ".join("%e" % v for v in calib[k])))
    with open(os.path.join(folder, "calib_velo_to_cam.txt"), "w") as f:
        f.write("calib_time: 15-Mar-2012 11:37:16\n")
        for k in ("R", "T"):
            f.write("%s: %s\n" % (k, " ".join("%e" % v for v in calib[k])))


def write_scans(root, frames=6, drives=None, points=1500):
    """<root>/<date>/calib_*.txt and <root>/<drive>/velodyne_points/data/<10 digits>.bin for `frames` frames per drive
    -> {(drive, frame): (n, 4) float32}.  Frame i of a drive has points + 7 i points (scan sizes differ within a batch)."""
    scans = {}
    for d, (drive, (h, w)) in enumerate(sorted((drives or DRIVES).items())):
        calib = calibration(w, h, d)
        write_calibration(os.path.join(root, drive.split("/")[0]), calib)
        folder = os.path.join(root, drive, "velodyne_points", "data")
        os.makedirs(folder, exist_ok=True)
        for i in range(frames):
            pts = scan(calib, w, h, points + 7 * i, 100 * d + i)
            pts.tofile(os.path.join(folder, "%010d.bin" % i))
            scans[(drive, i)] = pts
    return scans
