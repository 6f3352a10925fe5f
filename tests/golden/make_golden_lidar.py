"""Writes tests/golden/lidar.npz: three small synthetic velodyne calibrations and scans, and the depth maps that the
reference's own kitti_utils.generate_depth_map gives for them (cameras 2 and 3, vel_depth False and True).

The reference tree is only read when this script runs:

    python tests/golden/make_golden_lidar.py /path/to/reference

kitti_utils.py uses `np.int`, which current numpy no longer has: this script sets `np.int = int` before importing it.  That is
the only change; the maps are what the reference's code computes.  It reads files, so the calibrations and scans are written
to a temporary directory first; the .npz keeps them as numbers.

Fixtures (native W x H / points): "a" 33 x 17 / 3001, "b" 64 x 24 / 6000, "c" 40 x 20 / 1.  Every scan holds points behind the
sensor (x < 0, dropped), points with x == 0, and -- the multi-point ones -- 50 points within 0.4 m of the image plane, some of
them behind it: their depth is negative when vel_depth is False.  The points are spread a little beyond the image on every
side, so columns 0 and W-1 are hit like any other and the reference's edge-column grouping (sub2ind) has work to do.

The seed is the first one for which all of this holds (asserted below):
  * no kept point has u or v within 1e-6 of a half-integer (the reference's BLAS dot and a fixed-order sum differ by ~1e-12 px);
  * each multi-point fixture, for each camera, has an edge pair (y, W-1) / (y+1, 0) whose earliest point is on the right edge
    and one whose earliest point is on the left edge;
  * at least half of the hit pixels hold more than one point;
  * at least one vel_depth=False depth is negative before the clamp.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lidar_ref  # noqa: E402

FIXTURES = (("a", 33, 17, 3001), ("b", 64, 24, 6000), ("c", 40, 20, 1))


def rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def calibration(rng, W, H):
    """KITTI-shaped numbers at a small size: the velodyne looks along +x, the camera along +z."""
    f = 0.6 * W
    cx, cy = W / 2 + rng.uniform(-0.5, 0.5), H / 2 + rng.uniform(-0.5, 0.5)
    P2 = np.array([[f, 0, cx, 0.045 * f], [0, f, cy, -0.0003 * f], [0, 0, 1, 0.0027]])
    P3 = np.array([[f, 0, cx, -0.47 * f], [0, f, cy, 0.0021 * f], [0, 0, 1, 0.0031]])          # the right camera's baseline
    R_rect = rot(rng.randn(3), 0.01)
    R = rot(rng.randn(3), 0.02) @ np.array([[0, -1.0, 0], [0, 0, -1.0], [1.0, 0, 0]])
    T = np.array([-0.004, -0.076, -0.27]) + 0.01 * rng.randn(3)
    # through "%e" text and back, as the files hold them
    as_text = lambda a: np.array([float("%e" % v) for v in np.ravel(a)])
    return {"P_rect_02": as_text(P2), "P_rect_03": as_text(P3), "R_rect_00": as_text(R_rect), "R": as_text(R), "T": as_text(T),
            "S_rect_02": np.array([float(W), float(H)])}


def scan(rng, calib, W, H, n):
    """n points (n, 4) float32: chosen in the image of camera 2 (a little beyond it on every side), mapped back to the sensor."""
    if n == 1:
        u, v, Z = np.array([W / 2 + 0.2]), np.array([H / 2 - 0.3]), np.array([7.0])
    else:
        u, v = rng.uniform(-2.5, W + 3.5, n), rng.uniform(-2.5, H + 3.5, n)
        Z = rng.uniform(2, 30, n)
        near = rng.choice(n, 50, replace=False)
        Z[near] = rng.uniform(0.02, 0.4, 50) * np.where(np.arange(50) % 2, 1, -0.6)           # behind the plane: -0.24 .. -0.012
    P = calib["P_rect_02"].reshape(3, 4)
    q2 = Z + P[2, 3]
    cam = np.stack([(u * q2 - P[0, 2] * Z - P[0, 3]) / P[0, 0], (v * q2 - P[1, 2] * Z - P[1, 3]) / P[1, 1], Z], 1)
    velo = (cam @ calib["R_rect_00"].reshape(3, 3) - calib["T"]) @ calib["R"].reshape(3, 3)        # inverse rotations: transposes
    pts = np.concatenate([velo, rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)
    if n > 1:
        rest = np.setdiff1d(np.arange(n), near)
        behind = rng.choice(rest, n // 20, replace=False)
        pts[behind, 0] = -np.abs(pts[behind, 0]) - 0.01
        pts[rng.choice(np.setdiff1d(rest, behind), 5, replace=False), 0] = 0.0
    return pts


def write_tree(root, calib, pts):
    with open(os.path.join(root, "calib_cam_to_cam.txt"), "w") as f:
        f.write("calib_time: 09-Jan-2012 13:57:47\ncorner_dist: 9.950000e-02\n")
        for k in ("S_rect_02", "R_rect_00", "P_rect_02", "P_rect_03"):
            f.write("%s: %s\n" % (k, " ".join("%e" % v for v in calib[k])))
    with open(os.path.join(root, "calib_velo_to_cam.txt"), "w") as f:
        f.write("calib_time: 15-Mar-2012 11:37:16\n")
        for k in ("R", "T"):
            f.write("%s: %s\n" % (k, " ".join("%e" % v for v in calib[k])))
    pts.tofile(os.path.join(root, "scan.bin"))


def conditions(calib, pts, W, H):
    """The asserted properties of one fixture -> list of failures (empty: fine)."""
    bad = []
    negative = False
    for cam in (2, 3):
        P = lidar_ref.projection_matrix(calib, cam)
        kept = pts[pts[:, 0] >= 0].astype(np.float64)
        q = np.stack([((P[r, 0] * kept[:, 0] + P[r, 1] * kept[:, 1]) + P[r, 2] * kept[:, 2]) + P[r, 3] for r in range(3)], 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            u, v = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
        fin = np.isfinite(u) & np.isfinite(v)
        for c in (u[fin], v[fin]):
            if np.any(np.abs(c - np.floor(c) - 0.5) < 1e-6):
                bad.append("cam %d: a coordinate within 1e-6 of a half-integer" % cam)
        px, py = np.round(u) - 1, np.round(v) - 1
        inside = fin & (px >= 0) & (py >= 0) & (px < W) & (py < H)
        negative |= bool(np.any(q[inside, 2] < 0))
        if len(pts) == 1:
            if not inside.all():
                bad.append("cam %d: the single point misses the image" % cam)
            continue
        pix = (py[inside] * W + px[inside]).astype(np.int64)
        counts = np.bincount(pix, minlength=W * H)
        if 2 * np.count_nonzero(counts > 1) < np.count_nonzero(counts):
            bad.append("cam %d: fewer than half of the hit pixels hold several points" % cam)
        first = np.full(W * H, len(pix), np.int64)
        np.minimum.at(first, pix, np.arange(len(pix)))
        first = first.reshape(H, W)
        a, b = first[:-1, W - 1], first[1:, 0]
        both = (a < len(pix)) & (b < len(pix))
        if not np.any(both & (a < b)) or not np.any(both & (b < a)):
            bad.append("cam %d: edge pairs do not cover both orders" % cam)
    if len(pts) > 1 and not negative:
        bad.append("no negative depth")
    return bad


def main(ref):
    np.int = int                                 # kitti_utils.py:86 (see the docstring)
    sys.path.insert(0, ref)
    from kitti_utils import generate_depth_map
    seed = 1
    while True:
        rng = np.random.RandomState(seed)
        fixtures = []
        for name, W, H, n in FIXTURES:
            calib = calibration(rng, W, H)
            fixtures.append((name, W, H, calib, scan(rng, calib, W, H, n)))
        failures = [(name, f) for name, W, H, calib, pts in fixtures for f in conditions(calib, pts, W, H)]
        if not failures:
            break
        print("seed %d:" % seed, failures)
        seed += 1
    out = {"seed": np.int64(seed), "names": np.array([f[0] for f in fixtures])}
    for name, W, H, calib, pts in fixtures:
        with tempfile.TemporaryDirectory() as root:
            write_tree(root, calib, pts)
            for k, v in calib.items():
                out["%s_%s" % (name, k)] = v
            out["%s_points" % name] = pts
            for cam in (2, 3):
                for vel in (False, True):
                    m = generate_depth_map(root, os.path.join(root, "scan.bin"), cam, vel)
                    assert m.shape == (H, W) and m.dtype == np.float64
                    out["%s_map_cam%d_vel%d" % (name, cam, vel)] = m.astype(np.float32)
                    mine = lidar_ref.depth_map(pts, lidar_ref.projection_matrix(calib, cam), (W, H), vel)
                    print(name, cam, vel, "hit pixels", np.count_nonzero(m), "restatement differs at",
                          np.count_nonzero(mine != m.astype(np.float32)))
    path = os.path.join(HERE, "lidar.npz")
    np.savez_compressed(path, **out)
    print("seed", seed, "->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
