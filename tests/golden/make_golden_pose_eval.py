"""Writes tests/golden/pose_eval.npz: a small KITTI-like odometry trajectory, fp32 pose predictions for it, and the absolute
trajectory errors the reference's own evaluate_pose.py functions give for them.

dump_xyz and compute_ate (evaluate_pose.py:23-46) are taken from the reference file's source (ast) and run in a namespace
holding numpy only: importing evaluate_pose as a module would pull in the datasets and the networks.  The loop below is what
lines 104-125 do around them (global poses padded to 4x4, local poses by np.linalg.inv, one snippet per frame, np.mean /
np.std), for track lengths 5 (the reference's) and 3.  The reference tree is only read when this script runs:

    python tests/golden/make_golden_pose_eval.py /path/to/reference

The trajectory's rows go through "%e" text and back, as a poses/XX.txt file does: six decimals, so the rotation blocks are
orthogonal to ~1e-6 only -- an implementation that inverts a pose by transposing its rotation is off by about that much, one
that inverts the affine map agrees to ~1e-14.  The predictions are the local ground-truth poses with the translations at an
unknown scale (x 0.03) plus noise (sigma 0.002), so every ATE is well away from zero (a relative tolerance says nothing about an
ATE near 0) and the scale alignment of compute_ate has work to do.
"""
import ast
import io
import os
import sys

import numpy as np

M = 40                              # poses; 39 frame pairs, 39 snippets
SCALE, SIGMA = 0.03, 0.002


def reference_functions(ref):
    src = open(os.path.join(ref, "evaluate_pose.py")).read()
    tree = ast.parse(src)
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("dump_xyz", "compute_ate")]
    ns = {"np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "evaluate_pose.py", "exec"), ns)
    return ns["dump_xyz"], ns["compute_ate"]


def rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def trajectory(rng):
    """A car's drive: mostly forward (camera z) at ~1 m per frame, a slow turn about y with some pitch and roll."""
    G = np.eye(4)
    rows = []
    for i in range(M):
        rows.append(G[:3].reshape(12).copy())
        step = np.eye(4)
        step[:3, :3] = rot([0.05 * rng.randn(), 1.0, 0.05 * rng.randn()], 0.02 + 0.01 * rng.randn())
        step[:3, 3] = [0.02 * rng.randn(), 0.01 * rng.randn(), 1.0 + 0.2 * rng.rand()]
        G = G @ step
    text = io.StringIO()
    np.savetxt(text, np.array(rows), fmt="%e")                      # the format of KITTI's poses/XX.txt
    return np.loadtxt(io.StringIO(text.getvalue())).reshape(-1, 3, 4)


def local_poses(gt_global_poses):
    full = np.concatenate((gt_global_poses, np.zeros((gt_global_poses.shape[0], 1, 4))), 1)
    full[:, 3, 3] = 1
    return [np.linalg.inv(np.dot(np.linalg.inv(full[i - 1]), full[i])) for i in range(1, len(full))]


def score(dump_xyz, compute_ate, pred_poses, gt_local_poses, num_frames, track_length):
    ates = []
    for i in range(0, num_frames - 1):
        local_xyzs = np.array(dump_xyz(pred_poses[i:i + track_length - 1]))
        gt_local_xyzs = np.array(dump_xyz(gt_local_poses[i:i + track_length - 1]))
        ates.append(compute_ate(gt_local_xyzs, local_xyzs))
    return np.array(ates, np.float64), np.float64(np.mean(ates)), np.float64(np.std(ates))


def main(ref):
    dump_xyz, compute_ate = reference_functions(ref)
    rng = np.random.RandomState(7)
    gt = trajectory(rng)
    ortho = max(np.abs(g[:, :3].T @ g[:, :3] - np.eye(3)).max() for g in gt)
    assert 1e-8 < ortho < 1e-4, ortho
    locs = local_poses(gt)
    pred = np.array(locs)
    pred[:, :3, 3] = pred[:, :3, 3] * SCALE + SIGMA * rng.randn(M - 1, 3)
    pred = pred.astype(np.float32)
    res = {}
    for L in (5, 3):
        ates, mean, std = score(dump_xyz, compute_ate, pred, locs, M, L)
        assert ates.min() > 1e-3, ates.min()
        res["ates_%d" % L], res["mean_%d" % L], res["std_%d" % L] = ates, mean, std
        print("track_length %d: ATE %.4f .. %.4f, mean %.4f, std %.4f" % (L, ates.min(), ates.max(), mean, std))
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pose_eval.npz")
    np.savez_compressed(out, gt_global=gt, pred=pred, **res)
    print("wrote", out, os.path.getsize(out), "bytes; rotations orthogonal to %.1e" % ortho)


if __name__ == "__main__":
    main(sys.argv[1])
