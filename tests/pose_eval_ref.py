"""numpy restatement of the trajectory scoring of the pose evaluation (reference evaluate_pose.py:23-46, 104-125), written from
its formulas, in fp64:

  ground-truth local pose j = inv(inv(G[j]) G[j+1]), G the (3,4) pose row over (0,0,0,1), the inverse being the GENERAL affine
      one, [A^-1 | -A^-1 t] (the files' rotations are orthogonal to ~1e-6 only: no transpose shortcut);
  snippet i: points C_0 = I, C_k = C_{k-1} T[i+k-1] over T[i : i+track_length-1] clipped at the end of the array, the
      translation columns being the points -- once for the predictions, once for the local ground truth;
  ate: predicted points shifted so that the first ones coincide, scale = sum(gt pred) / sum(pred^2),
      sqrt(sum((pred scale - gt)^2)) / points;
  mean and population std over the snippets.

tests/golden/pose_eval.npz holds what the reference's own functions give (tests/golden/make_golden_pose_eval.py); with the
affine inverse in place of np.linalg.inv this agrees with it to ~1e-14, not bitwise.
"""
import numpy as np


def affine_inv(T):
    """Inverse of a 4x4 affine map [A t; 0 1] (adjugate of the 3x3 block)."""
    A, t = np.asarray(T[:3, :3], np.float64), np.asarray(T[:3, 3], np.float64)
    cof = np.empty((3, 3))
    for r in range(3):
        for c in range(3):
            r0, r1 = [k for k in range(3) if k != r]
            c0, c1 = [k for k in range(3) if k != c]
            cof[r, c] = (-1) ** (r + c) * (A[r0, c0] * A[r1, c1] - A[r0, c1] * A[r1, c0])
    det = A[0, 0] * cof[0, 0] + A[0, 1] * cof[0, 1] + A[0, 2] * cof[0, 2]
    out = np.eye(4)
    out[:3, :3] = cof.T / det
    out[:3, 3] = -(out[:3, :3] @ t)
    return out


def transpose_inv(T):
    """The shortcut that is NOT the reference's arithmetic: [R^T | -R^T t] (tests show that the fixture tells it apart)."""
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(out[:3, :3] @ T[:3, 3])
    return out


def pad(gt_global):
    g = np.asarray(gt_global, np.float64).reshape(-1, 3, 4)
    full = np.zeros((g.shape[0], 4, 4))
    full[:, :3] = g
    full[:, 3, 3] = 1
    return full


def gt_local_poses(gt_global, inv=affine_inv):
    G = pad(gt_global)
    return [inv(inv(G[j]) @ G[j + 1]) for j in range(len(G) - 1)]


def snippet_points(transforms, i, track_length):
    """(points, 3): the origin and the translation of every partial product of transforms[i : i+track_length-1]."""
    C = np.eye(4)
    pts = [C[:3, 3].copy()]
    for T in transforms[i:i + track_length - 1]:
        C = C @ np.asarray(T, np.float64)
        pts.append(C[:3, 3].copy())
    return np.array(pts)


def ate(gt_pts, pred_pts):
    pred = pred_pts + (gt_pts[0] - pred_pts[0])[None]
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.sum(gt_pts * pred) / np.sum(pred ** 2)
    return np.sqrt(np.sum((pred * scale - gt_pts) ** 2)) / gt_pts.shape[0]


def evaluate(pred, gt_global, track_length=5, inv=affine_inv):
    """-> (ates (N,), mean, std) for pred (N,4,4) and gt_global (N+1,3,4) or (N+1,12)."""
    locs = gt_local_poses(gt_global, inv)
    pred = list(np.asarray(pred))
    if len(pred) != len(locs):
        raise ValueError("%d predictions for %d ground-truth poses" % (len(pred), len(locs) + 1))
    ates = np.array([ate(snippet_points(locs, i, track_length), snippet_points(pred, i, track_length))
                     for i in range(len(locs))], np.float64)
    return ates, np.mean(ates), np.std(ates)
