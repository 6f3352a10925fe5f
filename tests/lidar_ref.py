"""Loop restatement of the reference's velodyne depth map (kitti_utils.py:46-98) for the lidar tests, independent of
depthcore/lidar.py: rules 1-9 of include/depthcore.h's dc_lidar_depth_maps comment, then KITTIRAWDataset.get_depth's resize --
by Pillow's NEAREST on a mode "F" image, the project's rule -- and np.fliplr."""
import numpy as np
from PIL import Image


def projection_matrix(calib, cam):
    """P (3,4) fp64 from the numbers of a calibration (keys P_rect_02, P_rect_03, R_rect_00, R, T), as kitti_utils.py:52-62."""
    v2c = np.vstack((np.hstack((calib["R"].reshape(3, 3), calib["T"].reshape(3, 1))), np.array([0, 0, 0, 1.0])))
    R = np.eye(4)
    R[:3, :3] = calib["R_rect_00"].reshape(3, 3)
    return np.dot(np.dot(calib["P_rect_0%d" % cam].reshape(3, 4), R), v2c)


def depth_map(points, P, size, vel_depth=False):
    """(n,4) float32 scan, P (3,4) fp64, size (W, H) -> (H, W) float32."""
    W, H = size
    pts = np.asarray(points, np.float32)
    pts = pts[pts[:, 0] >= 0]
    hits = {}                                   # (y, x) -> [(kept index, depth)], in kept order
    for i, p in enumerate(pts):
        x, y, z = float(p[0]), float(p[1]), float(p[2])
        q = [((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3] for r in range(3)]
        if q[2] == 0:
            continue                            # u, v are inf or nan: outside every image
        px, py = np.round(q[0] / q[2]) - 1, np.round(q[1] / q[2]) - 1
        if not (0 <= px < W and 0 <= py < H):
            continue
        d = np.float32(p[0]) if vel_depth else np.float32(q[2])
        hits.setdefault((int(py), int(px)), []).append((i, d))
    depth = np.zeros((H, W), np.float32)
    for (y, x), lst in hits.items():
        depth[y, x] = min(d for _, d in lst)
    # sub2ind = y (W-1) + x - 1 is one key for (y, W-1) and (y+1, 0): one group when both are hit
    for y in range(H - 1):
        a, b = hits.get((y, W - 1)), hits.get((y + 1, 0))
        if a and b:
            lo = min(d for _, d in a + b)
            if a[0][0] < b[0][0]:
                depth[y, W - 1], depth[y + 1, 0] = lo, b[-1][1]
            else:
                depth[y, W - 1], depth[y + 1, 0] = a[-1][1], lo
    depth[depth < 0] = 0
    return depth


def resize_flip(depth, out_hw=None, flip=False):
    """Pillow NEAREST resize of the float32 map to out_hw (Ho, Wo), then fliplr."""
    depth = np.asarray(depth, np.float32)
    if out_hw is not None:
        depth = np.array(Image.fromarray(depth, "F").resize((out_hw[1], out_hw[0]), Image.NEAREST))
    return np.ascontiguousarray(np.fliplr(depth) if flip else depth)
