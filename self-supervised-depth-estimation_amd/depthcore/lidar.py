"""Velodyne scans -> sparse depth maps: the reference's kitti_utils.py (read_calib_file, generate_depth_map) and the resize + flip
of KITTIRAWDataset.get_depth (datasets/kitti_dataset.py:71-86).

Two implementations of the same rules (include/depthcore.h: dc_lidar_depth_maps states them), equal bit for bit as float32:
  * the device op `ops.lidar_depth_maps` -- a batch of scans per call; what the loader and export_gt_depth.py use;
  * `depth_map_host` -- vectorised numpy (np.minimum.at plus the edge-column rule, no Python loop over points); what the
    datasets' `get_depth` and a machine without a GPU use.
The projection is evaluated in fp64 in one fixed order, ((P0*x + P1*y) + P2*z) + P3, where the reference's np.dot leaves the
order to BLAS: the two differ by at most an ulp of fp64, which the float32 output does not see unless a point projects
within ~1e-12 px of a half-integer pixel coordinate.

The resize to the dataset's full_res_shape is Pillow's NEAREST (what KITTIDepthDataset.get_depth uses), not the reference's
skimage.transform.resize(order=0): the index tables are obtained from Pillow itself (`nearest_tables`).
"""
import os

import numpy as np
import torch
from PIL import Image

_FLOAT_CHARS = set("0123456789.e+- ")
# numpy mirror of dc_lidar_img (include/depthcore.h), 128 bytes
LIDAR_IMG = np.dtype([("point_off", np.int64), ("n_points", np.int32), ("W", np.int32), ("H", np.int32), ("vel_depth", np.int32),
                      ("flip", np.int32), ("reserved", np.int32), ("P", np.float64, (12,))])


def read_calib(path):
    """KITTI calibration file -> {key: float64 array, or the string when the value is not numeric} (kitti_utils.py:17-36)."""
    data = {}
    with open(path, "r") as f:
        for line in f.readlines():
            if ":" not in line:
                continue
            key, value = line.split(":", 1)
            value = value.strip()
            data[key] = value
            if _FLOAT_CHARS.issuperset(value):
                try:
                    data[key] = np.array([float(v) for v in value.split(" ")])
                except ValueError:
                    pass
    return data


_calib_cache = {}


def velo_to_image(calib_dir, cam=2):
    """-> (P (3,4) float64, (W, H)): P = P_rect_0{cam} . [R_rect_00 | 0; 0 1] . [R T; 0 1] and the native image size S_rect_02
    (kitti_utils.py:50-62; S_rect_02 for camera 3 as well).  Cached per (calib_dir, cam)."""
    key = (os.path.abspath(calib_dir), int(cam))
    if key not in _calib_cache:
        cam2cam = read_calib(os.path.join(calib_dir, "calib_cam_to_cam.txt"))
        velo2cam = read_calib(os.path.join(calib_dir, "calib_velo_to_cam.txt"))
        v2c = np.hstack((velo2cam["R"].reshape(3, 3), velo2cam["T"][..., np.newaxis]))
        v2c = np.vstack((v2c, np.array([0, 0, 0, 1.0])))
        H, W = cam2cam["S_rect_02"][::-1].astype(np.int32)
        R = np.eye(4)
        R[:3, :3] = cam2cam["R_rect_00"].reshape(3, 3)
        P = np.dot(np.dot(cam2cam["P_rect_0" + str(int(cam))].reshape(3, 4), R), v2c)
        P.setflags(write=False)
        _calib_cache[key] = (P, (int(W), int(H)))
    return _calib_cache[key]


_table_cache = {}


def _nearest_axis(n_in, n_out):
    key = (int(n_in), int(n_out))
    if key not in _table_cache:
        if key[0] == key[1]:
            t = np.arange(key[0], dtype=np.int32)
        else:
            # Pillow's nearest pass steps its source coordinate in a double, pixel by pixel: ask Pillow, do not re-derive
            src = Image.fromarray(np.arange(key[0], dtype=np.int32).reshape(1, key[0]), "I")
            t = np.asarray(src.resize((key[1], 1), Image.NEAREST)).reshape(key[1]).astype(np.int32)
        t.setflags(write=False)
        _table_cache[key] = t
    return _table_cache[key]


def nearest_tables(native, out):
    """native (W, H), out (Wo, Ho) -> (rows (Ho,), cols (Wo,)) int32: the native row / column that Pillow's
    `resize(out, NEAREST)` reads for every output row / column (the identity when the sizes agree).  Cached per size pair."""
    return _nearest_axis(native[1], out[1]), _nearest_axis(native[0], out[0])


class Descriptors:
    """The host arguments of one dc_lidar_depth_maps call as ONE byte block, [desc B x 128 | rows B x Ho x 4 | cols B x Wo x 4]:
    `host` (uint8) is what the device copy must hold, at an 8-byte aligned address; desc / rows / cols are views of it."""

    def __init__(self, B, Ho, Wo):
        self.B, self.Ho, self.Wo = B, Ho, Wo
        self.host = np.zeros(B * (128 + 4 * (Ho + Wo)), np.uint8)
        self.rows_off, self.cols_off = B * 128, B * (128 + 4 * Ho)
        self.desc = self.host[:self.rows_off].view(LIDAR_IMG)
        self.rows = self.host[self.rows_off:self.cols_off].view(np.int32).reshape(B, Ho)
        self.cols = self.host[self.cols_off:].view(np.int32).reshape(B, Wo)


def descriptors(counts, P, sizes, out_size=None, vel_depth=False, flips=None):
    """The arguments of `ops.lidar_depth_maps` (see there) -> Descriptors; the scans lie back to back in the points buffer."""
    from ._lib import DepthcoreError
    B = len(counts)
    Pm = np.ascontiguousarray(np.asarray(P, np.float64)).reshape(-1, 12)
    vd = [bool(vel_depth)] * B if np.ndim(vel_depth) == 0 else [bool(v) for v in vel_depth]
    fl = [False] * B if flips is None else [bool(f) for f in flips]
    if B == 0 or Pm.shape[0] != B or len(sizes) != B or len(vd) != B or len(fl) != B:
        raise DepthcoreError("lidar_depth_maps: counts, P, sizes, vel_depth and flips take one entry per scan")
    sizes = [(int(w), int(h)) for w, h in sizes]
    if out_size is None:
        if len(set(sizes)) != 1:
            raise DepthcoreError("lidar_depth_maps: out_size=None needs one native size, got %s" % sorted(set(sizes)))
        Ho, Wo = sizes[0][1], sizes[0][0]
    else:
        Ho, Wo = int(out_size[0]), int(out_size[1])
    if Ho <= 0 or Wo <= 0 or any(w < 2 or h < 1 for w, h in sizes) or any(int(c) < 0 for c in counts):
        raise DepthcoreError("lidar_depth_maps: bad size or count (native sizes at least 2 x 1)")
    d = Descriptors(B, Ho, Wo)
    d.desc["n_points"] = np.asarray(counts, np.int64)
    d.desc["point_off"] = np.cumsum(d.desc["n_points"], dtype=np.int64) - d.desc["n_points"]
    d.desc["W"], d.desc["H"] = [s[0] for s in sizes], [s[1] for s in sizes]
    d.desc["vel_depth"], d.desc["flip"], d.desc["P"] = vd, fl, Pm
    for b, s in enumerate(sizes):
        d.rows[b], d.cols[b] = nearest_tables(s, (Wo, Ho))
    return d


def load_velodyne_points(filename):
    """(n, 4) float32 rows of a KITTI velodyne file (kitti_utils.py:8-14; column 3 is ignored by the projection)."""
    return np.fromfile(filename, dtype=np.float32).reshape(-1, 4)


def depth_map_host(points, P, size, vel_depth=False):
    """The reference's depth map of one scan on the host -> (H, W) float32.  points (n, >=3) float32, P (3,4) float64,
    size (W, H).  Vectorised: per-pixel minimum by np.minimum.at, then the edge-column rule on the two columns it touches."""
    W, H = int(size[0]), int(size[1])
    if W < 2 or H < 1:
        raise ValueError("depth_map_host: the native size must be at least 2 x 1, got %d x %d" % (W, H))
    pts = np.asarray(points, np.float32)
    P = np.asarray(P, np.float64).reshape(3, 4)
    pts = pts[pts[:, 0] >= 0]
    x, y, z = (pts[:, k].astype(np.float64) for k in range(3))
    q = [((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3] for r in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        px, py = np.rint(q[0] / q[2]) - 1, np.rint(q[1] / q[2]) - 1
    val = (px >= 0) & (py >= 0) & (px < W) & (py < H)
    ix, iy = px[val].astype(np.int64), py[val].astype(np.int64)
    d = (pts[:, 0] if vel_depth else q[2].astype(np.float32))[val]
    best = np.full(H * W, np.inf, np.float32)
    np.minimum.at(best, iy * W + ix, d)
    hit = np.zeros(H * W, bool)
    hit[iy * W + ix] = True
    depth = np.where(hit, best, np.float32(0)).reshape(H, W)
    # sub2ind = y (W-1) + x - 1 is shared by (y, W-1) and (y+1, 0): where both are hit, the pixel of the earlier first point takes
    # the minimum over both, the other keeps its LAST point's depth (kitti_utils.py:86-95)
    edge = np.flatnonzero((ix == 0) | (ix == W - 1))
    if H > 1 and edge.size:
        slot = iy[edge] * 2 + (ix[edge] != 0)
        first = np.full(2 * H, np.iinfo(np.int64).max, np.int64)
        last = np.full(2 * H, -1, np.int64)
        np.minimum.at(first, slot, edge)
        np.maximum.at(last, slot, edge)
        fa, fb = first[1:2 * H - 2:2], first[2::2]            # A = (y, W-1), B = (y+1, 0) for y = 0 .. H-2
        la, lb = last[1:2 * H - 2:2], last[2::2]
        both = np.flatnonzero((la >= 0) & (lb >= 0))
        lo = np.minimum(depth[both, W - 1], depth[both + 1, 0])
        a_first = fa[both] < fb[both]
        depth[both, W - 1] = np.where(a_first, lo, d[la[both]])
        depth[both + 1, 0] = np.where(a_first, d[lb[both]], lo)
    depth[depth < 0] = 0
    return depth


def resize_flip(depth, out_size=None, flip=False):
    """(H, W) map -> Pillow-NEAREST resize to out_size (Wo, Ho) (None: as is), then np.fliplr when `flip`."""
    if out_size is not None:
        rows, cols = nearest_tables((depth.shape[1], depth.shape[0]), out_size)
        depth = depth[rows][:, cols]
    return np.ascontiguousarray(depth[:, ::-1] if flip else depth)


def generate_depth_map(calib_dir, velo_filename, cam=2, vel_depth=False):
    """kitti_utils.generate_depth_map: (H, W) float64 array (holding float32-exact values) of one scan at its native size.
    Runs on the GPU when there is one (ops.lidar_depth_maps), else on the host (depth_map_host): the same values."""
    P, size = velo_to_image(calib_dir, cam)
    pts = load_velodyne_points(velo_filename)
    if torch.cuda.is_available():
        from . import ops
        dev = torch.device("cuda", torch.cuda.current_device())
        out = ops.lidar_depth_maps(torch.from_numpy(pts).to(dev), [len(pts)], P[None], [size], vel_depth=vel_depth)
        return out[0, 0].cpu().numpy().astype(np.float64)
    return depth_map_host(pts, P, size, vel_depth).astype(np.float64)
