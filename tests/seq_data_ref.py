"""The reference's sequence item (datasets/kitti_dataset_seq.py:100-197) restated on the CPU for the sequence tests, from
oracle.data_ref's resize / ColorJitter / ToTensor and tests/lidar_ref.py, independent of depthcore/data.py.

Per frame of a window and per level s (`get_color`):
    r = Lanczos resize of u[s-1] to (height >> s, width >> s);  m = mirror(r) if do_flip;
    u[s] = ColorJitter_fresh(m) if do_color_aug;  ("color", f, s, j) = u[s] / 255
with u[-1] the decoded frame.  The mirror therefore accumulates (levels 0 and 2 mirrored, 1 and 3 not, where resize and
mirror commute) and level s + 1 is resized from the jittered level s.  torchvision's Resize returns an image that already
has the target size unchanged; `resize_lanczos` skips both passes there.
"""
import numpy as np

from oracle import data_ref as D

WINDOW_FIRST = (1, 0, 2)      # centre, left, right: the reference's order
WINDOW_FRAMES = (0, -1, 1)


def frame_chain(native, height, width, num_scales=4, flip=False, jitter=None):
    """One frame through `get_color`: native (Hn, Wn, 3) uint8 -> [u[0], .., u[S-1]] uint8 HWC.
    jitter: None or [(order, factors)] per level."""
    u, out = native, []
    for s in range(num_scales):
        u = D.resize_lanczos(u, height >> s, width >> s)
        if flip:
            u = u[:, ::-1]
        if jitter is not None:
            u = D.color_jitter(np.ascontiguousarray(u), *jitter[s])
        out.append(np.ascontiguousarray(u))
    return out


def sequence_item(native, height, width, num_scales=4, flip=False, jitters=None):
    """native: (n + 2, Hn, Wn, 3) uint8; jitters: None or jitters[w][j][s] = (order, factors).
    -> {("color", f, s): (n, 3, h, w) float32, ("color_packed", f, 0): (n, H, W, 4) float32} for f in 0, -1, 1."""
    n = native.shape[0] - 2
    out = {}
    for w, (first, f) in enumerate(zip(WINDOW_FIRST, WINDOW_FRAMES)):
        chains = [frame_chain(native[first + j], height, width, num_scales, flip, jitters[w][j] if jitters is not None else None)
                  for j in range(n)]
        for s in range(num_scales):
            out[("color", f, s)] = np.stack([D.to_tensor(c[s]) for c in chains])
        rgb = np.stack([c[0].astype(np.float32) / np.float32(255.0) for c in chains]).astype(np.float32)
        out[("color_packed", f, 0)] = np.concatenate([rgb, np.zeros(rgb.shape[:-1] + (1,), np.float32)], -1)
    return out


def pillow_chain(native, height, width, num_scales=4, flip=False):
    """The resize / mirror part of `frame_chain` by the installed Pillow itself, level after level."""
    from PIL import Image
    img, out = Image.fromarray(native), []
    for s in range(num_scales):
        if img.size != (width >> s, height >> s):
            img = img.resize((width >> s, height >> s), Image.LANCZOS)
        if flip:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        out.append(np.asarray(img).copy())
    return out


def depth_gt(scans, P, size, flip):
    """`get_depth` for the n centre frames: scans = [(m, 4) float32] -> (n, 1, 375, 1242) float32, mirrored once if flip.
    P: the (3, 4) projection of camera 2 (lidar_ref.projection_matrix), size: the (W, H) of the calibration."""
    import lidar_ref
    return np.stack([lidar_ref.resize_flip(lidar_ref.depth_map(pts, P, size), (375, 1242), flip)[None] for pts in scans])
