"""The disparity-rendering contract of DESIGN 4l / include/depthcore.h (dc_disp_render) in plain numpy: the reference's
test_simple.py:137-141 -- vmin = min, vmax = np.percentile(., q), matplotlib's Normalize and colour-map look-up -- with every
type and rounding written out.  Test infrastructure: the one thing the kernel is held to (bitwise), itself held to
matplotlib + numpy by tests/golden/render.npz and tests/test_render_cpu.py.

Where numpy versions part: the virtual index (n-1) * (q/100) is formed in fp64 here (numpy 1.x, which the reference was
written against); numpy 2.x casts q to the array's fp32 first, which moves vmax by an ulp or so on large maps."""
import math
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "render.npz")


def magma_lut():
    """(matplotlib magma lut[:256, :3] * 255).astype(uint8), as the fixture recorded it from matplotlib."""
    return np.load(GOLDEN, allow_pickle=False)["lut"]


def order_statistics(d, q):
    """-> (lo, hi, g, s) for the flat fp32 map d: s sorted ascending, lo = floor(vi), hi = min(lo+1, n-1), g = vi - lo."""
    s = np.sort(np.asarray(d, np.float32).ravel())
    n = s.size
    vi = (n - 1) * (float(q) / 100.0)                       # Python floats: fp64
    lo = min(int(math.floor(vi)), n - 1)
    hi = min(lo + 1, n - 1)
    return lo, hi, vi - lo, s


def value_range(d, q=95.0):
    """(vmin, vmax) as np.float32: numpy's `_lerp` between the two exact order statistics."""
    lo, hi, g, s = order_statistics(d, q)
    a, b = s[lo], s[hi]
    diff = np.float32(b - a)                                 # fp32 - fp32 -> fp32
    if g < 0.5:
        v = np.float64(a) + np.float64(diff) * np.float64(g)
    else:
        v = np.float64(b) - np.float64(diff) * (np.float64(1.0) - np.float64(g))
    return s[0], np.float32(v)


def indices(d, vmin, vmax):
    """Table index of every pixel of the fp32 map d (any shape) for the range (vmin, vmax), int64."""
    d = np.asarray(d, np.float32)
    if np.float32(vmin) == np.float32(vmax):
        return np.zeros(d.shape, np.int64)
    x = (d.astype(np.float64) - np.float64(vmin)).astype(np.float32)
    x = (x.astype(np.float64) / (np.float64(vmax) - np.float64(vmin))).astype(np.float32)
    xa = x * np.float32(256.0)                               # fp32
    assert xa.dtype == np.float32
    idx = np.minimum(xa, np.float32(256.0)).astype(np.int64)  # truncation; the clamp first only keeps the cast defined
    idx = np.minimum(idx, 255)
    idx[xa < 0] = 0
    return idx


def render(d, q=95.0, lut=None):
    """One upsampled fp32 map (Ho, Wo) -> (rgb (Ho, Wo, 3) uint8, vmin, vmax)."""
    lut = magma_lut() if lut is None else np.asarray(lut, np.uint8)
    d = np.asarray(d, np.float32)
    vmin, vmax = value_range(d, q)
    return lut[indices(d, vmin, vmax)], vmin, vmax


def render_batch(d, q=95.0, lut=None):
    """(N,1,Ho,Wo) or (N,Ho,Wo) -> (rgb (N,Ho,Wo,3) uint8, range (N,2) float32): every image has its own range."""
    d = np.asarray(d, np.float32)
    if d.ndim == 4:
        d = d[:, 0]
    out = [render(x, q, lut) for x in d]
    return np.stack([o[0] for o in out]), np.array([[o[1], o[2]] for o in out], np.float32)


def matplotlib_render(d, q=95.0):
    """What test_simple.py:137-141 computes, with the installed matplotlib and numpy -> (rgb uint8, vmin, vmax)."""
    import matplotlib
    from matplotlib.colors import Normalize
    d = np.asarray(d, np.float32)
    vmin, vmax = d.min(), np.percentile(d, q)
    rgba = matplotlib.colormaps["magma"](Normalize(vmin=vmin, vmax=vmax)(d))
    return (rgba[..., :3] * 255).astype(np.uint8), vmin, vmax


# ---- cases shared by tests/golden/make_golden_render.py and the tests ----------------------------------------------------------
# the issue's list for the kernel: (h, w) -> (Ho, Wo)
GPU_SHAPES = [((192, 640), (375, 1242)), ((192, 640), (370, 1226)), ((6, 20), (41, 57)), ((3, 5), (3, 5)), ((1, 1), (1, 1)),
              ((2, 1), (7, 1))]
# the fixture's: name -> (h, w, Ho, Wo, kind, seed); small shapes only (a few kB)
FIXTURE_CASES = {
    "up_6x20": (6, 20, 41, 57, "sigmoid", 1),
    "same_3x5": (3, 5, 3, 5, "sigmoid", 2),
    "one_pixel": (1, 1, 1, 1, "sigmoid", 3),
    "column": (2, 1, 7, 1, "sigmoid", 4),
    "up_12x40": (12, 40, 37, 53, "sigmoid", 5),
    "narrow": (24, 80, 101, 7, "sigmoid", 6),
    "ties": (16, 24, 16, 24, "eighths", 7),
    "constant": (11, 13, 11, 13, "constant", 8),
    "near_constant": (5, 9, 11, 13, "constant", 8),          # the interpolation's rounding: two or three neighbouring values
}


def low_res_map(h, w, kind, seed):
    """A decoder-like (h, w) fp32 map in (0, 1): the sigmoid of seeded noise; "eighths": rounded to eighths (heavy ties);
    "constant": one value everywhere."""
    rng = np.random.RandomState(seed)
    d = (1.0 / (1.0 + np.exp(-1.5 * rng.randn(h, w)))).astype(np.float32)
    if kind == "eighths":
        d = (np.round(d * 8.0) / 8.0).astype(np.float32)
    elif kind == "constant":
        d = np.full((h, w), d[0, 0], np.float32)
    elif kind != "sigmoid":
        raise ValueError(kind)
    return d
