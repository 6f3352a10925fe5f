"""numpy statement of dc_log_panel's arithmetic contract (include/depthcore.h): fp32 operations in the stated order, indexing
instead of kernels, no torch.  The yardstick of tests/test_logpanel_gpu.py.

A tile is (src, kind, panel, up, x0, y0, thr) with src a numpy array: "rgb" (3,h,w) float32, "norm" / "unit" (h,w) float32,
"mask" (h,w) uint8."""
import numpy as np

F = np.float32


def unit_bytes(v):
    """v <= 0 or NaN -> 0, v >= 1 -> 255, else (uint8)(v * 255.0f + 0.5f): a rounded fp32 product, a rounded fp32 sum, truncation."""
    v = np.asarray(v, dtype=F)
    out = np.zeros(v.shape, np.uint8)
    with np.errstate(invalid="ignore"):
        hi = v >= F(1.0)
        mid = (v > F(0.0)) & ~hi                       # NaN fails both comparisons: stays 0
    out[hi] = 255
    t = v[mid] * F(255.0)
    t = t + F(0.5)
    assert t.dtype == F
    out[mid] = t.astype(np.int32).astype(np.uint8)
    return out


def norm_index(v):
    """normalize_image (the reference's utils.py) and the colour-table index: mi / ma exact, d = ma - mi or 1e5 when they are
    equal as floats, x = (v - mi) / d, xa = x * 256, idx = xa < 0 ? 0 : min((int)xa, 255)."""
    v = np.asarray(v, dtype=F)
    mi, ma = F(v.min()), F(v.max())
    d = F(ma - mi) if ma != mi else F(1e5)
    x = (v - mi) / d
    xa = x * F(256.0)
    assert x.dtype == F and xa.dtype == F
    return np.where(xa < F(0.0), 0, np.minimum(xa.astype(np.int64), 255)).astype(np.int64)


def tile_bytes(src, kind, up, thr=0, lut=None):
    """(h*up, w*up, 3) uint8: the pixels one tile covers.  Destination (y, x) reads source (y // up, x // up)."""
    src = np.asarray(src)
    if kind == "rgb":
        px = np.stack([unit_bytes(src[c]) for c in range(3)], -1)
    elif kind == "unit":
        px = np.repeat(unit_bytes(src)[..., None], 3, -1)
    elif kind == "mask":
        assert src.dtype == np.uint8
        px = np.repeat(np.where(src.astype(np.int64) >= int(thr), 255, 0).astype(np.uint8)[..., None], 3, -1)
    elif kind == "norm":
        px = np.asarray(lut, dtype=np.uint8)[norm_index(src)]
    else:
        raise ValueError(kind)
    h, w = px.shape[:2]
    ys, xs = np.arange(h * up) // up, np.arange(w * up) // up
    return px[ys[:, None], xs[None, :]]


def compose(tiles, n_panels, PH, PW, lut, background=0):
    """(n_panels, PH, PW, 3) uint8."""
    out = np.full((n_panels, PH, PW, 3), background, np.uint8)
    for t in tiles:
        src, kind, panel, up, x0, y0 = t[:6]
        thr = t[6] if len(t) > 6 else 0
        px = tile_bytes(src, kind, up, thr, lut)
        assert 0 <= panel < n_panels and x0 >= 0 and y0 >= 0 and y0 + px.shape[0] <= PH and x0 + px.shape[1] <= PW
        out[panel, y0:y0 + px.shape[0], x0:x0 + px.shape[1]] = px
    return out
