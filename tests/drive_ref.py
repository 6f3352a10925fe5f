"""The one-range-per-drive contract of include/depthcore.h (dc_disp_range_pooled, dc_disp_render_fixed) in plain numpy, stated
through tests/render_ref.py: the range is render_ref's `value_range` -- the minimum and numpy's `_lerp` between two exact order
statistics at the fp64 virtual index -- of the POOLED values of all N upsampled maps, and the colouring is render_ref's
`indices` with that one pair for every image.  Test infrastructure: what the kernels are held to, bitwise."""
import numpy as np

import render_ref as R


def pooled_range(d, q=95.0):
    """(N,1,Ho,Wo) or (N,Ho,Wo) upsampled fp32 maps -> (vmin, vmax) as np.float32 over all N * Ho * Wo values."""
    return R.value_range(np.asarray(d, np.float32).ravel(), q)


def render_fixed(d, vmin, vmax, lut=None):
    """(N,1,Ho,Wo) or (N,Ho,Wo) upsampled fp32 maps -> rgb (N,Ho,Wo,3) uint8, every image coloured against (vmin, vmax)."""
    lut = R.magma_lut() if lut is None else np.asarray(lut, np.uint8)
    d = np.asarray(d, np.float32)
    if d.ndim == 4:
        d = d[:, 0]
    return lut[R.indices(d, np.float32(vmin), np.float32(vmax))]


def render_drive(d, q=95.0, lut=None):
    """-> (rgb (N,Ho,Wo,3) uint8, vmin, vmax): the pooled range, then the fixed-range colouring."""
    vmin, vmax = pooled_range(d, q)
    return render_fixed(d, vmin, vmax, lut), vmin, vmax
