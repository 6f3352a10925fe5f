"""The 1x1 dispatcher's host-side queries (csrc/pointwise.hip: dc_pointwise_workspace / _stat_parts / _bwd_parts) against the
queries of the kernel family that the routing table of include/depthcore.h predicts, for both split modes.  No GPU: the
queries are host code and dc_set_gemm_split writes a plain global."""
import ctypes

import pytest

from depthcore import _lib

X3, G1, PW = "split bf16", "fp32-MFMA", "general"
# (B, Ci, Co, H, W, stride) -> family of (forward, data gradient, weight gradient) under dc_set_gemm_split(1); under mode 0 the
# split family's passes go to fp32-MFMA (every shape here that the split kernels take, the fp32-MFMA kernels take too)
SHAPES = {
    (2, 64, 96, 4, 8, 1): (X3, X3, X3),         # split takes all passes
    (2, 64, 128, 8, 16, 2): (X3, X3, X3),       # stride 2: the data gradient through the split kernels' scatter epilogue
    (8, 64, 32, 2, 6, 1): (G1, G1, G1),         # P = 12: split refuses, fp32-MFMA takes all three
    (3, 7, 5, 6, 10, 2): (PW, PW, PW),          # general kernels; 16-byte workspace floor
    (3, 2048, 512, 10, 32, 1): (X3, X3, X3),    # tiles span images (used with 3 BatchNorm groups)
}
PASSES = ("fwd", "dgrad", "wgrad")


def _family(mode, p, shape):
    fam = SHAPES[shape][PASSES.index(p)]
    return G1 if (fam == X3 and not mode) else fam


@pytest.fixture
def L():
    lib = _lib.lib()
    prev = lib.dc_get_gemm_split()
    try:
        yield lib
    finally:
        lib.dc_set_gemm_split(prev)


def test_shapes_land_where_the_comments_say(L):
    """the table above against the family-pinned predicates (the fp32-MFMA ones are not exported per pass: a statistics layout
    for one group exists iff those kernels take the shape's forward)"""
    for shape, fams in SHAPES.items():
        for p, fam in zip(PASSES, fams):
            assert bool(getattr(L, "dc_gemm1x1x3_%s_ok" % p)(*shape)) == (fam == X3), (shape, p)
        assert (L.dc_conv1x1_stat_parts(*shape, 1, None) > 0) == (fams[0] != PW), shape


@pytest.mark.parametrize("mode", [0, 1])
def test_workspace_is_the_chosen_familys(L, mode):
    L.dc_set_gemm_split(mode)
    for shape in SHAPES:
        B, Ci, Co, H, W, s = shape
        for k, p in enumerate(PASSES):
            fam = _family(mode, p, shape)
            if p == "wgrad":
                want = L.dc_gemm1x1x3_wgrad_workspace(*shape) if fam == X3 else L.dc_conv1x1_wgrad_workspace(*shape)
            else:
                want = L.dc_gemm1x1x3_workspace(Ci, Co) if fam == X3 else 0       # only the split kernels stage their weights
            assert L.dc_pointwise_workspace(k, None, *shape) == max(want, 16), (shape, p, mode)
            f = _lib.BnFold()                 # a fold struct that asks for nothing: same family, same bytes (groups = 1)
            f.groups = 1
            assert L.dc_pointwise_workspace(k, ctypes.byref(f), *shape) == max(want, 16), (shape, p, mode)
    assert L.dc_pointwise_workspace(3, None, 2, 64, 96, 4, 8, 1) == 16         # no such pass: the floor


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("groups", [1, 2, 3])
def test_partial_counts_are_the_chosen_familys(L, mode, groups):
    """Forward with a fold: split iff the mode is on and the split kernels have a statistics layout for these groups; data
    gradient with the BatchNorm epilogue: split iff the mode is on, stride 1, and they have a backward layout; else fp32-MFMA.
    Count and partials-per-group (ppg) both."""
    L.dc_set_gemm_split(mode)
    seen_split = 0
    for shape in SHAPES:
        if groups == 3 and shape[0] != 3:
            continue
        B, Ci, Co, H, W, s = shape
        for query, x3, g1 in (
                (L.dc_pointwise_stat_parts, lambda pp: L.dc_gemm1x1x3_stat_parts(B, Ci, Co, H, W, s, groups, pp),
                 lambda pp: L.dc_conv1x1_stat_parts(B, Ci, Co, H, W, s, groups, pp)),
                (L.dc_pointwise_bwd_parts, lambda pp: L.dc_gemm1x1x3_bwd_parts(B, Ci, Co, H, W, groups, pp) if s == 1 else 0,
                 lambda pp: L.dc_conv1x1_bwd_parts(B, Ci, Co, H, W, groups, pp) if s == 1 else 0)):
            want_ppg, got_ppg = ctypes.c_int(-7), ctypes.c_int(-7)
            split = bool(mode) and x3(None) > 0
            seen_split += split
            want = (x3 if split else g1)(ctypes.byref(want_ppg))
            got = query(B, Ci, Co, H, W, s, groups, ctypes.byref(got_ppg))
            assert (got, got_ppg.value) == (want, want_ppg.value), (shape, groups, mode, query.__name__)
            assert query(B, Ci, Co, H, W, s, groups, None) == want
    if mode and groups != 2:
        assert seen_split >= 2          # (the comparison is not vacuous: the two families' layouts differ, see ppg above)
    if not mode:
        assert seen_split == 0


def test_the_two_families_layouts_differ_on_a_shared_shape(L):
    """what the dispatcher protects: at (2, 64, 96, 4, 8) both families have the statistics epilogue, with different partials per
    group -- a count from one used with the other's launch would be wrong"""
    a, b = ctypes.c_int(0), ctypes.c_int(0)
    assert L.dc_gemm1x1x3_stat_parts(2, 64, 96, 4, 8, 1, 1, ctypes.byref(a)) > 0
    assert L.dc_conv1x1_stat_parts(2, 64, 96, 4, 8, 1, 1, ctypes.byref(b)) > 0
    assert a.value != b.value
