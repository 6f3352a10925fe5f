"""The prepared-weight cache's registry (csrc/weight_cache.hip: dc_wino_cache_*): owner ids, what `register` takes and refuses, and
that releasing one owner leaves the other's entries alone.  Bookkeeping only -- no call here reaches the device (a refresh does: that
is tests/test_weight_cache_gpu.py's ground).  Needs no GPU."""
import ctypes

import wino_bn_cases as WC

OK = 0


def _weights(n):
    """n distinct, 256-byte aligned host addresses (the registry keys on the pointer and never reads through it)"""
    buf = ctypes.create_string_buffer(256 * (n + 1))
    base = (ctypes.addressof(buf) + 255) & ~255
    return buf, [base + 256 * i for i in range(n)]


def test_registry_bookkeeping():
    L = WC.host_lib()
    variants = L.dc_wino_cache_variants()
    keep, (w0, w1, w2) = _weights(3)
    a, b = L.dc_wino_cache_new_owner(), L.dc_wino_cache_new_owner()
    try:
        assert a > 0 and b > 0 and a != b
        unknown = max(a, b) + 1000
        # what register refuses: a null weight, non-positive channels, an owner nobody created
        assert L.dc_wino_cache_register(a, None, 8, 8) == WC.EINVAL
        for ci, co in ((0, 8), (8, 0), (-1, 8), (8, -1)):
            assert L.dc_wino_cache_register(a, w0, ci, co) == WC.EINVAL
        assert L.dc_wino_cache_register(unknown, w0, 8, 8) == WC.EINVAL
        # ... none of which left an entry behind: the same pointer registers under either owner afterwards
        assert L.dc_wino_cache_register(a, w0, 8, 16) == OK
        assert L.dc_wino_cache_register(b, w1, 24, 8) == OK
        # the identical repeat is accepted; other channels or another owner for a registered pointer are not
        assert L.dc_wino_cache_register(a, w0, 8, 16) == OK
        assert L.dc_wino_cache_register(a, w0, 16, 8) == WC.EINVAL
        assert L.dc_wino_cache_register(a, w0, 8, 8) == WC.EINVAL
        assert L.dc_wino_cache_register(b, w0, 8, 16) == WC.EINVAL
        assert L.dc_wino_cache_register(a, w1, 24, 8) == WC.EINVAL
        # an owner nobody created has nothing to invalidate or refresh
        assert L.dc_wino_cache_invalidate(unknown) == WC.EINVAL
        assert L.dc_wino_cache_refresh(unknown, None) == WC.EINVAL
        assert L.dc_wino_cache_invalidate(a) == OK and L.dc_wino_cache_invalidate(b) == OK
        # releasing a drops a's entries only: b's repeat still succeeds (and its entry still refuses other channels), the
        # released pointer is free again -- for the other owner, with other channels --, and a is no owner any more
        assert L.dc_wino_cache_release_owner(a) == OK
        assert L.dc_wino_cache_register(b, w1, 24, 8) == OK
        assert L.dc_wino_cache_register(b, w1, 8, 24) == WC.EINVAL
        assert L.dc_wino_cache_register(a, w2, 8, 8) == WC.EINVAL
        assert L.dc_wino_cache_invalidate(a) == WC.EINVAL
        assert L.dc_wino_cache_register(b, w0, 16, 8) == OK
        # no launch met any of these weights: not one prepared variant was added
        assert L.dc_wino_cache_variants() == variants
    finally:
        L.dc_wino_cache_release_owner(a)
        L.dc_wino_cache_release_owner(b)
    assert L.dc_wino_cache_variants() == variants
    del keep
