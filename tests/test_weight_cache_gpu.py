"""The prepared-weight cache (csrc/weight_cache.hip: dc_wino_cache_*) through the C ABI, one small shape per kind of prepared weight:
0 the Winograd U (dc_wino3x3_fwd / _dgrad), 1 the bf16 direct kernels' packed weights (the same entries under the bf16 policy), 2 the
split 1x1 weights (dc_gemm1x1x3_fwd / _dgrad).  A launch computes the same bits whether its weight is unregistered, registered but
not yet prepared by a refresh, read from the cache, or invalidated -- and a launch that reads the cache does not look at the weight.

The checker is the launch itself in another state: every comparison is bitwise (the cached and the per-launch preparation run the
same device function on the same values).  No graph capture here (tests/test_train_gpu.py holds that ground) and no
dc_wino_cache_clear (other tests' owners live in this process)."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

OK = 0
WINO = (2, 16, 24, 6, 20)           # B, Ci, Co, H, W
C3B = (2, 16, 24, 2, 4)             # the smallest map c3b_eligible accepts: H = 2, W = 4
G1X3 = (1, 32, 32, 4, 4)            # the smallest shape of dc_gemm1x1x3_fwd_ok (and _dgrad_ok): 32 channels, 16 pixels


def _L():
    from depthcore import _lib
    return _lib.lib()


def _st():
    from depthcore import _lib
    return _lib.stream()


def _data(shape, k, seed):
    """x, gy and a fresh weight.  (The registry keys on the weight's address: finalisers of earlier tests' caches run first, so that
    no owner that is already garbage still holds the address the allocator hands out here.)"""
    gc.collect()
    B, Ci, Co, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Ci, H, W, generator=g).cuda()
    gy = torch.randn(B, Co, H, W, generator=g).cuda()
    w = (torch.randn(Co, Ci, k, k, generator=g) * (2.0 / (k * k * Ci)) ** 0.5).cuda()
    return x, gy, w


def _conv3x3_launches(shape, x, gy):
    """dc_wino3x3_fwd and dc_wino3x3_dgrad on `shape` as functions of the weight tensor (kind 0; kind 1 under the bf16 policy)"""
    L = _L()
    B, Ci, Co, H, W = shape
    ws = torch.empty(L.dc_wino3x3_workspace(B, Ci, Co, H, W), dtype=torch.uint8, device="cuda")

    def fwd(w):
        y = torch.empty(B, Co, H, W, device="cuda")
        assert L.dc_wino3x3_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), ws.data_ptr(), B, Ci, Co, H, W, _st()) == OK
        return y

    def dgrad(w):
        gx = torch.empty(B, Ci, H, W, device="cuda")
        assert L.dc_wino3x3_dgrad(gy.data_ptr(), w.data_ptr(), gx.data_ptr(), ws.data_ptr(), B, Ci, Co, H, W, _st()) == OK
        return gx

    return [fwd, dgrad]


def _gemm1x1x3_launches(shape, x, gy):
    L = _L()
    B, Ci, Co, H, W = shape
    assert L.dc_gemm1x1x3_fwd_ok(B, Ci, Co, H, W, 1) == 1 and L.dc_gemm1x1x3_dgrad_ok(B, Ci, Co, H, W, 1) == 1
    for smaller in ((B, Ci - 1, Co, H, W), (B, Ci, Co - 1, H, W), (B, Ci, Co, H, W - 1), (B, Ci, Co, H - 1, W)):
        assert L.dc_gemm1x1x3_fwd_ok(*smaller, 1) == 0
    ws = torch.empty(L.dc_gemm1x1x3_workspace(Ci, Co), dtype=torch.uint8, device="cuda")

    def fwd(w):
        y = torch.empty(B, Co, H, W, device="cuda")
        assert L.dc_gemm1x1x3_fwd(x.data_ptr(), w.data_ptr(), None, y.data_ptr(), ws.data_ptr(), B, Ci, Co, H, W, 1, 0, _st()) == OK
        return y

    def dgrad(w):
        dx = torch.empty(B, Ci, H, W, device="cuda")
        assert L.dc_gemm1x1x3_dgrad(gy.data_ptr(), w.data_ptr(), dx.data_ptr(), ws.data_ptr(), None, None, B, Ci, Co, H, W, 1, _st()) == OK
        return dx

    return [fwd, dgrad]


def _four_states(owner, w, Ci, Co, launches):
    L = _L()
    n0 = L.dc_wino_cache_variants()
    # (a) unregistered: prepared per launch, nothing joins the cache
    ref = [f(w) for f in launches]
    assert L.dc_wino_cache_variants() == n0
    assert L.dc_wino_cache_register(owner, w.data_ptr(), Ci, Co) == OK
    assert L.dc_wino_cache_refresh(owner, _st()) == OK
    # (b) registered, the variant unseen: it gets its buffer (one more variant per launch) and is still prepared in place
    for f, r in zip(launches, ref):
        n = L.dc_wino_cache_variants()
        assert torch.equal(f(w), r)
        assert L.dc_wino_cache_variants() == n + 1
    n1 = L.dc_wino_cache_variants()
    assert n1 == n0 + len(launches)
    # (c) after the next refresh: from the cache
    assert L.dc_wino_cache_refresh(owner, _st()) == OK
    for f, r in zip(launches, ref):
        assert torch.equal(f(w), r)
    # ... really from the cache: the weight changes under it (x 2 and x 0.5 are exact) and the launches do not notice, until
    # the owner invalidates -- then they compute what an unregistered copy of the new weight gives
    w.mul_(2.0)
    changed = [f(w.clone()) for f in launches]
    for f, r, c in zip(launches, ref, changed):
        assert not torch.equal(c, r)
        assert torch.equal(f(w), r)
    assert L.dc_wino_cache_invalidate(owner) == OK
    for f, c in zip(launches, changed):
        assert torch.equal(f(w), c)
    w.mul_(0.5)
    # (d) invalidated: prepared per launch again
    for f, r in zip(launches, ref):
        assert torch.equal(f(w), r)
    assert L.dc_wino_cache_variants() == n1
    return ref


def test_winograd_weights_in_four_states():
    L = _L()
    x, gy, w = _data(WINO, 3, 1)
    owner = L.dc_wino_cache_new_owner()
    try:
        _four_states(owner, w, WINO[1], WINO[2], _conv3x3_launches(WINO, x, gy))
    finally:
        L.dc_wino_cache_release_owner(owner)
        torch.cuda.synchronize()


def test_bf16_prepared_weights_in_four_states():
    from depthcore import _lib
    L = _L()
    x, gy, w = _data(C3B, 3, 2)
    launches = _conv3x3_launches(C3B, x, gy)
    f32 = launches[0](w)
    owner = L.dc_wino_cache_new_owner()
    prev = L.dc_set_matrix_precision(_lib.PREC_BF16)
    try:
        assert prev in (_lib.PREC_F32, _lib.PREC_BF16)
        ref = _four_states(owner, w, C3B[1], C3B[2], launches)
        assert not torch.equal(ref[0], f32)           # (the policy took: these were the bf16 kernels)
    finally:
        L.dc_set_matrix_precision(prev)
        L.dc_wino_cache_release_owner(owner)
        torch.cuda.synchronize()


def test_split_1x1_weights_in_four_states():
    L = _L()
    x, gy, w = _data(G1X3, 1, 3)
    owner = L.dc_wino_cache_new_owner()
    prev = L.dc_set_gemm_split(1)
    try:
        _four_states(owner, w, G1X3[1], G1X3[2], _gemm1x1x3_launches(G1X3, x, gy))
    finally:
        L.dc_set_gemm_split(prev)
        L.dc_wino_cache_release_owner(owner)
        torch.cuda.synchronize()


def test_releasing_one_owner_leaves_the_other_alone():
    L = _L()
    x, gy, wa = _data(WINO, 3, 4)
    wb = _data(WINO, 3, 5)[2]
    launches = _conv3x3_launches(WINO, x, gy)
    n0 = L.dc_wino_cache_variants()
    a, b = L.dc_wino_cache_new_owner(), L.dc_wino_cache_new_owner()
    try:
        ref = {}
        for owner, w in ((a, wa), (b, wb)):
            ref[owner] = [f(w) for f in launches]
            assert L.dc_wino_cache_register(owner, w.data_ptr(), WINO[1], WINO[2]) == OK
            assert L.dc_wino_cache_refresh(owner, _st()) == OK
            for f in launches:
                f(w)                                  # the variants are met ...
            assert L.dc_wino_cache_refresh(owner, _st()) == OK      # ... and prepared
        assert L.dc_wino_cache_variants() == n0 + 2 * len(launches)
        assert L.dc_wino_cache_release_owner(a) == OK
        assert L.dc_wino_cache_variants() == n0 + len(launches)      # b's are all there
        # b still reads its cache (its weight changes under it, unnoticed), with the results it had
        wb.mul_(2.0)
        for f, r in zip(launches, ref[b]):
            assert torch.equal(f(wb), r)
        wb.mul_(0.5)
        # the released weight is an unregistered weight again: prepared per launch, correct, and it joins nothing
        wa.mul_(2.0)
        changed = [f(wa.clone()) for f in launches]
        for f, r, c in zip(launches, ref[a], changed):
            assert torch.equal(f(wa), c) and not torch.equal(c, r)
        wa.mul_(0.5)
        for f, r in zip(launches, ref[a]):
            assert torch.equal(f(wa), r)
        assert L.dc_wino_cache_variants() == n0 + len(launches)
        assert L.dc_wino_cache_refresh(a, _st()) != OK
    finally:
        L.dc_wino_cache_release_owner(a)
        L.dc_wino_cache_release_owner(b)
        torch.cuda.synchronize()
    assert L.dc_wino_cache_variants() == n0
