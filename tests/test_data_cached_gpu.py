"""dc_data_cached_levels / GpuPreprocessor.cached: a batch gathered from cache slots that hold UNFLIPPED resized pyramids --
every key equals oracle/data_ref.preprocess_item of the native frame with the item's flip and jitter (torch.equal: the
comparison of tests/test_data_ragged_gpu.py), the mirror applied while the slot is read."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import data_case_image
from oracle import data_ref as D

pytestmark = pytest.mark.gpu

# contrast first / hue in front of contrast, contrast last (its mean is taken behind three steps, per level) / no jitter
JITTERS = [((1, 0, 2, 3), (1.17, 0.83, 0.91, 0.093)), ((0, 2, 3, 1), (0.85, 1.2, 1.1, -0.07)), None]
FLIPS = [True, False, False]
# shape -> (native sizes of the slots' frames, frame_idxs, slot of every image): three items each, so n = 6, 6 and 3 images.
# 32 x 64 is the smallest (level 3 is 4 x 8), 32 x 96 has level-3 rows of 36 bytes, 192 x 640 is the real slot size (many
# blocks per image).  Slots are out of order, and one slot serves a flipped and an unflipped image.
CASES = {(32, 64): ([(47, 155), (45, 150), (47, 155), (45, 150)], (0, -1), [2, 0, 3, 1, 2, 0]),
         (32, 96): ([(47, 155), (45, 150), (47, 155), (45, 150)], (0, 1), [3, 1, 0, 2, 3, 1]),
         (192, 640): ([(375, 1242), (370, 1224)], (0,), [1, 0, 1])}
B = 3


def _dev():
    return torch.device("cuda:0")


def _case(h, w):
    """Slots filled from the oracle's pyramids of UNFLIPPED native images -> (native, device arena, frame_idxs, slots)."""
    from depthcore.data import slot_layout
    from depthcore.frame_cache import tables_mirror_symmetric
    sizes, frames, slots = CASES[(h, w)]
    offsets, slot_bytes = slot_layout(h, w, 4)
    native = [data_case_image(hn, wn, 700 + 7 * k + h) for k, (hn, wn) in enumerate(sizes)]
    assert all(tables_mirror_symmetric(wn, w) for _, wn in sizes)
    arena = np.zeros(len(sizes) * slot_bytes + 5, np.uint8)                   # (a tail the last slot must not need)
    for k, img in enumerate(native):
        for s in range(4):
            img = D.resize_lanczos(img, h >> s, w >> s)
            arena[k * slot_bytes + offsets[s]:][:img.size] = img.reshape(-1)
    # the mix every shape carries: two images of one slot with different flips, slots out of order
    flip_of = [FLIPS[i % B] for i in range(len(slots))]
    assert len(slots) == len(frames) * B and slots != sorted(slots)
    assert any(slots[i] == slots[j] and flip_of[i] != flip_of[j] for i in range(len(slots)) for j in range(i))
    return native, torch.from_numpy(arena).to(_dev()), frames, slots


@pytest.fixture(scope="module")
def wanted():
    """oracle results, computed once per (shape, slot, flip, jitter)."""
    memo = {}

    def get(h, w, native, slot, flip, jitter):
        key = (h, w, slot, flip, jitter)
        if key not in memo:
            memo[key] = D.preprocess_item(native[slot], h, w, 4, flip, jitter)
        return memo[key]
    return get


def _check(out, wanted, h, w, native, frames, slots, flips, jitters):
    from depthcore import ops
    assert len(out) == 2 * len(frames) * 4 + len(frames)
    for i, f in enumerate(frames):
        pk = out[("color_packed", f, 0)]
        assert pk.shape == (B, h, w, 4) and pk.is_contiguous() and pk.data_ptr() % 16 == 0
        assert torch.equal(pk, ops.pack_rgbx(out[("color", f, 0)]))
        for b in range(B):
            want = wanted(h, w, native, slots[i * B + b], bool(flips[b]) if flips else False, jitters[b] if jitters else None)
            for s in range(4):
                for n in ("color", "color_aug"):
                    got = out[(n, f, s)]
                    assert got.shape == (B, 3, h >> s, w >> s) and got.dtype == torch.float32 and got.is_contiguous()
                    assert torch.equal(got[b].cpu(), torch.from_numpy(want[(n, s)])), (b, f, s, n)


@pytest.mark.parametrize("shape", sorted(CASES))
def test_every_key_vs_oracle(shape, wanted):
    from depthcore.data import GpuPreprocessor
    h, w = shape
    native, arena, frames, slots = _case(h, w)
    pre = GpuPreprocessor(h, w, num_scales=4, frame_idxs=frames, device=_dev())
    out = pre.cached(arena, slots, FLIPS, JITTERS)
    _check(out, wanted, h, w, native, frames, slots, FLIPS, JITTERS)
    assert out[("color_aug", 0, 0)].data_ptr() != out[("color", 0, 0)].data_ptr()


def test_no_jitter_means_color_aug_is_color(wanted):
    """color_aug = NULL: the write pass alone, and the dict's color_aug entries ARE the color tensors, as in `__call__`."""
    from depthcore.data import GpuPreprocessor
    h, w = 32, 64
    native, arena, frames, slots = _case(h, w)
    pre = GpuPreprocessor(h, w, num_scales=4, frame_idxs=frames, device=_dev())
    out = pre.cached(arena, slots, FLIPS, None)
    _check(out, wanted, h, w, native, frames, slots, FLIPS, None)
    assert out[("color_aug", -1, 2)].data_ptr() == out[("color", -1, 2)].data_ptr()
    plain = pre.cached(arena, slots)
    _check(plain, wanted, h, w, native, frames, slots, None, None)


def test_packed_null_and_rgbx_of_the_same_level():
    """The C entry with color_aug = packed = NULL writes the planar tensors alone, the same values; with packed,
    ("color_packed", f, 0) equals dc_data_to_rgbx of the scale-0 level the slot holds (mirrored where the item is flipped)."""
    from depthcore import _lib
    from depthcore.data import CACHED_IMG, GpuPreprocessor, slot_layout
    L = _lib.lib()
    h, w = 32, 96
    _, arena, frames, slots = _case(h, w)
    n = len(slots)
    _, slot_bytes = slot_layout(h, w, 4)
    pre = GpuPreprocessor(h, w, num_scales=4, frame_idxs=frames, device=_dev())
    full = pre.cached(arena, slots, FLIPS, JITTERS)
    desc = np.zeros(n, CACHED_IMG)
    desc["slot_off"] = np.asarray(slots, np.int64) * slot_bytes
    desc["flip"] = np.tile(np.asarray(FLIPS, bool), len(frames))
    desc_d = torch.from_numpy(desc.view(np.uint8)).to(_dev())
    color = [torch.full((n, 3, h >> s, w >> s), -1.0, device=_dev()) for s in range(4)]
    ptrs = (ctypes.c_void_p * 4)(*[c.data_ptr() for c in color])
    rc = L.dc_data_cached_levels(arena.data_ptr(), arena.numel(), desc.ctypes.data, desc_d.data_ptr(), n, h, w, 4, ptrs, None, None,
                                 None, None, None, _lib.stream(arena))
    assert rc == 0
    for s in range(4):
        assert torch.equal(color[s], torch.cat([full[("color", f, s)] for f in frames])), s
    level0 = arena.cpu().numpy()
    imgs = np.stack([level0[sl * slot_bytes:][:h * w * 3].reshape(h, w, 3)[:, ::-1 if FLIPS[i % B] else 1] for i, sl in enumerate(slots)])
    u8 = torch.from_numpy(np.ascontiguousarray(imgs)).to(_dev())
    rgbx = torch.empty((n, h, w, 4), dtype=torch.float32, device=_dev())
    assert L.dc_data_to_rgbx(u8.data_ptr(), rgbx.data_ptr(), n, h * w, _lib.stream(u8)) == 0
    assert torch.equal(rgbx, torch.cat([full[("color_packed", f, 0)] for f in frames]))


def test_slot_outside_the_arena_is_refused():
    from depthcore import _lib
    from depthcore.data import GpuPreprocessor, slot_layout
    h, w = 32, 64
    _, slot_bytes = slot_layout(h, w, 4)
    arena = torch.zeros(3 * slot_bytes, dtype=torch.uint8, device=_dev())
    pre = GpuPreprocessor(h, w, num_scales=4, frame_idxs=(0,), device=_dev())
    with pytest.raises(_lib.DepthcoreError, match="DC_EINVAL"):
        pre.cached(arena, [0, 3])
    with pytest.raises(_lib.DepthcoreError, match="DC_EINVAL"):
        pre.cached(arena[:-1], [2])
    with pytest.raises(_lib.DepthcoreError):
        pre.cached(arena, [0, 1], flips=[True])
    assert pre.cached(arena, [2, 0])[("color", 0, 3)].shape == (2, 3, 4, 8)


def test_frame_cache_build_equals_the_uint8_chain_of_call():
    """FrameCache.build through GpuPreprocessor.ragged_resize: two frames of different native sizes into an overflow slot
    and slot 0, out of order; level s of each slot equals, byte for byte, the uint8 level that `__call__(..., flips=None)`
    converts -- `_resize` applied level after level -- and the slot between them is not touched."""
    from depthcore.data import GpuPreprocessor, slot_layout
    from depthcore.frame_cache import FrameCache
    h, w, S = 32, 64, 4
    sizes = [(47, 155), (45, 150)]
    offsets, slot_bytes = slot_layout(h, w, S)
    native = [data_case_image(hn, wn, 900 + k) for k, (hn, wn) in enumerate(sizes)]
    packed = torch.from_numpy(np.concatenate([img.reshape(-1) for img in native])).to(_dev())
    cache = FrameCache(h, w, S, 3 * slot_bytes, 1, _dev())
    assert cache.capacity == 2 and cache.overflow_slot(0) == 2
    cache.arena.fill_(7)
    frames = [(0, 47, 155, 2), (47 * 155 * 3, 45, 150, 0)]
    pre = GpuPreprocessor(h, w, num_scales=S, frame_idxs=(0,), device=_dev())
    cache.build(pre, packed, frames)
    arena = cache.arena
    for (off, hn, wn, slot), img in zip(frames, native):
        level = torch.from_numpy(img[None]).to(_dev())
        for s in range(S):
            level = pre._resize(level, h >> s, w >> s, None)
            got = arena[slot * slot_bytes + offsets[s]:][:level.numel()]
            assert torch.equal(got, level.view(-1)), (slot, s)
    assert bool((arena[slot_bytes:2 * slot_bytes] == 7).all())
