"""GpuPreprocessor.ragged (dc_data_ragged_resize_axis): a batch whose items have different native sizes, two launches for
scale 0 -- every byte equals oracle/data_ref.preprocess_item applied per frame (torch.equal), and the uniform path."""
import numpy as np
import pytest
import torch

from helpers import data_case_image
from oracle import data_ref as D

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _batch(sizes, frames, seed):
    """native[f][b]: (Hn_b, Wn_b, 3) uint8, and the packed frame-major device buffer."""
    native = [[data_case_image(h, w, seed + 10 * f + b) for b, (h, w) in enumerate(sizes)] for f in range(frames)]
    packed = np.concatenate([img.reshape(-1) for row in native for img in row])
    return native, torch.from_numpy(packed).to(_dev())


def _check(out, native, sizes, frame_idxs, h, w, scales, flips, jitters):
    from depthcore import ops
    B = len(sizes)
    assert len(out) == 2 * len(frame_idxs) * scales + len(frame_idxs)
    for i, f in enumerate(frame_idxs):
        pk = out[("color_packed", f, 0)]
        assert pk.shape == (B, h, w, 4) and pk.is_contiguous() and pk.data_ptr() % 16 == 0
        assert torch.equal(pk, ops.pack_rgbx(out[("color", f, 0)]))
        for b in range(B):
            want = D.preprocess_item(native[i][b], h, w, scales, bool(flips[b]) if flips else False, jitters[b] if jitters else None)
            for s in range(scales):
                for n in ("color", "color_aug"):
                    got = out[(n, f, s)]
                    assert got.shape == (B, 3, h >> s, w >> s) and got.dtype == torch.float32 and got.is_contiguous()
                    assert torch.equal(got[b].cpu(), torch.from_numpy(want[(n, s)])), (b, f, s, n)


def test_mixed_batch_every_key_vs_oracle():
    """(50, 64) has the target width and is flipped: the mirrored-copy branch of the width pass; (32, 140) has the target
    height: the copy branch of the height pass."""
    from depthcore.data import GpuPreprocessor
    sizes = [(47, 155), (45, 150), (50, 64), (32, 140)]
    frame_idxs, h, w, scales = (0, -1, 1), 32, 64, 3
    flips = [1, 0, 1, 1]
    jitters = [((3, 0, 1, 2), (0.83, 1.17, 0.91, 0.093)), None, ((1, 2, 0, 3), (1.2, 0.8, 1.2, -0.1)), None]
    native, packed = _batch(sizes, 3, 300)
    pre = GpuPreprocessor(h, w, num_scales=scales, frame_idxs=frame_idxs, device=_dev())
    out = pre.ragged(packed, sizes, flips, jitters)
    _check(out, native, sizes, frame_idxs, h, w, scales, flips, jitters)
    assert out[("color_aug", 0, 0)].data_ptr() != out[("color", 0, 0)].data_ptr()
    # nothing flipped, nothing jittered: the (50, 64) item takes the plain-copy branch, color_aug IS color
    plain = pre.ragged(packed, sizes)
    _check(plain, native, sizes, frame_idxs, h, w, scales, None, None)
    assert plain[("color_aug", 1, 2)].data_ptr() == plain[("color", 1, 2)].data_ptr()


def test_two_tables_of_different_ksize_in_one_launch():
    """An upscaled item (20, 40) -> 32 x 64 (ksize 7 on both axes) next to a 3x downscaled one (ksize 19)."""
    from depthcore import _lib
    from depthcore.data import GpuPreprocessor
    sizes = [(20, 40), (96, 192), (20, 40)]
    L = _lib.lib()
    assert L.dc_resample_ksize(40, 64) == 7 and L.dc_resample_ksize(192, 64) == 19
    native, packed = _batch(sizes, 1, 400)
    flips = [True, True, False]
    pre = GpuPreprocessor(32, 64, num_scales=1, frame_idxs=(0,), device=_dev())
    out = pre.ragged(packed, sizes, flips, None)
    _check(out, native, sizes, (0,), 32, 64, 1, flips, None)


def test_block_walk_at_kitti_sizes():
    """192 x 640 from (375, 1242) and (370, 1224): three x-blocks with a ragged tail (640 = 2 * 256 + 128); rows 370..374
    exist for the first image only (the other's blocks above its height return)."""
    from depthcore.data import GpuPreprocessor
    sizes = [(375, 1242), (370, 1224)]
    native, packed = _batch(sizes, 1, 500)
    flips = [False, True]
    pre = GpuPreprocessor(192, 640, num_scales=1, frame_idxs=(0,), device=_dev())
    out = pre.ragged(packed, sizes, flips, None)
    _check(out, native, sizes, (0,), 192, 640, 1, flips, None)


def test_uniform_batch_equals_call_byte_for_byte():
    from depthcore.data import GpuPreprocessor
    sizes = [(47, 155)] * 3
    frame_idxs = (0, -1, 1)
    native, packed = _batch(sizes, 3, 600)
    flips = [True, False, True]
    jitters = [None, ((2, 3, 1, 0), (0.9, 1.1, 1.15, -0.04)), ((0, 1, 2, 3), (1.1, 0.85, 0.95, 0.07))]
    pre = GpuPreprocessor(32, 64, num_scales=4, frame_idxs=frame_idxs, device=_dev())
    want = pre(packed.view(3, 3, 47, 155, 3), flips, jitters)
    got = pre.ragged(packed, sizes, flips, jitters)
    assert sorted(got, key=str) == sorted(want, key=str)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k


def test_descriptors_outside_the_buffer_are_refused_before_any_launch():
    """DC_EINVAL (-1) from the host-side check, the destination untouched: an image past the end of src, one past the end
    of dst, a table of another size, a tap outside the image, a flip on the height pass; and ragged() refuses a buffer
    that is shorter than its sizes say."""
    from depthcore import _lib
    from depthcore.data import RAGGED_IMG, GpuPreprocessor, resample_table
    L = _lib.lib()
    dev = _dev()
    Hi, Wi, Wo = 8, 40, 16
    bounds, kk = resample_table(Wi, Wo)
    tab = np.array([[0, 0, kk.shape[1], Wi]], np.int32)
    src = torch.zeros(2 * Hi * Wi * 3, dtype=torch.uint8, device=dev)
    dst = torch.full((2 * Hi * Wo * 3,), 7, dtype=torch.uint8, device=dev)
    tab_d, bounds_d, kk_d = (torch.from_numpy(a).to(dev) for a in (tab, bounds, kk))

    def call(desc, axis=1, tab=tab, bounds=bounds, src_bytes=src.numel(), dst_bytes=dst.numel()):
        desc_d = torch.from_numpy(desc.view(np.uint8)).to(dev)
        return L.dc_data_ragged_resize_axis(src.data_ptr(), src_bytes, dst.data_ptr(), dst_bytes, desc.ctypes.data, desc_d.data_ptr(),
                                            len(desc), Wo, axis, tab.ctypes.data, tab_d.data_ptr(), 1, bounds.ctypes.data,
                                            bounds_d.data_ptr(), bounds.size, kk_d.data_ptr(), kk.size, _lib.stream(src))

    def desc(**kw):
        d = np.zeros(2, RAGGED_IMG)
        d[0] = (0, 0, Hi, Wi, 0, 0)
        d[1] = (Hi * Wi * 3, Hi * Wo * 3, Hi, Wi, 0, 1)
        for k, v in kw.items():
            d[1][k] = v
        return d
    bad_bounds = bounds.copy()
    bad_bounds[-1, 0] = Wi - 1                                         # the last output pixel's taps run past the row
    refused = [call(desc(src_off=Hi * Wi * 3 + 1)), call(desc(dst_off=Hi * Wo * 3 + 1)), call(desc(Hi=Hi + 1)), call(desc(src_off=-1)),
               call(desc(Wi=Wi + 1)), call(desc(table=1)), call(desc(table=-1)), call(desc(), src_bytes=src.numel() - 1),
               call(desc(), dst_bytes=dst.numel() - 1), call(desc(), bounds=bad_bounds), call(desc(), axis=0), call(desc(), axis=2)]
    torch.cuda.synchronize()
    assert refused == [-1] * len(refused), refused
    assert bool((dst == 7).all())
    assert call(desc()) == 0                                             # and the untouched descriptors are accepted
    torch.cuda.synchronize()
    assert not bool((dst == 7).all())
    pre = GpuPreprocessor(32, 64, num_scales=1, frame_idxs=(0,), device=dev)
    short = torch.zeros(47 * 155 * 3 - 1, dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.DepthcoreError, match="DC_EINVAL"):
        pre.ragged(short, [(47, 155)])
    with pytest.raises(_lib.DepthcoreError):
        pre.ragged(short.view(1, -1), [(47, 155)])


@pytest.mark.parametrize("native_size", [(32, 64), (40, 64), (32, 80)])
def test_call_equals_ragged_where_level_0_skips_a_pass(native_size):
    """`__call__` makes level 0 with `_resize` carrying the mirror and hands it to the level loop `ragged` uses: every key
    equals `ragged`'s on the same bytes.  (32, 64) is the target -- no resize pass, the mirror goes through dc_data_flip;
    (40, 64) -- the height pass only, the mirror through dc_data_flip; (32, 80) -- the width pass only, carrying it."""
    from depthcore.data import GpuPreprocessor
    hn, wn = native_size
    sizes, frame_idxs = [native_size] * 2, (0, -1, 1)
    flips, jitters = [True, False], [((2, 3, 1, 0), (0.9, 1.1, 1.15, -0.04)), None]
    _, packed = _batch(sizes, 3, 800)
    pre = GpuPreprocessor(32, 64, num_scales=4, frame_idxs=frame_idxs, device=_dev())
    want = pre.ragged(packed, sizes, flips, jitters)
    got = pre(packed.view(3, 2, hn, wn, 3), flips, jitters)
    assert len(want) == 2 * 3 * 4 + 3 and sorted(got, key=str) == sorted(want, key=str)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    assert not torch.equal(got[("color", 0, 0)][0], got[("color_aug", 0, 0)][0])        # item 0 is jittered, item 1 is not
    assert torch.equal(got[("color", 0, 0)][1], got[("color_aug", 0, 0)][1])
