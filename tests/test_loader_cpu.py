"""depthcore.loader.BatchLoader, host half (no GPU): the sampler is a function of (seed, epoch), shards partition the epoch,
the draws are sample_item's in item order, decode_batch packs the frames where GpuPreprocessor.ragged expects them."""
import numpy as np

from kitti_tree import DRIVES, write_raw_tree

DRIVE_A, DRIVE_B = sorted(DRIVES)


class _Names:
    """A dataset as far as the sampler is concerned: a length and is_train."""

    def __init__(self, n, is_train=True):
        self.n, self.is_train = n, is_train

    def __len__(self):
        return self.n


def _loader(n=23, batch=4, **kw):
    from depthcore.loader import BatchLoader
    return BatchLoader(_Names(n, kw.pop("is_train", True)), batch, device="cpu", **kw)


def test_same_seed_and_epoch_same_plan():
    a, b = _loader(seed=5), _loader(seed=5)
    assert len(a) == 23 // 4
    assert a.plan(3) == b.plan(3)
    a.set_epoch(3)
    assert a.plan() == b.plan(3)
    flat = [i for idx, _ in a.plan(3) for i in idx]
    assert len(flat) == 20 and len(set(flat)) == 20 and set(flat) <= set(range(23))        # drop_last, no repeats
    assert [idx for idx, _ in a.plan(3)] != [idx for idx, _ in a.plan(4)]                  # another epoch, another order
    assert [idx for idx, _ in a.plan(3)] != [idx for idx, _ in _loader(seed=6).plan(3)]    # another seed too
    assert flat != sorted(flat)
    assert [i for idx, _ in _loader(seed=5, shuffle=False).plan(3) for i in idx] == list(range(20))


def test_draws_are_sample_item_in_item_order():
    from depthcore.data import sample_item
    from depthcore.loader import epoch_rng
    ld = _loader(n=23, batch=4, seed=2)
    plan = ld.plan(7)
    rng = epoch_rng(2, 7)
    order = list(range(23))
    rng.shuffle(order)
    want = [sample_item(True, rng) for _ in range(20)]
    assert [i for idx, _ in plan for i in idx] == order[:20]
    assert [d for _, draws in plan for d in draws] == want
    assert any(d[0] for d in want) and any(d[1] is not None for d in want) and any(d[1] is None for d in want)
    # a loader that does not train draws nothing, and consumes nothing of the generator beyond the permutation
    val = _loader(n=23, batch=4, seed=2, is_train=False).plan(7)
    assert [i for idx, _ in val for i in idx] == order[:20]
    assert all(d == (False, None) for _, draws in val for d in draws)


def test_two_rank_shards_partition_the_epoch():
    single = [i for idx, _ in _loader(n=24, batch=2, seed=1).plan(4) for i in idx]
    shards = [_loader(n=24, batch=2, seed=1, rank=r, world_size=2) for r in (0, 1)]
    flat = [[i for idx, _ in s.plan(4) for i in idx] for s in shards]
    assert len(shards[0]) == len(shards[1]) == 6
    assert len(flat[0]) == len(flat[1]) == 12 and not set(flat[0]) & set(flat[1])
    assert flat[0] == single[0::2] and flat[1] == single[1::2]                    # strided shards of the same permutation
    assert sorted(flat[0] + flat[1]) == sorted(single) == list(range(24))         # their union is the single-rank epoch
    # an odd item count: both ranks still take the same number of steps
    odd = [_loader(n=9, batch=2, seed=1, rank=r, world_size=2) for r in (0, 1)]
    assert len(odd[0]) == len(odd[1]) == 2 and all(len(o.plan(0)) == 2 for o in odd)


def test_thread_count_is_bounded_by_the_option_not_the_machine():
    assert _loader(num_workers=12).threads == 12
    assert _loader(num_workers=64).threads == 16
    assert _loader(num_workers=0).threads == 1


def test_decode_batch_packing_and_offsets(tmp_path):
    """Frame-major packing: image f * B + b at the running offset, each (Hn_b, Wn_b, 3); a missing neighbour holds frame 0."""
    import datasets
    from depthcore.loader import BatchLoader
    px = write_raw_tree(str(tmp_path), frames=4)
    lines = ["%s 1 l" % DRIVE_A, "%s 0 l" % DRIVE_B, "%s 2 l" % DRIVE_A, "%s 2 l" % DRIVE_B]
    ds = datasets.KITTIRAWDataset(str(tmp_path), lines, 32, 64, [0, -1, 1], 4, is_train=True, img_ext=".png")
    ld = BatchLoader(ds, 3, num_workers=4, device="cpu")
    indices = [3, 0, 1]
    draws = [(True, None), (False, ((0, 1, 2, 3), (1.0, 1.1, 0.9, 0.05))), (True, None)]
    buf, sizes, flips, jitters, extras = ld.decode_batch(indices, draws)
    assert sizes == [DRIVES[DRIVE_B], DRIVES[DRIVE_A], DRIVES[DRIVE_B]]
    assert flips == [True, False, True] and jitters == [None, draws[1][1], None] and extras == {}
    assert buf.dtype == np.uint8 and buf.ndim == 1 and buf.size == 3 * sum(h * w * 3 for h, w in sizes)
    want = {(3, 0): (DRIVE_B, 2), (3, -1): (DRIVE_B, 1), (3, 1): (DRIVE_B, 3),
            (0, 0): (DRIVE_A, 1), (0, -1): (DRIVE_A, 0), (0, 1): (DRIVE_A, 2),
            (1, 0): (DRIVE_B, 0), (1, -1): (DRIVE_B, 0), (1, 1): (DRIVE_B, 1)}       # item 1 is frame 0: no frame -1
    off = 0
    for f in (0, -1, 1):
        for b, idx in enumerate(indices):
            h, w = sizes[b]
            drive, frame = want[(idx, f)]
            assert np.array_equal(buf[off:off + h * w * 3].reshape(h, w, 3), px[(drive, frame, "l")]), (f, b)   # not mirrored
            off += h * w * 3
    assert off == buf.size
    # into a caller's buffer (the loader's pinned staging): the same bytes, in place
    out = np.zeros(buf.size + 100, np.uint8)
    buf2 = ld.decode_batch(indices, draws, out=out)[0]
    assert np.shares_memory(buf2, out) and np.array_equal(buf2, buf) and not out[buf.size:].any()
    # default draws: nothing flipped, nothing jittered
    assert ld.decode_batch([0])[2:4] == ([False], [None])
    ld.close()


def test_decode_batch_carries_stereo_T(tmp_path):
    import datasets
    from depthcore.loader import BatchLoader
    write_raw_tree(str(tmp_path), frames=2, sides=("l", "r"))
    ds = datasets.KITTIRAWDataset(str(tmp_path), ["%s 1 l" % DRIVE_A, "%s 1 r" % DRIVE_B], 32, 64, [0, "s"], 4, is_train=True,
                                  img_ext=".png")
    ld = BatchLoader(ds, 2, num_workers=2, device="cpu")
    extras = ld.decode_batch([0, 1], [(True, None), (False, None)])[4]
    assert sorted(extras) == ["stereo_T"] and extras["stereo_T"].shape == (2, 4, 4)
    assert extras["stereo_T"][0, 0, 3] == np.float32(0.1) and extras["stereo_T"][1, 0, 3] == np.float32(0.1)
    ld.close()


def test_decode_packed_offsets_sizes_and_missing_file(tmp_path):
    """Two PNGs of different sizes -> their RGB bytes back to back in the order given, the sizes per file; a missing file
    is named in a FileNotFoundError."""
    import pytest
    from PIL import Image

    from depthcore.loader import decode_packed
    rng = np.random.RandomState(3)
    imgs = [rng.randint(0, 256, (5, 7, 3)).astype(np.uint8), rng.randint(0, 256, (4, 9, 3)).astype(np.uint8)]
    paths = []
    for k, img in enumerate(imgs):
        paths.append(str(tmp_path / "d" / ("%d.png" % k)))
        (tmp_path / "d").mkdir(exist_ok=True)
        Image.fromarray(img).save(paths[-1])
    packed, sizes = decode_packed([paths[1], paths[0], paths[1]])
    assert packed.dtype == np.uint8 and packed.ndim == 1 and packed.size == 2 * 4 * 9 * 3 + 5 * 7 * 3
    assert [tuple(s) for s in sizes] == [(4, 9), (5, 7), (4, 9)]
    off = 0
    for (h, w), k in zip(sizes, (1, 0, 1)):
        assert np.array_equal(packed[off:off + h * w * 3].reshape(h, w, 3), imgs[k])
        off += h * w * 3
    missing = str(tmp_path / "d" / "2.png")
    with pytest.raises(FileNotFoundError, match="image .*2.png of the split does not exist"):
        decode_packed([paths[0], missing])
