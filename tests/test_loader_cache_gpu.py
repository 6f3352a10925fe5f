"""BatchLoader(cache_bytes=...): with the frame cache on, the batches of every epoch are bit for bit those of the uncached
loader -- cold (frames decoded, resized into slots), warm (gathered from slots, nothing decoded), and with a cache that
holds only half the frames (the rest built in the overflow slots batch after batch)."""
import pytest
import torch

from kitti_tree import DRIVES, write_raw_tree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLOT = 8160                     # 32 x 64, four scales
FRAMES, ITEMS, BATCH = 3, 12, 2
OVERFLOW = FRAMES * BATCH


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    import datasets
    root = str(tmp_path_factory.mktemp("kitti"))
    write_raw_tree(root, frames=6)
    lines = ["%s %d l" % (drive, i) for drive in sorted(DRIVES) for i in range(6)]          # frames 0 and 5: a neighbour is missing
    return datasets.KITTIRAWDataset(root, lines, 32, 64, [0, -1, 1], 4, is_train=True, img_ext=".png")


def _epochs(dataset, prefetch, cache_bytes, epochs=2):
    """-> (loader, [batches of epoch 0, batches of epoch 1, ...], the cache's stats after every epoch)."""
    from depthcore.loader import BatchLoader
    ld = BatchLoader(dataset, BATCH, num_workers=4, device=DEV, seed=3, prefetch=prefetch, cache_bytes=cache_bytes)
    out, stats = [], []
    for e in range(epochs):
        ld.set_epoch(e)
        out.append(list(ld))
        torch.cuda.synchronize()
        stats.append(dict(ld.cache.stats) if ld.cache is not None else None)
    ld.close()
    return ld, out, stats


@pytest.fixture(scope="module")
def uncached(dataset):
    """The reference: two epochs of the loader as it is without a cache; computed once, left unchanged."""
    ld, out, _ = _epochs(dataset, 0, 0)
    assert ld.cache is None                                                  # cache_bytes=0: no cache object
    assert all(len(e) == ITEMS // BATCH for e in out)
    # the epochs contain flipped and jittered items, both drives' sizes inside one batch, and items whose neighbour is missing
    for e in range(2):
        plan = ld.plan(e)
        assert any(d[0] for _, draws in plan for d in draws) and any(d[1] is not None for _, draws in plan for d in draws)
        assert any(len({DRIVES[dataset.filenames[i].split()[0]] for i in idx}) == 2 for idx, _ in plan)
        assert any(not torch.equal(b[("color", 0, 0)], b[("color_aug", 0, 0)]) for b in out[e])
    assert sum(len(set(dataset.frame_paths(i))) < FRAMES for i in range(ITEMS)) == 4
    return out


def _same(got, want):
    assert len(got) == len(want)
    for e, (ge, we) in enumerate(zip(got, want)):
        assert len(ge) == len(we)
        for a, b in zip(ge, we):
            assert sorted(a, key=str) == sorted(b, key=str)
            for k in b:
                assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (e, k)


@pytest.mark.parametrize("prefetch", [0, 2])
def test_cold_and_warm_epochs_equal_the_uncached_loader(dataset, uncached, prefetch):
    ld, got, stats = _epochs(dataset, prefetch, (ITEMS + OVERFLOW) * SLOT)
    assert ld.cache.capacity == ITEMS
    _same(got, uncached)
    cold, warm = stats
    assert cold["inserted"] == ITEMS == len(ld.cache) and cold["bypassed"] == 0
    assert cold["hits"] + cold["misses"] == FRAMES * ITEMS and ITEMS <= cold["decoded"] <= cold["misses"]
    # epoch 1: every frame of every item is served from its slot, nothing is decoded
    assert warm["decoded"] == cold["decoded"] and warm["inserted"] == ITEMS
    assert warm["hits"] - cold["hits"] == FRAMES * ITEMS and warm["misses"] == cold["misses"]


def test_half_the_frames_fit_the_rest_goes_through_the_overflow_slots(dataset, uncached):
    ld, got, stats = _epochs(dataset, 2, (ITEMS // 2 + OVERFLOW) * SLOT)
    assert ld.cache.capacity == ITEMS // 2
    _same(got, uncached)
    assert stats[0]["inserted"] == stats[1]["inserted"] == ld.cache.capacity == len(ld.cache)
    assert stats[1]["decoded"] > stats[0]["decoded"] and stats[1]["hits"] > stats[0]["hits"]     # warm for half the frames only
    assert stats[1]["bypassed"] == 0


def test_held_batch_survives_further_fetches(dataset):
    """The overflow slots are rewritten by every later batch; a batch that was handed out does not live in them."""
    from depthcore.loader import BatchLoader
    ld = BatchLoader(dataset, BATCH, num_workers=4, device=DEV, seed=3, prefetch=2, cache_bytes=(1 + OVERFLOW) * SLOT)
    it = iter(ld)
    held = next(it)
    torch.cuda.synchronize()
    copy = {k: v.clone() for k, v in held.items()}
    next(it), next(it)
    torch.cuda.synchronize()
    for k in held:
        assert torch.equal(held[k], copy[k]), k
    it.close()
    ld.close()


def test_a_width_that_fails_the_gate_is_not_cached(dataset, uncached, monkeypatch):
    """A native width whose table were not mirror-symmetric: batches that hold such an item take the uncached path."""
    from depthcore import frame_cache
    monkeypatch.setattr(frame_cache.FrameCache, "symmetric", lambda self, width: width != 150)
    ld, got, stats = _epochs(dataset, 2, (ITEMS + OVERFLOW) * SLOT, epochs=1)
    _same(got, uncached[:1])
    assert stats[0]["bypassed"] > 0 and stats[0]["bypassed"] % (FRAMES * BATCH) == 0
    assert all("drive_0002" not in path for path in ld.cache.slots) and len(ld.cache) <= ITEMS // 2
