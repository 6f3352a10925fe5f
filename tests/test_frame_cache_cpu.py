"""depthcore.frame_cache without a GPU: the mirror-symmetry gate of the Lanczos tables, the fill-until-full index and its
stats, the slot layout, and the host-side refusals of dc_data_cached_levels (DC_EINVAL before anything is launched)."""
import ctypes

import numpy as np
import pytest

from oracle import data_ref as D

SLOT_192_640 = 489600


@pytest.mark.parametrize("sizes", [(1242, 640), (1224, 640), (1226, 640), (1238, 640), (1241, 640), (1242, 1024), (1224, 1024),
                                   (1226, 1024), (1238, 1024), (1241, 1024), (155, 64), (150, 64), (640, 80), (64, 8), (64, 64)])
def test_tables_are_mirror_symmetric(sizes):
    from depthcore.frame_cache import tables_mirror_symmetric, tables_symmetric
    assert tables_mirror_symmetric(*sizes) is True
    if sizes[0] != sizes[1]:
        assert tables_symmetric(*D.resample_coeffs(*sizes), sizes[0])        # and the oracle's own table


def test_one_changed_tap_or_bound_is_not_symmetric():
    from depthcore.data import resample_table
    from depthcore.frame_cache import tables_symmetric
    bounds, kk = resample_table(155, 64)
    assert tables_symmetric(bounds, kk, 155)
    tap = kk.copy()
    tap[10, 3] += 1
    assert not tables_symmetric(bounds, tap, 155)
    shifted = bounds.copy()
    shifted[5, 0] += 1
    assert not tables_symmetric(shifted, kk, 155)
    count = bounds.copy()
    count[-1, 1] -= 1
    assert not tables_symmetric(count, kk, 155)
    assert not tables_symmetric(bounds, kk, 156)                             # the table of another axis length


def test_mirror_commutes_with_the_pyramid_on_the_oracle():
    """What the gate stands for: resize(flip(x)) == flip(resize(x)) at every level, byte for byte."""
    rng = np.random.RandomState(0)
    for hn, wn in ((47, 155), (45, 150)):
        img = rng.randint(0, 256, (hn, wn, 3)).astype(np.uint8)
        a, b = img, img[:, ::-1]
        for s in range(4):
            a, b = D.resize_lanczos(a, 32 >> s, 64 >> s), D.resize_lanczos(b, 32 >> s, 64 >> s)
            assert np.array_equal(a[:, ::-1], b), (wn, s)


def test_slot_layout():
    from depthcore import _lib
    from depthcore.data import slot_layout
    offsets, total = slot_layout(192, 640, 4)
    assert offsets == [0, 368640, 368640 + 92160, 368640 + 92160 + 23040] and total == SLOT_192_640
    assert slot_layout(32, 64, 4) == ([0, 6144, 7680, 8064], 8160)
    assert slot_layout(32, 96, 1) == ([0], 9216)
    for bad in ((36, 64, 4), (32, 68, 4), (32, 64, 0), (32, 64, 5)):
        with pytest.raises(_lib.DepthcoreError):
            slot_layout(*bad)


def test_index_fills_until_full_and_counts():
    from depthcore.frame_cache import FrameCache
    overflow = 6
    c = FrameCache(192, 640, 4, (overflow + 3) * SLOT_192_640 + 17, overflow)
    assert c.slot_bytes == SLOT_192_640 and c.capacity == 3 and c.overflow == overflow and len(c) == 0
    assert c.lookup("a") is None
    assert [c.insert(p) for p in ("a", "b", "a", "c")] == [0, 1, 0, 2]           # a path that is present keeps its slot
    assert c.insert("d") is None and c.lookup("d") is None and len(c) == 3      # full: nothing is inserted, nothing evicted
    assert [c.lookup(p) for p in ("a", "b", "c")] == [0, 1, 2]
    assert c.stats == {"hits": 0, "misses": 0, "decoded": 0, "inserted": 3, "bypassed": 0}
    # the overflow slots lie behind the capacity, inside the budget
    assert [c.overflow_slot(k) for k in range(overflow)] == list(range(3, 3 + overflow))
    assert (c.overflow_slot(overflow - 1) + 1) * c.slot_bytes <= (overflow + 3) * SLOT_192_640 + 17
    with pytest.raises(IndexError):
        c.overflow_slot(overflow)
    c.stats["hits"] += 5
    c.clear()
    assert len(c) == 0 and c.lookup("a") is None and set(c.stats.values()) == {0} and c.insert("z") == 0
    # the gate of a native width is evaluated once
    assert c.symmetric(1242) and c._symmetric == {1242: True}


def test_budget_below_one_slot_plus_overflow_is_refused():
    from depthcore.frame_cache import FrameCache
    with pytest.raises(ValueError, match="overflow"):
        FrameCache(192, 640, 4, 36 * SLOT_192_640, 36)
    with pytest.raises(ValueError, match="overflow"):
        FrameCache(192, 640, 4, 37 * SLOT_192_640 - 1, 36)
    assert FrameCache(192, 640, 4, 37 * SLOT_192_640, 36).capacity == 1


def test_an_asymmetric_halving_refuses_the_cache(monkeypatch):
    from depthcore import frame_cache
    monkeypatch.setattr(frame_cache, "tables_mirror_symmetric", lambda a, b: (a, b) != (32, 16))
    with pytest.raises(ValueError, match="32 -> 16"):
        frame_cache.FrameCache(32, 64, 4, 100 * 8160, 6)
    assert frame_cache.FrameCache(32, 64, 2, 100 * 8160, 6).capacity > 0           # that halving is not part of two scales


def test_loader_has_no_cache_by_default_and_sizes_one_when_asked(tmp_path):
    import datasets
    from depthcore.loader import BatchLoader
    ds = datasets.KITTIRAWDataset(str(tmp_path), ["d 1 l"] * 4, 32, 64, [0, -1, 1], 4, is_train=True, img_ext=".png")
    assert BatchLoader(ds, 2, device="cpu").cache is None and BatchLoader(ds, 2, device="cpu", cache_bytes=0).cache is None
    ld = BatchLoader(ds, 2, device="cpu", cache_bytes=20 * 8160)
    assert ld.cache.overflow == 6 and ld.cache.capacity == 14 and ld.cache.slot_bytes == 8160
    with pytest.raises(ValueError):
        BatchLoader(ds, 2, device="cpu", cache_bytes=6 * 8160)


def test_option_frame_cache_gb():
    from options import MonodepthOptions, reference_option_names
    assert MonodepthOptions().parse([]).frame_cache_gb == 0
    assert MonodepthOptions().parse(["--frame_cache_gb", "22.5"]).frame_cache_gb == 22.5
    assert "frame_cache_gb" not in reference_option_names()


def test_trainer_gives_the_cache_to_the_train_loader_only_and_logs_it_per_epoch(tmp_path, capsys):
    import types

    import torch

    import trainer as T
    from kitti_tree import write_splits
    write_splits(str(tmp_path), "eigen_zhou", ["d 1 l"] * 4, ["d 1 l"] * 4)
    tr = T.Trainer.__new__(T.Trainer)
    tr.opt = types.SimpleNamespace(gru=None, dataset="kitti", png=True, splits_dir=str(tmp_path), split="eigen_zhou", data_path=str(tmp_path),
                                   height=32, width=64, frame_ids=[0, -1, 1], batch_size=2, num_workers=2, frame_cache_gb=20 * 8160 / 2 ** 30)
    tr.device, tr.rank, tr.world_size = torch.device("cpu"), 0, 1
    train, val = tr.build_loaders()
    assert val.cache is None and train.cache.capacity == 14 and train.cache.slot_bytes == 8160
    tr.opt.frame_cache_gb = 0.0
    assert all(ld.cache is None for ld in tr.build_loaders())
    # the loop's line per epoch
    tr.opt.frame_cache_gb = 20 * 8160 / 2 ** 30
    tr.build_loaders()
    tr.train_loader.cache.insert("a")
    tr.train_loader.cache.stats["hits"] = 7
    tr.train_loader.plan = lambda epoch=None: []                              # an epoch without batches: nothing touches a GPU
    tr.epoch, tr.step = 3, 0
    tr.set_train = lambda: None
    tr.on_step_stream = __import__("contextlib").nullcontext
    tr.model_lr_scheduler = types.SimpleNamespace(step=lambda: None)
    tr.run_epoch()
    assert capsys.readouterr().out.splitlines() == ["epoch   3 | frame cache: 1 of 14 slots | hits: 7 | misses: 0 | decoded: 0 | inserted: 1 | bypassed: 0"]


def test_cached_levels_refuses_bad_arguments_before_any_launch():
    """Every case of the header's list is DC_EINVAL from the host-side check: no HIP call is made, so made-up device
    pointers are fine here."""
    from depthcore import _lib
    from depthcore.data import CACHED_IMG
    L = _lib.lib()
    fake = 4096                                                              # never dereferenced
    slot = 8160                                                              # 32 x 64, 4 scales

    def call(n=2, h=32, w=64, scales=4, arena_bytes=3 * slot, slot_off=(0, 2 * slot), arena=fake, color=True, aug=True, steps=fake,
             packed=fake, desc_host=True):
        desc = np.zeros(max(n, 1), CACHED_IMG)
        desc["slot_off"][:len(slot_off)] = slot_off[:len(desc)]
        ptrs = (ctypes.c_void_p * 4)(*[fake] * max(min(scales, 4), 0))
        return L.dc_data_cached_levels(arena, arena_bytes, desc.ctypes.data if desc_host else None, fake, n, h, w, scales,
                                       ptrs if color else None, ptrs if aug else None, packed, steps, fake, fake, None)
    refused = {
        "slot past the arena": call(slot_off=(0, 2 * slot + 1)),
        "arena one byte short": call(arena_bytes=3 * slot - 1),
        "negative slot": call(slot_off=(-1, 0)),
        "slot offset beyond the arena": call(slot_off=(0, 4 * slot)),
        "n_img 0": call(n=0),
        "n_img negative": call(n=-1),
        "height not divisible by 8": call(h=36),
        "width not divisible by 8": call(w=68),
        "num_scales 0": call(scales=0),
        "num_scales 5": call(scales=5),
        "no arena": call(arena=None),
        "no host descriptors": call(desc_host=False),
        "no color": call(color=False),
        "color_aug without steps": call(steps=None),
        "packed not 16-byte aligned": call(packed=fake + 4),
    }
    assert all(rc == -1 for rc in refused.values()), refused
    # 36 x 68 is fine with fewer scales only as far as the divisibility goes: 2 scales need multiples of 2, and a slot of that
    # size no longer fits the first image's neighbour
    assert call(h=36, w=68, scales=2, slot_off=(0, 3 * slot - 36 * 68 * 3)) == -1
