#!/usr/bin/env python3
"""Times the data path of train.py on a tmp KITTI-shaped tree of JPEGs in the five native sizes of the raw drives.
Prints one JSON line:

  decode_images_per_s   PIL decode of 1242 x 375 JPEGs on min(num_workers, 16) threads (host only)
  data_step_*_ms        B x 3 frames, the five sizes mixed: GpuPreprocessor.ragged against the same batch grouped by size,
                        `__call__` per group, index_copy back into batch order (the existing kernels); runs alternate
  data_step_ragged_vs_cached_ms  the same batch served from a warm frame cache (GpuPreprocessor.cached) against ragged,
                        alternating blocks, every block's median listed
  loader_batches_per_s  BatchLoader with prefetch 2 and prefetch 0 (nothing consumes the batches but an event wait); `cache_cold` /
                        `cache_warm`: with a frame cache, the epoch that decodes every file and the epochs after it
  train_*_ms_per_step   Trainer.train_step fed by the loader, by the loader on a warm frame cache, and by one device-resident
                        synthetic batch; same process, alternating blocks (`synthetic_alone`: before the process has a loader)

    python tools/time_loader.py [--batch 12] [--height 192] [--width 640] [--num_workers 12] [--steps 40]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "self-supervised-depth-estimation_amd"))
import datasets  # noqa: E402
import trainer as T  # noqa: E402
from depthcore.data import GpuPreprocessor, slot_layout  # noqa: E402
from depthcore.frame_cache import FrameCache  # noqa: E402
from depthcore.loader import BatchLoader, _decode_into  # noqa: E402
from depthcore.synthetic import synthetic_batch  # noqa: E402

KITTI_SIZES = [(375, 1242), (370, 1224), (370, 1226), (374, 1238), (376, 1241)]


def write_tree(root, frames):
    """One drive per native size, `frames` JPEGs each (photo-like content: smooth gradients + noise, quality 92)."""
    lines = []
    rng = np.random.RandomState(0)
    for d, (h, w) in enumerate(KITTI_SIZES):
        drive = "2011_09_%02d/2011_09_%02d_drive_%04d_sync" % (26 + d, 26 + d, d + 1)
        folder = os.path.join(root, drive, "image_02", "data")
        os.makedirs(folder)
        y, x = np.mgrid[0:h, 0:w].astype(np.float32)
        for i in range(frames):
            img = np.stack([127 + 90 * np.sin(x / (40 + 9 * c) + i) * np.cos(y / (25 + 5 * c)) for c in range(3)], -1)
            img = np.clip(img + rng.randint(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(folder, "%010d.jpg" % i), quality=92)
            if 0 < i < frames - 1:
                lines.append("%s %d l" % (drive, i))
    return lines


def median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def grouped_baseline(pre, natives, sizes, flips, jitters, B):
    """The existing kernels on a mixed batch: one `__call__` per native size, results copied back into batch order."""
    out = {}
    for size in sorted(set(sizes)):
        idx = [b for b in range(B) if sizes[b] == size]
        native = torch.stack([torch.stack([natives[f][b] for b in idx]) for f in range(len(natives))])
        part = pre(native, [flips[b] for b in idx], [jitters[b] for b in idx])
        where = torch.tensor(idx, device=native.device)
        for k, v in part.items():
            if k not in out:
                out[k] = torch.empty((B,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device)
            out[k].index_copy_(0, where, v)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--num_workers", type=int, default=12)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--frames", type=int, default=26)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {"config": "resnet18 %d x %d x %d, %d decode threads" % (a.batch, a.height, a.width, min(a.num_workers, 16))}
    with tempfile.TemporaryDirectory() as root:
        lines = write_tree(root, a.frames)
        ds = datasets.KITTIRAWDataset(root, lines, a.height, a.width, [0, -1, 1], 4, is_train=True, img_ext=".jpg")
        B = a.batch

        # 0. the training step alone, before this process has a decode pool or a second stream's allocations
        tr = T.Trainer(T.default_options(batch_size=B, height=a.height, width=a.width), device=dev)
        tr.set_train()
        synth = synthetic_batch(B, a.height, a.width, dev, seed=1, packed=True)

        def steps_ms(src):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                tr.train_step(src())
            torch.cuda.synchronize()
            return round(1e3 * (time.perf_counter() - t0) / a.steps, 3)
        with tr.on_step_stream():
            for _ in range(5):
                tr.train_step(dict(synth))
            res["train_synthetic_alone_ms_per_step"] = [steps_ms(lambda: dict(synth)) for _ in range(2)]

        # 1. host decode alone
        ld = BatchLoader(ds, B, a.num_workers, dev, seed=0, prefetch=2)
        path = ds.frame_paths([i for i, l in enumerate(lines) if "drive_0001" in l][0])[0]
        bufs = [np.empty((375, 1242, 3), np.uint8) for _ in range(ld.threads)]
        n = 30 * ld.threads
        list(ld._pool_().map(lambda i: _decode_into(path, bufs[i % ld.threads]), range(ld.threads)))
        t0 = time.perf_counter()
        futures = [ld._pool_().submit(_decode_into, path, bufs[i % ld.threads]) for i in range(n)]
        for f in futures:
            f.result()
        res["decode_images_per_s"] = round(n / (time.perf_counter() - t0), 1)
        res["decode_threads"] = ld.threads

        # 2. the data step on a mixed batch: ragged against the grouped baseline, alternating
        indices, draws = ld.plan(0)[0]
        buf, sizes, flips, jitters, _ = ld.decode_batch(indices, draws)
        packed = torch.from_numpy(buf).to(dev)
        natives, off = [], 0
        for f in range(3):
            row = []
            for h, w in sizes:
                row.append(packed[off:off + h * w * 3].view(h, w, 3))
                off += h * w * 3
            natives.append(row)
        pre = GpuPreprocessor(a.height, a.width, 4, (0, -1, 1), dev)
        got, want = pre.ragged(packed, sizes, flips, jitters), grouped_baseline(pre, natives, sizes, flips, jitters, B)
        assert all(torch.equal(got[k], want[k]) for k in want), "ragged and grouped results differ"
        rag, grp = [], []
        for _ in range(3):
            rag.append(median_ms(lambda: pre.ragged(packed, sizes, flips, jitters), 15))
            grp.append(median_ms(lambda: grouped_baseline(pre, natives, sizes, flips, jitters, B), 15))
        res["data_step_native_sizes"] = len(set(sizes))
        res["data_step_ragged_ms"] = [round(v, 3) for v in rag]
        res["data_step_grouped_ms"] = [round(v, 3) for v in grp]

        # 2b. the same batch from a warm frame cache (GpuPreprocessor.cached: two launches) against ragged, alternating blocks
        cache = FrameCache(a.height, a.width, 4, (3 * B + 1) * slot_layout(a.height, a.width, 4)[1], 0, dev)
        assert all(cache.symmetric(w) for _, w in sizes), "a native width fails the symmetry gate"
        frames, off = [], 0
        for f in range(3):
            for h, w in sizes:
                frames.append((off, h, w, cache.insert("image %d" % len(frames))))
                off += h * w * 3
        cache.build(pre, packed, frames)
        slots = [fr[3] for fr in frames]
        warm = pre.cached(cache.arena, slots, flips, jitters)
        assert all(torch.equal(warm[k], got[k]) for k in got), "cached and ragged results differ"
        rag2, cac = [], []
        for _ in range(5):
            rag2.append(median_ms(lambda: pre.ragged(packed, sizes, flips, jitters), 15))
            cac.append(median_ms(lambda: pre.cached(cache.arena, slots, flips, jitters), 15))
        res["data_step_ragged_vs_cached_ms"] = {"ragged": [round(v, 3) for v in rag2], "cached": [round(v, 3) for v in cac]}
        del cache, warm

        # 3. the loader alone
        cache_bytes = (len(KITTI_SIZES) * a.frames + 3 * B + 1) * slot_layout(a.height, a.width, 4)[1]
        ldc = BatchLoader(ds, B, a.num_workers, dev, seed=1, prefetch=2, cache_bytes=cache_bytes)
        for epoch, name in enumerate(("cold", "warm", "warm")):      # the first epoch decodes every file, the later ones none
            ldc.set_epoch(epoch)
            it = iter(ldc)
            next(it)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            count = sum(1 for _ in it)
            torch.cuda.synchronize()
            res.setdefault("loader_batches_per_s_cache_%s" % name, []).append(round(count / (time.perf_counter() - t0), 1))
        res["loader_cache_stats"] = dict(ldc.cache.stats)
        for prefetch in (2, 0, 2, 0):
            ld2 = BatchLoader(ds, B, a.num_workers, dev, seed=1, prefetch=prefetch)
            it, count = iter(ld2), 0
            next(it)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in it:
                count += 1
            torch.cuda.synchronize()
            res.setdefault("loader_batches_per_s_prefetch%d" % prefetch, []).append(round(count / (time.perf_counter() - t0), 1))
            ld2.close()

        # 4. the training step fed by the loader against the same loop on device-resident synthetic inputs
        def cycle(loader, epoch=0):
            while True:
                loader.set_epoch(epoch)
                for batch in loader:
                    yield batch
                epoch += 1
        feed, feed_warm = cycle(ld), cycle(ldc, 3)       # ldc: the cached loader of 3, every file in its slot by now
        with tr.on_step_stream():
            for _ in range(5):
                tr.train_step(dict(synth))
                tr.train_step(next(feed))
                tr.train_step(next(feed_warm))
            for _ in range(3):
                for name, src in (("synthetic", lambda: dict(synth)), ("loader", lambda: next(feed)),
                                  ("loader_warm_cache", lambda: next(feed_warm))):
                    res.setdefault("train_%s_ms_per_step" % name, []).append(steps_ms(src))
        feed.close()
        feed_warm.close()
        assert ldc.cache.stats["decoded"] == res["loader_cache_stats"]["decoded"], "the warm loader decoded a file"
        ld.close()
        ldc.close()
        tr.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
