#!/usr/bin/env python3
"""Times the data path of train_gru.py at the reference's sequence lengths.  Prints one JSON line; per len_sequence n:

  unjittered_ms   one sequence item's data step without jitter: GpuPreprocessor.sequence (one (n + 2)-frame pyramid, the windows
                  handed out as slices) against the entry points that existed before it -- `GpuPreprocessor.__call__` on the
                  three materialised windows (F = 3, B = n) followed by the ops.stack_frames of Trainer._stack_sequence.  With
                  no flip both produce the same pixels (checked).  Alternating blocks, every block's median listed: the
                  spread of the baseline's blocks is the margin of the comparison.
  jittered_ms     the same item with a fresh ColorJitter per window, frame and level, against the per-level composition of
                  dc_data_resize_axis x2, dc_data_jitter, dc_data_to_tensor and dc_data_to_rgbx over the 3n images (checked equal)
  loader_items_per_s   SequenceLoader over a tmp drive of 1242 x 375 JPEGs, prefetch 2 and 0 (nothing consumes the items)

    python tools/time_seq_loader.py [--height 192] [--width 640] [--num_workers 12] [--lengths 10 3] [--lds_budget BYTES]
"""
import argparse
import json
import os
import random
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "self-supervised-depth-estimation_amd"))
import datasets  # noqa: E402
from depthcore import _lib, ops  # noqa: E402
from depthcore.data import HUE, GpuPreprocessor, hue_shift, sample_sequence  # noqa: E402
from depthcore.loader import SequenceLoader  # noqa: E402

DRIVE = "2011_09_26/2011_09_26_drive_0001_sync"


def write_drive(root, frames, h=375, w=1242):
    folder = os.path.join(root, DRIVE, "image_02", "data")
    os.makedirs(folder)
    rng = np.random.RandomState(0)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    out = []
    for i in range(frames):
        img = np.stack([127 + 90 * np.sin(x / (40 + 9 * c) + i) * np.cos(y / (25 + 5 * c)) for c in range(3)], -1)
        img = np.clip(img + rng.randint(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(folder, "%010d.jpg" % i), quality=92)
        out.append(img)
    return out


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


def windows_baseline(pre, windows, intrinsics, n):
    """What a per-position loader built from the older entry points would cost: the pyramid of the three windows, then the
    stack of Trainer._stack_sequence (12 colour groups, 8 intrinsics groups, one launch)."""
    out = pre(windows)
    keys = [("color", f, s) for f in (0, -1, 1) for s in range(4)]
    groups = [[out[k][j:j + 1] for j in range(n)] for k in keys] + [[v] * n for v in intrinsics]
    return dict(zip(keys, ops.stack_frames(groups)))


def composition(pre, native, jitters, n):
    """The jittered item from dc_data_resize_axis x2, dc_data_jitter, dc_data_to_tensor, dc_data_to_rgbx, level after level."""
    L, dev, S = _lib.lib(), native.device, pre.num_scales
    frames = [1 + j for j in range(n)] + list(range(n)) + [2 + j for j in range(n)]
    img = native[frames].contiguous()
    N = 3 * n
    sums = torch.empty(N, dtype=torch.int64, device=dev)
    color, packed = [], None
    for s in range(S):
        h, w = pre.height >> s, pre.width >> s
        img = pre._resize(img, h, w, None)
        st, pr = np.zeros((N, 4), np.int32), np.zeros((N, 4), np.float32)
        for i in range(N):
            order, factors = jitters[i // n][i % n][s]
            for k, op in enumerate(order):
                st[i, k], pr[i, k] = op, float(hue_shift(factors[op])) if op == HUE else factors[op]
        img = img.clone()
        st_d, pr_d = torch.from_numpy(st).to(dev), torch.from_numpy(pr).to(dev)
        _lib.check(L.dc_data_jitter(img.data_ptr(), N, h * w, st_d.data_ptr(), pr_d.data_ptr(), sums.data_ptr(), _lib.stream(img)), "dc_data_jitter")
        color.append(pre._to_tensor(img))
        if s == 0:
            packed = torch.empty((N, h, w, 4), dtype=torch.float32, device=dev)
            _lib.check(L.dc_data_to_rgbx(img.data_ptr(), packed.data_ptr(), N, h * w, _lib.stream(img)), "dc_data_to_rgbx")
    return color, packed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--num_workers", type=int, default=12)
    ap.add_argument("--lengths", type=int, nargs="+", default=[10, 3])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--lds_budget", type=int, default=0, help="dc_data_seq_plan's LDS budget in bytes (0: the library's): moves the tail's start")
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {"config": "%d x %d from 375 x 1242, %d decode threads" % (a.height, a.width, min(a.num_workers, 16))}
    with tempfile.TemporaryDirectory() as root:
        frames = write_drive(root, max(a.lengths) + 2 + 12)
        for n in a.lengths:
            r = res["n=%d" % n] = {}
            pre = GpuPreprocessor(a.height, a.width, 4, (0, -1, 1), dev)
            pre.seq_lds_budget = a.lds_budget
            native = torch.from_numpy(np.stack(frames[:n + 2])).to(dev)
            windows = torch.stack([native[1:n + 1], native[0:n], native[2:n + 2]]).contiguous()
            intrinsics = [v for _, v in sorted(pre.intrinsics(datasets.KITTISequenceDataset(root, a.height, a.width, n, [], False).K, 1).items())]
            plan = pre.sequence_plan(n, True)
            r["tail_start"], r["lds_bytes"] = int(plan.tail_start), int(plan.lds_bytes)
            # un-jittered
            got, want = pre.sequence(native), windows_baseline(pre, windows, intrinsics, n)
            assert all(torch.equal(got[k], want[k]) for k in want), "sequence and the stacked windows differ"
            new, old = [], []
            for _ in range(a.blocks):
                new.append(median_ms(lambda: pre.sequence(native), a.reps))
                old.append(median_ms(lambda: windows_baseline(pre, windows, intrinsics, n), a.reps))
            r["unjittered_ms"] = {"sequence": [round(v, 3) for v in new], "windows_then_stack": [round(v, 3) for v in old]}
            # jittered
            jitters, rng = None, random.Random(n)
            while jitters is None:                           # the first draw that decides for colour augmentation
                _, jitters = sample_sequence(True, rng, n, 4)
            got = pre.sequence(native, False, jitters)
            color, packed = composition(pre, native, jitters, n)
            for w, f in enumerate((0, -1, 1)):
                assert all(torch.equal(got[("color", f, s)], color[s][w * n:(w + 1) * n]) for s in range(4)), "jittered levels differ"
                assert torch.equal(got[("color_packed", f, 0)], packed[w * n:(w + 1) * n])
            new, old = [], []
            for _ in range(a.blocks):
                new.append(median_ms(lambda: pre.sequence(native, False, jitters), a.reps))
                old.append(median_ms(lambda: composition(pre, native, jitters, n), a.reps))
            r["jittered_ms"] = {"sequence": [round(v, 3) for v in new], "per_level_composition": [round(v, 3) for v in old]}
            # the loader alone
            items = [(DRIVE, range(x, x + n + 2)) for x in range(12)] * 3
            ds = datasets.KITTISequenceDataset(root, a.height, a.width, n, items, True, img_ext=".jpg")
            for prefetch in (2, 0, 2, 0):
                ld = SequenceLoader(ds, a.num_workers, dev, seed=1, prefetch=prefetch)
                it, count = iter(ld), 0
                next(it)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in it:
                    count += 1
                torch.cuda.synchronize()
                r.setdefault("loader_items_per_s_prefetch%d" % prefetch, []).append(round(count / (time.perf_counter() - t0), 1))
                ld.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
