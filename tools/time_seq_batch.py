#!/usr/bin/env python3
"""Times ConvGRU training at several sequence items per step (`--seq_batch`).  Prints one JSON line.

  train        resnet18, 192 x 640, len_sequence n = 10, device-resident synthetic items (nothing is decoded or uploaded): one
               Trainer per width S, `train_step` on a stacked time-major batch of S items.  The widths alternate inside each
               of `--rounds` rounds after a warm-up of every shape; a round times `--steps` steps between device events.
               Per width: frames/s (median, min and max over the rounds), ms per step, and the launches of one step from
               the framework profiler's device events (tools/time_eval_gru.py `device_launches`; a pass of its own, after
               the timing).  "existing" is a trainer built without the option (the path before it existed), timed in the
               same rounds: S = 1 must reproduce it.
  data_step    the per-item cost of the data step at 375 x 1242 -> 192 x 640: GpuPreprocessor.sequence on one item against
               GpuPreprocessor.sequence_batch on 4, un-jittered and jittered, alternating, ms per item.
  decode_ceiling_frames_per_s   what the loader's measured decode rate of 200-240 items/s (independent of S: the
               host decodes every frame once) allows at this n; a step that trains faster than this waits for the host.

    python tools/time_seq_batch.py [--widths 1,2,4,8] [--rounds 3] [--steps 30] [--len_sequence 10]
"""
import argparse
import json
import os
import random
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "self-supervised-depth-estimation_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trainer as T  # noqa: E402
from depthcore._lib import DepthcoreError  # noqa: E402
from depthcore.data import GpuPreprocessor, sample_sequence  # noqa: E402
from depthcore.synthetic import synthetic_sequence_batch  # noqa: E402
from time_eval_gru import device_launches, seconds  # noqa: E402


def spread(values, digits=1):
    v = sorted(values)
    return {"median": round(statistics.median(v), digits), "min": round(v[0], digits), "max": round(v[-1], digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="1,2,4,8")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--len_sequence", type=int, default=10)
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--data_reps", type=int, default=20)
    a = ap.parse_args()
    widths = [int(w) for w in a.widths.split(",")]
    if 1 not in widths:
        widths = [1] + widths
    n, H, W = a.len_sequence, a.height, a.width
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {"config": "resnet18 + ConvGRUBlocks_v5, %d x %d, len_sequence %d, fp32, eager, %d rounds of %d steps" % (H, W, n, a.rounds, a.steps)}

    # ---- train_step ------------------------------------------------------------------------------------------------------
    kw = dict(height=H, width=W, batch_size=1, gru="v5", len_sequence=n, num_layers=18)
    variants = [("existing", T.Trainer(T.default_options(**kw), device=dev, seed=0), 1)]
    variants += [("S=%d" % s, T.Trainer(T.default_options(seq_batch=s, **kw), device=dev, seed=0), s) for s in widths]
    batches = {s: synthetic_sequence_batch(n, H, W, dev, items=s, seed=s) for s in sorted({s for _, _, s in variants})}
    train, usable = {}, []
    for name, tr, s in variants:
        tr.set_train()
        try:
            for _ in range(3):                                       # warm-up: every shape of the timed windows
                tr.train_step(dict(batches[s]))
            torch.cuda.synchronize()
            usable.append((name, tr, s))
        except DepthcoreError as exc:                                # a width the kernels refuse is reported, not timed
            train[name] = {"not_measured": str(exc), "frames_per_step": s * n}
            print("%s: %s" % (name, exc), file=sys.stderr)
            tr.close()
    variants = usable
    times = {name: [] for name, _, _ in variants}

    def window(tr, s):
        for _ in range(a.steps):
            tr.train_step(dict(batches[s]))
    for _ in range(a.rounds):
        for name, tr, s in variants:
            with tr.on_step_stream():
                times[name].append(seconds(lambda tr=tr, s=s: window(tr, s)))
    res["train"] = train
    for name, tr, s in variants:
        fps = [a.steps * s * n / t for t in times[name]]
        train[name] = {"frames_per_s": spread(fps), "ms_per_step": round(1e3 * statistics.median(times[name]) / a.steps, 3)}
    for name, tr, s in variants:                                     # the profiler slows the host: after the timing, a pass of its own
        train[name]["launches_per_step"] = device_launches(lambda tr=tr, s=s: tr.train_step(dict(batches[s])))
    base = train["S=1"]["frames_per_s"]
    res["baseline_spread_percent"] = round(100.0 * (base["max"] - base["min"]) / base["median"], 2)
    for s in [s for s in widths[1:] if "frames_per_s" in train["S=%d" % s]]:
        res["speedup_S=%d_over_S=1" % s] = round(train["S=%d" % s]["frames_per_s"]["median"] / base["median"], 3)
    for _, tr, _ in variants:
        tr.close()
    del variants, batches
    torch.cuda.empty_cache()

    # ---- the data step, per item -------------------------------------------------------------------------------------------
    pre = GpuPreprocessor(H, W, 4, (0, -1, 1), dev)
    g = torch.Generator().manual_seed(2)
    items = 4
    native = torch.randint(0, 256, (items, n + 2, 375, 1242, 3), dtype=torch.uint8, generator=g).to(dev)
    rng, jit = random.Random(n), []
    while len(jit) < items:                                           # the first draws that decide for colour augmentation
        _, j = sample_sequence(True, rng, n, 4)
        if j is not None:
            jit.append(j)
    flips = [bool(i % 2) for i in range(items)]
    data = res["data_step_ms_per_item"] = {}
    for tag, jitters in (("unjittered", [None] * items), ("jittered", jit)):
        one = lambda: [pre.sequence(native[i], flips[i], jitters[i]) for i in range(items)]                           # noqa: E731
        four = lambda: pre.sequence_batch(native.view(-1), [(375, 1242)] * items, n, flips, jitters)                   # noqa: E731
        got, want = four(), one()
        S_rows = slice(0, None, items)
        assert all(torch.equal(got[k][S_rows], want[0][k]) for k in want[0]), "the step's item 0 differs from the single item"
        for fn in (one, four):
            for _ in range(3):
                fn()
        ms = {"S=1": [], "S=4": []}
        for _ in range(a.rounds):
            for name, fn in (("S=1", one), ("S=4", four)):
                ms[name].append(1e3 * seconds(lambda fn=fn: [fn() for _ in range(a.data_reps)]) / (a.data_reps * items))
        data[tag] = {name: spread(v, 3) for name, v in ms.items()}
        data[tag]["launches_S=1_one_item"] = device_launches(lambda: pre.sequence(native[0], flips[0], jitters[0]))
        data[tag]["launches_S=4_one_step"] = device_launches(four)
    res["decode_ceiling_frames_per_s"] = [200 * n, 240 * n]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
