#!/usr/bin/env python3
"""Times the ConvLSTM v8 front-end.  Prints one JSON line.

  cell / handover   depthcore.ops.lstm_cell and lstm_handover at the four v8 shapes of a 192 x 640 input (batch 1), forward
                    alone and forward + backward, against the stock torch formulation of the same formulas (tests/lstm_ref.py's
                    expressions, autograd for the backward) in the same process.  The two alternate inside each of `--rounds`
                    rounds after a warm-up; a round times `--reps` calls between device events, so a figure is a call as the
                    network issues it (launch overhead included), in microseconds: median, min and max over the rounds.
                    `gbytes_per_s` is the algorithmic traffic of the depthcore call (planes read + planes written, computed
                    from the shape) over its median time.
  train             a v8 training step next to a v5 step: resnet18, 192 x 640, len_sequence n, device-resident synthetic item,
                    eager; the two trainers alternate inside each round of `--steps` steps; ms per step and frames/s.

    python tools/time_lstm.py [--rounds 5] [--reps 200] [--steps 20] [--len_sequence 10]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "self-supervised-depth-estimation_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trainer as T  # noqa: E402
from depthcore import ops  # noqa: E402
from depthcore.synthetic import synthetic_sequence_batch  # noqa: E402
from time_eval_gru import seconds  # noqa: E402


def spread(values, digits=1):
    v = sorted(values)
    return {"median": round(statistics.median(v), digits), "min": round(v[0], digits), "max": round(v[-1], digits)}


def torch_cell(cc, c):
    i, f, o, g = torch.split(cc, cc.shape[1] // 4, dim=1)
    c_next = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c_next), c_next


def torch_handover(a, hp, hn):
    pre = torch.relu(a + (hp + hn) / 2)
    return pre, F.pixel_shuffle(torch.tanh(pre), 2)


def alternate(fns, rounds, reps):
    """{name: [seconds per call] per round}: every fn warmed up, then the fns take turns inside each round."""
    for fn in fns.values():
        for _ in range(50):                                      # (10 left the first shape of a process with rounds twice the others)
            fn()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(seconds(lambda fn=fn: [fn() for _ in range(reps)]) / reps)
    return out


def device_work(fn):
    """Launches (kernels, device copies and fills) that one fn() enqueues and the sum of their durations, from the framework
    profiler's device events: what the GPU has to do for a step, whatever the host needs to issue it."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        evs = [ev for ev in prof.events() if str(ev.device_type).endswith("CUDA")]
        return {"launches_per_step": len(evs) or None,
                "sum_of_kernel_durations_ms": round(sum(ev.time_range.elapsed_us() for ev in evs) / 1e3, 2) if evs else None}
    except Exception as exc:                                     # a measurement that could not be taken is reported as such
        print("device work not measured: %r" % (exc,), file=sys.stderr)
        return {"launches_per_step": None, "sum_of_kernel_durations_ms": None}


def pointwise(a):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    res = {"cell": {}, "handover": {}}
    for s in (3, 2, 1, 0):
        C, h, w = 2 * (16 << s), a.height >> s, a.width >> s
        shape = "C=%d %dx%d" % (C, h, w)
        cc = (2 * torch.randn(1, 4 * C, h, w, device=dev, generator=g)).requires_grad_()
        c = torch.randn(1, C, h, w, device=dev, generator=g).requires_grad_()
        gh, gc = torch.randn(1, C, h, w, device=dev, generator=g), torch.randn(1, C, h, w, device=dev, generator=g)
        x = [torch.randn(1, C, h, w, device=dev, generator=g).requires_grad_() for _ in range(3)]
        gu = torch.randn(1, C // 4, 2 * h, 2 * w, device=dev, generator=g)

        def both(fn, leaves, cots):
            def run():
                outs = fn(*leaves)
                torch.autograd.grad(outs, leaves, cots)
            return run

        def fwd(fn, leaves):
            def run():
                with torch.no_grad():
                    fn(*leaves)
            return run
        plane = 4.0 * C * h * w
        for name, dc_fn, th_fn, leaves, cots, bytes_f, bytes_fb in (
                ("cell", ops.lstm_cell, torch_cell, [cc, c], [gh, gc], 7 * plane, (7 + 7 + 5) * plane),
                ("handover", ops.lstm_handover, torch_handover, x, [gh, gu], 5 * plane, (5 + 3 + 3) * plane)):
            t = alternate({"depthcore_fwd": fwd(dc_fn, leaves), "torch_fwd": fwd(th_fn, leaves),
                           "depthcore_fwd_bwd": both(dc_fn, leaves, cots), "torch_fwd_bwd": both(th_fn, leaves, cots)}, a.rounds, a.reps)
            row = {k: spread([1e6 * v for v in vs]) for k, vs in t.items()}
            row["unit"] = "us per call"
            row["depthcore_fwd_gbytes_per_s"] = round(bytes_f / statistics.median(t["depthcore_fwd"]) / 1e9, 1)
            row["depthcore_fwd_bwd_gbytes_per_s"] = round(bytes_fb / statistics.median(t["depthcore_fwd_bwd"]) / 1e9, 1)
            for d in ("fwd", "fwd_bwd"):
                row["torch_over_depthcore_" + d] = round(statistics.median(t["torch_" + d]) / statistics.median(t["depthcore_" + d]), 2)
            res[name][shape] = row
    return res


def train(a):
    dev = torch.device("cuda:0")
    n, H, W = a.len_sequence, a.height, a.width
    kw = dict(height=H, width=W, batch_size=1, len_sequence=n, num_layers=18)
    trainers = {v: T.Trainer(T.default_options(gru=v, **kw), device=dev, seed=0) for v in ("v5", "v8")}
    batch = synthetic_sequence_batch(n, H, W, dev, items=1, seed=1)
    for tr in trainers.values():
        tr.set_train()
        for _ in range(3):
            tr.train_step(dict(batch))
    torch.cuda.synchronize()
    times = {v: [] for v in trainers}
    for _ in range(a.rounds):
        for v, tr in trainers.items():
            times[v].append(seconds(lambda tr=tr: [tr.train_step(dict(batch)) for _ in range(a.steps)]) / a.steps)
    out = {v: {"ms_per_step": spread([1e3 * t for t in ts], 2), "frames_per_s": spread([n / t for t in ts])} for v, ts in times.items()}
    out["v8_over_v5_ms"] = round(statistics.median(times["v8"]) / statistics.median(times["v5"]), 3)
    for v, tr in trainers.items():                     # the profiler slows the host: after the timing, a pass of its own
        out[v].update(device_work(lambda tr=tr: tr.train_step(dict(batch))))
    for tr in trainers.values():
        tr.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--len_sequence", type=int, default=10)
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--skip_train", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/time_lstm.py measures on the GPU; there is none here")
    torch.cuda.set_device(0)
    res = {"config": "ConvLSTM v8, %d x %d, batch 1, fp32; %d rounds, %d calls / %d steps per round, alternating"
           % (a.height, a.width, a.rounds, a.reps, a.steps)}
    res.update(pointwise(a))
    if not a.skip_train:
        res["train"] = dict(train(a), config="resnet18, len_sequence %d, eager, fused loss" % a.len_sequence)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
