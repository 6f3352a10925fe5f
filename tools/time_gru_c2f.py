#!/usr/bin/env python3
"""Times the coarse-to-fine ConvGRU front-end, gru_version v10.  Prints one JSON line.

  handover   depthcore.ops.gru_handover (one launch per direction) against the composition it replaces, ops.gru_blend followed by
             ops.lstm_handover (two launches per direction and the autograd sums between them), at the four v10 shapes of a
             192 x 640 input (batch 1), forward alone and forward + backward.  The two alternate inside each of `--rounds` rounds
             after a warm-up; a round times `--reps` calls between device events, so a figure is a call as the network issues it
             (launch overhead included), in microseconds: median, min and max over the rounds.
  train      a v10 training step next to a v8 and a v5 step: resnet18, 192 x 640, len_sequence n, device-resident synthetic
             item, eager; the trainers alternate inside each round of `--steps` steps; ms per step, frames/s, and the launches
             per step from a profiler pass of its own after the timing.
  eval       `--windows` windows of `--frames` frames through predict_disparities_windows at every width of `--widths` against
             the reference's loop (evaluate_depth_gru_fusion_my_v.py:662-697: one window at a time, frame by frame at batch 1,
             all four heads); windows per second, and the launches per advance / step of a warm GruWindowPredictor.

    python tools/time_gru_c2f.py [--rounds 5] [--reps 200] [--steps 20] [--len_sequence 10] [--windows 48] [--frames 11]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "self-supervised-depth-estimation_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import networks  # noqa: E402
import trainer as T  # noqa: E402
from depthcore import evaluate as E  # noqa: E402
from depthcore import ops  # noqa: E402
from depthcore.synthetic import synthetic_sequence_batch  # noqa: E402
from time_eval_gru import device_launches, seconds  # noqa: E402
from time_lstm import alternate, device_work, spread  # noqa: E402


def composed(gates, h, cnm, a):
    h_new = ops.gru_blend(gates, h, cnm)
    pre, up = ops.lstm_handover(a, h, h_new)
    return h_new, pre, up


def handover(a):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    res = {}
    for s in (3, 2, 1, 0):
        C, h, w = 2 * (16 << s), a.height >> s, a.width >> s
        rnd = lambda *shape: torch.randn(*shape, device=dev, generator=g)
        leaves = [torch.sigmoid(rnd(1, 2 * C, h, w)).requires_grad_(), rnd(1, C, h, w).requires_grad_(),
                  torch.tanh(rnd(1, C, h, w)).requires_grad_(), rnd(1, C, h, w).requires_grad_()]
        cots = [rnd(1, C, h, w), rnd(1, C, h, w), rnd(1, C // 4, 2 * h, 2 * w)]

        def both(fn):
            def run():
                torch.autograd.grad(fn(*leaves), leaves, cots)
            return run

        def fwd(fn):
            def run():
                with torch.no_grad():
                    fn(*leaves)
            return run
        t = alternate({"fused_fwd": fwd(ops.gru_handover), "composed_fwd": fwd(composed),
                       "fused_fwd_bwd": both(ops.gru_handover), "composed_fwd_bwd": both(composed)}, a.rounds, a.reps)
        row = {k: spread([1e6 * v for v in vs]) for k, vs in t.items()}
        row["unit"] = "us per call"
        plane = 4.0 * C * h * w                                  # fwd: u, h, cnm, a read; h_new, pre, up written
        row["fused_fwd_gbytes_per_s"] = round(7 * plane / statistics.median(t["fused_fwd"]) / 1e9, 1)
        for d in ("fwd", "fwd_bwd"):
            row["composed_over_fused_" + d] = round(statistics.median(t["composed_" + d]) / statistics.median(t["fused_" + d]), 2)
        res["C=%d %dx%d" % (C, h, w)] = row
    return res


def train(a):
    dev = torch.device("cuda:0")
    n, H, W = a.len_sequence, a.height, a.width
    kw = dict(height=H, width=W, batch_size=1, len_sequence=n, num_layers=18)
    trainers = {v: T.Trainer(T.default_options(gru=v, **kw), device=dev, seed=0) for v in ("v5", "v8", "v10")}
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
    for v in ("v5", "v8"):
        out["v10_over_%s_ms" % v] = round(statistics.median(times["v10"]) / statistics.median(times[v]), 3)
    for v, tr in trainers.items():                     # the profiler slows the host: after the timing, a pass of its own
        out[v].update(device_work(lambda tr=tr: tr.train_step(dict(batch))))
    for tr in trainers.values():
        tr.close()
    return out


def evaluation(a):
    widths = [int(w) for w in a.widths.split(",")]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    enc = networks.ResnetEncoder(18, False).to(dev)
    dec = networks.DepthDecoder(enc.num_ch_enc).to(dev)
    gru = networks.ConvGRUBlocks_v9((3, 3), True, "cpu", attention=False, height=a.height, width=a.width).to(dev)
    with torch.no_grad():
        for p in gru.parameters():
            p.normal_(0, 0.02)
    for net in (enc, dec, gru):
        net.eval()
    g = torch.Generator().manual_seed(1)
    wins = [torch.rand(a.frames, 3, a.height, a.width, generator=g).to(dev) for _ in range(a.windows)]

    def lockstep(width, ws=wins):
        def batch(j, ids, frame_of):
            rows = [ws[c][t:t + 1] for c, t in zip(ids, frame_of)]
            return rows[0] if len(rows) == 1 else ops.stack_frames([rows])[0]
        return E.predict_disparities_windows(enc, dec, gru, [w.shape[0] for w in ws], batch, streams=width)

    def reference_loop(ws=wins):
        outs = []
        with torch.no_grad():
            for frames in ws:
                states = gru.initial_states()
                for i in range(frames.shape[0]):
                    states, disp = gru(dec(enc(frames[i:i + 1]), True), states)
                outs.append(ops.disp_to_depth(disp[("disp", 0)], 0.1, 100.0)[0])
        return torch.cat(outs)

    variants = [("lockstep_%d" % w, (lambda w=w: lockstep(w))) for w in widths] + [("reference_loop", reference_loop)]
    for _, fn in variants:                                       # warm-up: every shape of the timed passes
        fn()
    times = {name: [] for name, _ in variants}
    for _ in range(a.rounds):
        for name, fn in variants:
            times[name].append(seconds(fn))
    res = {"config": "resnet18 + DepthDecoder + ConvGRUBlocks_v9(attention=False), %d windows x %d frames" % (a.windows, a.frames)}
    for name, ts in times.items():
        wps = sorted(a.windows / t for t in ts)
        res[name + "_windows_per_s"] = round(statistics.median(wps), 2)
        res[name + "_windows_per_s_range"] = [round(wps[0], 2), round(wps[-1], 2)]
    for w in widths:
        res["lockstep_%d_vs_reference_loop" % w] = round(res["lockstep_%d_windows_per_s" % w] / res["reference_loop_windows_per_s"], 3)
    res["max_abs_diff_vs_reference_loop"] = float((lockstep(widths[-1]) - reference_loop()).abs().max())
    for w in sorted({1, widths[-1]}):
        wp = E.GruWindowPredictor(enc, dec, gru, streams=w)
        x = torch.cat([s[0:1] for s in wins[:w]])
        wp.advance(x)
        wp.step(x)
        with torch.no_grad():
            out = dec(enc(x), True)
            maps = [out[("disp", s)].clone() for s in range(4)]
        res["lockstep_%d_launches_recurrent_part_of_advance" % w] = device_launches(lambda: wp.advance_maps(maps))
        res["lockstep_%d_launches_recurrent_part_of_step" % w] = device_launches(lambda: wp.step_maps(maps))
    n = device_launches(lambda: reference_loop(wins[:1]))
    res["reference_loop_launches_per_frame"] = None if n is None else round(n / a.frames, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--len_sequence", type=int, default=10)
    ap.add_argument("--windows", type=int, default=48)
    ap.add_argument("--frames", type=int, default=11)
    ap.add_argument("--widths", default="1,4,16")
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--skip_train", action="store_true")
    ap.add_argument("--skip_eval", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/time_gru_c2f.py measures on the GPU; there is none here")
    torch.cuda.set_device(0)
    res = {"config": "ConvGRU v10, %d x %d, batch 1, fp32; %d rounds, %d calls / %d steps per round, alternating"
           % (a.height, a.width, a.rounds, a.reps, a.steps)}
    res["handover"] = handover(a)
    if not a.skip_train:
        res["train"] = dict(train(a), config="resnet18, len_sequence %d, eager, fused loss" % a.len_sequence)
    if not a.skip_eval:
        res["eval"] = evaluation(a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
