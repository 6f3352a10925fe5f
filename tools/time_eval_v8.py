#!/usr/bin/env python3
"""Times the ConvLSTM v8 evaluation of depthcore.evaluate on synthetic device-resident frames: a seeded resnet18 +
DepthDecoder + ConvGRUBlocks_v8 over `--windows` windows of `--frames` frames at 192 x 640 (the Eigen split is 697 windows of up
to 7 frames), run
  - in lockstep (predict_disparities_windows) at every width of `--widths`, and
  - through the reference's loop (evaluate_depth_gru_fusion.py:578-614): one window at a time, frame by frame at batch 1,
    encoder -> decoder(pre_disp) -> ConvGRUBlocks_v8.forward with all four heads, the last frame's scale-0 disparity kept.
The variants alternate inside each of `--repeats` rounds after a warm-up of every shape; device events around each pass.  The
launch counts come from a profiler pass of their own after the timing (null when the profiler cannot see the device).
Prints one JSON line (windows per second: median, and min / max over the rounds).

    python tools/time_eval_v8.py [--windows 96] [--frames 7] [--widths 1,4,16] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "self-supervised-depth-estimation_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import networks  # noqa: E402
from depthcore import evaluate as E  # noqa: E402
from depthcore import ops  # noqa: E402
from time_eval_gru import device_launches, seconds  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=96)
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--widths", default="1,4,16")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=640)
    a = ap.parse_args()
    widths = [int(w) for w in a.widths.split(",")]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    enc = networks.ResnetEncoder(18, False).to(dev)
    dec = networks.DepthDecoder(enc.num_ch_enc).to(dev)
    lstm = networks.ConvGRUBlocks_v8((3, 3), True, "cpu", attention=False, height=a.height, width=a.width).to(dev)
    with torch.no_grad():
        for p in lstm.parameters():
            p.normal_(0, 0.02)
    for net in (enc, dec, lstm):
        net.eval()
    g = torch.Generator().manual_seed(1)
    wins = [torch.rand(a.frames, 3, a.height, a.width, generator=g).to(dev) for _ in range(a.windows)]

    def lockstep(width, ws=wins):
        def batch(j, ids, frame_of):
            rows = [ws[c][t:t + 1] for c, t in zip(ids, frame_of)]
            return rows[0] if len(rows) == 1 else ops.stack_frames([rows])[0]
        return E.predict_disparities_windows(enc, dec, lstm, [w.shape[0] for w in ws], batch, streams=width)

    def reference_loop(ws=wins):
        outs = []
        with torch.no_grad():
            for frames in ws:
                states = lstm.initial_states()
                for i in range(frames.shape[0]):
                    states, disp = lstm(dec(enc(frames[i:i + 1]), True), states)
                outs.append(ops.disp_to_depth(disp[("disp", 0)], 0.1, 100.0)[0])
        return torch.cat(outs)

    variants = [("lockstep_%d" % w, (lambda w=w: lockstep(w))) for w in widths] + [("reference_loop", reference_loop)]
    for _, fn in variants:                                       # warm-up: every shape of the timed passes
        fn()
    times = {name: [] for name, _ in variants}
    for _ in range(a.repeats):
        for name, fn in variants:
            times[name].append(seconds(fn))
    res = {"config": "resnet18 + DepthDecoder + ConvGRUBlocks_v8, %d windows x %d frames at %d x %d, fp32, %d rounds" % (
        a.windows, a.frames, a.height, a.width, a.repeats)}
    for name, ts in times.items():
        wps = sorted(a.windows / t for t in ts)
        res[name + "_windows_per_s"] = round(statistics.median(wps), 2)
        res[name + "_windows_per_s_range"] = [round(wps[0], 2), round(wps[-1], 2)]
    for w in widths:
        res["lockstep_%d_vs_reference_loop" % w] = round(res["lockstep_%d_windows_per_s" % w] / res["reference_loop_windows_per_s"], 3)
    # what the two compositions compute agrees (fp32, differently tiled convolutions)
    res["max_abs_diff_vs_reference_loop"] = float((lockstep(widths[-1]) - reference_loop()).abs().max())
    # launches per step of a warm WindowPredictor at width 1 and at the widest, per frame of the reference's loop
    for w in sorted({1, widths[-1]}):
        wp = E.WindowPredictor(enc, dec, lstm, streams=w)
        x = torch.cat([s[0:1] for s in wins[:w]])
        wp.advance(x)
        wp.step(x)
        res["lockstep_%d_launches_per_advance" % w] = device_launches(lambda: wp.advance(x))
        res["lockstep_%d_launches_per_step" % w] = device_launches(lambda: wp.step(x))
        maps = _maps(enc, dec, x)                                # the recurrent part alone, behind the encoder and decoder
        res["lockstep_%d_launches_recurrent_part_of_advance" % w] = device_launches(lambda: wp.advance_maps(maps))
        res["lockstep_%d_launches_recurrent_part_of_step" % w] = device_launches(lambda: wp.step_maps(maps))
    n = device_launches(lambda: reference_loop(wins[:1]))
    res["reference_loop_launches_per_frame"] = None if n is None else round(n / a.frames, 1)
    print(json.dumps(res))


def _maps(enc, dec, x):
    with torch.no_grad():
        out = dec(enc(x), True)
        return [out[("disp", s)].clone() for s in range(4)]


if __name__ == "__main__":
    main()
