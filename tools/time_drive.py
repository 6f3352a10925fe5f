#!/usr/bin/env python3
"""Times drive inference (depthcore.evaluate.predict_disparities_drive, render_drive's two ops) on synthetic device-resident
frames at 192 x 640 with a seeded resnet18 + DepthDecoder and the three recurrent front-ends:
  - v8 and v10 at n_prev 6 and 10: predict_disparities_drive against predict_disparities_windows fed the SAME windows (frame t:
    frames max(0, t - n_prev) .. t) frame by frame, both at `--streams` windows in lockstep;
  - v5: predict_disparities_drive in chunks of `--chunk` against SequencePredictor at width 1 stepped frame by frame;
  - frames the encoder sees per frame of the drive, counted by a forward hook in a pass of its own;
  - one range for the drive -- ops.disparity_range_pooled once + ops.render_disparity_fixed -- against ops.render_disparity
    (a range per image), `--frames` maps to 375 x 1242, rendered `--render_chunk` images a call, `--render_passes` passes over
    the drive inside one timed window (a single pass is well under a millisecond per frame); device buffers only.
The variants alternate inside each of `--repeats` rounds after a warm-up of every shape; device events around each pass.
Prints one JSON line (frames per second: median, and min / max over the rounds).

    python tools/time_drive.py [--frames 128] [--streams 16] [--chunk 16] [--repeats 5]
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
from time_eval_gru import seconds  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--streams", type=int, default=16)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--n_prev", default="6,10")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--photo", default="375,1242")
    ap.add_argument("--render_chunk", type=int, default=16)
    ap.add_argument("--render_passes", type=int, default=20)
    a = ap.parse_args()
    n_prevs = [int(v) for v in a.n_prev.split(",")]
    photo = tuple(int(v) for v in a.photo.split(","))
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    enc = networks.ResnetEncoder(18, False).to(dev)
    dec = networks.DepthDecoder(enc.num_ch_enc).to(dev)
    fronts = {"v8": networks.ConvGRUBlocks_v8((3, 3), True, "cpu", attention=False, height=a.height, width=a.width),
              "v10": networks.ConvGRUBlocks_v9((3, 3), True, "cpu", attention=False, height=a.height, width=a.width),
              "v5": networks.ConvGRUBlocks_v5(kernel_size=(3, 3), bias=True, device="cpu", height=a.height, width=a.width)}
    with torch.no_grad():
        for k in fronts:
            fronts[k] = fronts[k].to(dev)
            for p in fronts[k].parameters():
                p.normal_(0, 0.02)
    for net in [enc, dec] + list(fronts.values()):
        net.eval()
    g = torch.Generator().manual_seed(1)
    N = a.frames
    frames = torch.rand(N, 3, a.height, a.width, generator=g).to(dev)

    def drive(kind, n_prev=0):
        return E.predict_disparities_drive(enc, dec, fronts[kind], N, lambda lo, hi: frames[lo:hi], n_prev=n_prev, streams=a.streams,
                                           chunk=a.chunk)

    def windows(kind, n_prev):
        wins = [list(range(max(0, t - n_prev), t + 1)) for t in range(N)]

        def batch(j, ids, frame_of):
            rows = [frames[wins[c][f]:wins[c][f] + 1] for c, f in zip(ids, frame_of)]
            return rows[0] if len(rows) == 1 else ops.stack_frames([rows])[0]
        return E.predict_disparities_windows(enc, dec, fronts[kind], [len(w) for w in wins], batch, streams=a.streams)

    def v5_width_1():
        sp = E.SequencePredictor(enc, fronts["v5"], dec, streams=1)
        return torch.cat([sp.step(frames[t:t + 1]) for t in range(N)])

    variants = []
    for kind in ("v8", "v10"):
        for n_prev in n_prevs:
            variants.append(("%s_n_prev_%d_drive" % (kind, n_prev), (lambda k=kind, p=n_prev: drive(k, p))))
            variants.append(("%s_n_prev_%d_windows" % (kind, n_prev), (lambda k=kind, p=n_prev: windows(k, p))))
    variants += [("v5_drive", lambda: drive("v5")), ("v5_sequence_predictor_width_1", v5_width_1)]

    disp = drive("v5")                                           # (N,1,h,w) scaled disparities: what the renderer is given
    rc = min(a.render_chunk, N)
    rgb = torch.empty(rc * photo[0] * photo[1] * 3, dtype=torch.uint8, device=dev)

    def render_drive_range():
        for _ in range(a.render_passes):
            rng = ops.disparity_range_pooled(disp, photo)
            for c0 in range(0, N, rc):
                ops.render_disparity_fixed(disp[c0:c0 + rc], photo, rng, out=rgb)

    def render_frame_range():
        for _ in range(a.render_passes):
            for c0 in range(0, N, rc):
                ops.render_disparity(disp[c0:c0 + rc], photo)
    variants += [("render_drive_range", render_drive_range), ("render_frame_range", render_frame_range)]

    for _, fn in variants:                                       # warm-up: every shape of the timed passes
        fn()
    times = {name: [] for name, _ in variants}
    for _ in range(a.repeats):
        for name, fn in variants:
            times[name].append(seconds(fn))
    res = {"config": "resnet18 + DepthDecoder, %d frames at %d x %d, streams %d, chunk %d, fp32, %d rounds; render to %d x %d, %d a call, "
           "%d passes a window" % (N, a.height, a.width, a.streams, a.chunk, a.repeats, photo[0], photo[1], rc, a.render_passes)}
    for name, ts in times.items():
        fps = sorted(N * (a.render_passes if name.startswith("render_") else 1) / t for t in ts)
        res[name + "_frames_per_s"] = round(statistics.median(fps), 2)
        res[name + "_frames_per_s_range"] = [round(fps[0], 2), round(fps[-1], 2)]
    for kind in ("v8", "v10"):
        for n_prev in n_prevs:
            k = "%s_n_prev_%d" % (kind, n_prev)
            res[k + "_drive_vs_windows"] = round(res[k + "_drive_frames_per_s"] / res[k + "_windows_frames_per_s"], 3)
    res["v5_drive_vs_sequence_predictor_width_1"] = round(res["v5_drive_frames_per_s"] / res["v5_sequence_predictor_width_1_frames_per_s"], 3)
    res["render_drive_range_vs_frame_range"] = round(res["render_drive_range_frames_per_s"] / res["render_frame_range_frames_per_s"], 3)
    # frames through the encoder per frame of the drive (exact: a forward hook, outside the timing)
    seen = []
    hook = enc.register_forward_hook(lambda m, inp, out: seen.append(inp[0].shape[0]))
    for n_prev in n_prevs:
        for name, fn in (("drive", drive), ("windows", windows)):
            del seen[:]
            fn("v8", n_prev)
            res["encoder_frames_per_frame_n_prev_%d_%s" % (n_prev, name)] = round(sum(seen) / N, 3)
    hook.remove()
    # what the two compositions compute agrees (fp32, differently tiled convolutions)
    res["max_abs_diff_drive_vs_windows_v8"] = float((drive("v8", n_prevs[0]) - windows("v8", n_prevs[0])).abs().max())
    res["max_abs_diff_drive_vs_windows_v10"] = float((drive("v10", n_prevs[0]) - windows("v10", n_prevs[0])).abs().max())
    res["max_abs_diff_v5_drive_vs_width_1"] = float((drive("v5") - v5_width_1()).abs().max())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
