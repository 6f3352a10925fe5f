#!/usr/bin/env python3
"""Classic staging order against the staggered one (dc_set_wino_phase) on the weight-gradient shapes of a step, same process,
modes alternating, one pair of device events around every launch (median of the launches of a mode).

    timeout -k 10 300 python3 tools/ab_wino_phase.py [--out DIR] [--modes 1,-1,0] [B,Ci,Co,H,W ...]

Times dc_wino3x3_wgrad -- the wino_wgrad_kernel launch AND its slab reduction -- on the shapes of tools/sweep_wgrad.py.  The
weight of a shape is its launches per step (ResNet-18 depth encoder at batch 12, pose encoder at batch 24: 4 / 3 / 3 / 3
basic-block convolutions per stage; one launch per decoder level; the 32-channel levels take one-group blocks, which keep the
classic order in every mode and are the table's control rows).  The first mode is the baseline.  A mode may be the shipped
default only if its weighted sum is lower AND no shape with more than 2 % of the time is more than 2 % slower.  Writes the table
to DIR/ab_wino_phase.txt (default: build/ under the repository) as well as to stdout.  Run it under a time limit of its
own."""
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "self-supervised-depth-estimation_amd"))
from depthcore import _lib  # noqa: E402
from depthcore._lib import ptr  # noqa: E402

CLASSIC, AUTO = 1, -1
# (B, Ci, Co, H, W): launches per step
WGRAD = {(12, 64, 64, 48, 160): 4, (24, 64, 64, 48, 160): 4, (12, 128, 128, 24, 80): 3, (24, 128, 128, 24, 80): 3,
         (12, 256, 256, 12, 40): 3, (24, 256, 256, 12, 40): 3, (12, 512, 512, 6, 20): 3, (24, 512, 512, 6, 20): 3,
         (12, 512, 256, 12, 40): 1, (12, 256, 128, 24, 80): 1, (12, 128, 64, 48, 160): 1, (12, 96, 32, 96, 320): 1, (12, 64, 32, 48, 160): 1}


def per_launch_us(fn, n):
    """Median over n launches, each between its own pair of device events."""
    for _ in range(3):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3


def ab(L, fn, modes, reps=3, n=20):
    """{mode: best median} with the modes alternating inside every repetition."""
    best = {m: float("inf") for m in modes}
    for _ in range(reps):
        for m in modes:
            L.dc_set_wino_phase(m)
            best[m] = min(best[m], per_launch_us(fn, n))
    return best


def main():
    out_dir, modes, shapes = os.path.join(REPO, "build"), [CLASSIC, AUTO, 0], []
    it = iter(sys.argv[1:])
    for a in it:
        if a == "--out":
            out_dir = next(it)
        elif a == "--modes":
            modes = [int(v) for v in next(it).split(",")]
        else:
            shapes.append(tuple(int(v) for v in a.split(",")))
    weights = {s: WGRAD.get(s, 1) for s in shapes} if shapes else WGRAD
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    rows, lines = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    before = L.dc_set_wino_phase(CLASSIC)
    try:
        for (B, Ci, Co, H, W), wt in weights.items():
            x = torch.randn(B, Ci, H, W, device="cuda")
            y = torch.randn(B, Co, H, W, device="cuda")
            ws = torch.empty(L.dc_wino3x3_wgrad_workspace(B, Ci, Co, H, W), dtype=torch.uint8, device="cuda")
            dw = torch.empty(Co, Ci, 3, 3, device="cuda")
            fn = lambda: L.dc_wino3x3_wgrad(ptr(x), ptr(y), ptr(dw), ws.data_ptr(), B, Ci, Co, H, W, st)  # noqa: E731
            assert fn() == 0
            t = ab(L, fn, modes)
            rows.append((wt, t))
            say("B=%2d %3d->%3d %3dx%3d x%d | " % (B, Ci, Co, H, W, wt) + " | ".join(
                "mode %2d %7.1f us%s" % (m, t[m], "" if m == modes[0] else " (%+5.1f %%)" % (100 * (t[m] / t[modes[0]] - 1))) for m in modes))
    finally:
        L.dc_set_wino_phase(before)
    base = modes[0]
    total = {m: sum(wt * t[m] for wt, t in rows) for m in modes}
    for m in modes[1:]:
        worst = max((t[m] / t[base] - 1 for wt, t in rows if wt * t[base] > 0.02 * total[base]), default=0.0)
        ships = total[m] < total[base] and worst <= 0.02
        say("wgrad: mode %d %.0f us per step against mode %d %.0f us (%+.2f %%); worst shape above 2 %% of the time %+.1f %% -> %s"
            % (m, total[m], base, total[base], 100 * (total[m] / total[base] - 1), 100 * worst, "meets the rule" if ships else "does not meet the rule"))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "ab_wino_phase.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
