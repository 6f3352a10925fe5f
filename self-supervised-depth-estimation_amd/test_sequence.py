"""test_simple.py for the recurrent front-ends: a model trained by train_gru.py (encoder.pth, gru.pth, depth.pth) and a folder of
the consecutive frames of one drive in, for every frame `<name>_disp.npy` (the scaled disparity at network resolution, (1,1,h,w)
float32) and `<name>_disp.jpeg` (its magma rendering at the photo's size) out, and one `range.json`.

    python test_sequence.py --image_path <folder of consecutive frames> --load_weights_folder <weights_N>
                            --gru_version v5|v8|v10 [--n_prev_images 6] [--batch_size 16] [--ext jpg]
                            [--range drive|frame] [--percentile 95] [--out_dir D] [--num_layers 18]

The frames are the folder's files of the extension in natural numeric order of their names (2.jpg before 10.jpg); they must share
one native size.  The networks are loaded as evaluate_depth_gru.py loads them (the size is the one stored in encoder.pth).  The
model runs on the whole drive (depthcore.evaluate.predict_disparities_drive): v5 carries its hidden state from the first frame
to the last; v8 / v10 predict every frame from the window of that frame and the --n_prev_images frames before it
(evaluate_depth_gru.py's protocol; --n_prev_images 10 is the reference's for v10), every frame passing the encoder and the
decoder once.  --batch_size is both the number of frames per encoder batch and the number of windows in lockstep.

--range drive (the default) colours all frames with ONE range -- the minimum and the --percentile (95) of the whole drive's
upsampled disparities (depthcore.evaluate.render_drive) --, so that a surface keeps its colour from frame to frame; --range
frame ranges every frame by itself, the bytes test_simple.py writes for that disparity, which flicker as a video.  range.json
holds the mode, vmin, vmax (null with --range frame, where frame_ranges lists every frame's pair), the percentile, the number
of frames, the gru version and n_prev.

The photos are decoded on a small thread pool one batch ahead (PIL) and resized on the device (GpuPreprocessor, Pillow's bits);
the host encodes the JPEGs.  matplotlib, cv2 and torchvision are not imported, no video is written, nothing is fetched.
--no_cuda and every --gru_version but v5, v8 and v10 are refused, --post_process does not exist.
"""
import argparse
import concurrent.futures
import json
import os
import re
import sys

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

MIN_DEPTH, MAX_DEPTH = 0.1, 100.0                   # test_simple.py:133
PERCENTILE = 95.0                                   # test_simple.py:138
VERSIONS = ("v5", "v8", "v10")
DECODE_THREADS = 8


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Drive inference with a recurrent front-end: disparity .npy and magma .jpeg per frame.")
    parser.add_argument("--image_path", type=str, required=True, help="folder holding the consecutive frames of one drive")
    parser.add_argument("--load_weights_folder", type=str, required=True, help="checkpoint folder: encoder.pth, gru.pth, depth.pth")
    parser.add_argument("--gru_version", type=str, default="v5", help="v5 (ConvGRU), v8 (ConvLSTM) or v10 (coarse-to-fine ConvGRU)")
    parser.add_argument("--n_prev_images", type=int, default=6, help="v8 / v10: frames before a frame that its window holds")
    parser.add_argument("--batch_size", type=int, default=16, help="frames per encoder batch and windows in lockstep")
    parser.add_argument("--ext", type=str, default="jpg", help="image extension to search for in the folder")
    parser.add_argument("--range", type=str, default="drive", choices=["drive", "frame"],
                        help="drive: one colour range for all frames; frame: every frame by itself (test_simple.py's pictures)")
    parser.add_argument("--percentile", type=float, default=PERCENTILE, help="the upper end of the colour range (test_simple.py: 95)")
    parser.add_argument("--out_dir", type=str, default=None, help="where the outputs go (default: the image folder)")
    parser.add_argument("--num_layers", type=int, default=18, choices=[18, 34, 50, 101, 152], help="number of resnet layers")
    parser.add_argument("--no_cuda", action="store_true", help="refused: there is no CPU path")
    return parser.parse_args(argv)


def natural_key(name):
    """Digit runs compare as numbers: 2.jpg < 10.jpg, 0000000009.png < 0000000010.png, a2b < a10b."""
    return [int(p) if p.isdigit() else p for p in re.split(r"(\d+)", name)]


def find_frames(folder, ext):
    """The folder's files *.ext in natural numeric order of their names; a *_disp.ext is an output, not a frame."""
    if not os.path.isdir(folder):
        raise FileNotFoundError("Can not find a folder at args.image_path: {}".format(folder))
    suffix = ".{}".format(ext)
    names = [n for n in os.listdir(folder) if n.endswith(suffix) and not n[:-len(suffix)].endswith("_disp")
             and os.path.isfile(os.path.join(folder, n))]
    if not names:
        raise FileNotFoundError("{} holds no *.{} frame".format(folder, ext))
    return [os.path.join(folder, n) for n in sorted(names, key=natural_key)]


def check_args(args):
    """The refusals, before a file or the device is touched."""
    if args.no_cuda:
        raise ValueError("--no_cuda: there is no CPU path, the networks and the rendering run on HIP kernels only")
    if args.gru_version not in VERSIONS:
        raise NotImplementedError("--gru_version {!r}: drive inference covers v5 (ConvGRUBlocks_v5), v8 (ConvGRUBlocks_v8) and v10 "
                                  "(ConvGRUBlocks_v9 without attention)".format(args.gru_version))
    if args.batch_size <= 0:
        raise ValueError("--batch_size must be positive")
    if args.n_prev_images < 0:
        raise ValueError("--n_prev_images must not be negative")
    if not 0.0 <= args.percentile <= 100.0:
        raise ValueError("--percentile must lie in [0, 100]")


def native_size(paths):
    """(height, width) shared by all frames, from the files' headers; two sizes in one drive are refused."""
    first = None
    for p in paths:
        with Image.open(p) as im:
            size = (im.height, im.width)
        if first is None:
            first = (size, p)
        elif size != first[0]:
            raise ValueError("the frames of a drive share one size: {} is {}x{} but {} is {}x{} (width x height)".format(
                first[1], first[0][1], first[0][0], p, size[1], size[0]))
    return first[0]


def _decode(path):
    with open(path, "rb") as f:
        return np.asarray(Image.open(f).convert("RGB"))


class FrameFeeder:
    """batch_fn of predict_disparities_drive: frames lo .. hi - 1 decoded on the pool's threads (the next batch is submitted
    before this one is awaited), uploaded as one array and resized on the device."""

    def __init__(self, paths, size, height, width, device):
        from depthcore.data import GpuPreprocessor
        self.paths, self.size, self.device = paths, size, device
        self.prep = GpuPreprocessor(height, width, num_scales=1, frame_idxs=(0,), device=device)
        self.pool = concurrent.futures.ThreadPoolExecutor(DECODE_THREADS)
        self.pending = {}

    def _submit(self, lo, hi):
        for i in range(lo, min(hi, len(self.paths))):
            if i not in self.pending:
                self.pending[i] = self.pool.submit(_decode, self.paths[i])

    def __call__(self, lo, hi):
        self._submit(lo, hi)
        self._submit(hi, hi + (hi - lo))
        imgs = [self.pending.pop(i).result() for i in range(lo, hi)]
        for i, im in zip(range(lo, hi), imgs):
            if im.shape != self.size + (3,):
                raise ValueError("{} decodes to {}, its header said {}".format(self.paths[i], im.shape[:2], self.size))
        native = torch.from_numpy(np.stack(imgs)[None]).to(self.device)
        return self.prep(native)[("color", 0, 0)]

    def close(self):
        for f in self.pending.values():
            f.cancel()
        self.pool.shutdown(wait=True)


def predict_drive(args, keep_rgb=False):
    """-> one dict per frame: image, npy, jpeg (paths), size (Ho, Wo), range (vmin, vmax) and, with keep_rgb, rgb -- the
    (Ho, Wo, 3) uint8 array handed to PIL."""
    check_args(args)
    paths = find_frames(args.image_path, args.ext)
    size = native_size(paths)
    out_dir = args.out_dir or args.image_path
    os.makedirs(out_dir, exist_ok=True)

    import evaluate_depth_gru as EG
    from depthcore import evaluate as E

    device = torch.device("cuda", torch.cuda.current_device())
    opt = argparse.Namespace(load_weights_folder=args.load_weights_folder, num_layers=args.num_layers, gru_version=args.gru_version)
    encoder, front, decoder, height, width = EG.load_networks(opt, device)
    print("-> Predicting on a drive of {:d} frames with {} at {}x{}".format(len(paths), args.gru_version, width, height))
    feeder = FrameFeeder(paths, size, height, width, device)
    try:
        pred = E.predict_disparities_drive(encoder, decoder, front, len(paths), feeder, n_prev=args.n_prev_images,
                                           streams=args.batch_size, chunk=args.batch_size, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH)
    finally:
        feeder.close()
    summary = {"range": args.range, "vmin": None, "vmax": None, "percentile": args.percentile, "n_frames": len(paths),
               "gru_version": args.gru_version, "n_prev": args.n_prev_images}
    if args.range == "drive":
        images, (vmin, vmax) = E.render_drive(pred, size, args.percentile)
        ranges = [(float(vmin), float(vmax))] * len(paths)
        summary.update(vmin=float(vmin), vmax=float(vmax))
    else:
        images, per_frame = E.render_disparities(pred, size, args.percentile)
        ranges = [(float(r[0]), float(r[1])) for r in per_frame]
        summary["frame_ranges"] = [list(r) for r in ranges]
    scaled = pred.cpu().numpy()
    records = []
    for k, image_path in enumerate(paths):
        name = os.path.splitext(os.path.basename(image_path))[0]
        rec = {"image": image_path, "npy": os.path.join(out_dir, "{}_disp.npy".format(name)),
               "jpeg": os.path.join(out_dir, "{}_disp.jpeg".format(name)), "size": size, "range": ranges[k]}
        np.save(rec["npy"], scaled[k:k + 1])
        Image.fromarray(images[k]).save(rec["jpeg"])
        if keep_rgb:
            rec["rgb"] = images[k]
        records.append(rec)
    with open(os.path.join(out_dir, "range.json"), "w") as f:
        json.dump(summary, f, indent=1)
    print("-> Done: {:d} frames, colour range {} -- outputs in {}".format(
        len(paths), "per frame" if args.range == "frame" else "[{:.6g}, {:.6g}]".format(summary["vmin"], summary["vmax"]), out_dir))
    return records


def main(argv=None, keep_rgb=False):
    return predict_drive(parse_args(argv), keep_rgb)


if __name__ == "__main__":
    main()
