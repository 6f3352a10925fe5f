"""A tiny KITTI-shaped tree of PIL-written PNGs for the dataset / loader / training-loop tests."""
import os

import numpy as np
from PIL import Image

DRIVES = {"2011_09_26/2011_09_26_drive_0001_sync": (47, 155), "2011_09_28/2011_09_28_drive_0002_sync": (45, 150)}


def frame_pixels(h, w, seed):
    """Smooth-ish random (h, w, 3) uint8 image: structure at several scales, so that a resize has something to filter."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([127 + 80 * np.sin(x / (5 + c) + seed) * np.cos(y / (3 + c)) for c in range(3)], -1)
    return np.clip(img + rng.randint(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)


def write_raw_tree(root, frames=6, sides=("l",), drives=None):
    """<root>/<drive>/image_0{2,3}/data/<10 digits>.png, `frames` frames per drive -> {(drive, frame, side): pixels}."""
    pixels = {}
    for d, (drive, (h, w)) in enumerate(sorted((drives or DRIVES).items())):
        for side in sides:
            folder = os.path.join(root, drive, "image_0%d" % {"l": 2, "r": 3}[side], "data")
            os.makedirs(folder, exist_ok=True)
            for i in range(frames):
                img = frame_pixels(h, w, 1000 * d + 10 * i + (side == "r"))
                Image.fromarray(img).save(os.path.join(folder, "%010d.png" % i))
                pixels[(drive, i, side)] = img
    return pixels


def write_splits(splits_dir, split, train_lines, val_lines):
    os.makedirs(os.path.join(splits_dir, split), exist_ok=True)
    for mode, lines in (("train", train_lines), ("val", val_lines)):
        with open(os.path.join(splits_dir, split, "%s_files.txt" % mode), "w") as f:
            f.write("\n".join(lines) + "\n")
