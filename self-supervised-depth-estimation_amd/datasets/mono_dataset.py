"""The host half of the reference's MonoDataset (datasets/mono_dataset.py:41-211): which files make up an item, and nothing
else.  The reference's `__getitem__` also resizes, jitters and converts every frame in a CPU worker; here the item is the
DECODED native frames as uint8 arrays plus its metadata, and the pyramid belongs to the device
(depthcore.data.GpuPreprocessor.ragged, fed by depthcore.loader.BatchLoader).  The random draws (colour augmentation, flip)
are the loader's as well (depthcore.data.sample_item): an item is a pure function of (index, do_flip).
"""
import os

import numpy as np
from PIL import Image


def parse_line(line):
    """One line of a split file -> (folder, frame_index, side): "folder index side", or a single token (mono_dataset.py:145-156:
    any line that does not have three tokens is frame 0 without a side)."""
    tok = line.split()
    if len(tok) == 3:
        return tok[0], int(tok[1]), tok[2]
    return tok[0], 0, None


def load_rgb(path):
    """Decoded (H, W, 3) uint8 array of an image file (the reference's pil_loader: convert('RGB'))."""
    with open(path, "rb") as f:
        with Image.open(f) as img:
            return np.asarray(img.convert("RGB"))


class MonoDataset:
    """Constructor signature of the reference (mono_dataset.py:41-49).  Subclasses give `K`, `full_res_shape`,
    `get_image_path`, `check_depth` and `get_depth`."""

    def __init__(self, data_path, filenames, height, width, frame_idxs, num_scales, is_train=False, img_ext='.jpg'):
        self.data_path = data_path
        self.filenames = list(filenames)
        self.height, self.width = height, width
        self.frame_idxs = list(frame_idxs)
        self.num_scales = num_scales
        self.is_train = is_train
        self.img_ext = img_ext
        self.load_depth = self.check_depth()

    def __len__(self):
        return len(self.filenames)

    def frame_paths(self, index):
        """The image file of every entry of `frame_idxs`, in that order: "s" is the other side's image of the same instant
        (mono_dataset.py:161-163); a temporal neighbour whose file does not exist is replaced by frame 0 (:165-170: the first
        and last frame of a drive)."""
        folder, frame_index, side = parse_line(self.filenames[index])
        centre = self.get_image_path(folder, frame_index, side)
        paths = []
        for i in self.frame_idxs:
            if i == "s":
                path = self.get_image_path(folder, frame_index, {"r": "l", "l": "r"}[side])
            elif i == 0:
                path = centre
            else:
                path = self.get_image_path(folder, frame_index + i, side)
                if not os.path.exists(path):
                    path = centre
            paths.append(path)
        return paths

    device_depth = False      # True: the class has `depth_source`, and a loader may build "depth_gt" on the device from it

    def metadata(self, index, do_flip=False, device_depth=False):
        """Everything of an item that is not a colour image: "depth_gt" (1, H, W) float32 when the dataset has ground truth
        (:198-201), "stereo_T" (4, 4) float32 when "s" is among the frames (:203-209: the baseline of 0.1 units changes sign
        with the side and with the flip).  device_depth=True: the caller builds "depth_gt" itself from `depth_source` when
        the class allows it (`device_depth`), so it is left out here."""
        folder, frame_index, side = parse_line(self.filenames[index])
        out = {}
        if self.load_depth and not (device_depth and self.device_depth):
            out["depth_gt"] = np.expand_dims(self.get_depth(folder, frame_index, side, do_flip), 0).astype(np.float32)
        if "s" in self.frame_idxs:
            stereo_T = np.eye(4, dtype=np.float32)
            baseline_sign = -1 if do_flip else 1
            side_sign = -1 if side == "l" else 1
            stereo_T[0, 3] = side_sign * baseline_sign * 0.1
            out["stereo_T"] = stereo_T
        return out

    def get_item(self, index, do_flip=False):
        """{("color", f, -1): (Hn, Wn, 3) uint8 as decoded -- NOT mirrored: the device's width pass carries the flip --, plus
        `metadata(index, do_flip)`}."""
        item = {("color", f, -1): load_rgb(p) for f, p in zip(self.frame_idxs, self.frame_paths(index))}
        item.update(self.metadata(index, do_flip))
        return item

    def __getitem__(self, index):
        return self.get_item(index)

    def get_image_path(self, folder, frame_index, side):
        raise NotImplementedError

    def check_depth(self):
        raise NotImplementedError

    def get_depth(self, folder, frame_index, side, do_flip):
        raise NotImplementedError
