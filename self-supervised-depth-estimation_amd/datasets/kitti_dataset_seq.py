"""KITTI sequence items for the ConvGRU front-end (reference datasets/kitti_dataset_seq.py `KITTIDataset_v1` and the tuple
generation of gru_utils.py:88-122).  Host-side and decode-only, like the other datasets: which files make up an item.  The
pyramid, the mirror and the per-image ColorJitter belong to the device (depthcore.data.GpuPreprocessor.sequence, fed by
depthcore.loader.SequenceLoader), the random draws to the loader (depthcore.data.sample_sequence).

An item is n + 2 consecutive frames of one drive's left camera: the centre window is frames 1..n, the left window 0..n-1, the
right window 2..n+1.  Its "depth_gt" is the velodyne map of the n centre frames through camera 2."""
import os
import random

import numpy as np

from depthcore import lidar


def count_frames(data_path, drive):
    """The number of files in <drive>/image_02/data (gru_utils.py:88-99)."""
    return len(os.listdir(os.path.join(data_path, drive, "image_02", "data")))


def generate_sequences(data_path, drives, n, n_tuples, rng=random):
    """The items of a list of drives ("date/drive" lines), in the order of the list (gru_utils.py:101-122 with k = 2):
    per drive max(n_frames // n, n_tuples) start frames drawn by `rng.sample(range(n_frames - 1 - n - 2), count)`, each the
    item (drive, range(x, x + n + 2)).  Drawn once, when the loaders are built.  A drive too short for its sample raises
    ValueError, as random.sample does, naming the drive."""
    n, n_tuples = int(n), int(n_tuples)
    if n < 1:
        raise ValueError("generate_sequences: a sequence has at least one centre frame, got n = %d" % n)
    items = []
    for drive in drives:
        n_frames = count_frames(data_path, drive)
        count = max(n_frames // n, n_tuples)
        right_boundary = n_frames - 1 - n - 2
        if right_boundary < count:
            raise ValueError("%s has %d frames: too short for %d sequences of %d + 2 frames (%d start frames to draw from)"
                             % (drive, n_frames, count, n, max(right_boundary, 0)))
        items.extend((drive, range(x, x + n + 2)) for x in rng.sample(range(right_boundary), count))
    return items


class KITTISequenceDataset:
    """The reference's positional constructor (kitti_dataset_seq.py:29) plus `img_ext`.  sequences: [(drive, frame range)]
    as `generate_sequences` makes them."""
    device_depth = True        # the loader projects the scans on the device (depthcore/loader.py)
    frame_idxs = [0, -1, 1]
    num_scales = 4

    def __init__(self, data_path, height, width, n, sequences, is_train, img_ext=".jpg"):
        self.data_path = data_path
        self.height, self.width, self.n = int(height), int(width), int(n)
        self.sequences = list(sequences)
        self.is_train = bool(is_train)
        self.img_ext = img_ext
        self.full_res_shape = (1242, 375)                      # (width, height)
        self.K = np.array([[0.58, 0, 0.5, 0],
                           [0, 1.92, 0.5, 0],
                           [0, 0, 1, 0],
                           [0, 0, 0, 1]], dtype=np.float32)   # kitti_dataset_seq.py:58-61, scaled per level by GpuPreprocessor.intrinsics
        for drive, frames in self.sequences:
            if len(frames) != self.n + 2:
                raise ValueError("%s: an item of n = %d has %d frames, got %d" % (drive, self.n, self.n + 2, len(frames)))
        self.load_depth = self.check_depth()

    def __len__(self):
        return len(self.sequences)

    def get_image_path(self, frame_index, sequence_name):
        scene_date, scene_name = sequence_name.split("/")
        return os.path.join(self.data_path, scene_date, scene_name, "image_02", "data", "{:010d}{}".format(int(frame_index), self.img_ext))

    def velo_path(self, frame_index, sequence_name):
        scene_date, scene_name = sequence_name.split("/")
        return os.path.join(self.data_path, scene_date, scene_name, "velodyne_points/data", "{:010d}.bin".format(int(frame_index)))

    def frame_paths(self, index):
        """The n + 2 image files of item `index`, in frame order."""
        drive, frames = self.sequences[index]
        return [self.get_image_path(x, drive) for x in frames]

    def scan_paths(self, index):
        """The velodyne scans of the n centre frames."""
        drive, frames = self.sequences[index]
        return [self.velo_path(x, drive) for x in list(frames)[1:-1]]

    def calib_dir(self, index):
        return os.path.join(self.data_path, self.sequences[index][0].split("/")[0])

    def check_depth(self):
        """Whether the first item's first centre scan exists.  (The reference's method reads `self.filenames`, which its class
        never sets, and its `__getitem__` builds "depth_gt" unconditionally; here drives without scans train without the
        depth metrics, as with the other datasets.)"""
        return bool(self.sequences) and os.path.isfile(self.scan_paths(0)[0])

    def get_depth(self, frame_index, sequence_name, do_flip):
        """(375, 1242) float32 on the host: generate_depth_map(calib, scan, 2), resized to full_res_shape, mirrored with the
        flip (kitti_dataset_seq.py:177-197) -- the values the loader's device projection produces."""
        P, size = lidar.velo_to_image(os.path.join(self.data_path, sequence_name.split("/")[0]), 2)
        depth = lidar.depth_map_host(lidar.load_velodyne_points(self.velo_path(frame_index, sequence_name)), P, size)
        return lidar.resize_flip(depth, self.full_res_shape, do_flip)


KITTIDataset_v1 = KITTISequenceDataset       # the reference's name
