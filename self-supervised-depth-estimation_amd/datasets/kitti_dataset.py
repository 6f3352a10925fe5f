"""KITTI file layouts (reference datasets/kitti_dataset.py): raw drives, odometry sequences and the depth benchmark's
ground-truth maps.  Host-side only: paths, the normalised intrinsics and the ground-truth depth."""
import os

import numpy as np
from PIL import Image

from depthcore import lidar

from .mono_dataset import MonoDataset, parse_line


class KITTIDataset(MonoDataset):
    def __init__(self, *args, **kwargs):
        # intrinsics normalised by the image size (kitti_dataset.py:25-28): scaled per pyramid level by
        # GpuPreprocessor.intrinsics
        self.K = np.array([[0.58, 0, 0.5, 0],
                           [0, 1.92, 0.5, 0],
                           [0, 0, 1, 0],
                           [0, 0, 0, 1]], dtype=np.float32)
        self.full_res_shape = (1242, 375)                      # (width, height), as PIL takes it
        self.side_map = {"2": 2, "3": 3, "l": 2, "r": 3}
        super().__init__(*args, **kwargs)

    def check_depth(self):
        return False


class KITTIRAWDataset(KITTIDataset):
    """Raw drives: <data_path>/<date>/<drive>/image_0{2,3}/data/<10 digits><ext>, with "depth_gt" projected from the velodyne
    scans <drive>/velodyne_points/data/<10 digits>.bin through the date folder's calibration (kitti_dataset.py:33-43, 71-86)
    when the first line's scan exists; without scans check_depth() is False and the training loop skips the depth metrics,
    as the reference does.

    device_depth: the loader may project the scans on the device instead of calling `get_depth` -- it takes `depth_source`
    and passes device_depth=True to `metadata` (depthcore/loader.py); `get_depth` is the host path of the same values."""
    device_depth = True

    def get_image_path(self, folder, frame_index, side):
        return os.path.join(self.data_path, folder, "image_0{}/data".format(self.side_map[side]),
                            "{:010d}{}".format(frame_index, self.img_ext))

    def velo_path(self, folder, frame_index):
        return os.path.join(self.data_path, folder, "velodyne_points/data", "{:010d}.bin".format(int(frame_index)))

    def check_depth(self):
        folder, frame_index, side = parse_line(self.filenames[0])
        return side is not None and os.path.isfile(self.velo_path(folder, frame_index))

    def depth_source(self, index):
        """-> (scan path, calibration folder, camera 2 | 3) of item `index`."""
        folder, frame_index, side = parse_line(self.filenames[index])
        return self.velo_path(folder, frame_index), os.path.join(self.data_path, folder.split("/")[0]), self.side_map[side]

    def get_depth(self, folder, frame_index, side, do_flip):
        """(375, 1242) float32: the native-size map (vel_depth=False), resized to full_res_shape by Pillow's NEAREST rule (the
        reference: skimage.transform.resize(order=0); identical for 1242 x 375 drives) and mirrored with the flip."""
        P, size = lidar.velo_to_image(os.path.join(self.data_path, folder.split("/")[0]), self.side_map[side])
        depth = lidar.depth_map_host(lidar.load_velodyne_points(self.velo_path(folder, frame_index)), P, size)
        return lidar.resize_flip(depth, self.full_res_shape, do_flip)


class KITTIOdomDataset(KITTIDataset):
    """Odometry: <data_path>/sequences/<2 digits>/image_{2,3}/<6 digits><ext>."""

    def get_image_path(self, folder, frame_index, side):
        return os.path.join(self.data_path, "sequences/{:02d}".format(int(folder)), "image_{}".format(self.side_map[side]),
                            "{:06d}{}".format(frame_index, self.img_ext))


class KITTIDepthDataset(KITTIDataset):
    """Raw-drive images with the depth benchmark's maps: <folder>/proj_depth/groundtruth/image_0{2,3}/<10 digits>.png,
    uint16 in 1/256 m."""

    def get_image_path(self, folder, frame_index, side):
        return os.path.join(self.data_path, folder, "image_0{}/data".format(self.side_map[side]),
                            "{:010d}{}".format(frame_index, self.img_ext))

    def depth_path(self, folder, frame_index, side):
        return os.path.join(self.data_path, folder, "proj_depth/groundtruth/image_0{}".format(self.side_map[side]),
                            "{:010d}.png".format(frame_index))

    def check_depth(self):
        folder, frame_index, side = parse_line(self.filenames[0])
        return side is not None and os.path.isfile(self.depth_path(folder, frame_index, side))

    def get_depth(self, folder, frame_index, side, do_flip):
        with Image.open(self.depth_path(folder, frame_index, side)) as img:
            depth_gt = np.array(img.resize(self.full_res_shape, Image.NEAREST)).astype(np.float32) / 256
        return np.fliplr(depth_gt) if do_flip else depth_gt
