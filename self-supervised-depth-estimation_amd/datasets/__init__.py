from .mono_dataset import MonoDataset, parse_line                                                   # noqa: F401
from .kitti_dataset import KITTIDataset, KITTIRAWDataset, KITTIOdomDataset, KITTIDepthDataset      # noqa: F401
