from .mono_dataset import MonoDataset, parse_line                                                   # noqa: F401
from .kitti_dataset import KITTIDataset, KITTIRAWDataset, KITTIOdomDataset, KITTIDepthDataset      # noqa: F401
from .kitti_dataset_seq import KITTISequenceDataset, KITTIDataset_v1, generate_sequences            # noqa: F401
