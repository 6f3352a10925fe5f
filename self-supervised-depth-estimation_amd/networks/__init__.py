"""Drop-in for the reference's `networks` package on the hot path (networks/__init__.py:1-9)."""
from .resnet_encoder import ResnetEncoder
from .resnet_encoder_attention import ResnetEncoderAttention


ATTENTION_MODELS = ("rn_encoder_with_attention", "rn_fusion")     # trainer_dpt.py:78-92


def depth_encoder_class(model):
    """The depth encoder that the option `--model` names: ResnetEncoderAttention for the two self-attention models of the
    reference's trainer_dpt.py:78-92, the plain ResnetEncoder for every other value (the default "dpt_gru" included)."""
    return ResnetEncoderAttention if model in ATTENTION_MODELS else ResnetEncoder
from .depth_decoder import DepthDecoder
from .pose_decoder import PoseDecoder
from .pose_cnn import PoseCNN
from .fusion import Fusion_v3, FeatureFusionBlock_v3, ResidualAttentionUnit, AttentionConv, UpscalePS
from .convgru import ConvGRUBlocks_v5, ConvGRUModel_v1, ConvGRUCell
from .convlstm import ConvGRUBlocks_v8, ConvLSTMModel_v1, ConvLSTMCell_v1, FeatureFusionBlock_v2
from .convgru_c2f import ConvGRUBlocks_v9
