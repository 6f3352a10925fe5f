"""ResnetEncoderAttention: the ResNet encoder with a 7x7 local self-attention layer behind every stage (reference
networks/resnet_encoder_attention.py:123-166; selected by trainer_dpt.py:78-92 with --model rn_encoder_with_attention / rn_fusion),
with the reference's constructor, forward and state_dict layout: `encoder.*` plus
`atten{1..4}.{rel_h, rel_w, key_conv.weight, query_conv.weight, value_conv.weight}`.

AttentionConv here is the instantiation the encoder uses (kernel 7, stride 1, padding 3, no bias, C -> C; reference
networks/attention.py:9-60 = resnet_encoder_attention.py:23-74): the three 1x1 convolutions are ops.conv1x1 GEMMs (they follow
ops.matrix_precision; shapes outside the tiled kernels take the general / direct kernels, as everywhere in the trunk), the
attention itself is ONE fused fp32 kernel per direction (ops.local_attention7, csrc/sasa.hip) in place of the reference's two
(B,C,H,W,7,7) unfolds, logits, softmax and einsum operand.  `groups` is kept for the constructor signature only: the product
q * k is per channel and the einsum sums over taps, so it has no effect on any output or gradient.
The 2- and 4-channel AttentionConv of the Fusion_v3 front-end (kernel 3, bias) stays in networks/fusion.py.
"""
import torch
import torch.nn as nn
import torch.nn.init as init

from depthcore import ops as _ops
from .resnet_encoder import ResnetEncoder, _conv


class AttentionConv(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, groups=1, bias=False):
        super().__init__()
        if (kernel_size, stride, padding, bool(bias)) != (7, 1, 3, False) or in_channels != out_channels or out_channels % 2:
            raise NotImplementedError("AttentionConv of the attention encoder: kernel_size 7, stride 1, padding 3, bias=False, "
                                      "C -> C with C even (resnet_encoder_attention.py:150-153); got kernel_size=%r stride=%r "
                                      "padding=%r bias=%r %d -> %d" % (kernel_size, stride, padding, bias, in_channels, out_channels))
        assert out_channels % groups == 0, "out_channels should be divided by groups. (example: out_channels: 40, groups: 4)"
        self.out_channels, self.kernel_size, self.stride, self.padding, self.groups = out_channels, kernel_size, stride, padding, groups
        self.rel_h = nn.Parameter(torch.randn(out_channels // 2, 1, 1, kernel_size, 1), requires_grad=True)
        self.rel_w = nn.Parameter(torch.randn(out_channels // 2, 1, 1, 1, kernel_size), requires_grad=True)
        self.key_conv = nn.Conv2d(in_channels, out_channels, kernel_size=1, bias=bias)
        self.query_conv = nn.Conv2d(in_channels, out_channels, kernel_size=1, bias=bias)
        self.value_conv = nn.Conv2d(in_channels, out_channels, kernel_size=1, bias=bias)
        self.reset_parameters()

    def forward(self, x):
        # (padding x by 3 and convolving without a bias = convolving and treating out-of-image taps as k = v = 0: the kernel's
        # contract, so the padded tensor never exists)
        q, k, v = _conv(self.query_conv, x), _conv(self.key_conv, x), _conv(self.value_conv, x)
        return _ops.local_attention7(q, k, v, self.rel_h, self.rel_w)

    def reset_parameters(self):                                  # attention.py:54-60
        init.kaiming_normal_(self.key_conv.weight, mode="fan_out", nonlinearity="relu")
        init.kaiming_normal_(self.value_conv.weight, mode="fan_out", nonlinearity="relu")
        init.kaiming_normal_(self.query_conv.weight, mode="fan_out", nonlinearity="relu")
        init.normal_(self.rel_h, 0, 1)
        init.normal_(self.rel_w, 0, 1)


class ResnetEncoderAttention(ResnetEncoder):
    """resnet_encoder_attention.py:123-166: atten1..atten4 (64, 128, 256, 512 channels, kernel 7, padding 3, groups 8) on the
    output of layer1..layer4; the attention output is the feature map AND the next stage's input.  The reference builds these
    widths whatever the trunk, so over the 256..2048-channel stages of resnet50+ it cannot run: refused here."""

    def __init__(self, num_layers, pretrained, num_input_images=1):
        if num_layers > 34:
            raise ValueError("ResnetEncoderAttention builds 64..512-channel attention layers (resnet_encoder_attention.py:150-153): "
                             "num_layers must be 18 or 34, got {}".format(num_layers))
        super().__init__(num_layers, pretrained, num_input_images)
        self.atten1 = AttentionConv(64, 64, kernel_size=7, padding=3, groups=8)
        self.atten2 = AttentionConv(128, 128, kernel_size=7, padding=3, groups=8)
        self.atten3 = AttentionConv(256, 256, kernel_size=7, padding=3, groups=8)
        self.atten4 = AttentionConv(512, 512, kernel_size=7, padding=3, groups=8)

    def _after_stage(self, n, t):
        return getattr(self, "atten%d" % n)(t)
