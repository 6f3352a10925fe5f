"""Coarse-to-fine ConvGRU front-end, `gru_version = v10` (reference networks/rnn.py:472-569 `ConvGRUBlocks_v9` built with
attention=False; :101-158 `ConvGRUCell` / `ConvGRUModel_v1`, :739-779 `FeatureFusionBlock_v2`; caller trainer_gru.py:716-764
`run_gru_v9_v10`) with the reference's constructor and state_dict layout: `cgru_{0..3}.cgru_1.conv_gates.{weight,bias}`,
`cgru_{k}.cgru_1.conv_can.{weight,bias}`, `cgru_{k}.h0_layer1`, `fusion_{0..3}.resConfUnit{1,2}.conv{1,2}.{weight,bias}`,
`fusion_{k}.conv3x3.conv.{weight,bias}`.

It is v8's arrangement (networks/convlstm.py) with the ConvLSTM cells replaced by ConvGRU cells: one learned initial state per
scale and no cell state.  Behind the depth decoder (run with pre_disp=True), per frame and scale s = 3, 2, 1, 0:
    x_s     = dec_3                      (s = 3)        cat(dec_s, up_{s+1})      (s < 3)
    gates   = sigmoid(conv_gates(cat(x_s, h)))           fused conv block, [reset | update]
    cnm     = tanh(conv_can(cat(x_s, reset * h)))        dc_gru_rh + fused conv block
    a       = resConfUnit1(cat(dec_3, dec_3) if s == 3 else x_s)
    h', pre, up = GRU hand-over(gates, h, cnm, a)        dc_gru_handover: h' = (1 - u) h + u cnm, pre = relu(a + (h + h') / 2),
                                                         up = pixel_shuffle(tanh(pre), 2)
    disp_s  = sigmoid(conv3x3(reflect_pad(resConfUnit2(pre))))
The ReLU inside the hand-over is the reference's in-place nn.ReLU of resConfUnit2, as for v8: the tensor that is shuffled is
tanh(relu(.)).  `--gru_version v9` is the same block with ResidualAttentionUnits in the fusion blocks (attention=True): not built.
The frames are chained by plain autograd."""
import torch
import torch.nn as nn

from depthcore import ops as _ops
from depthcore._lib import DepthcoreError
from .convgru import ConvGRUModel_v1
from .convlstm import FeatureFusionBlock_v2


class ConvGRUBlocks_v9(nn.Module):
    """networks/rnn.py:472-569.  The reference hard-codes the 192 x 640 map sizes and the decoder's channel counts; `height` /
    `width` / `num_ch_dec` reproduce those numbers by default and let other input sizes be built, as ConvGRUBlocks_v8 does."""

    def __init__(self, kernel_size, bias, device, attention=True, height=192, width=640, num_ch_dec=(16, 32, 64, 128)):
        super().__init__()
        if attention:
            raise NotImplementedError("ConvGRUBlocks_v9(attention=True) is gru_version v9, whose fusion blocks hold residual "
                                      "attention units: not built; v10 is ConvGRUBlocks_v9(attention=False) (trainer_gru.py:146-152)")
        ch = [int(c) for c in num_ch_dec]
        for s in range(4):
            # scale 3 has no upscaled hand-over to concatenate: input 128, hidden 256; below it input = hidden = 2 * num_ch_dec[s]
            dims = {"input_dim": ch[3] if s == 3 else 2 * ch[s], "hidden_dim_1": 2 * ch[s], "height": height >> s, "width": width >> s}
            setattr(self, "cgru_%d" % s, ConvGRUModel_v1(dims, kernel_size, bias, device))
        for s in range(4):
            setattr(self, "fusion_%d" % s, FeatureFusionBlock_v2(2 * ch[s], up=(s != 0), attention=False))

    def cells(self):
        return [getattr(self, "cgru_%d" % s) for s in range(4)]

    def initial_states(self):
        return [cell.h0_layer1 for cell in self.cells()]

    def _scale(self, s, x, input_1, h_prev):
        """One scale of a frame -> (h', disparity, up or None)."""
        if not x.is_cuda:
            raise DepthcoreError("ConvGRUBlocks_v9 runs on depthcore kernels only; there is no CPU path")
        cell, fusion = getattr(self, "cgru_%d" % s).cgru_1, getattr(self, "fusion_%d" % s)
        B = x.shape[0]
        if h_prev.shape[0] == 1 and B > 1:                      # the learned h0 shared over a batch
            h_prev = h_prev.expand((B,) + tuple(h_prev.shape[1:]))
        g, c = cell.conv_gates, cell.conv_can
        gates = _ops.conv3x3_block(x, h_prev, g.weight, g.bias, False, _ops.ACT_SIGMOID, _ops.PAD_ZERO)            # rnn.py:125-130
        rh = _ops.gru_reset_times_state(gates, h_prev)
        cnm = _ops.conv3x3_block(x, rh, c.weight, c.bias, False, _ops.ACT_TANH, _ops.PAD_ZERO)                     # rnn.py:132-134
        h_new, pre, up = _ops.gru_handover(gates, h_prev, cnm, fusion.resConfUnit1(input_1), need_up=fusion.up)     # rnn.py:136, 533, 767-773
        # (unit2's leading ReLU finds pre non-negative already: the value pass of the in-place ReLU that made it so)
        return h_new, fusion.conv3x3(fusion.resConfUnit2(pre), act=_ops.ACT_SIGMOID), up

    def forward(self, dec_outputs, hidden_states):
        """One frame: dec_outputs[("disp", s)] the decoder's pre_disp map of scale s, hidden_states[s] = h.  Returns
        ([h' for s = 0..3], {("disp", s): disparity})."""
        new, disp, up = [None] * 4, {}, None
        for s in (3, 2, 1, 0):
            dec = dec_outputs[("disp", s)]
            x = dec if s == 3 else torch.cat([dec, up], 1)
            new[s], disp[("disp", s)], up = self._scale(s, x, torch.cat([dec, dec], 1) if s == 3 else x, hidden_states[s])
        return new, disp

    def run_sequence(self, dec_outputs):
        """trainer_gru.py:747-763 for batch_size 1: dec_outputs[("disp", s)] (n, C_s, h_s, w_s) holds the decoder maps of the n
        frames of one sequence; the frames are walked in order from the learned h0; returns {("disp", s): (n, 1, h_s, w_s)}."""
        n = dec_outputs[("disp", 0)].shape[0]
        states = self.initial_states()
        outs = {s: [] for s in range(4)}
        for i in range(n):
            states, disp = self({("disp", s): dec_outputs[("disp", s)][i:i + 1] for s in range(4)}, states)
            for s in range(4):
                outs[s].append(disp[("disp", s)])
        return {("disp", s): torch.cat(outs[s], 0) for s in range(4)}
