"""Coarse-to-fine ConvGRU front-end, `gru_version = v10` (reference networks/rnn.py:472-569 `ConvGRUBlocks_v9` built with
attention=False; :101-158 `ConvGRUCell` / `ConvGRUModel_v1`, :739-779 `FeatureFusionBlock_v2`; caller trainer_gru.py:716-764
`run_gru_v9_v10`) with the reference's constructor and state_dict layout: `cgru_{0..3}.cgru_1.conv_gates.{weight,bias}`,
`cgru_{k}.cgru_1.conv_can.{weight,bias}`, `cgru_{k}.h0_layer1`, `fusion_{0..3}.resConfUnit{1,2}.conv{1,2}.{weight,bias}`,
`fusion_{k}.conv3x3.conv.{weight,bias}`.

It is v8's arrangement (networks/convlstm.py: CoarseToFineBlocks) with the ConvLSTM cells replaced by ConvGRU cells: one
learned initial state per scale and no cell state.  Behind the depth decoder (run with pre_disp=True), per frame and scale s = 3, 2, 1, 0:
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
from depthcore import ops as _ops
from depthcore._lib import DepthcoreError
from .convgru import ConvGRUModel_v1
from .convlstm import CoarseToFineBlocks


class ConvGRUBlocks_v9(CoarseToFineBlocks):
    """networks/rnn.py:472-569: ConvGRU cells, a scale's state is h."""

    def __init__(self, kernel_size, bias, device, attention=True, height=192, width=640, num_ch_dec=(16, 32, 64, 128)):
        super().__init__(ConvGRUModel_v1, "ConvGRUBlocks_v9(attention=True) is gru_version v9, whose fusion blocks hold residual "
                         "attention units: not built; v10 is ConvGRUBlocks_v9(attention=False) (trainer_gru.py:146-152)",
                         kernel_size, bias, device, attention, height, width, num_ch_dec)

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
