"""ConvLSTM recurrent front-end, `gru_version = v8` (reference networks/rnn.py:32-97 `ConvLSTMCell_v1` / `ConvLSTMModel_v1`,
:371-469 `ConvGRUBlocks_v8`, :739-779 `FeatureFusionBlock_v2`, :783-791 `UpscalePS`; caller trainer_gru.py:402-460
`run_gru_v8`) with the reference's constructors and state_dict layout: `cgru_{0..3}.clstm_1.conv.{weight,bias}`,
`cgru_{k}.h0_layer1`, `cgru_{k}.c0_layer1`, `fusion_{0..3}.resConfUnit{1,2}.conv{1,2}.{weight,bias}`,
`fusion_{k}.conv3x3.conv.{weight,bias}`.

v8 sits BEHIND the depth decoder (run with pre_disp=True: its 16/32/64/128-channel maps instead of disparities) and works
coarse to fine.  Per frame and scale s = 3, 2, 1, 0:
    x_s            = dec_3                      (s = 3)        cat(dec_s, up_{s+1})      (s < 3)
    (h', c')       = LSTM_s(x_s, (h, c))                       one fused conv block over (x_s, h) + dc_lstm_cell
    input_1        = cat(dec_3, dec_3)          (s = 3)        x_s                       (s < 3)
    pre_s, up_s    = hand-over(unit1(input_1), h, h')          dc_lstm_handover: relu(a + (h + h') / 2), pixel_shuffle(tanh(pre), 2)
    disp_s         = sigmoid(conv3x3(reflect_pad(unit2(pre_s))))
The ReLU inside the hand-over is the reference's: `resConfUnit2(pre_output)` applies its in-place nn.ReLU to `pre_output`
before `self.upscale(pre_output)` reads it, so the tensor that is shuffled is tanh(relu(...)).
Every 3x3 convolution is a fused conv block (depthcore.ops.conv3x3_block); the frames are chained by plain autograd."""
import torch
import torch.nn as nn

from depthcore import ops as _ops
from depthcore._lib import DepthcoreError
from layers import Conv3x3
from .fusion import ResidualConvUnit


class ConvLSTMCell_v1(nn.Module):
    """networks/rnn.py:32-79."""

    def __init__(self, input_dim, hidden_dim, kernel_size, bias):
        super().__init__()
        if tuple(kernel_size) != (3, 3) or not bias:
            raise NotImplementedError("ConvLSTMCell_v1 kernels cover kernel_size (3, 3) with bias (trainer_gru.py:141-144)")
        self.input_dim, self.hidden_dim = input_dim, hidden_dim
        self.kernel_size = kernel_size
        self.padding = kernel_size[0] // 2, kernel_size[1] // 2
        self.bias = bias
        self.conv = nn.Conv2d(input_dim + hidden_dim, 4 * hidden_dim, kernel_size, padding=self.padding, bias=bias)

    def forward(self, input_tensor, cur_state):
        if not input_tensor.is_cuda:
            raise DepthcoreError("ConvLSTMCell_v1 runs on depthcore kernels only; there is no CPU path")
        h_cur, c_cur = cur_state
        B = input_tensor.shape[0]
        if h_cur.shape[0] == 1 and B > 1:                       # the learned h0 shared over a batch (trainer_gru.py:420-429)
            h_cur = h_cur.expand((B,) + tuple(h_cur.shape[1:]))
        # [i | f | o | g] = conv(cat(x, h)): the concatenation is index arithmetic in the block's staging      rnn.py:67-70
        cc = _ops.conv3x3_block(input_tensor, h_cur, self.conv.weight, self.conv.bias, False, _ops.ACT_NONE, _ops.PAD_ZERO)
        return _ops.lstm_cell(cc, c_cur)                        # rnn.py:71-79


class ConvLSTMModel_v1(nn.Module):
    """networks/rnn.py:82-97: one cell + its learned initial states `h0_layer1`, `c0_layer1` (1, hidden, H, W), zeros at init."""

    def __init__(self, dim_dict, kernel_size, bias, device):
        super().__init__()
        self.clstm_1 = ConvLSTMCell_v1(dim_dict["input_dim"], dim_dict["hidden_dim_1"], kernel_size, bias)
        self.h0_layer1, self.c0_layer1 = self.init_hidden(dim_dict["hidden_dim_1"], dim_dict["height"], dim_dict["width"], device)
        self.height, self.width, self.hidden_dim = dim_dict["height"], dim_dict["width"], dim_dict["hidden_dim_1"]

    def init_hidden(self, hidden_dim, height, width, device):
        return (nn.Parameter(torch.zeros(1, hidden_dim, height, width, device=device), requires_grad=True),
                nn.Parameter(torch.zeros(1, hidden_dim, height, width, device=device), requires_grad=True))

    def forward(self, x, hidden_state_1):
        return self.clstm_1(x, hidden_state_1)


class FeatureFusionBlock_v2(nn.Module):
    """networks/rnn.py:739-779 with ResidualConvUnits (attention=False, as trainer_gru.py:141-144 builds v8):
        unit(u, t) = u.conv2(relu(u.conv1(relu(t)))) + relu(t)
        pre        = relu(unit(resConfUnit1, input_1) + input_2)
        output     = sigmoid(conv3x3(reflect_pad(unit(resConfUnit2, pre))))
        output_up  = pixel_shuffle(tanh(pre), 2)
    `forward(input_1, input_2)` is the reference's; `fuse(input_1, h_prev, h_new)` is the same block with
    input_2 = (h_prev + h_new) / 2 formed inside the hand-over launch (what ConvGRUBlocks_v8 calls)."""

    def __init__(self, features, up=True, attention=True):
        super().__init__()
        if attention:
            raise NotImplementedError("FeatureFusionBlock_v2 with ResidualAttentionUnits: the trainer builds v8 with attention=False")
        self.up = up
        self.resConfUnit1 = ResidualConvUnit(features)
        self.resConfUnit2 = ResidualConvUnit(features)
        self.conv3x3 = Conv3x3(features, 1)
        self.sigmoid = nn.Sigmoid()

    def fuse(self, input_1, h_prev, h_new):
        pre, output_up = _ops.lstm_handover(self.resConfUnit1(input_1), h_prev, h_new, need_up=self.up)
        # (unit2's leading ReLU finds pre non-negative already: the value pass of the in-place ReLU that made it so)
        output = self.conv3x3(self.resConfUnit2(pre), act=_ops.ACT_SIGMOID)
        return (output, output_up) if self.up else output

    def forward(self, input_1, input_2):
        return self.fuse(input_1, input_2, input_2)             # (x + x) / 2 is x bit for bit; its two half gradients sum to d


class CoarseToFineBlocks(nn.Module):
    """The arrangement that ConvGRUBlocks_v8 (rnn.py:371-469) and ConvGRUBlocks_v9 (:472-569, networks/convgru_c2f.py) share:
    per scale a recurrent model `cgru_{s}` with its learned initial state(s) and a FeatureFusionBlock_v2 `fusion_{s}`, walked
    coarse to fine with the pixel-shuffled hand-over of a scale concatenated to the decoder map of the next finer one.  A
    subclass names its cell model and gives
        initial_states()                  -> [state of scale s for s = 0..3]
        _scale(s, x, input_1, state)      -> (new state, disparity, up or None)      one scale of a frame
    The reference hard-codes the 192 x 640 map sizes and the decoder's channel counts; `height` / `width` / `num_ch_dec`
    reproduce those numbers by default and let other input sizes be built, as ConvGRUBlocks_v5 does."""

    def __init__(self, cell_model, refusal, kernel_size, bias, device, attention, height, width, num_ch_dec):
        """cell_model(dims, kernel_size, bias, device): a scale's recurrent model; refusal: the text for attention=True."""
        super().__init__()
        if attention:
            raise NotImplementedError(refusal)
        ch = [int(c) for c in num_ch_dec]
        for s in range(4):
            # scale 3 has no upscaled hand-over to concatenate: input 128, hidden 256; below it input = hidden = 2 * num_ch_dec[s]
            dims = {"input_dim": ch[3] if s == 3 else 2 * ch[s], "hidden_dim_1": 2 * ch[s], "height": height >> s, "width": width >> s}
            setattr(self, "cgru_%d" % s, cell_model(dims, kernel_size, bias, device))
        for s in range(4):
            setattr(self, "fusion_%d" % s, FeatureFusionBlock_v2(2 * ch[s], up=(s != 0), attention=False))

    def cells(self):
        return [getattr(self, "cgru_%d" % s) for s in range(4)]

    def forward(self, dec_outputs, hidden_states):
        """One frame: dec_outputs[("disp", s)] the decoder's pre_disp map of scale s, hidden_states[s] the state of scale s as
        initial_states() gives it.  Returns ([new state for s = 0..3], {("disp", s): disparity})."""
        new, disp, up = [None] * 4, {}, None
        for s in (3, 2, 1, 0):
            dec = dec_outputs[("disp", s)]
            x = dec if s == 3 else torch.cat([dec, up], 1)
            new[s], disp[("disp", s)], up = self._scale(s, x, torch.cat([dec, dec], 1) if s == 3 else x, hidden_states[s])
        return new, disp

    def run_sequence(self, dec_outputs):
        """trainer_gru.py:437-460 / :747-763 for batch_size 1: dec_outputs[("disp", s)] (n, C_s, h_s, w_s) holds the decoder maps
        of the n frames of one sequence; the frames are walked in order from the learned initial states; returns
        {("disp", s): (n, 1, h_s, w_s)}."""
        n = dec_outputs[("disp", 0)].shape[0]
        states = self.initial_states()
        outs = {s: [] for s in range(4)}
        for i in range(n):
            states, disp = self({("disp", s): dec_outputs[("disp", s)][i:i + 1] for s in range(4)}, states)
            for s in range(4):
                outs[s].append(disp[("disp", s)])
        return {("disp", s): torch.cat(outs[s], 0) for s in range(4)}


class ConvGRUBlocks_v8(CoarseToFineBlocks):
    """networks/rnn.py:371-469: ConvLSTM cells, a scale's state is (h, c)."""

    def __init__(self, kernel_size, bias, device, attention=False, height=192, width=640, num_ch_dec=(16, 32, 64, 128)):
        super().__init__(ConvLSTMModel_v1, "ConvGRUBlocks_v8(attention=True): the attention variant is not built "
                         "(trainer_gru.py:141-144 passes attention=False)", kernel_size, bias, device, attention, height, width, num_ch_dec)

    def initial_states(self):
        return [(cell.h0_layer1, cell.c0_layer1) for cell in self.cells()]

    def _scale(self, s, x, input_1, state):
        new = getattr(self, "cgru_%d" % s)(x, state)
        out = getattr(self, "fusion_%d" % s).fuse(input_1, state[0], new[0])
        return (new,) + (out if s else (out, None))
