"""Plain-torch restatement of the ConvLSTM v8 front-end (reference networks/rnn.py:32-97, 371-469, 739-791; caller
trainer_gru.py:402-460) for the tests: dtype-agnostic (the kernels are judged against it in fp64), functional over a state
dict, no in-place operation -- the reference's in-place ReLUs are written out as what they compute.

    lstm_cell(cc, c_cur)                     rnn.py:70-79 from the raw convolution output cc = [i | f | o | g]
    handover(a, h_prev, h_new)               pre = relu(a + (h_prev + h_new) / 2), up = pixel_shuffle(tanh(pre), 2)
    fusion_block(in1, in2, st, prefix, up)   FeatureFusionBlock_v2(attention=False)
    v8_forward / v8_sequence                 ConvGRUBlocks_v8.forward / run_gru_v8's frame loop
"""
import torch
import torch.nn.functional as F

NUM_CH_DEC = (16, 32, 64, 128)


def lstm_cell(cc, c_cur):
    i, f, o, g = torch.split(cc, cc.shape[1] // 4, dim=1)
    c_next = torch.sigmoid(f) * c_cur + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c_next), c_next


def handover(a, h_prev, h_new, need_up=True):
    pre = torch.relu(a + (h_prev + h_new) / 2)
    return pre, (F.pixel_shuffle(torch.tanh(pre), 2) if need_up else None)


def conv_lstm_cell(x, state, st, prefix):
    """ConvLSTMCell_v1: st[prefix + "conv.weight" / "conv.bias"]."""
    h, c = state
    B = x.shape[0]
    h = h.expand(B, -1, -1, -1)
    cc = F.conv2d(torch.cat([x, h], 1), st[prefix + "conv.weight"], st[prefix + "conv.bias"], padding=1)
    return lstm_cell(cc, c.expand(B, -1, -1, -1))


def res_unit(t, st, prefix):
    r = torch.relu(t)
    y = F.conv2d(r, st[prefix + "conv1.weight"], st[prefix + "conv1.bias"], padding=1)
    return F.conv2d(torch.relu(y), st[prefix + "conv2.weight"], st[prefix + "conv2.bias"], padding=1) + r


def fusion_tail(pre, st, prefix):
    y = res_unit(pre, st, prefix + "resConfUnit2.")
    return torch.sigmoid(F.conv2d(F.pad(y, (1, 1, 1, 1), mode="reflect"), st[prefix + "conv3x3.conv.weight"], st[prefix + "conv3x3.conv.bias"]))


def fusion_block(input_1, input_2, st, prefix, up=True):
    pre, output_up = handover(res_unit(input_1, st, prefix + "resConfUnit1."), input_2, input_2, up)
    return fusion_tail(pre, st, prefix), output_up


def v8_forward(dec, states, st):
    """dec[s]: decoder map of scale s (B, C_s, h_s, w_s); states[s] = (h, c).  -> (new states, [disp_0..disp_3])."""
    new, disp, up = [None] * 4, [None] * 4, None
    for s in (3, 2, 1, 0):
        x = dec[s] if s == 3 else torch.cat([dec[s], up], 1)
        new[s] = conv_lstm_cell(x, states[s], st, "cgru_%d.clstm_1." % s)
        a = res_unit(torch.cat([dec[s], dec[s]], 1) if s == 3 else x, st, "fusion_%d.resConfUnit1." % s)
        pre, up = handover(a, states[s][0].expand_as(new[s][0]), new[s][0], s != 0)
        disp[s] = fusion_tail(pre, st, "fusion_%d." % s)
    return new, disp


def v8_sequence(dec, st, states=None):
    """dec[s] (n, C_s, h_s, w_s): one sequence; from `states` (default: the learned ones of `st`) -> [disp_s (n, 1, h_s, w_s)]."""
    if states is None:
        states = [(st["cgru_%d.h0_layer1" % s], st["cgru_%d.c0_layer1" % s]) for s in range(4)]
    outs = [[] for _ in range(4)]
    for i in range(dec[0].shape[0]):
        states, disp = v8_forward([d[i:i + 1] for d in dec], states, st)
        for s in range(4):
            outs[s].append(disp[s])
    return [torch.cat(o, 0) for o in outs]


def v8_layout(height=192, width=640, num_ch_dec=NUM_CH_DEC):
    """[(state_dict key, shape)] of ConvGRUBlocks_v8 in registration order."""
    lay = []
    for s in range(4):
        hid = 2 * num_ch_dec[s]
        cin = num_ch_dec[3] if s == 3 else 2 * num_ch_dec[s]
        p = "cgru_%d." % s
        lay += [(p + "h0_layer1", (1, hid, height >> s, width >> s)), (p + "c0_layer1", (1, hid, height >> s, width >> s)),
                (p + "clstm_1.conv.weight", (4 * hid, cin + hid, 3, 3)), (p + "clstm_1.conv.bias", (4 * hid,))]
    for s in range(4):
        lay += fusion_layout(2 * num_ch_dec[s], "fusion_%d." % s)
    return lay


def fusion_layout(f, p=""):
    """[(state_dict key, shape)] of FeatureFusionBlock_v2(f, attention=False)."""
    lay = []
    for u in ("resConfUnit1.", "resConfUnit2."):
        for c in ("conv1.", "conv2."):
            lay += [(p + u + c + "weight", (f, f, 3, 3)), (p + u + c + "bias", (f,))]
    return lay + [(p + "conv3x3.conv.weight", (1, f, 3, 3)), (p + "conv3x3.conv.bias", (1,))]


def seeded(layout, seed, scale, dtype=torch.float32):
    """make_golden.seeded_state's recipe over a layout: scale * randn per tensor, in order, from one seeded generator."""
    g = torch.Generator().manual_seed(seed)
    return {k: (scale * torch.randn(shp, generator=g)).to(dtype) for k, shp in layout}
