"""Plain-torch restatement of the coarse-to-fine ConvGRU front-end, gru_version v10 (reference networks/rnn.py:101-143,
472-569, 739-791; caller trainer_gru.py:716-764) for the tests: dtype-agnostic (the kernels are judged against it in fp64),
functional over a state dict, no in-place operation.  The fusion block's parts are tests/lstm_ref.py's.

    gru_gates(x, h, st, prefix)              sigmoid(conv_gates(cat(x, h))) = [reset | update]
    gru_candidate(x, h, gates, st, prefix)   tanh(conv_can(cat(x, reset * h)))
    gru_handover(gates, h_prev, cnm, a)      h_new = (1 - u) h_prev + u cnm, then lstm_ref.handover(a, h_prev, h_new)
    v10_forward / v10_sequence               ConvGRUBlocks_v9.forward / run_gru_v9_v10's frame loop
"""
import torch
import torch.nn.functional as F

import lstm_ref as LR

NUM_CH_DEC = LR.NUM_CH_DEC


def gru_gates(x, h, st, prefix):
    return torch.sigmoid(F.conv2d(torch.cat([x, h], 1), st[prefix + "conv_gates.weight"], st[prefix + "conv_gates.bias"], padding=1))


def gru_candidate(x, h, gates, st, prefix):
    reset = gates[:, :h.shape[1]]
    return torch.tanh(F.conv2d(torch.cat([x, reset * h], 1), st[prefix + "conv_can.weight"], st[prefix + "conv_can.bias"], padding=1))


def gru_handover(gates, h_prev, cnm, a, need_up=True):
    """-> (h_new, pre, up): the GRU's tail and FeatureFusionBlock_v2's join with input_2 = (h_prev + h_new) / 2."""
    u = gates[:, h_prev.shape[1]:]
    h_new = (1 - u) * h_prev + u * cnm
    pre, up = LR.handover(a, h_prev, h_new, need_up)
    return h_new, pre, up


def v10_forward(dec, states, st):
    """dec[s]: decoder map of scale s (B, C_s, h_s, w_s); states[s] = h.  -> (new states, [disp_0..disp_3])."""
    new, disp, up = [None] * 4, [None] * 4, None
    for s in (3, 2, 1, 0):
        x = dec[s] if s == 3 else torch.cat([dec[s], up], 1)
        h = states[s].expand(x.shape[0], -1, -1, -1)
        p = "cgru_%d.cgru_1." % s
        gates = gru_gates(x, h, st, p)
        cnm = gru_candidate(x, h, gates, st, p)
        a = LR.res_unit(torch.cat([dec[s], dec[s]], 1) if s == 3 else x, st, "fusion_%d.resConfUnit1." % s)
        new[s], pre, up = gru_handover(gates, h, cnm, a, s != 0)
        disp[s] = LR.fusion_tail(pre, st, "fusion_%d." % s)
    return new, disp


def v10_sequence(dec, st, states=None):
    """dec[s] (n, C_s, h_s, w_s): one sequence; from `states` (default: the learned ones of `st`) -> [disp_s (n, 1, h_s, w_s)]."""
    if states is None:
        states = [st["cgru_%d.h0_layer1" % s] for s in range(4)]
    outs = [[] for _ in range(4)]
    for i in range(dec[0].shape[0]):
        states, disp = v10_forward([d[i:i + 1] for d in dec], states, st)
        for s in range(4):
            outs[s].append(disp[s])
    return [torch.cat(o, 0) for o in outs]


def v10_layout(height=192, width=640, num_ch_dec=NUM_CH_DEC):
    """[(state_dict key, shape)] of ConvGRUBlocks_v9(attention=False) in registration order."""
    lay = []
    for s in range(4):
        hid = 2 * num_ch_dec[s]
        cin = num_ch_dec[3] if s == 3 else 2 * num_ch_dec[s]
        p = "cgru_%d." % s
        lay += [(p + "h0_layer1", (1, hid, height >> s, width >> s)),
                (p + "cgru_1.conv_gates.weight", (2 * hid, cin + hid, 3, 3)), (p + "cgru_1.conv_gates.bias", (2 * hid,)),
                (p + "cgru_1.conv_can.weight", (hid, cin + hid, 3, 3)), (p + "cgru_1.conv_can.bias", (hid,))]
    for s in range(4):
        lay += LR.fusion_layout(2 * num_ch_dec[s], "fusion_%d." % s)
    return lay
