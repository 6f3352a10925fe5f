"""The project's own statement of the attention encoder's 7x7 local self-attention (csrc/sasa.hip, ops.local_attention7,
networks/resnet_encoder_attention.py), in plain torch and any dtype, written from the formulas and not from the reference's
text -- a loop over the 49 taps, no unfold, no einsum, no groups:

    q = Wq x, k = Wk x, v = Wv x      (1x1, no bias; taps outside the image carry k = v = 0 and stay in the softmax)
    logit_t[c] = q[c] (k_t[c] + rel_t[c]),   rel_t[c] = rel_h[c, dy] for c < C/2, rel_w[c - C/2, dx] otherwise
    y[c] = sum_t softmax_t(logit)[c] v_t[c],   lse = logsumexp_t(logit)

    attention(q, k, v, rel_h, rel_w) -> (y, lse)           differentiable by autograd
    attention_grads(q, k, v, rel_h, rel_w, y, lse, gy)     the gather-form gradients (dq, dk, dv, drel_h, drel_w) stated directly
    attention_conv(x, st, prefix)                           the layer over a state dict with the reference's key names
    encoder_forward(state, img, num_layers, training, kinks)  the attention encoder: oracle.resnet_ref's blocks and the kinks
                                                              composed with attention_conv
    golden_inputs(case)                                     the seeded inputs of tests/golden/sasa.npz (rebuilt, never stored)

tests/test_sasa_cpu.py pins `attention_conv` and its autograd gradients, and `attention_grads`, to the reference module's fp64
results in tests/golden/sasa.npz.
"""
import zlib

import torch
import torch.nn.functional as F

K, R = 7, 3
PARAM_KEYS = ("rel_h", "rel_w", "key_conv.weight", "query_conv.weight", "value_conv.weight")
# (B, C, H, W, input scale): one pixel; a map smaller than the window; two images with the rel split at an odd C/2; a ragged
# wide map; logit spreads beyond fp32's exp range
GOLDEN_CASES = [(1, 2, 1, 1, 1.0), (1, 4, 2, 3, 1.0), (2, 6, 5, 9, 1.0), (1, 6, 6, 20, 1.0), (1, 4, 8, 8, 3.5)]
WIDE = GOLDEN_CASES[-1]
GROUPS_CASE, GROUPS = GOLDEN_CASES[2], 3          # stored a second time from the reference module built with groups = 3


def case_tag(case):
    return "%dx%dx%dx%d" % tuple(case[:4])


def golden_inputs(case):
    """x, the five parameters (reference shapes) and the output cotangent of a golden case, fp64 masters of fp32 values."""
    B, C, H, W, scale = case
    g = torch.Generator().manual_seed(zlib.crc32(repr(("sasa", tuple(case))).encode()))
    rn = lambda *s: torch.randn(*s, generator=g)
    st = {"rel_h": rn(C // 2, 1, 1, K, 1), "rel_w": rn(C // 2, 1, 1, 1, K)}
    for n in ("key_conv", "query_conv", "value_conv"):
        st[n + ".weight"] = rn(C, C, 1, 1) * (2.0 / C) ** 0.5            # the scale of kaiming_normal_(fan_out, relu)
    x = scale * rn(B, C, H, W)
    gy = rn(B, C, H, W)
    return x.double(), {k: v.double() for k, v in st.items()}, gy.double()


def rel_table(rel_h, rel_w):
    """(C, 7, 7) table of rel_t[c] from rel_h (C/2 * 7 values, indexed by dy) and rel_w (C/2 * 7, indexed by dx)."""
    rh, rw = rel_h.reshape(-1, K), rel_w.reshape(-1, K)
    return torch.cat([rh[:, :, None].expand(-1, K, K), rw[:, None, :].expand(-1, K, K)], 0)


def _shift(t, dy, dx):
    """t at pixel + (dy - 3, dx - 3), zero outside the image."""
    H, W = t.shape[-2:]
    return F.pad(t, (R, R, R, R))[..., dy:dy + H, dx:dx + W]


def logits(q, k, rel_h, rel_w):
    """(49, B, C, H, W)"""
    rel = rel_table(rel_h, rel_w)
    return torch.stack([q * (_shift(k, dy, dx) + rel[:, dy, dx].view(1, -1, 1, 1)) for dy in range(K) for dx in range(K)])


def attention(q, k, v, rel_h, rel_w):
    lg = logits(q, k, rel_h, rel_w)
    lse = torch.logsumexp(lg, 0)
    y = 0
    for t in range(K * K):
        y = y + torch.exp(lg[t] - lse) * _shift(v, t // K, t % K)
    return y, lse


def _unshift(t, dy, dx):
    """The adjoint of _shift: the contribution of tap (dy, dx) of every pixel p, landed on p + (dy - 3, dx - 3)."""
    H, W = t.shape[-2:]
    return F.pad(t, (R, R, R, R))[..., 2 * R - dy:2 * R - dy + H, 2 * R - dx:2 * R - dx + W]


def attention_grads(q, k, v, rel_h, rel_w, y, lse, gy):
    """a_t = exp(logit_t - lse), dl_t = a_t gy (v_t - y);  dq = sum_t dl_t (k_t + rel_t);  dk[p'] = sum_t (dl_t q)[p' - o_t];
    dv[p'] = sum_t (a_t gy)[p' - o_t];  drel_h[c, dy] = sum_{b,p,dx} dl_t q (c < C/2);  drel_w[c, dx] = sum_{b,p,dy} dl_t q."""
    C = q.shape[1]
    rel = rel_table(rel_h, rel_w)
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(q)
    drel = torch.zeros(C, K, K, dtype=q.dtype)
    for dy in range(K):
        for dx in range(K):
            kr = _shift(k, dy, dx) + rel[:, dy, dx].view(1, -1, 1, 1)
            a = torch.exp(q * kr - lse)
            dl = a * gy * (_shift(v, dy, dx) - y)
            dq = dq + dl * kr
            dk = dk + _unshift(dl * q, dy, dx)
            dv = dv + _unshift(a * gy, dy, dx)
            drel[:, dy, dx] = (dl * q).sum((0, 2, 3))
    return dq, dk, dv, drel[:C // 2].sum(2).reshape(rel_h.shape), drel[C // 2:].sum(1).reshape(rel_w.shape)


def attention_conv(x, st, prefix=""):
    q, k, v = (F.conv2d(x, st[prefix + n + "_conv.weight"]) for n in ("query", "key", "value"))
    return attention(q, k, v, st[prefix + "rel_h"], st[prefix + "rel_w"])[0]


def logit_spread(x, st, prefix=""):
    """(largest max_t - min_t of the logits, largest |logit|) of attention_conv on x."""
    q, k = (F.conv2d(x, st[prefix + n + "_conv.weight"]) for n in ("query", "key"))
    lg = logits(q, k, st[prefix + "rel_h"], st[prefix + "rel_w"])
    return float((lg.max(0).values - lg.min(0).values).max()), float(lg.abs().max())


def encoder_forward(state, img, num_layers=18, training=True, kinks=None):
    """The attention encoder's five feature maps: the stem and layer1..4 of oracle.resnet_ref, attention_conv behind every
    stage, its output being the feature map and the next stage's input.  Keys: `encoder.*`, `atten{1..4}.*`."""
    from oracle.kinks import Kinks
    from oracle.resnet_ref import BLOCKS, _basic, _bn
    assert num_layers <= 34
    kn = kinks if kinks is not None else Kinks()
    st = {k[len("encoder."):]: v for k, v in state.items() if k.startswith("encoder.")}
    x = (img - 0.45) / 0.225
    x = kn.relu(_bn(F.conv2d(x, st["conv1.weight"], None, 2, 3), st, "bn1", training))
    feats = [x]
    x = kn.max_pool(x)
    for li, n in enumerate(BLOCKS[num_layers], start=1):
        for j in range(n):
            x = _basic(x, st, "layer%d.%d" % (li, j), 2 if (li > 1 and j == 0) else 1, training, kn)
        x = attention_conv(x, state, "atten%d." % li)
        feats.append(x)
    return feats
