"""Recurrent front-ends: the ConvGRU gate ops, the frame stacking, the level node of a training sequence, the inference step
of lockstep streams, the ConvLSTM state update and hand-over with their one-launch inference form, and the coarse-to-fine
ConvGRU's one-launch hand-over (the GRU's tail joined with the fusion block's hand-over) with its inference form.

Imports `_lib`, `_autograd`, `convs` (the fused block's activation and padding codes) and `data` (`seq_rows`); `ops`
re-exports every name.
"""
import ctypes

import torch

from . import _lib
from ._autograd import WgradLanes, _bias_grad_dst, _c, _grad_dst, _precision, _slot, _use_precision
from ._lib import DepthcoreError, check, ptr, stream
from .convs import ACT_SIGMOID, ACT_TANH, PAD_ZERO
from .data import seq_rows


def _gate_dims(gates, state, mult, err, rows=True):
    """(B, C, P) of a state (B, C, H, W) whose gates are (B, mult * C, H, W): mult 2 for the GRU's [reset | update], 4 for the
    LSTM's [i | f | o | g].  rows=False leaves the leading dimension alone (inference buffers may hold more rows than a step
    takes).  `err`: the caller's error text, formed only on a mismatch."""
    if (state.dim() != 4 or tuple(gates.shape[1:]) != (mult * state.shape[1],) + tuple(state.shape[2:])
            or (rows and gates.shape[0] != state.shape[0])):
        raise DepthcoreError(err())
    return state.shape[0], state.shape[1], state.shape[2] * state.shape[3]


def _gather_copy(src, dst, n, st):
    """dc_gather_copy of segments (src[i] -> dst[i], n[i] floats; raw addresses) on stream `st`, 96 segments per launch (the
    kernel's argument table)."""
    L = _lib.lib()
    for i in range(0, len(src), 96):
        k = len(src[i:i + 96])
        check(L.dc_gather_copy((ctypes.c_void_p * k)(*src[i:i + 96]), (ctypes.c_void_p * k)(*dst[i:i + 96]),
                               (ctypes.c_size_t * k)(*n[i:i + 96]), k, st), "dc_gather_copy")


# ----------------------------------------------------------------------------------------------
# f2 ConvGRU cell gate arithmetic + sequence residual        (reference networks/rnn.py:101-143, trainer_gru.py:637-639)
# ----------------------------------------------------------------------------------------------
class _GruRH(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gates, h):
        L = _lib.lib()
        gt, hh = _c(gates.detach()), _c(h.detach())
        B, C, P = _gate_dims(gt, hh, 2, lambda: "gates %s do not match state %s" % (tuple(gt.shape), tuple(hh.shape)))
        rh = torch.empty_like(hh)
        check(L.dc_gru_rh_fwd(ptr(gt), ptr(hh), ptr(rh), B, C, P, stream(hh)), "dc_gru_rh_fwd")
        ctx.save_for_backward(gt, hh)
        return rh

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        gt, hh = ctx.saved_tensors
        B, C = hh.shape[0], hh.shape[1]
        P = hh.shape[2] * hh.shape[3]
        g_c = _c(g)
        dg, dh = torch.empty_like(gt), torch.empty_like(hh)
        check(L.dc_gru_rh_bwd(ptr(gt), ptr(hh), ptr(g_c), ptr(dg), ptr(dh), B, C, P, stream(hh)), "dc_gru_rh_bwd")
        return dg, dh


class _GruBlend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gates, h, cnm):
        L = _lib.lib()
        gt, hh, cc = _c(gates.detach()), _c(h.detach()), _c(cnm.detach())
        def err():
            return "gates %s / candidate %s do not match state %s" % (tuple(gt.shape), tuple(cc.shape), tuple(hh.shape))
        B, C, P = _gate_dims(gt, hh, 2, err)
        if cc.shape != hh.shape:
            raise DepthcoreError(err())
        out = torch.empty_like(hh)
        check(L.dc_gru_blend_fwd(ptr(gt), ptr(hh), ptr(cc), ptr(out), B, C, P, stream(hh)), "dc_gru_blend_fwd")
        ctx.save_for_backward(gt, hh, cc)
        return out

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        gt, hh, cc = ctx.saved_tensors
        B, C = hh.shape[0], hh.shape[1]
        P = hh.shape[2] * hh.shape[3]
        g_c = _c(g)
        dg, dh, dc = torch.empty_like(gt), torch.empty_like(hh), torch.empty_like(cc)
        check(L.dc_gru_blend_bwd(ptr(gt), ptr(hh), ptr(cc), ptr(g_c), ptr(dg), ptr(dh), ptr(dc), B, C, P, stream(hh)), "dc_gru_blend_bwd")
        return dg, dh, dc


class _GruResidual(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, H):
        L = _lib.lib()
        ff, HH = _c(f.detach()), _c(H.detach())
        n = ff.shape[0]
        M = ff[0].numel()
        if tuple(HH.shape) != (n + 1,) + tuple(ff.shape[1:]):
            raise _lib.DepthcoreError("hidden states %s must be (n+1, ...) for features %s" % (tuple(HH.shape), tuple(ff.shape)))
        out = torch.empty_like(ff)
        check(L.dc_gru_residual_fwd(ptr(ff), ptr(HH), ptr(out), n, M, stream(ff)), "dc_gru_residual_fwd")
        ctx.dims = (n, M, HH.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        n, M, hshape = ctx.dims
        g_c = _c(g)
        dH = torch.empty(hshape, dtype=torch.float32, device=g.device)
        check(L.dc_gru_residual_bwd(ptr(g_c), ptr(dH), n, M, stream(g_c)), "dc_gru_residual_bwd")
        return g_c, dH


def stack_frames(groups):
    """[[t_0, t_1, ...], ...] -> [torch.cat(group, 0) for group in groups] in ONE launch (dc_gather_copy): the sequence trainer's
    stacking of the frames of a sequence along the batch (trainer_gru.py:819-821, 886-896, 943-944).  float32 device tensors
    without a gradient (inputs of the step); a group's members share their trailing shape."""
    outs, src, dst, n, keep = [], [], [], [], []
    for g in groups:
        ts = [_c(t.detach()) for t in g]
        if any(t.dtype != torch.float32 or not t.is_cuda or t.shape[1:] != ts[0].shape[1:] for t in ts):
            raise _lib.DepthcoreError("stack_frames takes float32 device tensors that agree in their trailing shape")
        out = torch.empty((sum(t.shape[0] for t in ts),) + tuple(ts[0].shape[1:]), dtype=torch.float32, device=ts[0].device)
        off = 0
        for t in ts:
            src.append(t.data_ptr()); dst.append(out.data_ptr() + 4 * off); n.append(t.numel())
            off += t.numel()
        keep.append(ts)
        outs.append(out)
    if src:
        _gather_copy(src, dst, n, stream(outs[0]))
    return outs


def gru_reset_times_state(gates, h):
    """r * h with r = gates[:, :C]."""
    return _GruRH.apply(gates, h)


def gru_blend(gates, h, cnm):
    """(1 - u) * h + u * cnm with u = gates[:, C:]."""
    return _GruBlend.apply(gates, h, cnm)


def gru_sequence_residual(features, hidden_states):
    """features (n,C,H,W) + (H[1:] + H[:-1]) / 2 with H (n+1,C,H,W)."""
    return _GruResidual.apply(features, hidden_states)


class _plan_streams:
    """`with _plan_streams(S)`: the calling thread's Winograd launches plan their reduction as ONE of S stacked streams would
    (dc_set_wino_plan_streams), so that a sequence's results in a lockstep step are those of its single-sequence call.  S == 1
    touches nothing."""

    def __init__(self, streams):
        self.streams, self.before = int(streams), None

    def __enter__(self):
        if self.streams > 1:
            self.before = _lib.lib().dc_set_wino_plan_streams(self.streams)
            if self.before < 1:
                raise _lib.DepthcoreError("dc_set_wino_plan_streams(%d) failed" % self.streams)
        return self

    def __exit__(self, *exc):
        if self.before is not None:
            _lib.lib().dc_set_wino_plan_streams(self.before)
        return False


class _GruLevel(torch.autograd.Function):
    """One feature level of `run_gru_v5` for a sequence of n frames (batch_size 1, trainer_gru.py:607-639) as ONE autograd node:
    the cell runs over the frames from the learned initial state, every tensor of every step lives in one buffer per kind
    (gates / r*h / candidate / the n+1 hidden states -- a step reads and writes its slot by pointer, so there is neither a
    per-frame slice node nor a torch.cat of the trace), and the backward walks the frames in reverse itself: each step's
    gradient of h_i is ACCUMULATED into the slot that already holds the residual's and the later step's share
    (dc_gru_blend_bwd_acc, dc_gru_rh_bwd_acc, the gate convolution's data-gradient store with the slot as its own addend), the
    feature gradient leaves the gate convolution's store with the candidate convolution's and the residual's share added on the
    way, and the shared parameters get their gradients from ONE weight-gradient pass per convolution over the n frames as a
    batch once the walk is done (per-frame passes + a sum over frames otherwise).  Against the per-op
    graph (ConvGRUCell.forward, kept for single calls) that is ~9 elementwise sums, 3 fills / copies and 1.7 concatenations
    fewer per cell step: 137 + 47 + 25 launches of a C4 step.
    S > 1 (beyond the reference): the rows hold S sequences time-major (`seq_rows`: frame j of stream s is row j * S + s), every
    launch of a time step takes the S streams as its batch, the weight-gradient pass takes the n * S rows, and the gradient of
    the initial state the streams share is the sum of their rows (dc_gru_state_bwd).  S == 1 issues exactly the calls above."""

    @staticmethod
    def forward(ctx, feats, h0, wg, bg, wc, bc, S=1):
        L = _lib.lib()
        ff = _c(feats.detach())
        rows, C, H, W = ff.shape
        P = H * W
        S = int(S)
        if S < 1 or rows % S or rows < S:
            raise _lib.DepthcoreError("ConvGRU level: %d rows are not the frames of %d lockstep streams" % (rows, S))
        n = rows // S
        if tuple(h0.shape) != (1, C, H, W) or tuple(wg.shape) != (2 * C, 2 * C, 3, 3) or tuple(wc.shape) != (C, 2 * C, 3, 3):
            raise _lib.DepthcoreError("ConvGRU level: state %s / gate weights %s / candidate weights %s do not match features %s" % (
                tuple(h0.shape), tuple(wg.shape), tuple(wc.shape), tuple(ff.shape)))
        w_g, b_g, w_c, b_c = _c(wg.detach()), _c(bg.detach()), _c(wc.detach()), _c(bc.detach())
        dev = ff.device
        Hs = torch.empty((n + 1) * S, C, H, W, dtype=torch.float32, device=dev)
        if S == 1:
            Hs[0].copy_(h0.detach()[0])
        else:
            gru_infer_init([_c(h0.detach())], [Hs[:S]])                                              # the shared h0, one row per stream
        gates = torch.empty(rows, 2 * C, H, W, dtype=torch.float32, device=dev)
        rh = torch.empty(rows, C, H, W, dtype=torch.float32, device=dev)
        cnm = torch.empty(rows, C, H, W, dtype=torch.float32, device=dev)
        ctx.prec = _use_precision(_precision[0])
        with _plan_streams(S):      # a stream's sums are ordered as in its single-sequence call, whatever S is
            ws = torch.empty(max(L.dc_conv3x3_fwd_workspace(C, C, S, 2 * C, H, W), L.dc_conv3x3_fwd_workspace(C, C, S, C, H, W)),
                             dtype=torch.uint8, device=dev)
            st = stream(ff)
            for i in range(n):
                t = seq_rows(i, S)                                # time step i of the S streams: one contiguous slab
                x, h = ff[t], Hs[t]
                # [reset | update] = sigmoid(conv_gates(cat(x, h)))                                       rnn.py:125-130
                check(L.dc_conv3x3_fwd(ptr(x), C, 0, ptr(h), C, ptr(w_g), ptr(b_g), ptr(gates[t]), ws.data_ptr(), S, 2 * C, H, W,
                                       ACT_SIGMOID, PAD_ZERO, st), "dc_conv3x3_fwd")
                check(L.dc_gru_rh_fwd(ptr(gates[t]), ptr(h), ptr(rh[t]), S, C, P, st), "dc_gru_rh_fwd")
                # cnm = tanh(conv_can(cat(x, reset * h)))                                                   rnn.py:132-134
                check(L.dc_conv3x3_fwd(ptr(x), C, 0, ptr(rh[t]), C, ptr(w_c), ptr(b_c), ptr(cnm[t]), ws.data_ptr(), S, C, H, W,
                                       ACT_TANH, PAD_ZERO, st), "dc_conv3x3_fwd")
                check(L.dc_gru_blend_fwd(ptr(gates[t]), ptr(h), ptr(cnm[t]), ptr(Hs[seq_rows(i + 1, S)]), S, C, P, st),
                      "dc_gru_blend_fwd")                                                                # rnn.py:136
        out = torch.empty_like(ff)
        check(L.dc_gru_residual_fwd(ptr(ff), ptr(Hs), ptr(out), n, S * C * P, st), "dc_gru_residual_fwd")   # trainer_gru.py:637-639
        ctx.save_for_backward(ff, Hs, gates, rh, cnm, w_g, w_c)
        ctx.streams = S
        ctx.slots = tuple(_slot(t) for t in (wg, bg, wc, bc))
        for t, k in ((wg, 2), (wc, 4)):
            if ctx.needs_input_grad[k]:
                WgradLanes.count_use(t)
        return out

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        ff, Hs, gates, rh, cnm, w_g, w_c = ctx.saved_tensors
        rows, C, H, W = ff.shape
        S = ctx.streams
        n = rows // S
        P = H * W
        dev = ff.device
        need = ctx.needs_input_grad
        g_c = _c(g)
        st = stream(ff)
        f32 = dict(dtype=torch.float32, device=dev)
        dHs = torch.empty_like(Hs)
        check(L.dc_gru_residual_bwd(ptr(g_c), ptr(dHs), n, S * C * P, st), "dc_gru_residual_bwd")
        dfe = torch.empty_like(ff)
        dgates, dcn = torch.empty(rows, 2 * C, H, W, **f32), torch.empty(rows, C, H, W, **f32)     # g of the two convolutions' outputs, per frame
        dxc, drh = torch.empty(S, C, H, W, **f32), torch.empty(S, C, H, W, **f32)
        _use_precision(ctx.prec)
        with _plan_streams(S):      # the workspace is sized and the walk's data gradients are planned as one stream's
            ws = torch.empty(max(L.dc_conv3x3_bwd_workspace(C, C, b, co, H, W) for b in (S, rows) for co in (C, 2 * C)),
                             dtype=torch.uint8, device=dev)
            for i in range(n - 1, -1, -1):
                t = seq_rows(i, S)
                x, h, gt, dh = ff[t], Hs[t], gates[t], dHs[t]
                dg, dc = dgates[t], dcn[t]
                # h_{i+1} = (1-u) h_i + u cnm: dHs[i+1] is complete here (residual + step i+1)
                check(L.dc_gru_blend_bwd_acc(ptr(gt), ptr(h), ptr(cnm[t]), ptr(dHs[seq_rows(i + 1, S)]), ptr(dg), ptr(dh), ptr(dc),
                                             S, C, P, st), "dc_gru_blend_bwd_acc")
                # candidate convolution over cat(x, r*h), data gradients only: that of x takes the residual's share (g[i]) along
                check(L.dc_conv3x3_bwd_add(ptr(x), C, 0, ptr(rh[t]), C, ptr(w_c), ptr(cnm[t]), ptr(dc), ptr(dxc), ptr(drh),
                                           ptr(g_c[t]), None, None, None, ws.data_ptr(), S, C, H, W, ACT_TANH, PAD_ZERO, st),
                      "dc_conv3x3_bwd_add")
                check(L.dc_gru_rh_bwd_acc(ptr(gt), ptr(h), ptr(drh), ptr(dg), ptr(dh), S, C, P, st), "dc_gru_rh_bwd_acc")
                # gate convolution over cat(x, h): d x = own + (candidate's + residual's), d h_i = own + what the slot holds
                check(L.dc_conv3x3_bwd_add(ptr(x), C, 0, ptr(h), C, ptr(w_g), ptr(gt), ptr(dg), ptr(dfe[t]), ptr(dh),
                                           ptr(dxc), ptr(dh), None, None, ws.data_ptr(), S, 2 * C, H, W, ACT_SIGMOID, PAD_ZERO, st),
                      "dc_conv3x3_bwd_add")
        # the parameters are shared by the n steps and nothing downstream waits for their gradients: ONE weight-gradient pass
        # per convolution with the n * S frames as its batch (sum over frames and streams = sum over the batch), after the walk.
        # Hs / rh hold the state each frame READ in their first n * S rows (time-major: row j * S + s), as the frames do.
        outs = [None] * 4
        for k, (like, x1, y, gy, co, act) in enumerate(((w_g, Hs, gates, dgates, 2 * C, ACT_SIGMOID), (w_c, rh, cnm, dcn, C, ACT_TANH))):
            if not (need[2 + 2 * k] or need[3 + 2 * k]):
                continue
            dw = _grad_dst(ctx.slots[2 * k], like) if need[2 + 2 * k] else None
            db = _bias_grad_dst(ctx.slots[2 * k + 1], co, dev) if need[3 + 2 * k] else None
            check(L.dc_conv3x3_bwd_add(ptr(ff), C, 0, ptr(x1), C, ptr(like), ptr(y), ptr(gy), None, None, None, None, ptr(dw), ptr(db),
                                       ws.data_ptr(), rows, co, H, W, act, PAD_ZERO, st), "dc_conv3x3_bwd_add")
            outs[2 * k], outs[2 * k + 1] = dw, db
        dh0 = None
        if need[1]:
            if S == 1:
                dh0 = dHs[0:1]
            else:                                             # the streams share h0: its gradient is the sum of their rows
                dh0 = torch.empty(1, C, H, W, **f32)
                check(L.dc_gru_state_bwd(ptr(dHs), ptr(dh0), S, C * P, st), "dc_gru_state_bwd")
        return (dfe if need[0] else None, dh0) + tuple(outs) + (None,)


def gru_level_sequence(features, h0, conv_gates, conv_can, streams=1):
    """features (n,C,H,W) of one sequence, h0 (1,C,H,W) -> features + (H[1:] + H[:-1]) / 2, H the hidden states of the cell
    (conv_gates / conv_can: its two nn.Conv2d) run over the frames in order (trainer_gru.py:607-639 at one level).
    streams = S > 1: features (n * S, C, H, W) hold S sequences time-major (`seq_rows`); they advance in lockstep from the
    shared h0 -- the same four launches per time step with S as their batch -- and the parameters' and h0's gradients are the
    sums over the streams."""
    return _GruLevel.apply(features, h0, conv_gates.weight, conv_gates.bias, conv_can.weight, conv_can.bias, int(streams))


# ---- inference form of the cell step: B independent streams, every level in one launch (dc_gru_infer_*) ---------------------
def _infer_rows(name, B, *groups):
    """The tensors of an inference step, one list per kind and one entry per level: contiguous float32 device tensors whose
    leading dimension holds the streams.  No autograd here: a tensor that requires grad is detached.  -> (lists, B)."""
    nlev = len(groups[0])
    if not 1 <= nlev <= 8 or any(len(g) != nlev for g in groups):
        raise DepthcoreError("%s: 1..8 levels, one tensor per level and kind" % name)
    groups = [[t.detach() for t in g] for g in groups]
    rows = min(t.shape[0] for g in groups for t in g)
    B = rows if B is None else int(B)
    if not 1 <= B <= rows:
        raise DepthcoreError("%s: B = %d streams of buffers that hold %d" % (name, B, rows))
    return groups, B


def _infer_levels(gates, h, cnm=None, f=None, rh=None, out=None):
    """The dc_gru_infer_level array of a step's tensors (shapes checked: gates (S,2C,H,W), the others (S,C,H,W))."""
    lv = (_lib.GruInferLevel * len(h))()
    for k, hh in enumerate(h):
        _, C, P = _gate_dims(gates[k], hh, 2, lambda: "level %d: gates %s do not match state %s" % (
            k, tuple(gates[k].shape), tuple(hh.shape)), rows=False)
        lv[k].gates, lv[k].h, lv[k].C, lv[k].P = ptr(gates[k]), ptr(hh), C, P
        for field, ts in (("cnm", cnm), ("f", f), ("rh", rh), ("out", out)):
            if ts is not None:
                if ts[k].shape[1:] != hh.shape[1:]:
                    raise DepthcoreError("level %d: %s %s does not match state %s" % (k, field, tuple(ts[k].shape), tuple(hh.shape)))
                setattr(lv[k], field, ptr(ts[k]))
    return lv


def gru_infer_rh(gates, h, rh, B=None):
    """rh[k][:B] = gates[k][:B, :C] * h[k][:B] for every level k, one launch (dc_gru_infer_rh).  Lists with one tensor per
    level; B: the streams stepped, a prefix of the buffers' rows (default: all).  Writes into `rh`; no autograd."""
    (gates, h, rh), B = _infer_rows("gru_infer_rh", B, gates, h, rh)
    check(_lib.lib().dc_gru_infer_rh(_infer_levels(gates, h, rh=rh), len(h), B, stream(h[0])), "dc_gru_infer_rh")
    return rh


def gru_infer_tail(gates, cnm, f, h, out, B=None):
    """The rest of a cell step after the candidate convolution, every level in one launch (dc_gru_infer_tail): with
    u = gates[k][:B, C:], h_next = (1 - u) * h + u * cnm, out[k][:B] = f[k] + (h_next + h) / 2, and h[k][:B] IS OVERWRITTEN by
    h_next.  `f[k]` may hold just the B rows; no autograd."""
    (gates, cnm, f, h, out), B = _infer_rows("gru_infer_tail", B, gates, cnm, f, h, out)
    check(_lib.lib().dc_gru_infer_tail(_infer_levels(gates, h, cnm=cnm, f=f, out=out), len(h), B, stream(h[0])), "dc_gru_infer_tail")
    return out


def gru_infer_init(h0, state, B=None):
    """state[k][b] = h0[k][0] for b < B, every level in one launch (dc_gru_infer_init): the learned initial states (1,C,H,W)
    broadcast over the streams of the state buffers (S,C,H,W).  `h0` is only read."""
    (h0, state), _ = _infer_rows("gru_infer_init", 1, h0, state)
    rows = min(s.shape[0] for s in state)
    B = rows if B is None else int(B)
    if not 1 <= B <= rows or any(a.shape[0] != 1 or a.shape[1:] != s.shape[1:] for a, s in zip(h0, state)):
        raise DepthcoreError("gru_infer_init: h0 (1,C,H,W) into B <= S rows of state (S,C,H,W)")
    n = len(state)
    check(_lib.lib().dc_gru_infer_init((ctypes.c_void_p * n)(*[ptr(a) for a in h0]), (ctypes.c_void_p * n)(*[ptr(s) for s in state]),
                                       (ctypes.c_size_t * n)(*[a.numel() for a in h0]), n, B, stream(state[0])), "dc_gru_infer_init")
    return state


def copy_segments(srcs, dsts):
    """dsts[i].copy_(srcs[i]) for contiguous float32 device tensors of pairwise equal size, 96 pairs per launch
    (dc_gather_copy): the rows of a lockstep step go to their scenes' outputs this way."""
    if len(srcs) != len(dsts) or any(s.numel() != d.numel() or s.numel() == 0 for s, d in zip(srcs, dsts)):
        raise DepthcoreError("copy_segments: pairs of tensors of equal, non-zero size")
    if srcs:
        _gather_copy([ptr(t.detach()) for t in srcs], [ptr(t) for t in dsts], [t.numel() for t in srcs], stream(dsts[0]))


# ----------------------------------------------------------------------------------------------
# f3 ConvLSTM v8: state update and coarse-to-fine hand-over   (reference networks/rnn.py:70-79, 767-773, 783-791)
# ----------------------------------------------------------------------------------------------
def _rows(t, B, what):
    """A learned initial state (1, C, H, W) shared by B > 1 items, expanded: its gradient's sum over B is autograd's (a plain,
    ordered torch reduction)."""
    if t.shape[0] == 1 and B > 1:
        return t.expand((B,) + tuple(t.shape[1:]))
    if t.shape[0] != B:
        raise DepthcoreError("%s has %d rows for a batch of %d" % (what, t.shape[0], B))
    return t


class _LstmCell(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cc, c_cur):
        L = _lib.lib()
        g, c = _c(cc.detach()), _c(c_cur.detach())
        B, C, P = _gate_dims(g, c, 4, lambda: "gate pre-activations %s do not match the cell state %s" % (
            tuple(g.shape), tuple(c.shape)))
        h_next, c_next = torch.empty_like(c), torch.empty_like(c)
        check(L.dc_lstm_cell_fwd(ptr(g), ptr(c), ptr(h_next), ptr(c_next), B, C, P, stream(c)), "dc_lstm_cell_fwd")
        ctx.save_for_backward(g, c)
        ctx.set_materialize_grads(False)        # a state nobody reads (the last frame's c) arrives as None -> NULL
        return h_next, c_next

    @staticmethod
    def backward(ctx, g_h, g_c):
        if g_h is None and g_c is None:
            return None, None
        L = _lib.lib()
        g, c = ctx.saved_tensors
        B, C, P = c.shape[0], c.shape[1], c.shape[2] * c.shape[3]
        gh = _c(g_h) if g_h is not None else None
        gc = _c(g_c) if g_c is not None else None
        d_cc, d_c = torch.empty_like(g), torch.empty_like(c)
        check(L.dc_lstm_cell_bwd(ptr(g), ptr(c), ptr(gh), ptr(gc), ptr(d_cc), ptr(d_c), B, C, P, stream(c)), "dc_lstm_cell_bwd")
        return d_cc, d_c


def lstm_cell(cc, c_cur):
    """(h_next, c_next) of a ConvLSTM step from the raw output cc (B, 4C, H, W) = [i | f | o | g] of the cell's convolution and
    the cell state c_cur (B, C, H, W), or (1, C, H, W): a learned initial state shared over the batch."""
    return _LstmCell.apply(cc, _rows(c_cur, cc.shape[0], "c_cur"))


class _LstmHandover(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, h_prev, h_new, need_up):
        L = _lib.lib()
        aa, hp, hn = _c(a.detach()), _c(h_prev.detach()), _c(h_new.detach())
        if aa.dim() != 4 or hp.shape != aa.shape or hn.shape != aa.shape or aa.shape[1] % 4:
            raise DepthcoreError("hand-over takes three (B, C, h, w) tensors with C a multiple of 4, got %s %s %s"
                                 % (tuple(aa.shape), tuple(hp.shape), tuple(hn.shape)))
        B, C, h, w = aa.shape
        pre = torch.empty_like(aa)
        up = torch.empty(B, C // 4, 2 * h, 2 * w, dtype=torch.float32, device=aa.device) if need_up else None
        check(L.dc_lstm_handover_fwd(ptr(aa), ptr(hp), ptr(hn), ptr(pre), ptr(up), B, C, h, w, stream(aa)), "dc_lstm_handover_fwd")
        ctx.save_for_backward(pre)
        ctx.set_materialize_grads(False)
        return pre, up

    @staticmethod
    def backward(ctx, g_pre, g_up):
        need = ctx.needs_input_grad
        if (g_pre is None and g_up is None) or not any(need[:3]):
            return None, None, None, None
        L = _lib.lib()
        pre, = ctx.saved_tensors
        B, C, h, w = pre.shape
        gp = _c(g_pre) if g_pre is not None else None
        gu = _c(g_up) if g_up is not None else None
        d = [torch.empty_like(pre) if need[k] else None for k in range(3)]
        check(L.dc_lstm_handover_bwd(ptr(pre), ptr(gp), ptr(gu), ptr(d[0]), ptr(d[1]), ptr(d[2]), B, C, h, w, stream(pre)),
              "dc_lstm_handover_bwd")
        return d[0], d[1], d[2], None


def lstm_handover(a, h_prev, h_new, need_up=True):
    """pre = relu(a + (h_prev + h_new) / 2) and up = pixel_shuffle(tanh(pre), 2) (None without need_up) in one launch:
    FeatureFusionBlock_v2's join of the residual unit's output with the mean hidden state, and its UpscalePS.  h_prev may be
    (1, C, h, w): the learned initial hidden state shared over the batch."""
    return _LstmHandover.apply(a, _rows(h_prev, a.shape[0], "h_prev"), h_new, bool(need_up))


def _step_outputs(name, h_, B, ts):
    """The hand-over tensors of an inference step (ts: y, r, pre, up, each a tensor or None) against B rows of the state h_
    (S >= B, C, hh, w) -> (address of up or None, its row stride).  up holds (C/4, 2hh, 2w) per row and may be a channel slice
    of a wider contiguous buffer, whose row stride is passed down."""
    C, hh, w = h_.shape[1:]
    P = hh * w
    for k in ("y", "r", "pre"):
        if ts[k] is not None and (ts[k].dim() != 4 or ts[k].shape[0] < B or ts[k].shape[1:] != h_.shape[1:]):
            raise DepthcoreError("%s: %s %s does not match %d rows of the state %s" % (name, k, tuple(ts[k].shape), B, tuple(h_.shape)))
    up_, stride = ts["up"], 0
    if up_ is not None:
        if C % 4 or up_.dim() != 4 or up_.shape[0] < B or tuple(up_.shape[1:]) != (C // 4, 2 * hh, 2 * w) or \
                up_.stride()[1:] != (4 * P, 2 * w, 1) or (up_.shape[0] > 1 and up_.stride(0) < C * P):
            raise DepthcoreError("%s: up %s (strides %s) is not (>= %d, %d, %d, %d) with contiguous rows" % (
                name, tuple(up_.shape), up_.stride(), B, C // 4, 2 * hh, 2 * w))
        if up_.dtype != torch.float32 or not up_.is_cuda:
            raise DepthcoreError("%s: up must be a float32 device tensor" % name)
        stride = up_.stride(0) if up_.shape[0] > 1 else C * P
    return (None if up_ is None else up_.data_ptr()), stride


def _infer_step(name, inputs, mult, gate_err, states, y, r, pre, up, B):
    """The body of lstm_infer_step and gru_c2f_infer_step: nothing reaches autograd, the shapes and rows are checked, and the entry
    dc_<name>(*inputs, y, r, *states, pre, up, up's row stride, B, C, hh, w, stream) is called once.  inputs {label: tensor}: first
    the gates (>= B, mult * C, hh, w) -- gate_err is their mismatch text -- then operands of >= B rows of the state's shape;
    states {label: tensor}: h first, all (S >= B, C, hh, w), rewritten in place in their first B rows."""
    inputs = {k: t.detach() for k, t in inputs.items()}
    states = {k: t.detach() for k, t in states.items()}
    ts = {k: (None if t is None else t.detach()) for k, t in dict(y=y, r=r, pre=pre, up=up).items()}
    (gt, *rest), h_ = inputs.values(), next(iter(states.values()))
    B = gt.shape[0] if B is None else int(B)
    _, C, _ = _gate_dims(gt, h_, mult, lambda: gate_err % (tuple(gt.shape), tuple(h_.shape)), rows=False)
    hh, w = h_.shape[2], h_.shape[3]
    if any(t.shape != h_.shape for t in states.values()) or any(t.dim() != 4 or t.shape[1:] != h_.shape[1:] for t in rest) \
            or not 1 <= B <= min(t.shape[0] for t in (gt, *rest, h_)):
        raise DepthcoreError("%s: B = %d streams of %s" % (name, B, ", ".join(
            "%s %s" % (k, tuple(t.shape)) for k, t in list(inputs.items()) + list(states.items()))))
    up_ptr, stride = _step_outputs(name, h_, B, ts)
    check(getattr(_lib.lib(), "dc_" + name)(*[ptr(t) for t in inputs.values()], ptr(ts["y"]), ptr(ts["r"]), *[ptr(t) for t in states.values()],
                                            ptr(ts["pre"]), up_ptr, stride, B, C, hh, w, stream(h_)), "dc_" + name)


def lstm_infer_step(cc, h, c, y=None, r=None, pre=None, up=None, B=None):
    """A v8 frame at one scale for B lockstep streams in ONE launch (dc_lstm_infer_step), no autograd:
        c' = sigmoid(f) * c + sigmoid(i) * tanh(g),  h' = sigmoid(o) * tanh(c'),  pre = relu((y + r) + (h + h') / 2),
        up = pixel_shuffle(tanh(pre), 2),  h[:B] <- h',  c[:B] <- c'.
    cc (B, 4C, hh, w) = [i | f | o | g]; h, c (S >= B, C, hh, w) state buffers REWRITTEN IN PLACE in their first B rows; y, r
    (resConfUnit1.conv2's output, the unit's ReLU-ed input) both or neither -- neither is the state update alone; pre
    (>= B, C, hh, w) and up are written where given.  up holds (C/4, 2hh, 2w) per row and may be a channel slice of a wider
    contiguous buffer (the upper half of the next scale's cat(dec, up)): its row stride is passed down.  B: default cc's rows."""
    _infer_step("lstm_infer_step", dict(cc=cc), 4, "gate pre-activations %s do not match the state %s", dict(h=h, c=c), y, r, pre, up, B)


# ----------------------------------------------------------------------------------------------
# f3 coarse-to-fine ConvGRU v10: the GRU's tail and the hand-over in one launch   (reference networks/rnn.py:136, 533, 767-791)
# ----------------------------------------------------------------------------------------------
class _GruHandover(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gates, h_prev, cnm, a, need_up):
        L = _lib.lib()
        gt, hp, cn, aa = _c(gates.detach()), _c(h_prev.detach()), _c(cnm.detach()), _c(a.detach())
        def err():
            return "gates %s / candidate %s / unit output %s do not match the state %s" % (
                tuple(gt.shape), tuple(cn.shape), tuple(aa.shape), tuple(hp.shape))
        B, C, _ = _gate_dims(gt, hp, 2, err)
        if cn.shape != hp.shape or aa.shape != hp.shape or (need_up and C % 4):
            raise DepthcoreError(err() + (" (the shuffle needs C % 4 == 0)" if need_up and C % 4 else ""))
        h, w = hp.shape[2:]
        h_new, pre = torch.empty_like(hp), torch.empty_like(hp)
        up = torch.empty(B, C // 4, 2 * h, 2 * w, dtype=torch.float32, device=hp.device) if need_up else None
        check(L.dc_gru_handover_fwd(ptr(gt), ptr(hp), ptr(cn), ptr(aa), ptr(h_new), ptr(pre), ptr(up), B, C, h, w, stream(hp)),
              "dc_gru_handover_fwd")
        ctx.save_for_backward(gt, hp, cn, pre)                 # all the backward reads
        ctx.set_materialize_grads(False)                       # an output nobody reads (the last frame's state) arrives as None -> NULL
        return h_new, pre, up

    @staticmethod
    def backward(ctx, g_h, g_pre, g_up):
        if (g_h is None and g_pre is None and g_up is None) or not any(ctx.needs_input_grad[:4]):
            return None, None, None, None, None
        L = _lib.lib()
        gt, hp, cn, pre = ctx.saved_tensors
        B, C, h, w = hp.shape
        gh, gp, gu = [None if g is None else _c(g) for g in (g_h, g_pre, g_up)]
        d_gates, d_h, d_cnm, d_a = torch.empty_like(gt), torch.empty_like(hp), torch.empty_like(cn), torch.empty_like(pre)
        check(L.dc_gru_handover_bwd(ptr(gt), ptr(hp), ptr(cn), ptr(pre), ptr(gh), ptr(gp), ptr(gu), ptr(d_gates), ptr(d_h), ptr(d_cnm),
                                    ptr(d_a), B, C, h, w, stream(hp)), "dc_gru_handover_bwd")
        return d_gates, d_h, d_cnm, d_a, None


def gru_handover(gates, h_prev, cnm, a, need_up=True):
    """(h_new, pre, up) of a v10 frame at one scale in one launch (dc_gru_handover_fwd): with u = gates[:, C:],
    h_new = (1 - u) * h_prev + u * cnm, pre = relu(a + (h_prev + h_new) / 2), up = pixel_shuffle(tanh(pre), 2) (None without
    need_up).  gates (B, 2C, h, w) = [reset | update] after the sigmoid, cnm the candidate, a resConfUnit1's output.  h_prev may
    be (1, C, h, w): the learned initial state shared over the batch."""
    return _GruHandover.apply(gates, _rows(h_prev, a.shape[0], "h_prev"), cnm, a, bool(need_up))


def gru_c2f_infer_step(gates, cnm, h, y=None, r=None, pre=None, up=None, B=None):
    """A v10 frame at one scale for B lockstep streams in ONE launch (dc_gru_c2f_infer_step), no autograd: with u = gates[:, C:],
        h' = (1 - u) * h + u * cnm,  pre = relu((y + r) + (h + h') / 2),  up = pixel_shuffle(tanh(pre), 2),  h[:B] <- h'.
    gates (B, 2C, hh, w), cnm (>= B, C, hh, w); h (S >= B, C, hh, w) the state buffer, REWRITTEN IN PLACE in its first B rows;
    y, r, pre, up as lstm_infer_step's.  B: default gates' rows."""
    _infer_step("gru_c2f_infer_step", dict(gates=gates, cnm=cnm), 2, "gates %s do not match the state %s", dict(h=h), y, r, pre, up, B)
