"""Autograd plumbing shared by every binding module: decision observers, the matrix-core precision policy, gradient
destinations, weight-gradient lanes and the gradient joins of tensors with several consumers (GradFork, SkipSum).

The lowest layer above `_lib`: `convnode`, the binding modules behind `ops` (photo, layer_ops, convs, eval_ops, attention,
recurrent) and `bnfold` import it, it imports none of them.  `ops` re-exports every name, so each piece of mutable state
(`_precision`, the observer list, the WgradLanes class attributes) is one object.
"""
import collections
import contextlib
import os
import threading
import weakref

import torch

from . import _lib
from ._lib import check


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# ---- decision observers -------------------------------------------------------------------------------------------------
# Instrumentation hook (no test logic lives here): a callable registered with `add_decision_observer` is told every discrete
# decision the forward takes -- `("relu", y)` with the fused op's output (the decision is y > 0), `("maxpool", code)` with the
# argmax codes -- in call order.  ReLUs that are folded into a convolution's loader never materialise their output: they hand
# over a thunk, which is only evaluated while an observer is registered.  The parity tests build their tape on this
# (tests/kink_tape.py); nothing in the training path registers one.
_decision_observers = []


def add_decision_observer(fn):
    _decision_observers.append(fn)


def remove_decision_observer(fn):
    _decision_observers.remove(fn)


# ---- matrix-core precision of the convolutions (include/depthcore.h: dc_set_matrix_precision) ----------------------------
# "f32": exact fp32 MFMA (the reference's arithmetic, the default).  "bf16": the reduced-precision-networks policy of BASELINE
# configs[4] -- convolution operands rounded to bf16 on their way into LDS, fp32 accumulation, everything else (tensors in HBM,
# master weights, BatchNorm statistics, the photometric loss) fp32.  The C library keeps the setting per calling thread; a
# convolution records the precision of its forward and its backward (run by autograd's thread) uses the same.
PRECISIONS = {"f32": _lib.PREC_F32, "bf16": _lib.PREC_BF16}
_precision = [_lib.PREC_F32]
_tls = threading.local()


class matrix_precision:
    """with ops.matrix_precision("bf16"): ...  -- convolutions issued inside use the bf16 matrix cores."""

    def __init__(self, name):
        if name not in PRECISIONS:
            raise _lib.DepthcoreError("matrix precision must be one of %s, got %r" % (sorted(PRECISIONS), name))
        self.prec = PRECISIONS[name]

    def __enter__(self):
        self.prev, _precision[0] = _precision[0], self.prec
        return self

    def __exit__(self, *exc):
        _precision[0] = self.prev
        return False


def _use_precision(prec):
    """Make `prec` the calling thread's library setting (one C call, only when it changes)."""
    if getattr(_tls, "prec", _lib.PREC_F32) != prec:
        rc = _lib.lib().dc_set_matrix_precision(prec)
        if rc < 0:
            check(rc, "dc_set_matrix_precision")
        _tls.prec = prec
    return prec


def _record_kink(kind, t):
    """`t`: the tensor that carries the decision, or a thunk that forms it (folded ReLUs never materialise theirs)."""
    if _decision_observers:
        t = t() if callable(t) else t
        for fn in _decision_observers:
            fn(kind, t)


def _slot(param):
    """forward(): the parameter's slice of its flat DDP gradient bucket, if depthcore.ddp.GradBuckets gave it one."""
    return getattr(param, "_dc_grad_slot", None)


def _grad_dst(slot, like):
    """backward(): where a parameter gradient is written -- the armed bucket slice (autograd adopts it as `.grad`, so the
    gradient exchange needs no pack copy) or, at world size 1 / on a second use of the parameter, a fresh tensor."""
    if slot is not None and slot.armed:
        return slot.take()
    return torch.empty_like(like) if like is not None else None


def _bias_grad_dst(slot, n, device):
    """backward(): where the gradient of a bias of `n` values is written -- the armed bucket slice, else a fresh (n,) tensor."""
    gb = _grad_dst(slot, None)
    return gb if gb is not None else torch.empty(n, dtype=torch.float32, device=device)


# ---- weight gradients off the backward's critical path ----------------------------------------------------------------------
class WgradLanes:
    """Only the data gradients feed the next backward op; a weight gradient is not read before the optimiser.  While active
    (`with WgradLanes.active(): loss.backward()`), the convolutions launch their weight-gradient kernels on a companion
    HIP stream of the stream their backward runs on ("lane"): the kernels of the data-gradient chain and the weight-gradient
    kernels then share the chip, one side's blocks filling the other's partial rounds and prologues, instead of queueing
    behind each other.  Leaving the context joins every lane into the current stream (before the optimiser / the gradient
    exchange read the gradients).

    A parameter used MORE than once in the graph keeps its weight gradients on the backward's own stream: autograd sums
    the uses' gradients right away, on a stream that knows nothing about the lane.  Uses are counted by the forwards."""
    _on = False
    _lanes = {}          # (device index, raw handle of the backward's stream) -> companion stream
    _uses = {}           # id(parameter) -> forward uses since the last join
    _used = {}           # lane with work enqueued since the last join -> the stream whose backward it accompanies
    _held = collections.deque()     # (event recorded behind a lane's kernels, the tensors they read): kept alive until it completes
    _record_stream = os.environ.get("DC_LANES_RECORD_STREAM", "0") == "1"

    @classmethod
    @contextlib.contextmanager
    def active(cls, on=True):
        prev, cls._on = cls._on, bool(on)
        try:
            yield
        finally:
            cls._on = prev
            cls.join()

    @classmethod
    def join(cls):
        for lane, parent in cls._used.items():
            torch.cuda.current_stream(lane.device).wait_stream(lane)
            # the tensors a lane reads (held below) go back to the pool of the stream that OWNS them -- the backward's stream,
            # e.g. the pose side stream -- so that stream waits for the lane too before its blocks can be handed out again
            parent.wait_stream(lane)
        cls._used = {}
        cls._uses = {}
        cls._held.clear()        # (whatever reuses this memory is enqueued behind the waits above)

    @classmethod
    def count_use(cls, param):
        cls._uses[id(param)] = cls._uses.get(id(param), 0) + 1

    @classmethod
    @contextlib.contextmanager
    def lane(cls, param, *reads):
        """Inside: the current stream is the lane (or unchanged when the lane cannot be used).  `reads`: tensors of the
        backward's stream that the weight-gradient kernel reads."""
        if not (cls._on and param is not None and reads[0].is_cuda and cls._uses.get(id(param), 0) == 1 and param.grad is None):
            yield
            return
        dev = reads[0].device
        cur = torch.cuda.current_stream(dev)
        key = (dev.index, cur.cuda_stream)
        lane = cls._lanes.get(key)
        if lane is None:
            lane = cls._lanes[key] = torch.cuda.Stream(dev)       # (normal priority, below the step stream's: Trainer.on_step_stream)
        lane.wait_stream(cur)
        with torch.cuda.stream(lane):
            yield
        # The tensors the lane reads belong to the backward's stream and autograd frees them as soon as this backward returns.
        # They are kept alive HERE until the lane's kernels have finished (an event behind them, polled on the next calls),
        # so that their memory goes back to the allocator only when it is really free.  (`record_stream` gives the same
        # safety by deferring the REUSE, but the allocator then grows a whole pool of not-yet-reusable blocks: 16 GB reserved
        # for 3.5 GB allocated at C2, 84 GB for 16.6 GB at C3 in tools/soak.py.)
        if cls._record_stream:               # (A/B of the first version: DC_LANES_RECORD_STREAM=1)
            for t in reads:
                t.record_stream(lane)
        else:
            ev = torch.cuda.Event()
            ev.record(lane)
            cls._held.append((ev, reads))
            while cls._held and cls._held[0][0].query():
                cls._held.popleft()
        cls._used[lane] = cur


def _lane_param(ctx, idx, weight):
    """forward(): the parameter whose weight gradient may take a lane (WgradLanes), counted as used once more."""
    if not ctx.needs_input_grad[idx]:
        return None
    WgradLanes.count_use(weight)
    return weight


# ----------------------------------------------------------------------------------------------
# a1 the gradient of a residual block's input: summed inside conv1's data-gradient kernel, not by autograd
# ----------------------------------------------------------------------------------------------
_parked_forks = weakref.WeakSet()     # GradForks holding a parked gradient (assert_no_dangling_sums)


class GradFork:
    """The input x of a residual block without a downsample branch has two consumers: conv1 and the skip connection into the
    last BatchNorm (+ add + ReLU).  Autograd would add their two gradients in a separate elementwise pass (31 such passes per
    C2 step, 42 at C3).  With a GradFork shared by the two ops, the last BatchNorm's backward -- which always runs first:
    conv1's output feeds it -- parks the skip's gradient here and reports NO gradient for its `res` input; conv1's backward
    picks it up and its data-gradient kernel adds it in the store epilogue (dc_wino3x3_dgrad_add / dc_conv1x1_dgrad_add), so
    x receives the complete gradient from conv1 alone.  One backward pass per forward (no double backward / retain_graph
    replays): a fork that is asked twice, or whose parked gradient is never collected, raises -- the latter from
    `assert_no_dangling_sums()` (a pair fork whose second reader never runs its backward, e.g. a ("disp", i > 0) output of
    the depth decoder that is left out of the loss: the parked gradient would be lost silently otherwise)."""
    __slots__ = ("addend", "armed", "pair", "arrived", "__weakref__")

    def __init__(self, pair=False):
        self.addend = None
        self.armed = True
        # pair: x feeds TWO convolutions with the addend epilogue (Bottleneck conv1 and the 1x1 `downsample`): whichever
        # backward runs first parks its data gradient and reports none, the second adds it (no assumption about the order)
        self.pair = pair
        self.arrived = 0

    def arrive(self):
        """pair forks: 0 for the first convolution backward to get here, 1 for the second."""
        if not self.pair or self.arrived >= 2:
            raise _lib.DepthcoreError("GradFork: more backward calls than the two convolutions that share the input")
        self.arrived += 1
        return self.arrived - 1

    def park(self, dres):
        if not self.armed or self.addend is not None:
            raise _lib.DepthcoreError("GradFork: the skip gradient was produced twice (a second backward through the same block?)")
        self.addend = dres
        _parked_forks.add(self)

    def take(self):
        if not self.armed:
            raise _lib.DepthcoreError("GradFork: conv1's backward ran twice for one forward")
        self.armed = False
        a, self.addend = self.addend, None
        _parked_forks.discard(self)
        if self.pair and a is None:
            raise _lib.DepthcoreError("GradFork: the first convolution's data gradient was never parked")
        return a


def _fork_addend(ctx, xx):
    """The skip gradient parked for this convolution's input (GradFork), or None."""
    if ctx.fork is None:
        return None
    add = ctx.fork.take()
    if add is not None and not ctx.needs_input_grad[0]:
        raise _lib.DepthcoreError("GradFork: a skip gradient is waiting but the convolution's input gradient was not requested")
    if add is not None and (add.shape != xx.shape or not add.is_contiguous()):
        raise _lib.DepthcoreError("GradFork: skip gradient %s does not match the block input %s" % (tuple(add.shape), tuple(xx.shape)))
    return add


class SkipSum:
    """A tensor with a PRIMARY consumer whose data-gradient kernel can add another gradient on its way out (the stem output's
    max-pool, a stage's first block) and SECONDARY consumers that run their backward earlier (the depth decoder's skip
    connections, networks/depth_decoder.py:57-59).  The producer tags the tensor (`t._dc_skip = SkipSum()`); the primary
    `arm()`s it in its forward when its backward is certain to run; a secondary `offer()`s its gradient in its backward --
    taken and reported as None while the sum is armed and empty, handed back (autograd then sums as usual) otherwise; the
    primary `take()`s whatever was offered and adds it in its store epilogue.  The elementwise sums autograd would launch
    (16 per C2 step, 41 us for the stem's output alone) become one more read in kernels that write the gradient anyway.
    An offered gradient that nobody took is a lost gradient: `assert_no_dangling_sums()` (Trainer, after every backward)."""
    __slots__ = ("addend", "armed", "__weakref__")
    _pending = weakref.WeakSet()

    def __init__(self):
        self.addend, self.armed = None, False

    def arm(self):
        self.armed = True

    def offer(self, g):
        if g is None or not self.armed or self.addend is not None:
            return g
        self.addend = g
        SkipSum._pending.add(self)
        return None

    def take(self):
        self.armed = False
        a, self.addend = self.addend, None
        SkipSum._pending.discard(self)
        return a


def skip_of(t):
    """The SkipSum a producer attached to tensor `t`, or None."""
    return getattr(t, "_dc_skip", None) if t is not None else None


def assert_no_dangling_sums():
    left = [s for s in SkipSum._pending if s.addend is not None]
    for s in left:
        s.take()
    forks = [f for f in _parked_forks if f.addend is not None]
    for f in forks:
        f.addend, f.armed = None, False
        _parked_forks.discard(f)
    if left:
        raise _lib.DepthcoreError("%d gradient(s) were handed to a SkipSum whose primary consumer never collected them" % len(left))
    if forks:
        raise _lib.DepthcoreError("%d gradient(s) were parked in a GradFork whose other reader never ran its backward (an output "
                                  "of the fused decoder left out of the loss?): the gradient below that point is incomplete"
                                  % len(forks))
