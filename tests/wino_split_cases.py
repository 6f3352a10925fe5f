"""Case tables, seeded input builders, plain-torch statements and the transcribed workspace layout for ONE Winograd launch whose
reduction is SPLIT (csrc/wino.hip: wino_ps_kernel over gridDim.z slabs, wino_ysum_kernel behind it): the plain launches
(dc_wino3x3_fwd / dc_wino3x3_dgrad / dc_wino3x3_dgrad_add), the loader fold (dc_wino3x3_fwd_bn with in_scale / in_shift only) and
the fused 3x3 block (dc_conv3x3_fwd / dc_conv3x3_bwd_add).  Shared by tests/test_wino_split_cases_cpu.py (no GPU: the tables reach
their mechanisms, the transcription agrees with the library's host queries, the cases are well conditioned),
tests/test_wino_split_shapes_gpu.py (the kernels against the statement, slab by slab) and tests/wino_split_forced_child.py (the
splits no shape makes the cost model pick, under DC_WINO_FORCE).  DESIGN.md, "The split reductions at their slab edges", has the
tables with their reasons, the gates and the measured figures.

    Case                     (kind, B, Ci, Co, H, W, groups, addend, force); kind: fwd, dgrad or loader (the forward with the loader
                             fold); force: None or the "mr,nr,ks" of DC_WINO_FORCE
    build(case)              seeded fp32 inputs (the loader's through wino_bn_cases.build: its ReLU margin and planted ties)
    evaluate(case, inp, dt)  the statement in `dt`
    slab_statements(...)     the fp64 statement restricted to each slab's reduction channels
    reference(case)          cached (inputs, fp64 result, fp32 result); nobody may modify what it returns
    launch_mech(...)         what ONE wino_ps_kernel launch reaches, from the transcriptions alone; mech(case) for a table case
    block_mech(case)         the same for the two Winograd launches of a fused-block case (conv_block_cases.Case)

The plan (region, tile variant, split) is wino_bn_cases.ps_plan; what is transcribed here is what a split adds (wino_launch):
    slabs start wino_uhat_bytes(Ci, Co) behind the workspace pointer, slab s holds nout = B M H W floats, and reduces the chunks
    [s cps, min(nchunks, (s + 1) cps)), cps = ceil(nchunks / ksplit), i.e. the channels [8 s cps, min(K, 8 (s + 1) cps));
    a slab whose range is empty is written all the same (zeros); dc_wino3x3_workspace sizes the slabs for the split CAP of the
    larger of the two tensors, not for the split the plan picks."""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

import wino_bn_cases as WC

Case = collections.namedtuple("Case", "kind B Ci Co H W groups addend force")

TENSOR_TOL = WC.TENSOR_TOL
E32_MAX = WC.E32_MAX
PSK = WC.PSK
ceil_div = WC.ceil_div
rel_err = WC.rel_err
SMALL_OUT = 2 << 20           # bytes: outputs up to here may split 4 or 8 ways (wino_ksplit_cap)
LOCKSTEP = 3                  # dc_set_wino_plan_streams(3): the ConvGRU sequence batch as three streams


# ---- the workspace layout, transcribed (csrc/wino.hip, csrc/wino4.hip) ---------------------------------------------------------------
def al256(v):
    return (v + 255) & ~255


def ksplit_cap(nout):
    """wino_ksplit_cap: the largest split of a launch that writes nout floats."""
    return 8 if nout * 4 <= SMALL_OUT else 2


def slab_bytes(nout, streams=1):
    """wino_slab_bytes: the slabs of the largest split nout floats may take (a stream's share of them under plan streams)."""
    return ksplit_cap(nout // streams if streams > 1 else nout) * nout * 4


def uhat_bytes(Ci, Co):
    """wino_uhat_bytes: the transformed weights in front of the slabs."""
    return al256(ceil_div(Ci, 32) * 32 * ceil_div(Co, 32) * 32 * 16 * 4)


def wino4_uhat_bytes(Ci, Co):
    return al256(ceil_div(Ci, 16) * 16 * ceil_div(Co, 16) * 16 * 36 * 4)


def workspace_bytes(B, Ci, Co, H, W, streams=1):
    """dc_wino3x3_workspace: the weights of whichever kernel family the entry may route to, then the slabs of either pass."""
    import conv_block_cases as CC
    head = max(uhat_bytes(Ci, Co), wino4_uhat_bytes(Ci, Co), CC.c3b_weights_bytes(Ci, Co))
    return head + al256(max(slab_bytes(B * Ci * H * W, streams), slab_bytes(B * Co * H * W, streams)))


def slab_offset_floats(Ci, Co, s, nout):
    """Where slab s starts, in floats behind the workspace pointer."""
    return uhat_bytes(Ci, Co) // 4 + s * nout


def parse_force(force):
    """DC_WINO_FORCE as wino_plan reads it: (MT, G, ks) or None where the string is refused."""
    if not force:
        return None
    v = [int(t) for t in force.split(",")]
    mr, nr, fks = v[0], v[1], (v[2] if len(v) > 2 else 0)
    if mr not in (1, 2) or nr not in (2, 4) or (mr == 1 and nr == 4):
        return None
    return 16 * mr, nr // 2, fks


def split_plan(B, K, M, Ho, Wo, force=None, streams=1):
    """wino_plan with what wino_bn_cases.ps_plan leaves out: the plan streams (tile variant and split are those of ONE stream's
    batch, the geometry is the whole batch's) and the forced plan, clamped as wino_plan clamps it."""
    Bp = B // streams if streams > 1 and B % streams == 0 else B
    pick = WC.ps_plan(Bp, K, M, Ho, Wo)
    p = WC.ps_plan(B, K, M, Ho, Wo)._replace(MT=pick.MT, G=pick.G, ksplit=pick.ksplit)
    f = parse_force(force)
    if f:
        cap = ksplit_cap(Bp * M * Ho * Wo) if (Ho * Wo) % 4 == 0 and p.nchunks >= 2 else 1
        p = p._replace(MT=f[0], G=f[1], ksplit=max(1, min(f[2], cap, p.nchunks // 2)) if f[2] > 0 else p.ksplit)
    return p


def launch_mech(B, K, M, H, W, P=1, force=None, streams=1):
    """What one wino_ps_kernel launch over an H x W input reaches (P = 2: the full correlation, output (H + 2) x (W + 2))."""
    Ho, Wo = H + 2 * P - 2, W + 2 * P - 2
    p = split_plan(B, K, M, Ho, Wo, force, streams)
    cps = ceil_div(p.nchunks, p.ksplit)
    begins = [s * cps for s in range(p.ksplit)]
    chunks = [max(0, min(p.nchunks, b + cps) - b) for b in begins]
    return {"plan": p, "ksplit": p.ksplit, "MT": p.MT, "G": p.G, "nchunks": p.nchunks, "cps": cps, "slab_chunks": chunks,
            "ranges": [(min(K, b * PSK), min(K, (b + cps) * PSK)) for b in begins],
            "empty": sum(1 for n in chunks if n == 0), "beyond": sum(1 for b in begins if b > p.nchunks),
            "at_end": sum(1 for b in begins if b == p.nchunks), "ragged_last": 0 < [n for n in chunks if n][-1] < cps,
            "m_fast": B * H * W >= 16 * M, "ragged_M": M % 16 != 0 and M % 32 != 0, "K_mod_8": K % PSK, "K": K, "M": M,
            "nout": B * M * Ho * Wo, "nsub": p.nsub, "odd_H": Ho % 2 == 1}


def conv_dims(c):
    """(K, M) of the case's launch: the data gradient reduces over Co and writes Ci channels."""
    return (c.Co, c.Ci) if c.kind == "dgrad" else (c.Ci, c.Co)


def mech(c, streams=1):
    K, M = conv_dims(c)
    return launch_mech(c.B, K, M, c.H, c.W, force=c.force, streams=streams)


def block_mech(c, force=None):
    """{fwd, dgrad_same, dgrad_full} of a fused-block case: the forward launch, the P = 1 plan wino_dgrad_split_ok asks about, and
    the full-correlation launch the block falls back to when that plan splits."""
    Cin = c.C0 + c.C1
    return {"fwd": launch_mech(c.B, Cin, c.Co, c.H, c.W, force=force), "dgrad_same": launch_mech(c.B, c.Co, Cin, c.H, c.W, force=force),
            "dgrad_full": launch_mech(c.B, c.Co, Cin, c.H, c.W, P=2, force=force)}


# ---- the tables (DESIGN.md lists what each row is there for; tests/test_wino_split_cases_cpu.py asserts it from mech()) ------------
# (B, K, M, H, W): K reduction channels, M output channels.  Every shape runs as a forward (Ci = K, Co = M), as a data gradient
# (Ci = M, Co = K) and as a data gradient with an addend, which the slab sum adds last.
SHAPES = [
    (1, 128, 5, 2, 2),            # 8 slabs of two chunks each on ONE tile; M = 5 below one block
    (1, 129, 5, 2, 2),            # 17 chunks over 8 slabs: 3,3,3,3,3,2 and two EMPTY slabs that begin beyond the last chunk; K % 8 = 1
    (1, 128, 5, 6, 20),           # the same split with blocks ordered x-fast (m_fast) on the 3x10 region
    (1, 129, 5, 6, 20),           # ... with the empty slabs
    (1, 137, 1, 2, 2),            # 18 chunks over 8 slabs: slab 6 begins exactly AT the last chunk's end, slab 7 beyond it; M = 1
    (3, 129, 512, 10, 16),        # 4 slabs, the last one ragged (5,5,5,2); 16-channel tile; three images
    (3, 128, 512, 7, 44),         # 4 slabs on the 32-channel tile; odd H
    (3, 128, 512, 10, 16),        # 8 slabs on the 32-channel tile
    (3, 256, 512, 12, 40),        # 2.9 MB output: the 2-slab cap of outputs over 2 MB; 32 chunks
    WC.SPLIT_REDUCTION,           # (1, 512, 512, 6, 20): the shape the other pins name; 8 slabs of 8 chunks
]
# (B, K, M, H, W, groups): dc_wino3x3_fwd_bn with in_scale / in_shift only (MODE 1); K % 8 == 0
LOADER_SHAPES = [
    (1, 128, 5, 2, 2, 1),         # 8 slabs on one tile
    (2, 136, 5, 2, 2, 2),         # 17 chunks: two empty slabs, whose scale / shift read is clamped; one image per group
    (2, 136, 5, 6, 20, 1),        # the same split, m_fast, the 3x10 region
    (4, 128, 24, 6, 20, 2),       # two images per group; M = 24 ragged
    (3, 128, 512, 10, 16, 1),     # 8 slabs on the 32-channel tile
]
# Splits the cost model picks for no shape (searched up to 4 Mi elements): reached under DC_WINO_FORCE = "mr,nr,ks" in a child process
FORCED_SHAPES = [
    ("fwd", 1, 72, 40, 6, 20, 1, "1,2,4"),        # 9 chunks over 4 slabs (3,3,3,0): the empty slab begins exactly at nchunks
    ("dgrad", 1, 72, 40, 6, 20, 1, "1,2,4"),
    ("fwd", 3, 136, 40, 6, 20, 1, "2,4,4"),       # a split on the 32 x 64 variant (G = 2): 5,5,5,2; odd nsub, M = 40 ragged
    ("dgrad", 3, 136, 40, 6, 20, 1, "2,4,4"),
    ("loader", 2, 136, 40, 6, 20, 2, "2,4,4"),    # ... whose one block holds both BatchNorm groups
    ("fwd", 1, 129, 5, 2, 2, 1, "2,2,8"),         # the empty slabs beyond the end on the 32-channel tile
]


def case_of(kind, B, K, M, H, W, groups=1, addend=0, force=None):
    Ci, Co = (M, K) if kind == "dgrad" else (K, M)
    return Case(kind, B, Ci, Co, H, W, groups, addend, force)


FWD = [case_of("fwd", *s) for s in SHAPES]
DGRAD = [case_of("dgrad", *s, addend=a) for s in SHAPES for a in (0, 1)]
LOADER = [case_of("loader", *s) for s in LOADER_SHAPES]
FORCED = [case_of(k, B, K, M, H, W, g, int(k == "dgrad"), f) for k, B, K, M, H, W, g, f in FORCED_SHAPES]
CASES = FWD + DGRAD + LOADER
DETERMINISM = {"fwd": case_of("fwd", 3, 129, 512, 10, 16), "dgrad": case_of("dgrad", 1, 129, 5, 6, 20, addend=1),
               "loader": case_of("loader", 2, 136, 5, 6, 20, 1)}
# dc_set_wino_plan_streams(3): the batch of three is planned as ONE stream's launch.  On the first shape (the one the issue of
# this pin names) the two plans coincide anyway; on the second the batch of three would take 2 slabs, a single stream 8.
LOCKSTEP_SHAPES = [(3, 512, 512, 6, 20), (3, 512, 512, 12, 40)]


def fused_cases():
    """conv_block_cases.Case rows whose fused Winograd launches split (dsplit = 2: the split store would be taken if the plan let it)."""
    import conv_block_cases as CC
    K, R, Z = CC.K, CC.REFLECT, CC.ZERO
    return [
        # the fused slab sum (bias, activation) behind the forward; the data gradient of these does not split
        K(2, 128, 0, 0, 5, 6, 20, CC.ACT_ELU, R, dsplit=2),                                   # plain source; Co = 5: the bias index wraps at every plane, over two images
        K(2, 128, 1, 0, 24, 4, 8, CC.ACT_SIGMOID, Z, add0=1, dsplit=2),                       # nearest-x2 upsampled source
        K(2, 64, 0, 72, 5, 4, 4, CC.ACT_RELU, R, add0=1, add1="separate", dsplit=2),          # concat, 17 chunks: two empty slabs
        K(1, 128, 1, 8, 8, 4, 4, CC.ACT_TANH, R, bias=0, dsplit=2),                           # upsampled + concat; an activation without a bias
        K(2, 136, 0, 0, 24, 6, 20, CC.ACT_NONE, Z, dsplit=2),                                 # a bias without an activation
        K(2, 136, 0, 0, 24, 6, 20, CC.ACT_NONE, Z, bias=0, dsplit=2),                         # neither: the plain sum in the fused launch
        # the data gradient splits too: wino_dgrad_split_ok refuses, the full correlation (P = 2) runs split, the fold pass follows
        K(2, 128, 0, 0, 128, 4, 4, CC.ACT_ELU, Z, dsplit=2),                                  # 8 slabs either way, no addend
        K(1, 128, 0, 8, 129, 4, 4, CC.ACT_RELU, Z, add0=1, add1="separate", dsplit=2),        # Co = 129: empty slabs in the data gradient; concat, addends
        K(1, 128, 1, 0, 128, 4, 8, CC.ACT_SIGMOID, Z, add0=1, dsplit=2),                      # upsampled source, zero pad, addend
        K(1, 256, 0, 0, 128, 6, 20, CC.ACT_TANH, R, add0=1, dsplit=2),                        # reflection (Co > 64 refuses the ring too); the 3x10 region, an 8 x 22 map
    ]


FUSED_FULL_DGRAD = 4          # how many of fused_cases() (the last ones) split their data gradient as well


def case_id(c):
    tail = {"fwd": "", "dgrad": "-add%d" % c.addend, "loader": "-g%d" % c.groups}[c.kind]
    return "%s-%dx%dto%dx%dx%d%s%s" % (c.kind, c.B, c.Ci, c.Co, c.H, c.W, tail, "-force" + c.force.replace(",", ".") if c.force else "")


def params(cases):
    import pytest
    return [pytest.param(c, id=case_id(c)) for c in cases]


# ---- the builder and the statement ---------------------------------------------------------------------------------------------------
def _bn_case(c):
    return WC.Case("fwd", c.B, c.Ci, c.Co, c.H, c.W, c.groups, 1, 0, 0, 0)


def build(c):
    """fp32 inputs of one case (CPU tensors).  A data gradient always gets an addend; the launch passes it when the case says so."""
    if c.kind == "loader":
        full = WC.build(_bn_case(c), tag="wino_split")
        return {k: full[k] for k in ("x", "w", "s", "t")}
    g = torch.Generator().manual_seed(zlib.crc32(repr(("wino_split", c.kind, c.B, c.Ci, c.Co, c.H, c.W)).encode()))
    rn = lambda *shape: torch.randn(*shape, generator=g)
    inp = {"w": rn(c.Co, c.Ci, 3, 3) * (2.0 / (9 * c.Ci)) ** 0.5}
    if c.kind == "fwd":
        inp["x"] = rn(c.B, c.Ci, c.H, c.W)
    else:
        inp["gy"] = rn(c.B, c.Co, c.H, c.W)
        inp["addend"] = rn(c.B, c.Ci, c.H, c.W)
    return inp


def _operand(c, inp, dt):
    """What the convolution reduces over, in `dt`: x, the loader's relu(s x + t), or gy."""
    if c.kind == "fwd":
        return inp["x"].to(dt)
    if c.kind == "dgrad":
        return inp["gy"].to(dt)
    gi = torch.arange(c.B) // (c.B // c.groups)
    bc = lambda v: v.to(dt)[gi][:, :, None, None]
    return F.relu(bc(inp["s"]) * inp["x"].to(dt) + bc(inp["t"]))


def _conv(c, a, w, lo, hi):
    """The case's convolution over the reduction channels [lo, hi) alone."""
    if c.kind == "dgrad":
        return torch.nn.grad.conv2d_input((c.B, c.Ci, c.H, c.W), w[lo:hi], a[:, lo:hi], padding=1)
    return F.conv2d(a[:, lo:hi], w[:, lo:hi], padding=1)


def evaluate(c, inp, dt):
    """The statement in `dt`, the addend apart: conv2d(x, w), conv2d(relu(s x + t), w) or conv2d_input(gy, w), padding 1."""
    K, _ = conv_dims(c)
    return _conv(c, _operand(c, inp, dt), inp["w"].to(dt), 0, K)


@functools.lru_cache(maxsize=None)
def _reference(base):
    inp = build(base)
    return inp, evaluate(base, inp, torch.float64), evaluate(base, inp, torch.float32)


def reference(c):
    """(inputs, fp64 result, fp32 result) of one case; shared and read-only.  Cases that differ in the addend or the forced plan
    share the convolution."""
    inp, r64, r32 = _reference(c._replace(addend=0, force=None))
    if c.addend:
        return inp, r64 + inp["addend"].double(), r32 + inp["addend"]
    return inp, r64, r32


@functools.lru_cache(maxsize=None)
def _slab_statements(base, ranges):
    inp = _reference(base)[0]
    a, w = _operand(base, inp, torch.float64), inp["w"].double()
    return [None if lo >= hi else _conv(base, a, w, lo, hi) for lo, hi in ranges]


def slab_statements(c, ranges):
    """[fp64 statement over slab s's channels, None for an empty slab]; shared and read-only."""
    return _slab_statements(c._replace(addend=0, force=None), tuple(ranges))


def assert_well_conditioned(c):
    """A condition on the inputs, not on the kernel: finite, torch's fp32 evaluation within E32_MAX of fp64, a result of order one;
    the loader's ReLU decisions no rounding question (wino_bn_cases' margin and planted ties)."""
    inp, r64, r32 = reference(c)
    assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all())
    e32 = rel_err(r32, r64)
    assert e32 < E32_MAX, e32
    assert float(r64.abs().max()) > 0.1
    if c.kind == "loader":
        bc = _bn_case(c)
        pre = WC.preact(bc, inp["x"], inp["s"], inp["t"])
        ties = WC.tie_mask(bc, c.Ci)
        assert bool((pre[ties] == 0).all()) and bool((pre[~ties].abs() >= WC.MARGIN).all())
        assert 0.2 < float((pre > 0).double().mean()) < 0.8
    return e32


host_lib = WC.host_lib


def parts_query(c):
    """dc_wino3x3_stat_parts (forward) / dc_wino3x3_bwd_parts (data gradient) of the case: 0 = the launch has no epilogue."""
    L = host_lib()
    fn = L.dc_wino3x3_bwd_parts if c.kind == "dgrad" else L.dc_wino3x3_stat_parts
    return fn(c.B, c.Ci, c.Co, c.H, c.W, c.groups, None)


# ---- one launch and its gates (GPU; shared by tests/test_wino_split_shapes_gpu.py and tests/wino_split_forced_child.py) ------------
DEV = "cuda:0"


def launch(c, inp, streams=1):
    """One launch of `c` on the fp32 inputs `inp` (under dc_set_wino_plan_streams(streams)).  The output and the WHOLE workspace --
    exactly dc_wino3x3_workspace bytes -- sit between guard bands and start as NaN.  Returns (output, workspace) as CPU tensors;
    asserts the return code, the guards and that the addend came back unchanged."""
    import ctypes
    import conv_block_cases as CC
    from depthcore import _lib
    from depthcore._lib import ptr
    L = _lib.lib()
    B, Ci, Co, H, W = c.B, c.Ci, c.Co, c.H, c.W
    d = {k: v.to(DEV).contiguous() for k, v in inp.items()}
    st = _lib.stream(d["w"])
    prev = L.dc_set_wino_plan_streams(streams)
    try:
        nbytes = L.dc_wino3x3_workspace(B, Ci, Co, H, W)
        assert nbytes == workspace_bytes(B, Ci, Co, H, W, streams) and nbytes % 4 == 0
        ws = CC.Guarded(nbytes // 4)
        _, M = conv_dims(c)
        out = CC.Guarded(B * M * H * W)
        if c.kind == "fwd":
            rc = L.dc_wino3x3_fwd(ptr(d["x"]), ptr(d["w"]), out.ptr(), ws.ptr(), B, Ci, Co, H, W, st)
        elif c.kind == "loader":
            fold = _lib.BnFold()
            fold.groups, fold.in_scale, fold.in_shift = c.groups, ptr(d["s"]), ptr(d["t"])
            rc = L.dc_wino3x3_fwd_bn(ptr(d["x"]), ptr(d["w"]), out.ptr(), ws.ptr(), B, Ci, Co, H, W, ctypes.byref(fold), st)
        elif c.addend:
            add = d["addend"].clone()
            rc = L.dc_wino3x3_dgrad_add(ptr(d["gy"]), ptr(d["w"]), out.ptr(), ptr(add), ws.ptr(), B, Ci, Co, H, W, st)
        else:
            rc = L.dc_wino3x3_dgrad(ptr(d["gy"]), ptr(d["w"]), out.ptr(), ws.ptr(), B, Ci, Co, H, W, st)
    finally:
        L.dc_set_wino_plan_streams(prev)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert out.intact() and ws.intact(), "a write outside the output or the workspace"
    if c.kind == "dgrad" and c.addend:
        assert torch.equal(CC.bits(add), CC.bits(d["addend"])), "the addend was modified"
    return out.body.cpu().view(B, M, H, W), ws.body.cpu()


def gate(c, inp, out, ws, streams=1, tag="wino_split_parity"):
    """The tensor, slab and slab-sum gates of one plain or loader launch.  Prints `<tag> <case> <tensor> e_hip e32 share` for the
    output and for the worst slab before it asserts.  Returns (share of the tensor bound, worst share of a slab's bound)."""
    import conv_block_cases as CC
    m = mech(c, streams)
    _, r64, r32 = reference(c)
    ks, nout = m["ksplit"], m["nout"]
    name = "gx" if c.kind == "dgrad" else "y"
    finite = bool(torch.isfinite(out).all())
    err, e32 = rel_err(out, r64), rel_err(r32, r64)
    print("%s %-40s %-8s %.2e %.1e %5.1f%%   split %d x %s, MT %d G %d" % (tag, case_id(c), name, err, e32, 100 * err / TENSOR_TOL, ks,
                                                                          m["slab_chunks"], m["MT"], m["G"]))
    # the slabs, read back from the workspace
    off = slab_offset_floats(c.Ci, c.Co, 0, nout)
    assert off + ks * nout <= ws.numel()
    slabs = [ws[off + s * nout: off + (s + 1) * nout].view(out.shape) for s in range(ks)]
    refs = slab_statements(c, m["ranges"])
    worst, worst_s, problems = 0.0, -1, []
    for s, (slab, ref) in enumerate(zip(slabs, refs)):
        if ref is None:
            if not bool((CC.bits(slab) == 0).all()):
                problems.append("the empty slab %d is not +0.0 everywhere" % s)
            continue
        if not bool(torch.isfinite(slab).all()):
            problems.append("slab %d has an element that is not finite" % s)
            continue
        e = rel_err(slab, ref)
        if e > worst:
            worst, worst_s = e, s
    print("%s %-40s %-8s %.2e %.1e %5.1f%%   %d empty" % (tag, case_id(c), "slab%d" % worst_s, worst, e32, 100 * worst / TENSOR_TOL, m["empty"]))
    assert finite, "%s has an element that is not finite" % name
    assert err <= TENSOR_TOL, (name, err)
    assert not problems, problems
    assert worst <= TENSOR_TOL, ("slab", worst_s, worst)
    # nothing behind the last slab was touched: the device ran the transcribed number of slabs
    assert bool(torch.isnan(ws[off + ks * nout:]).all()), "the workspace behind slab %d was written" % (ks - 1)
    # the slab sum: fp32 additions in slab order, the addend last -- the host reproduces them exactly
    v = slabs[0].clone()
    for s in range(1, ks):
        v = v + slabs[s]
    if c.kind == "dgrad" and c.addend:
        v = v + inp["addend"]
    assert torch.equal(CC.bits(v), CC.bits(out)), "the output is not the fp32 sum of its slabs in slab order"
    return err / TENSOR_TOL, worst / TENSOR_TOL
