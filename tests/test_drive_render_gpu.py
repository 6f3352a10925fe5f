"""One colour range for a whole drive, through the C ABI: dc_disp_range_pooled held bitwise to the numpy statement
tests/drive_ref.py on the device-upsampled maps (ops.upsample_bilinear writes the bilinear_at bits the kernels recompute), and
dc_disp_render_fixed held bytewise to the same statement and to dc_disp_render.  Every output and the workspace sit between
sentinel guard bands that must come back intact; the float outputs start as NaN.  Every figure is printed before it is judged."""
import numpy as np
import pytest
import torch

import drive_ref as DR
import render_ref as R
from test_wino_bn_shapes_gpu import _Guarded

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# (N, h, w, Ho, Wo): one image; a non-integer ratio; the identity; a large ratio; several blocks per image (70 * 300 = 21000
# pixels are 11 tiles of 2048)
SHAPES = [(1, 6, 10, 13, 27), (3, 6, 10, 13, 27), (2, 4, 8, 4, 8), (5, 3, 5, 37, 41), (2, 8, 16, 70, 300)]
QS = (0.0, 50.0, 95.0, 100.0)
KINDS = ("sigmoid", "constant", "pair", "ties")


def _maps(kind, N, h, w, seed=0):
    """(N,1,h,w) fp32 on the device.  pair: one frame constant high, the others constant low, so that the pooled percentile
    falls between two frames (N = 1: the upper rows high, the lower rows low -- there is no second frame)."""
    if kind == "sigmoid":
        d = np.stack([R.low_res_map(h, w, "sigmoid", 200 + seed + i) for i in range(N)])
    elif kind == "ties":
        d = np.stack([R.low_res_map(h, w, "eighths", 300 + seed + i) for i in range(N)])
    elif kind == "constant":
        d = np.full((N, h, w), 0.53414851, np.float32)
    elif kind == "pair":
        d = np.full((N, h, w), 0.125, np.float32)
        if N > 1:
            d[0] = 0.875
        else:
            d[0, :h // 2] = 0.875
    elif kind == "signed":                           # negative values and both zeros
        rng = np.random.RandomState(400 + seed)
        d = rng.randn(N, h, w).astype(np.float32)
        flat = d.reshape(-1)
        flat[::5] = 0.0
        flat[2::5] = -0.0
        assert np.signbit(flat).any() and (flat < 0).any() and (flat > 0).any()
    else:
        raise ValueError(kind)
    return torch.from_numpy(np.ascontiguousarray(d, np.float32)[:, None]).to(DEV)


def _up(d, Ho, Wo):
    from depthcore import ops
    return (d if tuple(d.shape[2:]) == (Ho, Wo) else ops.upsample_bilinear(d, Ho, Wo)).cpu().numpy()


def _pooled(d, Ho, Wo, q):
    """One dc_disp_range_pooled on a workspace of exactly *_ws_bytes -> the two floats (host), guards checked."""
    from depthcore import _lib
    L = _lib.lib()
    N, _, h, w = d.shape
    nws = L.dc_disp_range_pooled_ws_bytes(N, h, w, Ho, Wo)
    assert nws > 0 and nws % 4 == 0
    ws, rng = _Guarded(nws // 4), _Guarded(2)
    rc = L.dc_disp_range_pooled(_lib.ptr(d), rng.body.data_ptr(), N, h, w, Ho, Wo, float(q), ws.body.data_ptr(), nws, _lib.stream(d))
    torch.cuda.synchronize()
    assert rc == 0 and ws.intact() and rng.intact()
    return rng.body.cpu().numpy().copy()


def _fixed(d, Ho, Wo, rng, lut=None):
    """One dc_disp_render_fixed -> (N,Ho,Wo,3) uint8 (host); the bytes behind the image up to the next dword and both guard bands
    must come back untouched."""
    from depthcore import _lib, ops
    L = _lib.lib()
    N, _, h, w = d.shape
    nb = N * Ho * Wo * 3
    out = _Guarded((nb + 3) // 4)
    before = out.body.view(torch.uint8).cpu().numpy().copy()
    lut = ops.magma_lut(DEV) if lut is None else lut
    rng = torch.as_tensor(np.asarray(rng, np.float32)).to(DEV).contiguous()
    rc = L.dc_disp_render_fixed(_lib.ptr(d), _lib.ptr(lut, torch.uint8), _lib.ptr(rng), out.body.data_ptr(), N, h, w, Ho, Wo, _lib.stream(d))
    torch.cuda.synchronize()
    assert rc == 0 and out.intact()
    host = out.body.view(torch.uint8).cpu().numpy()
    assert host[nb:].tobytes() == before[nb:].tobytes()
    return host[:nb].reshape(N, Ho, Wo, 3).copy()


def _same(got, want, zero_sign_free=False):
    """Bitwise; zero_sign_free: a zero may differ in its sign (numpy's sort leaves the order of -0.0 and +0.0 open, the
    kernel's keys put -0.0 first)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if got.tobytes() == want.tobytes():
        return True
    return zero_sign_free and all(g == 0 and w == 0 for g, w in zip(got, want) if g.tobytes() != w.tobytes())


@pytest.mark.parametrize("shape", SHAPES)
def test_pooled_range_bitwise(shape):
    N, h, w, Ho, Wo = shape
    for kind in KINDS:
        d = _maps(kind, N, h, w)
        up = _up(d, Ho, Wo)
        for q in QS:
            got = _pooled(d, Ho, Wo, q)
            want = np.array(DR.pooled_range(up, q), np.float32)
            print("\n%s %-8s q=%5.1f: pooled range %r, statement %r" % (shape, kind, q, got.tolist(), want.tolist()))
            assert _same(got, want), (kind, q)
            assert _same(_pooled(d, Ho, Wo, q), got)                       # two calls: the same bits
            if kind == "constant" and (h, w) == (Ho, Wo):
                assert got[0] == got[1] == np.float32(0.53414851)
        if kind == "pair" and N > 1:                                       # the pooled percentile lies BETWEEN the frames
            share = 100.0 * (N - 1) / N                                    # of the values that are low
            below, above = _pooled(d, Ho, Wo, share - 5.0), _pooled(d, Ho, Wo, min(share + 5.0, 100.0))
            assert abs(below[1] - 0.125) < 1e-6 and abs(above[1] - 0.875) < 1e-6      # (an upsampled constant is constant to an ulp)
            n = N * Ho * Wo                                                # the rank's two neighbours are the last low and the first high value
            q_mid = 100.0 * ((N - 1) * Ho * Wo - 0.5) / (n - 1)
            mid = _pooled(d, Ho, Wo, q_mid)
            assert _same(mid, np.array(DR.pooled_range(up, q_mid), np.float32)) and 0.125 < mid[1] < 0.875, mid


def test_pooled_range_signed_values_and_zeros():
    for shape in ((3, 6, 10, 13, 27), (2, 4, 8, 4, 8)):
        N, h, w, Ho, Wo = shape
        d = _maps("signed", N, h, w)
        up = _up(d, Ho, Wo)
        for q in QS + (37.5,):
            got, want = _pooled(d, Ho, Wo, q), np.array(DR.pooled_range(up, q), np.float32)
            print("\n%s signed q=%5.1f: pooled range %r, statement %r" % (shape, q, got.tolist(), want.tolist()))
            assert _same(got, want, zero_sign_free=True), q
            assert got[0] < 0 and got[0] == up.min()


def test_one_image_is_dc_disp_render_range():
    from depthcore import ops
    for shape in SHAPES:
        N, h, w, Ho, Wo = shape
        for kind in KINDS:
            d = _maps(kind, N, h, w, seed=7)
            for q in QS:
                _, per_image = ops.render_disparity(d, (Ho, Wo), q)
                per_image = per_image.cpu().numpy()
                for i in range(N if N <= 3 else 1):
                    assert _same(_pooled(d[i:i + 1], Ho, Wo, q), per_image[i]), (shape, kind, q, i)


@pytest.mark.parametrize("shape", SHAPES)
def test_render_fixed_bytewise(shape):
    from depthcore import ops
    N, h, w, Ho, Wo = shape
    lut_np = R.magma_lut()
    for kind in KINDS:
        d = _maps(kind, N, h, w, seed=3)
        up = _up(d, Ho, Wo)
        rng = _pooled(d, Ho, Wo, 95.0)
        got = _fixed(d, Ho, Wo, rng)
        want = DR.render_fixed(up, rng[0], rng[1])
        nbad = int((got != want).sum())
        print("\n%s %-8s: range %r, bytes differing %d" % (shape, kind, rng.tolist(), nbad))
        assert got.tobytes() == want.tobytes(), "%d bytes differ" % nbad
        assert _fixed(d, Ho, Wo, rng).tobytes() == got.tobytes()           # two calls: the same bytes
        # the whole chain is the statement's
        assert got.tobytes() == DR.render_drive(up, 95.0)[0].tobytes()
        # a range with vmin == vmax: index 0 everywhere
        assert (_fixed(d, Ho, Wo, [0.5, 0.5]) == lut_np[0]).all()
        # values above vmax take the last colour, values at or below vmin the first
        lo, hi = float(up.min()), float(up.max())
        mid = np.float32(0.5 * (lo + hi))
        if lo < mid < hi:                                                  # (a near-constant map has no fp32 value in between)
            clipped = _fixed(d, Ho, Wo, [lo, mid])
            assert clipped.tobytes() == DR.render_fixed(up, lo, mid).tobytes()
            assert (up[:, 0] > mid).any() and (clipped[up[:, 0] > mid] == lut_np[255]).all()
            assert (clipped[up[:, 0] <= lo] == lut_np[0]).all()
    # fed the range dc_disp_render computed for an image, it is that call's picture
    d = _maps("sigmoid", N, h, w, seed=5)
    rgb, per_image = ops.render_disparity(d, (Ho, Wo), 95.0)
    for i in range(N):
        assert _fixed(d[i:i + 1], Ho, Wo, per_image[i].cpu().numpy())[0].tobytes() == rgb[i].cpu().numpy().tobytes(), i
    # a custom table
    lut = torch.from_numpy(np.random.RandomState(3).randint(0, 256, (256, 3)).astype(np.uint8)).to(DEV)
    rng = _pooled(d, Ho, Wo, 50.0)
    assert _fixed(d, Ho, Wo, rng, lut).tobytes() == DR.render_fixed(_up(d, Ho, Wo), rng[0], rng[1], lut.cpu().numpy()).tobytes()


def test_refusals_write_nothing():
    from depthcore import _lib
    L = _lib.lib()
    d = _maps("sigmoid", 2, 6, 10)
    nws = L.dc_disp_range_pooled_ws_bytes(2, 6, 10, 13, 27)
    ws, rng, rgb = _Guarded(nws // 4), _Guarded(2), _Guarded(2 * 13 * 27 * 3 // 4 + 1)
    lut = torch.zeros(256, 3, dtype=torch.uint8, device=DEV)
    st = _lib.stream(d)
    ok = dict(disp=_lib.ptr(d), rng=rng.body.data_ptr(), N=2, h=6, w=10, Ho=13, Wo=27, q=95.0, ws=ws.body.data_ptr(), nws=nws)

    def pooled(**kw):
        a = dict(ok, **kw)
        return L.dc_disp_range_pooled(a["disp"], a["rng"], a["N"], a["h"], a["w"], a["Ho"], a["Wo"], a["q"], a["ws"], a["nws"], st)

    for kw in (dict(disp=None), dict(rng=None), dict(ws=None), dict(N=0), dict(N=65536), dict(h=0), dict(w=0), dict(Ho=0), dict(Wo=-1),
               dict(q=-1.0), dict(q=100.5), dict(q=float("nan")),
               dict(N=65535, Ho=300, Wo=300)):                               # N Ho Wo >= 2^32: refused before the maps are read
        assert pooled(**kw) == -1, kw
    assert pooled(nws=nws - 1) == -3 and pooled(nws=0) == -3                # a short workspace
    assert L.dc_disp_range_pooled_ws_bytes(65535, 6, 10, 300, 300) == 0
    for kw in (dict(disp=None), dict(lut=None), dict(rng=None), dict(rgb=None), dict(N=0), dict(h=0), dict(Wo=0),
               dict(rgb=rgb.body.data_ptr() + 2)):
        a = dict(dict(disp=_lib.ptr(d), lut=_lib.ptr(lut, torch.uint8), rng=_lib.ptr(d), rgb=rgb.body.data_ptr(), N=2, h=6, w=10, Ho=13,
                      Wo=27), **kw)
        assert L.dc_disp_render_fixed(a["disp"], a["lut"], a["rng"], a["rgb"], a["N"], a["h"], a["w"], a["Ho"], a["Wo"], st) == -1, kw
    torch.cuda.synchronize()
    for g in (ws, rng, rgb):
        assert g.intact() and bool(torch.isnan(g.body).all())               # nothing was written


def test_ops_and_render_drive():
    """The Python layer: ops.disparity_range_pooled / ops.render_disparity_fixed are the ABI's results; evaluate.render_drive
    renders in chunks through its pinned buffer and returns the statement's bytes and pair."""
    from depthcore import evaluate as E
    from depthcore import ops
    from depthcore._lib import DepthcoreError
    d = _maps("sigmoid", 5, 12, 40, seed=9)
    size = (37, 53)
    up = _up(d, *size)
    rng = ops.disparity_range_pooled(d, size)
    assert rng.shape == (2,) and rng.dtype == torch.float32 and rng.is_cuda
    assert _same(rng.cpu().numpy(), _pooled(d, size[0], size[1], 95.0))
    rgb = ops.render_disparity_fixed(d, size, rng)
    assert rgb.shape == (5,) + size + (3,) and rgb.dtype == torch.uint8 and rgb.is_cuda and rgb.is_contiguous()
    want, vmin, vmax = DR.render_drive(up, 95.0)
    assert rgb.cpu().numpy().tobytes() == want.tobytes()
    for chunk in (2, 5, 64):
        images, pair = E.render_drive(d, size, chunk=chunk)
        assert isinstance(images, np.ndarray) and images.dtype == np.uint8 and images.shape == (5,) + size + (3,)
        assert images.tobytes() == want.tobytes() and _same(pair, (vmin, vmax))
    images, pair = E.render_drive(d.cpu().numpy(), size, percentile=50.0, chunk=3)   # host input
    assert images.tobytes() == DR.render_drive(up, 50.0)[0].tobytes()
    # the drive's range is not a frame's: a darker frame stays darker
    dark = d.clone()
    dark[1] *= 0.25
    images, (vmin, vmax) = E.render_drive(dark, size)
    per_frame, ranges = E.render_disparities(dark, size)
    assert ranges[1, 1] < vmax and not (images[1] == R.magma_lut()[255]).all(-1).any()
    assert (per_frame[1] == R.magma_lut()[255]).all(-1).any()
    for bad in (dict(size=(0, 5)), dict(percentile=-1.0), dict(percentile=float("nan"))):
        with pytest.raises(DepthcoreError):
            ops.disparity_range_pooled(d, **dict(dict(size=(8, 8)), **bad))
    with pytest.raises(DepthcoreError):
        ops.disparity_range_pooled(d[:0], (8, 8))
    with pytest.raises(DepthcoreError):
        ops.render_disparity_fixed(d, (8, 8), rng.cpu())
    with pytest.raises(DepthcoreError):
        ops.render_disparity_fixed(d, (8, 8), rng, out=torch.empty(5, dtype=torch.uint8, device=DEV))
