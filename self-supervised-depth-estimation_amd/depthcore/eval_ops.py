"""Evaluation and logging ops (no gradient): depth metrics, pose trajectory error, velodyne depth maps, flip post-processing,
the benchmark's 16-bit depth maps, magma disparity rendering and the training-log panels.

Imports `_lib` and `_autograd` only; `ops` re-exports every name.  The magma table cache `_MAGMA` lives here, once.
"""
import ctypes

import torch

from . import _lib
from ._autograd import _c
from ._lib import DepthcoreError, check, ptr, stream


# ----------------------------------------------------------------------------------------------
# depth metrics of validation  (trainer.py:624-652, evaluate_depth.py:190-235, layers.py:251-269)
# ----------------------------------------------------------------------------------------------
TRAINER_CROP = (153, 371, 44, 1197)      # trainer.py:638 (garg / eigen crop of a 375 x 1242 frame)
_PROTOCOLS = {"trainer": _lib.EVAL_TRAINER, "eigen": _lib.EVAL_EIGEN, "gt_positive": _lib.EVAL_GT_POSITIVE}


def eigen_crop(Hg, Wg):
    """evaluate_depth.py:207-208: the crop rows / columns as numpy computes them (fp64 products, truncated to int32)."""
    import numpy as np
    c = np.array([0.40810811 * Hg, 0.99189189 * Hg, 0.03594771 * Wg, 0.96405229 * Wg]).astype(np.int32)
    return tuple(int(v) for v in c)


def _depth_errors(pred, gt, protocol, crop, median_scaling, scale_factor, image_ids=None):
    """-> (metrics (G, 7), ratios (G,), host copy of [metrics | ratios | status]) after ONE device-to-host copy.
    image_ids: the caller's numbers of the B images, for the error message of an empty mask."""
    if protocol not in _PROTOCOLS:
        raise ValueError("protocol: 'trainer' (trainer.py:624-652), 'eigen' (evaluate_depth.py:190-235) or 'gt_positive' "
                         "(evaluate_depth.py:210-211)")
    L = _lib.lib()
    p, g = _c(pred.detach()), _c(gt.detach())
    if p.dim() != 4 or g.dim() != 4 or p.shape[1] != 1 or g.shape[1] != 1 or p.shape[0] != g.shape[0]:
        raise DepthcoreError("depth_errors: pred (B,1,h,w) and gt (B,1,Hg,Wg), got %s and %s" % (tuple(p.shape), tuple(g.shape)))
    B, _, h, w = p.shape
    Hg, Wg = g.shape[-2:]
    eigen = protocol != "trainer"                  # per-image groups (either mask of evaluate_depth.py)
    if protocol == "gt_positive":
        crop = (0, Hg, 0, Wg)                       # the whole frame (the kernel ignores crop for this protocol)
    elif crop is None:
        crop = eigen_crop(Hg, Wg) if eigen else TRAINER_CROP
    G = B if eigen else 1
    buf = torch.empty(G * 9, dtype=torch.float32, device=p.device)       # metrics | ratios | status (int32)
    d = _lib.DepthEvalDesc()
    d.B, d.h, d.w, d.Hg, d.Wg = B, h, w, Hg, Wg
    d.protocol = _PROTOCOLS[protocol]
    for i in range(4):
        d.crop[i] = int(crop[i])
    d.median_scaling = int(bool(median_scaling))
    d.scale_factor = float(scale_factor)
    d.ratios = buf[G * 7:].data_ptr()
    status = buf[G * 8:].view(torch.int32)
    d.status = ptr(status, torch.int32)
    ws = torch.empty(L.dc_depth_errors_workspace(ctypes.byref(d)), dtype=torch.uint8, device=p.device)
    check(L.dc_depth_errors(ctypes.byref(d), ptr(p), ptr(g), ptr(buf), ws.data_ptr(), stream(p)), "dc_depth_errors")
    host = buf.cpu()
    bad = [i for i, v in enumerate(host[G * 8:].view(torch.int32).tolist()) if v != 0]
    if bad:
        what = ("image %d" % image_ids[bad[0]] if image_ids is not None else "image %d of the batch" % bad[0]) if eigen else "the batch"
        raise DepthcoreError("depth_errors (%s protocol): the mask of %s selects no pixel (%s)" % (protocol, what, _lib._ERR.get(
            host[G * 8:].view(torch.int32)[bad[0]].item(), "status %d")))
    return buf[:G * 7].view(G, 7), buf[G * 7:G * 8], host


def depth_errors(pred, gt, protocol="trainer", crop=None, median_scaling=True, scale_factor=1.0):
    """Depth metrics abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3 of `pred` (B,1,h,w) against `gt` (B,1,Hg,Wg), pred
    bilinearly upsampled to gt's size on the way (dc_depth_errors: one launch chain, medians by radix selection, fp64 sums,
    bitwise reproducible).
      protocol="trainer": Trainer.compute_depth_losses (trainer.py:624-652) -- pred is depth; gt > 0 inside `crop` (default
        rows 153:371, cols 44:1197); torch.median; one ratio for the whole batch.  Returns a (7,) device tensor.
      protocol="eigen": evaluate_depth.py:198-232 -- pred is scaled disparity (depth = 1 / disp * scale_factor);
        1e-3 < gt < 80 inside the fractional Eigen crop; np.median; per image.  Returns ((B, 7), ratios (B,)).
      protocol="gt_positive": as "eigen" but the mask is gt > 0 over the whole frame (`crop` is not used) -- every split
        but "eigen" in evaluate_depth.py:210-211 (eigen_benchmark).  Returns ((B, 7), ratios (B,)).
    median_scaling=False: --disable_median_scaling (ratios are then 1).  A group whose mask selects no pixel raises
    DepthcoreError naming it (this waits for the result: one small device-to-host copy per call)."""
    out, ratios, _ = _depth_errors(pred, gt, protocol, crop, median_scaling, scale_factor)
    if protocol == "trainer":
        return out[0]
    return out, ratios


# ----------------------------------------------------------------------------------------------
# pose evaluation: the trajectory scoring of evaluate_pose.py:23-46, 104-125
# ----------------------------------------------------------------------------------------------
def pose_ate(pred, gt_global, track_length=5):
    """Absolute trajectory error of every `track_length`-frame snippet (dc_pose_ate: fp64, two launches, bitwise reproducible).
    pred (N,4,4) float32 source-to-target transforms on the device; gt_global (N+1,3,4) float64 rows of KITTI's poses/XX.txt
    on the device.  -> (ates (N,), mean, std) as views of ONE host float64 tensor: the call ends with the only device-to-host
    copy.  A snippet whose predicted points all coincide is NaN (0 / 0 as in numpy), and so are mean and std then."""
    L = _lib.lib()
    p, g = _c(pred.detach()), _c(gt_global.detach())
    if p.dim() != 3 or tuple(p.shape[1:]) != (4, 4) or g.dim() != 3 or tuple(g.shape[1:]) != (3, 4):
        raise DepthcoreError("pose_ate: pred (N,4,4) and gt_global (M,3,4), got %s and %s" % (tuple(p.shape), tuple(g.shape)))
    N, M = p.shape[0], g.shape[0]
    if M < 2 or N != M - 1:
        raise DepthcoreError("pose_ate: %d predicted transforms need %d ground-truth poses, got %d" % (N, N + 1, M))
    if int(track_length) < 1:
        raise DepthcoreError("pose_ate: track_length must be at least 1")
    out = torch.empty(N + 2, dtype=torch.float64, device=p.device)
    check(L.dc_pose_ate(ptr(p), ptr(g, torch.float64), ptr(out, torch.float64), N, M, int(track_length), stream(p)), "dc_pose_ate")
    host = out.cpu()
    return host[:N], host[N], host[N + 1]


# ----------------------------------------------------------------------------------------------
# velodyne depth maps: kitti_utils.generate_depth_map + KITTIRAWDataset.get_depth's resize and flip, a batch per call
# ----------------------------------------------------------------------------------------------
def lidar_depth_maps(points, counts, P, sizes, out_size=None, vel_depth=False, flips=None):
    """Sparse depth maps of B velodyne scans (dc_lidar_depth_maps: three launches on the current stream, bitwise reproducible).
      points: (N, 4) float32 device tensor, the scans back to back in file layout (column 3 is ignored), 16-byte aligned;
      counts: B ints, the points of every scan (0 gives an all-zero map), sum <= N;
      P: (B, 3, 4) float64 on the host (numpy or CPU tensor), lidar.velo_to_image's matrix of every scan;
      sizes: B native (W, H);  out_size: (Ho, Wo) of the result, resized from the native size by Pillow's NEAREST rule
        (lidar.nearest_tables) -- None: the native size, which all scans must then share;
      vel_depth: one bool or B of them (True: the depth is x_velo, the export's convention);  flips: B bools (np.fliplr).
    -> (B, 1, Ho, Wo) float32.  The descriptors and index tables are small host arrays (lidar.descriptors): one host-to-device
    copy per call; a caller whose upload already carries them uses `lidar_depth_maps_staged`."""
    from .lidar import descriptors
    d = descriptors(counts, P, sizes, out_size, vel_depth, flips)
    return lidar_depth_maps_staged(points, d, torch.from_numpy(d.host).to(points.device))


def lidar_depth_maps_staged(points, d, block):
    """`lidar_depth_maps` with the descriptors already on the device: d is lidar.descriptors(...), block a uint8 device tensor
    holding the bytes of d.host at an 8-byte aligned address (the loader's one upload carries them behind the scans)."""
    L = _lib.lib()
    pts = points.detach()
    if pts.dim() != 2 or pts.shape[1] != 4:
        raise DepthcoreError("lidar_depth_maps: points (N, 4), got %s" % (tuple(pts.shape),))
    if block.dtype != torch.uint8 or block.numel() != d.host.size or block.data_ptr() % 8 or block.device != pts.device:
        raise DepthcoreError("lidar_depth_maps: the device block must be the %d descriptor bytes, 8-byte aligned, on %s"
                             % (d.host.size, pts.device))
    dev, n_points = pts.device, pts.shape[0]
    if n_points == 0:                 # every scan is empty: the entry point still wants a valid pointer
        pts = torch.zeros((1, 4), dtype=torch.float32, device=dev)
    ws_bytes = L.dc_lidar_workspace_bytes(d.B, int(d.desc["W"].max()), int(d.desc["H"].max()))
    if ws_bytes == 0:
        raise DepthcoreError("lidar_depth_maps: native sizes up to %d x %d are out of range" % (d.desc["W"].max(), d.desc["H"].max()))
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    out = torch.empty((d.B, 1, d.Ho, d.Wo), dtype=torch.float32, device=dev)
    base = ptr(block, torch.uint8)
    check(L.dc_lidar_depth_maps(ptr(pts), n_points, d.desc.ctypes.data, base, d.B, d.rows.ctypes.data, base + d.rows_off,
                                d.cols.ctypes.data, base + d.cols_off, d.Ho, d.Wo, ptr(out), ws.data_ptr(), ws_bytes, stream(pts)),
          "dc_lidar_depth_maps")
    return out


# ----------------------------------------------------------------------------------------------
# depth evaluation: the prediction side of evaluate_depth.py:95-135 and its benchmark export (:159-171)
# ----------------------------------------------------------------------------------------------
def flip_concat(x):
    """torch.cat((x, torch.flip(x, [3])), 0) of evaluate_depth.py:123 in one launch (dc_flip_concat): (B,C,H,W) -> (2B,C,H,W).
    No gradient (an evaluation input)."""
    L = _lib.lib()
    xx = _c(x.detach())
    if xx.dim() != 4:
        raise DepthcoreError("flip_concat: (B,C,H,W), got %s" % (tuple(xx.shape),))
    B, C, H, W = xx.shape
    out = torch.empty((2 * B, C, H, W), dtype=torch.float32, device=xx.device)
    check(L.dc_flip_concat(ptr(xx), ptr(out), B, C, H, W, stream(xx)), "dc_flip_concat")
    return out


def post_process_disparity(disp, min_depth, max_depth):
    """The decoder's sigmoid disparity (2B,1,h,w) of the batch [x; flip_w(x)] -> (B,1,h,w) post-processed scaled disparity
    (dc_disp_post_process): disp_to_depth's scaled disparity of both halves (bit for bit ops.disp_to_depth's), the second
    mirrored back, blended as batch_post_process_disparity (evaluate_depth.py:48-56) in its own types -- fp32 mean, fp64 masks
    and products -- and rounded to fp32 once.  No gradient."""
    L = _lib.lib()
    d = _c(disp.detach())
    if d.dim() != 4 or d.shape[1] != 1 or d.shape[0] % 2:
        raise DepthcoreError("post_process_disparity: (2B,1,h,w), got %s" % (tuple(d.shape),))
    B, _, h, w = d.shape
    out = torch.empty((B // 2, 1, h, w), dtype=torch.float32, device=d.device)
    check(L.dc_disp_post_process(ptr(d), ptr(out), B // 2, h, w, float(min_depth), float(max_depth), stream(d)),
          "dc_disp_post_process")
    return out


STEREO_SCALE_FACTOR = 5.4       # evaluate_depth.py:24
BENCHMARK_SIZE = (352, 1216)    # evaluate_depth.py:166 (cv2's (width, height) = (1216, 352))


def depth_png16(disp, size=BENCHMARK_SIZE, scale=STEREO_SCALE_FACTOR):
    """KITTI benchmark depth maps of evaluate_depth.py:165-169 (dc_depth_png16): scaled disparity (N,1,h,w) ->
    (N, Ho, Wo) uint16 = uint16(clip(scale / bilinear(disp), 0, 80) * 256), the upsample F.interpolate(bilinear,
    align_corners=False)'s (bit for bit ops.upsample_bilinear's).  The PNG encoding is the caller's."""
    L = _lib.lib()
    d = _c(disp.detach())
    if d.dim() != 4 or d.shape[1] != 1:
        raise DepthcoreError("depth_png16: (N,1,h,w), got %s" % (tuple(d.shape),))
    N, _, h, w = d.shape
    Ho, Wo = int(size[0]), int(size[1])
    out = torch.empty((N, Ho, Wo), dtype=torch.uint16, device=d.device)
    check(L.dc_depth_png16(ptr(d), out.data_ptr(), N, h, w, Ho, Wo, float(scale), stream(d)), "dc_depth_png16")
    return out


# ----------------------------------------------------------------------------------------------
# single-image inference: the colour image of test_simple.py:126-145
# ----------------------------------------------------------------------------------------------
_MAGMA = {}


def magma_lut(device=None):
    """matplotlib's 256-entry magma quantised as test_simple.py:141 does, (lut[:256, :3] * 255).astype(uint8): a (256,3) uint8
    tensor from the literal in depthcore/_magma.py (matplotlib is not a dependency).  device=None: on the host."""
    if "host" not in _MAGMA:
        from ._magma import MAGMA_LUT8_HEX
        raw = bytes.fromhex(MAGMA_LUT8_HEX)
        if len(raw) != 768:
            raise DepthcoreError("depthcore/_magma.py: expected 768 bytes, got %d" % len(raw))
        _MAGMA["host"] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).view(256, 3)
    if device is None:
        return _MAGMA["host"]
    device = torch.device(device)
    if device not in _MAGMA:
        _MAGMA[device] = _MAGMA["host"].to(device)
    return _MAGMA[device]


def _render_disparity(disp, size, percentile, lut, buf=None):
    """dc_disp_render into `buf`, a uint8 device tensor laid out [rgb (N*Ho*Wo*3) | pad to 4 | range (N*2 fp32)] (allocated when
    None) -> (rgb, range, buf): views of it, so that a caller brings both to the host with one copy."""
    L = _lib.lib()
    d = _c(disp.detach())
    if d.dim() != 4 or d.shape[1] != 1:
        raise DepthcoreError("render_disparity: (N,1,h,w), got %s" % (tuple(d.shape),))
    N, _, h, w = d.shape
    Ho, Wo = int(size[0]), int(size[1])
    q = float(percentile)
    if N < 1 or h < 1 or w < 1 or Ho < 1 or Wo < 1:
        raise DepthcoreError("render_disparity: empty input %s or target size %s" % (tuple(d.shape), (Ho, Wo)))
    if not 0.0 <= q <= 100.0:
        raise DepthcoreError("render_disparity: percentile must be in [0, 100], got %r" % (percentile,))
    if lut is None:
        lut = magma_lut(d.device)
    if tuple(lut.shape) != (256, 3) or lut.dtype != torch.uint8 or lut.device != d.device:
        raise DepthcoreError("render_disparity: lut must be a (256,3) uint8 tensor on %s, got %s %s on %s"
                             % (d.device, tuple(lut.shape), lut.dtype, lut.device))
    nrgb = N * Ho * Wo * 3
    roff = (nrgb + 3) & ~3
    if buf is None:
        buf = torch.empty(roff + N * 8, dtype=torch.uint8, device=d.device)
    rgb = buf[:nrgb].view(N, Ho, Wo, 3)
    rng = buf[roff:roff + N * 8].view(torch.float32).view(N, 2)
    nws = L.dc_disp_render_ws_bytes(N, h, w, Ho, Wo)
    if nws == 0:
        raise DepthcoreError("render_disparity: unsupported shape %s -> %s" % (tuple(d.shape), (Ho, Wo)))
    ws = torch.empty(nws, dtype=torch.uint8, device=d.device)
    check(L.dc_disp_render(ptr(d), ptr(_c(lut), torch.uint8), ptr(rgb, torch.uint8), ptr(rng), N, h, w, Ho, Wo, q, ws.data_ptr(),
                           nws, stream(d)), "dc_disp_render")
    return rgb, rng, buf


def render_disparity(disp, size, percentile=95.0, lut=None):
    """The colour image of test_simple.py:126-145 (dc_disp_render): disp (N,1,h,w) -> (rgb (N,Ho,Wo,3) uint8 -- interleaved, what
    PIL.Image.fromarray takes -- and range (N,2) float32 = (vmin, vmax) of every image), device tensors on the current stream.
    Each image is upsampled to size = (Ho, Wo) by F.interpolate(bilinear, align_corners=False)'s expression (bit for bit
    ops.upsample_bilinear's, never stored), normalised between its own minimum and its own `percentile` (numpy's linear
    interpolation between two exact order statistics, found by radix selection) as matplotlib's Normalize does, and looked up
    in `lut`, a (256,3) uint8 device tensor (default: magma).  Values above the percentile take the last colour; a constant
    image takes the first.  Non-finite input is outside the contract.  Bitwise reproducible.  No gradient."""
    rgb, rng, _ = _render_disparity(disp, size, percentile, lut)
    return rgb, rng


def _drive_maps(disp, size, what):
    d = _c(disp.detach())
    if d.dim() != 4 or d.shape[1] != 1:
        raise DepthcoreError("%s: (N,1,h,w), got %s" % (what, tuple(d.shape)))
    N, _, h, w = d.shape
    Ho, Wo = int(size[0]), int(size[1])
    if N < 1 or h < 1 or w < 1 or Ho < 1 or Wo < 1:
        raise DepthcoreError("%s: empty input %s or target size %s" % (what, tuple(d.shape), (Ho, Wo)))
    return d, N, h, w, Ho, Wo


def disparity_range_pooled(disp, size, percentile=95.0):
    """ONE (vmin, vmax) for all N maps of a drive (dc_disp_range_pooled): disp (N,1,h,w) -> a (2,) float32 device tensor on the
    current stream.  render_disparity's range -- the minimum and numpy's `percentile` between exact order statistics -- of the
    pooled N * Ho * Wo values of the maps upsampled to size = (Ho, Wo); the upsampled maps are never stored.  N * Ho * Wo must
    stay below 2^32.  Bitwise reproducible; no host synchronisation.  No gradient."""
    L = _lib.lib()
    d, N, h, w, Ho, Wo = _drive_maps(disp, size, "disparity_range_pooled")
    q = float(percentile)
    if not 0.0 <= q <= 100.0:
        raise DepthcoreError("disparity_range_pooled: percentile must be in [0, 100], got %r" % (percentile,))
    nws = L.dc_disp_range_pooled_ws_bytes(N, h, w, Ho, Wo)
    if nws == 0:
        raise DepthcoreError("disparity_range_pooled: unsupported shape %s -> %s (N * Ho * Wo must be below 2^32, N at most 65535)"
                             % (tuple(d.shape), (Ho, Wo)))
    ws = torch.empty(nws, dtype=torch.uint8, device=d.device)
    rng = torch.empty(2, dtype=torch.float32, device=d.device)
    check(L.dc_disp_range_pooled(ptr(d), ptr(rng), N, h, w, Ho, Wo, q, ws.data_ptr(), nws, stream(d)), "dc_disp_range_pooled")
    return rng


def render_disparity_fixed(disp, size, rng, lut=None, out=None):
    """render_disparity's colouring against ONE range for all images (dc_disp_render_fixed, one launch): disp (N,1,h,w), rng a
    (2,) float32 device tensor (vmin, vmax) -- disparity_range_pooled's, or any other -- -> rgb (N,Ho,Wo,3) uint8 on the device
    (`out`: a contiguous uint8 device tensor of at least N*Ho*Wo*3 elements to render into).  Values above vmax take the last
    colour, values below vmin the first; vmin == vmax gives the first colour everywhere.  No gradient."""
    L = _lib.lib()
    d, N, h, w, Ho, Wo = _drive_maps(disp, size, "render_disparity_fixed")
    if not torch.is_tensor(rng) or rng.numel() != 2 or rng.dtype != torch.float32 or rng.device != d.device:
        raise DepthcoreError("render_disparity_fixed: rng must be a (2,) float32 tensor on %s" % (d.device,))
    if lut is None:
        lut = magma_lut(d.device)
    if tuple(lut.shape) != (256, 3) or lut.dtype != torch.uint8 or lut.device != d.device:
        raise DepthcoreError("render_disparity_fixed: lut must be a (256,3) uint8 tensor on %s, got %s %s on %s"
                             % (d.device, tuple(lut.shape), lut.dtype, lut.device))
    nrgb = N * Ho * Wo * 3
    if out is None:
        out = torch.empty(nrgb, dtype=torch.uint8, device=d.device)
    if out.dtype != torch.uint8 or out.device != d.device or not out.is_contiguous() or out.numel() < nrgb:
        raise DepthcoreError("render_disparity_fixed: out must be a contiguous uint8 tensor of %d elements on %s" % (nrgb, d.device))
    rgb = out.view(-1)[:nrgb].view(N, Ho, Wo, 3)
    check(L.dc_disp_render_fixed(ptr(d), ptr(_c(lut), torch.uint8), ptr(_c(rng).view(2)), ptr(rgb, torch.uint8), N, h, w, Ho, Wo,
                                 stream(d)), "dc_disp_render_fixed")
    return rgb


# ----------------------------------------------------------------------------------------------
# training-log image panels: the pictures of trainer.py:666-698, composed on the device
# ----------------------------------------------------------------------------------------------
TILE_KINDS = {"rgb": _lib.TILE_RGB, "norm": _lib.TILE_NORM, "unit": _lib.TILE_UNIT, "mask": _lib.TILE_MASK}


def log_panels(tiles, n_panels, size, lut=None, background=0, buf=None):
    """`n_panels` interleaved uint8 images (n_panels, PH, PW, 3), size = (PH, PW), composed from `tiles` (dc_log_panel: at most
    three launches on the current stream, bitwise reproducible).  A tile is (src, kind, panel, up, x0, y0[, thr]):
      src: a device tensor -- "rgb" (3,h,w) float32, "norm" / "unit" (h,w) float32, "mask" (h,w) uint8;
      kind: "rgb" | "norm" | "unit" | "mask" (or the DC_TILE_* number): [0, 1] -> bytes by round-half-up per channel; the
        reference's normalize_image and the colour table `lut` ((256,3) uint8 on the device, default magma); [0, 1] -> grey;
        src >= thr ? 255 : 0;
      panel, (x0, y0): the destination image and the tile's top-left corner in it; up: integer nearest-neighbour factor, the
        tile covers (h*up) x (w*up) pixels.
    Tiles of one panel must not overlap and must lie inside it; a pixel no tile covers holds `background`.  `buf`: a uint8
    device tensor of at least n_panels*PH*PW*3 bytes to compose into (the result is a view of it); None allocates.  The tile
    descriptors are a small host array: one host-to-device copy per call.  No gradient."""
    L = _lib.lib()
    PH, PW = int(size[0]), int(size[1])
    n = len(tiles)
    if n < 1:
        raise DepthcoreError("log_panels: no tiles")
    desc = (_lib.PanelTile * n)()
    keep, dev = [], None
    for i, t in enumerate(tiles):
        src, kind, panel, up, x0, y0 = t[:6]
        thr = t[6] if len(t) > 6 else 0
        kind = TILE_KINDS.get(kind, kind)
        if kind not in TILE_KINDS.values():
            raise DepthcoreError("log_panels: tile %d: unknown kind %r" % (i, t[1]))
        s = _c(src.detach())
        p = ptr(s, torch.uint8 if kind == _lib.TILE_MASK else torch.float32)
        if s.dim() != (3 if kind == _lib.TILE_RGB else 2) or (kind == _lib.TILE_RGB and s.shape[0] != 3):
            raise DepthcoreError("log_panels: tile %d: a %s tile reads %s, got %s"
                                 % (i, t[1], "(3,h,w)" if kind == _lib.TILE_RGB else "(h,w)", tuple(s.shape)))
        dev = s.device if dev is None else dev
        if s.device != dev:
            raise DepthcoreError("log_panels: tile %d lives on %s, the others on %s" % (i, s.device, dev))
        keep.append(s)
        d = desc[i]
        d.src, d.src_elems, d.kind, d.panel = p, s.numel(), kind, int(panel)
        d.h, d.w, d.up, d.x0, d.y0, d.thr = int(s.shape[-2]), int(s.shape[-1]), int(up), int(x0), int(y0), int(thr)
    if lut is None:
        lut = magma_lut(dev)
    if tuple(lut.shape) != (256, 3) or lut.dtype != torch.uint8 or lut.device != dev:
        raise DepthcoreError("log_panels: lut must be a (256,3) uint8 tensor on %s, got %s %s on %s"
                             % (dev, tuple(lut.shape), lut.dtype, lut.device))
    nbytes = max(int(n_panels), 0) * max(PH, 0) * max(PW, 0) * 3
    if buf is None:
        buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    if buf.dtype != torch.uint8 or buf.device != dev or buf.numel() < nbytes or not buf.is_contiguous():
        raise DepthcoreError("log_panels: buf must be a contiguous uint8 tensor of at least %d bytes on %s" % (nbytes, dev))
    # one upload: [descriptors | the range keys' workspace] (sizeof(dc_panel_tile) = 48 keeps the keys 8-byte aligned)
    nd, nws = ctypes.sizeof(desc), L.dc_log_panel_ws_bytes(n)
    host = torch.zeros(nd + nws, dtype=torch.uint8)
    ctypes.memmove(host.data_ptr(), ctypes.addressof(desc), nd)
    block = host.to(dev)
    base = block.data_ptr()
    check(L.dc_log_panel(ctypes.addressof(desc), base, n, ptr(_c(lut), torch.uint8), buf.data_ptr(), int(n_panels), PH, PW,
                         int(background), base + nd, nws, stream(buf)), "dc_log_panel")
    return buf[:nbytes].view(int(n_panels), PH, PW, 3)
