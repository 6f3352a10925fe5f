"""Training-log image panels on the device: ops.log_panels (dc_log_panel) held byte for byte to the contract's numpy restatement
(tests/logpanel_ref.py), Trainer.log_images tile by tile against the tensors it read, and training left bitwise where it was."""
import os

import numpy as np
import pytest
import torch

import logpanel_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B, H, W = 2, 64, 128


def _lut():
    from depthcore import ops
    return ops.magma_lut().numpy()


def _check(tiles, n_panels, PH, PW, background=0, lut=None, odd_buf=False):
    """tiles with numpy sources -> the device panels of two calls, both equal to logpanel_ref.compose byte for byte."""
    from depthcore import ops
    dev_tiles = [(torch.from_numpy(np.ascontiguousarray(t[0])).to(DEV),) + tuple(t[1:]) for t in tiles]
    lut_np = _lut() if lut is None else lut
    lut_dev = None if lut is None else torch.from_numpy(lut).to(DEV)
    got = []
    for _ in range(2):
        buf = None
        if odd_buf:                                   # a buffer that starts one byte past a dword: the clear's head and tail
            buf = torch.full((n_panels * PH * PW * 3 + 6,), 99, dtype=torch.uint8, device=DEV)[1:]
        out = ops.log_panels(dev_tiles, n_panels, (PH, PW), lut=lut_dev, background=background, buf=buf)
        assert out.shape == (n_panels, PH, PW, 3) and out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous()
        if odd_buf:
            assert out.data_ptr() % 4 == 1 and buf[n_panels * PH * PW * 3:].tolist() == [99] * 5     # nothing past the panels
        got.append(out.cpu().numpy())
    want = R.compose(tiles, n_panels, PH, PW, lut_np, background)
    nbad = int((got[0] != want).sum())
    print("\n%d tiles -> (%d, %d, %d, 3): bytes differing %d" % (len(tiles), n_panels, PH, PW, nbad))
    assert got[0].tobytes() == want.tobytes(), "%d bytes differ" % nbad
    assert got[1].tobytes() == got[0].tobytes()                                # two calls: equal bytes
    return got[0]


# ---------------------------------------------------------------------------------------------- kernel vs logpanel_ref
def _rgb_sources():
    """Three 5 x 7 RGB sources (315 values): k / 255 for all 256 k, values below 0 and above 1, NaN, and values in between."""
    rng = np.random.default_rng(7)
    vals = np.concatenate([(np.arange(256) / 255).astype(np.float32),
                           np.array([-3.0, -1e-6, -0.0, 1.0 + 1e-6, 2.5, 1e30, np.nan, np.nan], np.float32),
                           rng.random(315 - 256 - 8).astype(np.float32)])
    vals = vals[rng.permutation(315)]
    assert np.isnan(vals).sum() == 2 and (vals < 0).any() and (vals > 1).any()
    return [vals[i * 105:(i + 1) * 105].reshape(3, 5, 7) for i in range(3)]


@pytest.mark.parametrize("up", [1, 3])
def test_rgb_bytes(up):
    srcs = _rgb_sources()
    tiles = [(s, "rgb", 0, up, 1 + i * (7 * up + 1), i) for i, s in enumerate(srcs)]           # odd and even x0, staggered rows
    out = _check(tiles, 1, 5 * up + 3, 3 * (7 * up + 1) + 2, background=17)
    # fp32(k / 255) comes back as k: seen through the first source's k / 255 entries
    s0 = srcs[0]
    exact = np.isin(s0, (np.arange(256) / 255).astype(np.float32))
    px = out[0, 0:5 * up:up, 1:1 + 7 * up:up].transpose(2, 0, 1)
    assert np.array_equal(px[exact], np.round(s0[exact].astype(np.float64) * 255).astype(np.uint8))


def _ramp(h, w, reverse=False):
    v = (0.01 + 0.98 * np.arange(h * w, dtype=np.float64) / max(h * w - 1, 1)).astype(np.float32)
    rng = np.random.default_rng(h * w)
    v[1:-1] = v[1:-1][rng.permutation(h * w - 2)] if h * w > 2 else v[1:-1]       # the extremes stay first and last
    return (v[::-1] if reverse else v).reshape(h, w).copy()


def test_norm_constant_and_single_pixel():
    const = np.full((6, 9), 0.37, np.float32)
    one = np.array([[0.8]], np.float32)
    out = _check([(const, "norm", 0, 1, 0, 0), (one, "norm", 0, 4, 10, 1)], 1, 6, 15, background=3)
    lut = _lut()
    assert (out[0, :, :9] == lut[0]).all() and (out[0, 1:5, 10:14] == lut[0]).all()     # every index is 0


@pytest.mark.parametrize("reverse", [False, True])
def test_norm_extremes_at_the_ends(reverse):
    src = _ramp(33, 65, reverse)
    assert {float(src.flat[0]), float(src.flat[-1])} == {float(src.min()), float(src.max())}
    out = _check([(src, "norm", 0, 1, 3, 1)], 1, 35, 70, background=17)
    lut = _lut()
    lo, hi = (out[0, 33, 67], out[0, 1, 3]) if reverse else (out[0, 1, 3], out[0, 33, 67])
    assert (lo == lut[0]).all() and (hi == lut[255]).all()


def test_norm_many_blocks_and_upsampled():
    rng = np.random.default_rng(3)
    big = (1.0 / (1.0 + np.exp(-rng.standard_normal((96, 160))))).astype(np.float32)       # more than one block each pass
    small = rng.random((12, 20)).astype(np.float32) * np.float32(0.2) - np.float32(0.1)    # negative values: the keys' order
    _check([(big, "norm", 0, 1, 0, 0), (small, "norm", 1, 8, 0, 0), (big[:48, :80].copy(), "norm", 0, 2, 160, 0)], 2, 96, 320)


def test_norm_one_ulp_apart():
    a = np.float32(0.5)
    b = np.nextafter(a, np.float32(1))
    src = np.where(np.arange(35).reshape(5, 7) % 3 == 0, b, a).astype(np.float32)
    out = _check([(src, "norm", 0, 2, 1, 0)], 1, 10, 15)
    lut = _lut()
    assert (out[0, 0, 1] == lut[255]).all() and (out[0, 0, 3] == lut[0]).all()


@pytest.mark.parametrize("thr", [1, 2])
def test_mask_threshold(thr):
    src = (np.arange(6 * 10) % 4).astype(np.uint8).reshape(6, 10)
    out = _check([(src, "mask", 0, 1, 1, 0, thr), (src[:, 1:4].copy(), "mask", 0, 2, 12, 0, thr)], 1, 12, 19, background=17)
    assert np.array_equal(out[0, :6, 1:11, 1], np.where(src >= thr, 255, 0))


def test_unit_grey():
    rng = np.random.default_rng(5)
    src = rng.random((7, 11)).astype(np.float32)
    src[0, :4] = [0.0, 1.0, 0.5, np.float32(0.5 / 255)]
    out = _check([(src, "unit", 0, 1, 0, 0), (src, "unit", 0, 2, 11, 0)], 1, 14, 33)
    assert out[0, 0, :3, 0].tolist() == [0, 255, 128] and (out[0, ..., 0] == out[0, ..., 2]).all()


@pytest.mark.parametrize("PW", [5, 7])
def test_unaligned_rows_edges_two_panels_and_background(PW):
    """Rows of 3 * PW bytes (15, 21: no row but the first starts on a dword), tiles at odd x0, tiles that touch the right and
    bottom edges, two panels in one call, a region no tile covers, and a panel buffer at an odd address."""
    rng = np.random.default_rng(PW)
    rgb = rng.random((3, 3, PW - 1)).astype(np.float32)
    nrm = rng.random((2, 2)).astype(np.float32)
    msk = (rng.integers(0, 4, (3, 2))).astype(np.uint8)
    unit = rng.random((1, PW)).astype(np.float32)
    tiles = [(rgb, "rgb", 0, 1, 1, 0),                        # odd x0, reaches the right edge
             (nrm, "norm", 0, 2, PW - 4, 5),                  # bottom-right corner of panel 0 (rows 5..8)
             (msk, "mask", 1, 1, 3, 2, 2),                    # odd x0 in panel 1
             (unit, "unit", 1, 1, 0, 8)]                      # the last row of the last panel, edge to edge
    for odd in (False, True):
        out = _check(tiles, 2, 9, PW, background=17, odd_buf=odd)
        assert (out[0, :, 0] == 17).all() and (out[0, 3:5] == 17).all() and (out[1, :2] == 17).all() and (out[1, 5:8] == 17).all()


def test_custom_table():
    lut = np.stack([np.arange(256), 255 - np.arange(256), (np.arange(256) * 7) % 256], -1).astype(np.uint8)
    _check([(_ramp(9, 13), "norm", 0, 1, 0, 0)], 1, 9, 13, lut=lut)


# ---------------------------------------------------------------------------------------------- the trainer
def _trainer(**kw):
    import trainer as T
    o = T.default_options(batch_size=B, height=H, width=W, num_layers=18, **kw)
    tr = T.Trainer(o, device=DEV)
    tr.set_train()
    return tr


def _batch(seed=0):
    from depthcore.synthetic import synthetic_batch
    return synthetic_batch(B, H, W, DEV, seed=seed)


MODES = {"fused": {}, "layer_by_layer": dict(fused_loss=False), "materialize": dict(materialize_logs=1),
         "predictive_mask": dict(predictive_mask=True, disable_automasking=True), "v1_multiscale": dict(v1_multiscale=True)}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_trainer_panels_equal_the_reference_on_their_sources(mode, tmp_path):
    from depthcore import logimg
    from PIL import Image
    tr = _trainer(log_images=2, log_dir=str(tmp_path), model_name="run", **MODES[mode])
    inputs = _batch(1)
    outputs, _ = tr.train_step(inputs)
    host, sources = tr.log_images("train", inputs, outputs, step=5, return_sources=True)
    assert isinstance(host, np.ndarray) and host.dtype == np.uint8 and host.shape == (2, 6 * H, 3 * W, 3)
    o, lut = tr.opt, _lut()
    layout = logimg.panel_layout(o, outputs)
    assert sorted(sources) == sorted((j, r, c) for j in range(2) for r, c, *_ in layout)
    cells = {(r, c): (kind, up) for r, c, kind, _, up in layout}
    covered = np.zeros((6, 3), bool)
    for (j, r, c), src in sources.items():
        kind, up = cells[(r, c)]
        want = R.tile_bytes(src.cpu().numpy(), kind, up, logimg.mask_threshold(o), lut)
        assert want.shape == (H, W, 3), (r, c, want.shape)
        assert np.array_equal(host[j, r * H:(r + 1) * H, c * W:(c + 1) * W], want), (mode, j, r, c)     # exact: no tolerance
        covered[r, c] = True
    for r, c in zip(*np.nonzero(~covered)):                                    # blank cells keep the background
        assert (host[:, r * H:(r + 1) * H, c * W:(c + 1) * W] == 0).all()
    assert covered[0].all() and covered[1].tolist() == [True, False, True] and covered[2:, 0].all()
    for j in range(2):
        # row 0: round(255 * frame).  The synthetic frames are arbitrary floats, not decoded bytes: the contract's fp32 product
        # 255 * v carries up to half an ulp of 255 (2^-17) of rounding and the sum with 0.5 as much again, so a value that close
        # to a tie k + 0.5 may fall on either side of it.  Away from ties (2^-15, twice that) the bytes are equal; at a tie they
        # are within one.
        for c, f in enumerate((-1, 0, 1)):
            x = 255 * inputs[("color", f, 0)][j].cpu().numpy().astype(np.float64).transpose(1, 2, 0)
            want = np.floor(x + 0.5)
            tie = np.abs(x + 0.5 - np.round(x + 0.5)) < 2.0 ** -15
            got = host[j, :H, c * W:(c + 1) * W].astype(np.float64)
            print("\n%s item %d frame %d: %d of %d values within 2^-15 of a tie" % (mode, j, f, int(tie.sum()), tie.size))
            assert tie.mean() < 1e-3 and np.array_equal(got[~tie], want[~tie]) and (np.abs(got - want)[tie] <= 1).all()
        # row 1: the warped predictions are those of the step (or of its recomputation: the same kernels on the same values)
        for c, f in ((0, -1), (2, 1)):
            assert sources[(j, 1, c)].shape == (3, H, W) and bool(torch.isfinite(sources[(j, 1, c)]).all())
            if ("color", f, 0) in outputs:
                assert torch.equal(sources[(j, 1, c)], outputs[("color", f, 0)][j])
    if mode in ("fused", "v1_multiscale"):
        assert ("color", -1, 0) not in outputs                                # the recomputation did not leak into the step's dict
        auto = (outputs[("argmin", 0)] >= 2).cpu().numpy().astype(np.uint8) * 255
        for j in range(2):
            assert np.array_equal(host[j, 2 * H:3 * H, W:2 * W, 0], auto[j])
    if mode == "predictive_mask":
        assert covered[2:, 1:].all()
    for j in range(2):
        path = os.path.join(str(tmp_path), "run", "train", "images", "0000005_%d.jpg" % j)
        assert os.path.isfile(path)
        with Image.open(path) as im:
            assert im.size == (3 * W, (2 + 4) * H) and im.mode == "RGB" and im.format == "JPEG"
    assert sorted(os.listdir(os.path.join(str(tmp_path), "run", "train", "images"))) == ["0000005_0.jpg", "0000005_1.jpg"]


def test_recomputed_predictions_are_the_materialized_ones(tmp_path):
    """Two trainers of one seed, one of them with materialize_logs: the warped images log_images recomputes for ONE item of the
    plain fused step (a slice of the batch) are bit for bit the ones the materializing step wrote for that item."""
    a = _trainer(log_images=1, log_dir=str(tmp_path), model_name="a")
    b = _trainer(log_images=2, log_dir=str(tmp_path), model_name="b", materialize_logs=1)
    inputs = _batch(2)
    oa, _ = a.train_step(inputs)
    ob, _ = b.train_step(inputs)
    ha, sa = a.log_images("train", inputs, oa, return_sources=True)
    hb, sb = b.log_images("train", inputs, ob, return_sources=True)
    assert ha.shape == (1, 6 * H, 3 * W, 3) and hb.shape == (2, 6 * H, 3 * W, 3)
    for c in (0, 2):
        assert torch.equal(sa[(0, 1, c)], sb[(0, 1, c)])
    assert np.array_equal(ha[0, :2 * H], hb[0, :2 * H]) and np.array_equal(ha[0, 2 * H:, :W], hb[0, 2 * H:, :W])
    # the automask: the argmin plane at threshold 2 and the float identity_selection draw the same picture
    assert np.array_equal(ha[0], hb[0])
    assert sorted(os.listdir(os.path.join(str(tmp_path), "a", "train", "images"))) == ["0000001_0.jpg"]


@pytest.mark.parametrize("cpu_noise", [0, 1])
def test_training_is_untouched(cpu_noise, tmp_path):
    batches = [_batch(10 + i) for i in range(3)]

    def run(log):
        tr = _trainer(log_images=2, log_dir=str(tmp_path), model_name="log%d" % log, cpu_tiebreak_noise=cpu_noise)
        losses = []
        for i, inputs in enumerate(batches):
            outputs, l = tr.train_step(dict(inputs))
            losses.append(l["loss"].detach().clone())
            if log:
                step, graphs = tr.step, dict(tr._graphs)
                tr.log_images("train", inputs, outputs)
                assert tr.step == step and tr._graphs == graphs and all(m.training for m in tr.models.values())
        torch.cuda.synchronize()
        return losses, [p.detach().clone() for p in tr.parameters_to_train], torch.get_rng_state()
    la, pa, ra = run(False)
    lb, pb, rb = run(True)
    assert all(torch.equal(x, y) for x, y in zip(la, lb))
    assert len(pa) == len(pb) and all(torch.equal(x, y) for x, y in zip(pa, pb))
    assert torch.equal(ra, rb)                                                 # the CPU generator was not drawn from
    assert len(os.listdir(os.path.join(str(tmp_path), "log1", "train", "images"))) == 6
    assert not os.path.exists(os.path.join(str(tmp_path), "log0", "train", "images"))
