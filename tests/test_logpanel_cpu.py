"""No-GPU checks of the training-log image panels: the C ABI of dc_log_panel (symbols, struct layout, every host-side refusal --
made before any HIP call, so they run here), the contract's numpy restatement, depthcore.logimg.panel_layout, and where
run_epoch calls Trainer.log_images."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import logpanel_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DC_EINVAL, DC_EWORKSPACE = -1, -3
DUMMY = 0x10000                       # a non-null, 4-byte aligned address that is never dereferenced


# ---------------------------------------------------------------------------------------------- ABI
def test_symbols_are_exported_and_bound():
    from depthcore import _lib
    L = _lib.lib()
    for name in ("dc_log_panel", "dc_log_panel_ws_bytes"):
        assert hasattr(L, name) and name in _lib.EXPORTS


def test_panel_tile_layout_matches_c(tmp_path):
    from depthcore import _lib
    fields = [n for n, _ in _lib.PanelTile._fields_]
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "depthcore.h"\nint main(){printf("%zu",sizeof(dc_panel_tile));'
                 + "".join('printf(" %%zu",offsetof(dc_panel_tile,%s));' % n for n in fields)
                 + 'printf(" %d %d %d %d\\n",DC_TILE_RGB,DC_TILE_NORM,DC_TILE_UNIT,DC_TILE_MASK);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(c), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    T = _lib.PanelTile
    want = [ctypes.sizeof(T)] + [getattr(T, n).offset for n in fields] + [_lib.TILE_RGB, _lib.TILE_NORM, _lib.TILE_UNIT, _lib.TILE_MASK]
    assert got == want


def test_ws_bytes_without_gpu():
    from depthcore import _lib
    L = _lib.lib()
    assert L.dc_log_panel_ws_bytes(0) == 0 and L.dc_log_panel_ws_bytes(-3) == 0
    assert 0 < L.dc_log_panel_ws_bytes(1) <= L.dc_log_panel_ws_bytes(72)


# ---------------------------------------------------------------------------------------------- host checks
def _tile(**kw):
    d = dict(src=DUMMY, src_elems=6 * 8, kind=1, panel=0, h=6, w=8, up=2, x0=0, y0=0, thr=0)
    d.update(kw)
    return d


def _call(tiles, n_tiles=None, lut=DUMMY, panels=DUMMY, n_panels=2, PH=24, PW=40, background=0, ws=DUMMY, ws_bytes=None):
    from depthcore import _lib
    L = _lib.lib()
    arr = (_lib.PanelTile * max(len(tiles), 1))()
    for a, t in zip(arr, tiles):
        for k, v in t.items():
            setattr(a, k, v)
    n = len(tiles) if n_tiles is None else n_tiles
    if ws_bytes is None:
        ws_bytes = L.dc_log_panel_ws_bytes(max(n, 1))
    # the device copy is a dummy address too: a call that passed the checks would launch on it, so every case here must be refused
    return L.dc_log_panel(ctypes.addressof(arr), DUMMY, n, lut, panels, n_panels, PH, PW, background, ws, ws_bytes, None)


REFUSED = {
    "n_tiles 0": dict(tiles=[_tile()], n_tiles=0),
    "n_panels 0": dict(tiles=[_tile()], n_panels=0),
    "n_panels 65536": dict(tiles=[_tile()], n_panels=65536),
    "PH 0": dict(tiles=[_tile()], PH=0),
    "PW 0": dict(tiles=[_tile()], PW=0),
    "null lut": dict(tiles=[_tile()], lut=None),
    "null panels": dict(tiles=[_tile()], panels=None),
    "null src": dict(tiles=[_tile(src=None)]),
    "kind 4": dict(tiles=[_tile(kind=4)]),
    "kind -1": dict(tiles=[_tile(kind=-1)]),
    "up 0": dict(tiles=[_tile(up=0)]),
    "h 0": dict(tiles=[_tile(h=0)]),
    "w 0": dict(tiles=[_tile(w=0)]),
    "panel -1": dict(tiles=[_tile(panel=-1)]),
    "panel == n_panels": dict(tiles=[_tile(panel=2)]),
    "leaves on the right": dict(tiles=[_tile(x0=25)]),
    "leaves at the bottom": dict(tiles=[_tile(y0=13)]),
    "negative x0": dict(tiles=[_tile(x0=-1)]),
    "negative y0": dict(tiles=[_tile(y0=-1)]),
    "overlap": dict(tiles=[_tile(), _tile(x0=15, y0=11)]),
    "src_elems short": dict(tiles=[_tile(src_elems=47)]),
    "src_elems short for rgb": dict(tiles=[_tile(kind=0, src_elems=3 * 48 - 1)]),
    "misaligned float src": dict(tiles=[_tile(src=DUMMY + 2)]),
    "misaligned unit src": dict(tiles=[_tile(kind=2, src=DUMMY + 1)]),
    "background 256": dict(tiles=[_tile()], background=256),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_host_checks_refuse(name):
    assert _call(**REFUSED[name]) == DC_EINVAL, name


def test_neighbours_of_the_refusals_reach_the_workspace_check():
    """The same descriptors made legal pass every host check: with a workspace one byte short they stop at DC_EWORKSPACE (still
    nothing launched), which shows that the refusals above are about the one field each of them changes."""
    from depthcore import _lib
    L = _lib.lib()
    legal = [
        [_tile()],
        [_tile(x0=24, y0=12, panel=1)],                               # touches the right and bottom edges
        [_tile(), _tile(x0=16), _tile(y0=12)],                        # abutting tiles do not overlap
        [_tile(), _tile(panel=1)],                                    # the same place in another panel
        [_tile(kind=3, src=DUMMY + 1)],                               # a mask's bytes need no alignment
        [_tile(kind=0, src_elems=3 * 48)],
    ]
    for tiles in legal:
        short = L.dc_log_panel_ws_bytes(len(tiles)) - 1
        assert _call(tiles, ws_bytes=short) == DC_EWORKSPACE, tiles
    assert _call([_tile()], ws_bytes=0) == DC_EWORKSPACE


def test_ops_refuse_cpu_tensors():
    from depthcore import ops
    with pytest.raises(ops.DepthcoreError):
        ops.log_panels([(torch.zeros(4, 4), "unit", 0, 1, 0, 0)], 1, (4, 4))


# ---------------------------------------------------------------------------------------------- the numpy restatement
def test_reference_byte_rule():
    k = np.arange(256)
    v = (k / 255).astype(np.float32)                                  # fp32(k / 255) maps back to k
    assert R.unit_bytes(v).tolist() == k.tolist()
    edge = np.array([-1.0, -0.0, 0.0, 1.0, 1.5, np.nan, np.inf, -np.inf, 0.6 / 255, 0.4 / 255, 254.6 / 255, 1e-30], np.float32)
    assert R.unit_bytes(edge).tolist() == [0, 0, 0, 255, 255, 0, 255, 0, 1, 0, 255, 0]


def test_reference_norm_and_compose():
    lut = np.stack([np.arange(256)] * 3, -1).astype(np.uint8)
    assert R.norm_index(np.full((3, 4), 0.25, np.float32)).max() == 0          # constant: d = 1e5, every index 0
    ramp = np.linspace(0, 1, 33 * 65, dtype=np.float32).reshape(33, 65)
    idx = R.norm_index(ramp)
    assert idx[0, 0] == 0 and idx[-1, -1] == 255 and (np.diff(idx.ravel()) >= 0).all()
    out = R.compose([(ramp, "norm", 1, 1, 2, 3), (np.array([[0, 1], [2, 3]], np.uint8), "mask", 0, 3, 1, 0, 2)], 2, 40, 70, lut, 17)
    assert out.shape == (2, 40, 70, 3) and out[1, 3, 2, 0] == 0 and out[1, 35, 66, 0] == 255 and out[1, 36, 66, 0] == 17
    assert out[0, :6, 1:7, 0].tolist() == [[0] * 6] * 3 + [[255] * 6] * 3 and out[0, 0, 0, 0] == 17


# ---------------------------------------------------------------------------------------------- panel_layout
def _opt(**kw):
    d = dict(height=64, width=128, scales=[0, 1, 2, 3], predictive_mask=False, disable_automasking=False, avg_reprojection=False,
             v1_multiscale=False)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _cells(opt, have=()):
    from depthcore import logimg
    return {(r, c): (kind, key, up) for r, c, kind, key, up in logimg.panel_layout(opt, have)}


def _geometry_ok(opt, have=()):
    """No two tiles share a cell and every tile lies inside ((2 + len(scales)) * H, 3 * W)."""
    from depthcore import logimg
    layout = logimg.panel_layout(opt, have)
    PH, PW = logimg.panel_size(opt)
    assert (PH, PW) == ((2 + len(opt.scales)) * opt.height, 3 * opt.width)
    rects = [(c * opt.width, r * opt.height, opt.width, opt.height) for r, c, *_ in layout]
    for i, (x, y, w, h) in enumerate(rects):
        assert 0 <= x and x + w <= PW and 0 <= y and y + h <= PH
        for x2, y2, w2, h2 in rects[:i]:
            assert not (x < x2 + w2 and x2 < x + w and y < y2 + h2 and y2 < y + h)
    return layout


FRAMES_ROW = {(0, c): ("rgb", ("inputs", ("color", f, 0)), 1) for c, f in enumerate((-1, 0, 1))}
PRED_ROW = {(1, 0): ("rgb", ("outputs", ("color", -1, 0)), 1), (1, 2): ("rgb", ("outputs", ("color", 1, 0)), 1)}


def test_layout_default():
    from depthcore import logimg
    opt = _opt()
    want = {**FRAMES_ROW, **PRED_ROW}
    for i, s in enumerate(opt.scales):
        want[(2 + i, 0)] = ("norm", ("outputs", ("disp", s)), 2 ** s)
        want[(2 + i, 1)] = ("mask", ("outputs", ("argmin", s)), 1)
    assert _cells(opt) == want and len(_geometry_ok(opt)) == len(want)
    assert logimg.mask_threshold(opt) == 2
    # the float automask of the layer-by-layer loss / materialize_logs replaces the argmin plane, scale by scale
    got = _cells(opt, {"identity_selection/0", "identity_selection/2"})
    assert got[(2, 1)] == ("unit", ("outputs", "identity_selection/0"), 1) and got[(3, 1)] == want[(3, 1)]
    assert got[(4, 1)] == ("unit", ("outputs", "identity_selection/2"), 1)


def test_layout_predictive_mask():
    opt = _opt(predictive_mask=True, disable_automasking=True)
    want = {**FRAMES_ROW, **PRED_ROW}
    for i, s in enumerate(opt.scales):
        want[(2 + i, 0)] = ("norm", ("outputs", ("disp", s)), 2 ** s)
        for ch in range(2):
            want[(2 + i, 1 + ch)] = ("unit", ("predictive_mask", ("disp", s), ch), 2 ** s)
    assert _cells(opt) == want and len(_geometry_ok(opt)) == len(want)


def test_layout_no_automask():
    opt = _opt(disable_automasking=True)
    want = {**FRAMES_ROW, **PRED_ROW}
    for i, s in enumerate(opt.scales):
        want[(2 + i, 0)] = ("norm", ("outputs", ("disp", s)), 2 ** s)
    assert _cells(opt) == want and len(_geometry_ok(opt)) == len(want)


def test_layout_avg_reprojection_v1_multiscale_and_two_scales():
    from depthcore import logimg
    opt = _opt(avg_reprojection=True)
    assert logimg.mask_threshold(opt) == 1 and _cells(opt)[(2, 1)] == ("mask", ("outputs", ("argmin", 0)), 1)
    _geometry_ok(opt)
    v1 = _opt(v1_multiscale=True)
    got = _cells(v1, {"identity_selection/1"})
    assert [got[(2 + i, 1)][2] for i in range(4)] == [1, 2, 4, 8] and got[(3, 1)][0] == "unit" and got[(4, 1)][0] == "mask"
    _geometry_ok(v1)
    two = _opt(scales=[0, 2])
    got = _cells(two)
    assert sorted(got) == sorted(list(FRAMES_ROW) + list(PRED_ROW) + [(2, 0), (2, 1), (3, 0), (3, 1)])
    assert got[(3, 0)] == ("norm", ("outputs", ("disp", 2)), 4) and got[(3, 1)] == ("mask", ("outputs", ("argmin", 2)), 1)
    assert logimg.panel_size(two) == (4 * 64, 3 * 128)
    _geometry_ok(two)


def test_log_images_option_defaults_to_off():
    import trainer as T
    assert T.default_options().log_images == 0 and T.default_options(log_images=4).log_images == 4


# ---------------------------------------------------------------------------------------------- the loop
class _StubLoader:
    def __init__(self, n):
        self.n, self.epoch = n, 0

    def __len__(self):
        return self.n

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __iter__(self):
        return iter([{"x": torch.full((1,), float(10 * self.epoch + i))} for i in range(self.n)])


def _stub(tmp_path, **kw):
    """A Trainer without __init__ (as tests/test_train_loop_cpu.py builds it): the loop's own state, recording stand-ins for the
    step, validation, log and log_images."""
    import trainer as T
    tr = T.Trainer.__new__(T.Trainer)
    opt = dict(num_epochs=1, save_frequency=2, log_frequency=2, batch_size=2, scheduler_step_size=1, learning_rate=1e-4,
               log_dir=str(tmp_path), model_name="stub", fusion=None, gru=None, h_s_epoch=10)
    opt.update(kw)
    tr.opt = types.SimpleNamespace(**opt)
    tr.device = torch.device("cpu")
    tr.step = tr.epoch = 0
    tr.models = {}
    tr.train_loader, tr.val_loader, tr._val_iter = _StubLoader(4), _StubLoader(3), None
    w = torch.nn.Parameter(torch.zeros(1))
    tr.model_optimizer = torch.optim.SGD([w], tr.opt.learning_rate)
    tr.model_lr_scheduler = torch.optim.lr_scheduler.StepLR(tr.model_optimizer, tr.opt.scheduler_step_size, 0.1)
    tr.calls = []

    def train_step(inputs):
        tr.step += 1
        return {"out": inputs["x"] + 100}, {"loss": torch.tensor(0.5 + tr.step)}

    def val(inputs):
        return {"out": inputs["x"] + 200}, {"loss": torch.tensor(2.0)}
    real_log = tr.log

    def log(mode, losses, step=None):
        tr.calls.append(("log", mode, step))
        real_log(mode, losses, step)

    def log_images(mode, inputs, outputs, step=None, return_sources=False):
        tr.calls.append(("log_images", mode, step, float(inputs["x"]), float(outputs["out"])))
    tr.train_step, tr.val, tr.log, tr.log_images = train_step, val, log, log_images
    tr.save_model = lambda: None
    return tr


def test_run_epoch_logs_images_after_every_log(tmp_path):
    tr = _stub(tmp_path, log_images=2)
    tr.train()
    kinds = [c[:3] for c in tr.calls]
    # batches 0 and 2 are log steps: scalars, then pictures, for the training batch and then for the validation batch
    assert kinds == [(k, m, s) for s in (0, 2) for m in ("train", "val") for k in ("log", "log_images")]
    # each with its own batch and that batch's outputs
    assert [c[3:] for c in tr.calls if c[0] == "log_images"] == [(0.0, 100.0), (0.0, 200.0), (2.0, 102.0), (1.0, 201.0)]


@pytest.mark.parametrize("kw", [{}, {"log_images": 0}])
def test_run_epoch_without_the_option_never_logs_images(tmp_path, kw, capsys):
    tr = _stub(tmp_path, **kw)
    tr.train()
    assert [c[:3] for c in tr.calls] == [("log", m, s) for s in (0, 2) for m in ("train", "val")]
    assert not os.path.exists(os.path.join(str(tmp_path), "stub", "train", "images"))
    assert not os.path.exists(os.path.join(str(tmp_path), "stub", "val", "images"))
    assert sorted(os.listdir(os.path.join(str(tmp_path), "stub", "train"))) == ["scalars.jsonl"]
    assert len(capsys.readouterr().out.splitlines()) == 2              # the two terminal lines of log_time, nothing else
