"""The pictures of the reference's log() (trainer.py:666-698) as one panel per logged item, composed on the device
(ops.log_panels -> dc_log_panel): the host receives uint8 panels, not the float tensors they are drawn from.

One item's panel has three columns of H x W tiles:
  row 0          the input frames ("color", -1, 0), ("color", 0, 0), ("color", 1, 0);
  row 1          the warped predictions ("color", -1, 0) and ("color", 1, 0) of `outputs` (columns 0 and 2; only when scale 0 is
                 trained, as in the reference);
  row 2 + i      scale s = opt.scales[i]: the disparity ("disp", s), normalised between its own minimum and maximum and coloured
                 (magma), enlarged 2**s times; then
                   default              column 1: the automask -- the float "identity_selection/s" when the step produced it,
                                        else ("argmin", s) >= the number of identity channels (2, or 1 with avg_reprojection);
                   predictive_mask      columns 1 and 2: the two channels of outputs["predictive_mask"][("disp", s)];
                   disable_automasking  nothing.
Every other cell keeps the background.  The reference's down-scaled input frames color_{f}_{s}, s > 0, are not drawn.
"""
from . import ops

COLUMNS = 3
FRAMES = (-1, 0, 1)


def mask_threshold(opt):
    """The automask from the argmin plane: the identity losses are the first channels of `combined` (trainer.py:597), two of
    them, or one with avg_reprojection; a pixel is kept where a reprojection channel wins."""
    return 1 if opt.avg_reprojection else 2


def panel_rows(opt):
    return 2 + len(opt.scales)


def panel_size(opt):
    """(PH, PW) of one item's panel."""
    return panel_rows(opt) * opt.height, COLUMNS * opt.width


def panel_layout(opt, outputs_have):
    """The tiles of one item's panel: a list of (row, column, kind, key, up) in units of H x W cells.  `outputs_have`: the keys
    of the step's `outputs` (anything supporting `in`).  kind is one of ops.TILE_KINDS; key names the source --
    ("inputs", k), ("outputs", k) or ("predictive_mask", k, channel) -- and `up` is the nearest-neighbour factor that brings it
    to H x W.  Pure: no tensors, no GPU."""
    tiles = [(0, c, "rgb", ("inputs", ("color", f, 0)), 1) for c, f in enumerate(FRAMES)]
    if 0 in opt.scales:
        tiles += [(1, c, "rgb", ("outputs", ("color", f, 0)), 1) for c, f in enumerate(FRAMES) if f != 0]
    for i, s in enumerate(opt.scales):
        row = 2 + i
        tiles.append((row, 0, "norm", ("outputs", ("disp", s)), 2 ** s))
        if opt.predictive_mask:
            tiles += [(row, 1 + ch, "unit", ("predictive_mask", ("disp", s), ch), 2 ** s) for ch in range(2)]
        elif not opt.disable_automasking:
            up = 2 ** s if opt.v1_multiscale else 1
            name = "identity_selection/{}".format(s)
            if name in outputs_have:
                tiles.append((row, 1, "unit", ("outputs", name), up))
            else:
                tiles.append((row, 1, "mask", ("outputs", ("argmin", s)), up))
    return tiles


def _source(inputs, outputs, key, item):
    if key[0] == "inputs":
        return inputs[key[1]][item]
    if key[0] == "predictive_mask":
        return outputs["predictive_mask"][key[1]][item, key[2]]
    t = outputs[key[1]][item]
    return t[0] if t.dim() == 3 and t.shape[0] == 1 else t         # ("disp", s) is (B,1,h,w); argmin / identity_selection (B,h,w)


def training_panels(opt, inputs, outputs, items, buf=None, return_sources=False):
    """Panels (len(items), PH, PW, 3) uint8 on the device for the batch items `items`: the layout turned into tiles and ONE
    ops.log_panels call for all of them.  With `return_sources` also {(panel, row, column): the tensor the tile was read from}."""
    H, W = opt.height, opt.width
    layout = panel_layout(opt, outputs)
    thr = mask_threshold(opt)
    tiles, sources = [], {}
    for p, item in enumerate(items):
        for row, col, kind, key, up in layout:
            src = _source(inputs, outputs, key, item).detach()
            tiles.append((src, kind, p, up, col * W, row * H, thr))
            sources[(p, row, col)] = src
    panels = ops.log_panels(tiles, len(items), panel_size(opt), buf=buf)
    return (panels, sources) if return_sources else panels
