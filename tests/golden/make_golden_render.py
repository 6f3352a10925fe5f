"""Writes tests/golden/render.npz: small disparity maps and the colour bytes / vmax that matplotlib + numpy produce for them
with the reference's own statements, plus matplotlib's magma table quantised to bytes.

The five statements of the reference's test_simple.py (lines 137-141: the host copy, np.percentile, Normalize, ScalarMappable,
the uint8 cast) are taken from the reference file's source by line number and run in a namespace holding numpy, matplotlib and
the upsampled tensor only.  The reference tree is only read when this script runs:

    python tests/golden/make_golden_render.py /path/to/reference

(A photo one pixel wide or high makes those statements fail on their own squeeze(); for the two such cases the same matplotlib
and numpy calls are made on the unsqueezed map.)  Per case (tests/render_ref.py: FIXTURE_CASES) the fixture holds the low-resolution map `<name>_disp`, its upsampled map
`<name>_up` (torch's CPU F.interpolate(bilinear, align_corners=False), what the reference renders), matplotlib's bytes
`<name>_rgb` and -- only where the fp64 virtual index of the contract and the installed numpy's agree bitwise -- `<name>_vmax`
(numpy 2.x forms the index in the array's fp32: DESIGN 4l).  Before anything is written the script asserts that
tests/render_ref.py gives the same bytes for every case and the same vmax for every stored vmax: a case that does not agree is
to be replaced, not tolerated."""
import os
import sys

import matplotlib as mpl
import matplotlib.cm as cm
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import render_ref as R  # noqa: E402

FIRST, LAST = 137, 141


def reference_statements(ref):
    lines = open(os.path.join(ref, "test_simple.py")).read().splitlines()[FIRST - 1:LAST]
    assert "disp_resized_np" in lines[0] and "colormapped_im" in lines[-1], lines
    return compile("\n".join(l.strip() for l in lines), "test_simple.py", "exec")


def main(ref):
    code = reference_statements(ref)
    table = (mpl.colormaps["magma"](np.arange(256))[:, :3] * 255).astype(np.uint8)
    res = {"lut": table}
    for name, (h, w, Ho, Wo, kind, seed) in R.FIXTURE_CASES.items():
        disp = R.low_res_map(h, w, kind, seed)
        up = torch.nn.functional.interpolate(torch.from_numpy(disp)[None, None], (Ho, Wo), mode="bilinear", align_corners=False)
        if min(Ho, Wo) > 1:
            ns = {"np": np, "mpl": mpl, "cm": cm, "disp_resized": up}
            exec(code, ns)
            up_np, rgb = ns["disp_resized_np"], ns["colormapped_im"]
        else:
            # the statements' squeeze() drops the unit axis of a one-pixel-wide photo and their [:, :, :3] then fails: the same
            # matplotlib and numpy calls on the two-dimensional map (render_ref.matplotlib_render)
            up_np = up[0, 0].numpy()
            rgb, _, vm = R.matplotlib_render(up_np, 95.0)
            ns = {"vmax": vm}
        assert up_np.shape == (Ho, Wo) and rgb.shape == (Ho, Wo, 3) and rgb.dtype == np.uint8
        want, vmin, vmax = R.render(up_np, 95.0, table)
        assert want.tobytes() == rgb.tobytes(), "%s: the contract and matplotlib differ in %d bytes" % (name, (want != rgb).sum())
        assert vmin == up_np.min()
        res[name + "_disp"], res[name + "_up"], res[name + "_rgb"] = disp, up_np, rgb
        same = np.float32(ns["vmax"]).tobytes() == vmax.tobytes()
        if same:
            res[name + "_vmax"] = np.float32(ns["vmax"])
        print("%-10s (%d,%d)->(%d,%d) %-8s bytes equal, vmax %s (contract %.9g, numpy %.9g)"
              % (name, h, w, Ho, Wo, kind, "equal" if same else "DIFFERS: not stored", vmax, ns["vmax"]))
    out = os.path.join(HERE, "render.npz")
    np.savez_compressed(out, **res)
    print("wrote", out, os.path.getsize(out), "bytes; matplotlib", mpl.__version__, "numpy", np.__version__)


if __name__ == "__main__":
    main(sys.argv[1])
