"""dc_lidar_depth_maps through ctypes for the tests that hand it their own buffers or deliberately bad arguments."""
import numpy as np

BAD_ARGUMENTS = ["n_img=0", "n_img<0", "Ho=0", "Wo<0", "W=0", "W=1", "H=0", "count<0", "off<0", "range past the buffer",
                 "offset past the buffer", "row entry = H", "row entry < 0", "col entry = W", "col entry < 0", "points null",
                 "desc_host null", "desc_dev null", "rows_host null", "rows_dev null", "cols_host null", "cols_dev null", "out null",
                 "workspace null"]


def arguments(counts, sizes, out_hw, n_points=None):
    """Valid host-side arguments for scans of `counts` points and native `sizes` (W, H): -> dict(desc, rows, cols, n_points, Ho,
    Wo); rows / cols are the identity clipped to the native size (any in-range table is legal)."""
    from depthcore.lidar import LIDAR_IMG
    B, (Ho, Wo) = len(counts), out_hw
    desc = np.zeros(B, LIDAR_IMG)
    desc["n_points"] = counts
    desc["point_off"] = np.cumsum(counts) - np.asarray(counts)
    desc["W"], desc["H"] = [s[0] for s in sizes], [s[1] for s in sizes]
    desc["P"] = np.array([[10, 0, 5, 0, 0, 10, 5, 0, 0, 0, 1, 0]], np.float64)
    rows = np.stack([np.minimum(np.arange(Ho), s[1] - 1) for s in sizes]).astype(np.int32)
    cols = np.stack([np.minimum(np.arange(Wo), s[0] - 1) for s in sizes]).astype(np.int32)
    return {"desc": desc, "rows": rows, "cols": cols, "n_points": int(sum(counts)) if n_points is None else n_points, "Ho": Ho, "Wo": Wo}


def spoil(args, what):
    """Make one argument of `arguments(...)` (two images at least, the second with points) invalid, in place -> pointer names
    to pass as NULL."""
    d = args["desc"]
    null = []
    if what == "n_img=0":
        args["n_img"] = 0
    elif what == "n_img<0":
        args["n_img"] = -1
    elif what == "Ho=0":
        args["Ho"] = 0
    elif what == "Wo<0":
        args["Wo"] = -3
    elif what == "W=0":
        d["W"][1] = 0
    elif what == "W=1":
        d["W"][1] = 1
    elif what == "H=0":
        d["H"][0] = 0
    elif what == "count<0":
        d["n_points"][0] = -1
    elif what == "off<0":
        d["point_off"][1] = -1
    elif what == "range past the buffer":
        d["n_points"][1] += 1
    elif what == "offset past the buffer":
        d["point_off"][1] = args["n_points"] + 1
        d["n_points"][1] = 0
    elif what == "row entry = H":
        args["rows"][1, -1] = d["H"][1]
    elif what == "row entry < 0":
        args["rows"][0, 0] = -1
    elif what == "col entry = W":
        args["cols"][0, 3] = d["W"][0]
    elif what == "col entry < 0":
        args["cols"][1, 0] = -1
    elif what.endswith(" null"):
        null = [what[:-5]]
    else:
        raise KeyError(what)
    return null


def call(L, args, points, desc_dev, rows_dev, cols_dev, out, workspace, workspace_bytes, stream=None, null=()):
    """The raw entry point; points / *_dev / out / workspace are addresses (ints)."""
    p = {"points": points, "desc_host": args["desc"].ctypes.data, "desc_dev": desc_dev, "rows_host": args["rows"].ctypes.data,
         "rows_dev": rows_dev, "cols_host": args["cols"].ctypes.data, "cols_dev": cols_dev, "out": out, "workspace": workspace}
    for k in null:
        p[k] = None
    return L.dc_lidar_depth_maps(p["points"], args["n_points"], p["desc_host"], p["desc_dev"], args.get("n_img", len(args["desc"])),
                                 p["rows_host"], p["rows_dev"], p["cols_host"], p["cols_dev"], args["Ho"], args["Wo"], p["out"],
                                 p["workspace"], workspace_bytes, stream)
