"""bench.py on the product path at a small size: a plain run times exactly --steps steps and reports only the headline, its
`--dump-outputs` files are the last timed step's outputs, losses and parameters, and `--full` still adds the diagnostics."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
BENCH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "2", "--height", "64", "--width", "128"]


def _line(args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, BENCH] + SMALL + args, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_and_dump_outputs(tmp_path):
    d = _line(["--dump-outputs", str(tmp_path)])
    assert d["steps"] == 3 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    assert abs(d["value"] - 2 * 3 / (3 * d["ms_per_step"] * 1e-3)) <= 1e-2 * d["value"]
    assert d["dtype"].startswith("f32") and d["unit"] == "images/s"
    for k in ("roofline", "phases_ms", "windows_ms_per_step", "cpu_baseline"):
        assert k not in d, k
    names = set(os.listdir(tmp_path))
    assert {"losses.loss.npy", "outputs.disp_0.npy", "outputs.disp_3.npy", "parameters.npy"} <= names, sorted(names)
    assert np.load(tmp_path / "outputs.disp_0.npy").shape == (2, 1, 64, 128)
    for n in names:
        a = np.load(tmp_path / n)
        assert a.dtype == np.float32 and np.isfinite(a).all(), n
    loss = float(np.load(tmp_path / "losses.loss.npy"))
    assert abs(loss - d["loss_last"]) <= 1e-5 * abs(loss)


def test_full_run_keeps_the_diagnostics():
    d = _line(["--full", "--no-cpu-baseline", "--windows", "2"])
    assert d["steps"] == 3 and len(d["windows_ms_per_step"]) == 2 and d["windows_ms_per_step"][0] == d["ms_per_step"]
    assert d["roofline"]["kernel"] and "photometric" in d["roofline"] and d["phases_ms"]["forward"] > 0
