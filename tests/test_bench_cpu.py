"""bench.py's multi-rank plumbing on a machine without GPUs: the self-launcher (fresh child per rank, rendezvous on
127.0.0.1, rank 0's single JSON line relayed), its refusal to print a mislabelled line, and the bucketed exchange of
depthcore/ddp.py over gloo inside it.  The GPU step itself is replaced by the `--rehearse` stand-in (flagged in the line)."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _run(args, env=None, timeout=240):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, BENCH] + args, env=e, capture_output=True, text=True, timeout=timeout)


def test_gpus_2_without_gpus_refuses_cleanly():
    import torch
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("needs a machine with fewer than 2 GPUs")
    r = _run(["--gpus", "2", "--steps", "2", "--warmup", "1"])
    assert r.returncode == 2, (r.returncode, r.stderr[-400:])
    assert r.stdout.strip() == ""                       # no mislabelled n_gpus:1 line
    assert "--gpus 2" in r.stderr and "GPU" in r.stderr


def test_world_size_mismatch_is_an_error():
    r = _run(["--gpus", "2", "--rehearse"], env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and r.stdout.strip() == ""
    assert "WORLD_SIZE" in r.stderr


def test_self_launch_two_ranks_rehearsal_over_gloo():
    r = _run(["--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "2", "--rehearse"], env={"DC_DIST_BACKEND": "gloo"})
    assert r.returncode == 0, r.stderr[-800:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1                              # ONE line, from rank 0
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1 and d["rehearsal"] is True
    assert d["config"]["global_batch"] == 4 and d["config"]["parallelism"] == "dp2"
    assert d["grad_bytes_allreduced_per_step"] > 0 and d["value"] > 0


def test_dump_outputs_repeat_run_for_run(tmp_path):
    """`--dump-outputs DIR`: the last timed step's arrays as float32 .npy files, identical for two runs with the same arguments
    (here on the CPU stand-in step; tests/test_bench_gpu.py runs it on the product path)."""
    import numpy as np
    for d in ("a", "b"):
        r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2", "--rehearse", "--dump-outputs", str(tmp_path / d)])
        assert r.returncode == 0, r.stderr[-800:]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert "losses.loss.npy" in names and "parameters.npy" in names
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.array_equal(a, b), n
    loss = float(np.load(tmp_path / "a" / "losses.loss.npy"))
    assert abs(loss - json.loads(r.stdout.strip().splitlines()[-1])["loss_last"]) <= 1e-6 * abs(loss) + 1e-6


def test_dump_outputs_fit_64_mb(tmp_path):
    """Arrays that do not fit together are cut to a fixed, seeded sample (indices ascending); small ones stay whole."""
    import numpy as np
    import torch
    import bench
    arrays = {"outputs.big": torch.arange(20_000_000, dtype=torch.float32), "outputs.small": torch.ones(3, 4, dtype=torch.float64),
              "parameters": torch.arange(10_000_000, dtype=torch.float32).neg()}
    bench.write_outputs(str(tmp_path / "a"), arrays)
    bench.write_outputs(str(tmp_path / "b"), arrays)
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64 << 20
    small = np.load(tmp_path / "a" / "outputs.small.npy")
    assert small.shape == (3, 4) and small.dtype == np.float32 and (small == 1).all()
    big, par = np.load(tmp_path / "a" / "outputs.big.npy"), np.load(tmp_path / "a" / "parameters.npy")
    assert big.dtype == np.float32 and 5_000_000 < big.size < 20_000_000 and (np.diff(big) >= 0).all()
    assert 5_000_000 < par.size < 10_000_000 and (np.diff(par) <= 0).all()
    for n in ("outputs.big.npy", "parameters.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n))
