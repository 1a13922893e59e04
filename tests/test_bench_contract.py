"""bench.py driver-contract tests (CPU): JSON line shape + torchrun ws=2."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup",
                 "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                 "dtype", "data", "config"}


def _last_json_line(out):
    for line in reversed(out.strip().splitlines()):
        line = line.strip()
        if line.startswith("{"):
            return json.loads(line)
    raise AssertionError(f"no JSON line in output:\n{out}")


def test_bench_single_process_cpu():
    r = subprocess.run(
        [sys.executable, "bench.py", "--device", "cpu", "--steps", "2",
         "--warmup", "1", "--layers", "1,1,1,1"],
        cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    j = _last_json_line(r.stdout)
    assert REQUIRED_KEYS.issubset(j.keys())
    assert j["n_gpus"] == 1 and j["steps"] == 2 and j["value"] > 0
    assert j["data"] == "synthetic" and j["scaling"] == "weak"
    assert j["config"]["parallelism"] == "dp1"


def _run_dump(out, steps, warmup, *extra):
    import numpy as np

    r = subprocess.run(
        [sys.executable, "bench.py", "--device", "cpu", "--steps", str(steps),
         "--warmup", str(warmup), "--layers", "1,1,1,1",
         "--dump-outputs", str(out), *extra],
        cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return _last_json_line(r.stdout), {p.name: np.load(p) for p in out.iterdir()}


def test_bench_dump_outputs_cpu(tmp_path):
    """--dump-outputs writes one step's results as float .npy files; that
    step starts from the seeded initial state (parameters, running
    statistics, optimizer state), so the files do not depend on how many
    steps ran before it; --steps sets the timed step count that ms_per_step
    and value are derived from; --full is accepted."""
    import numpy as np

    j, files = _run_dump(tmp_path / "a", 3, 0, "--full")
    assert j["steps"] == 3 and j["warmup"] == 0
    images = j["config"]["global_batch"] * j["steps"]
    assert abs(j["value"] * j["ms_per_step"] * j["steps"] / 1000.0 - images) \
        < 1e-6 * images

    assert set(files) == {"losses.npy", "params.npy", "buffers.npy"}
    for name, arr in files.items():
        assert arr.dtype in (np.float32, np.float64), name
        assert np.isfinite(arr).all(), name
        assert arr.ndim == 1 and arr.size > 0, name
    assert sum(a.nbytes for a in files.values()) <= 64 * 2 ** 20
    assert files["losses.npy"].shape == (2,)

    # fp32 on CPU: one step from identical state differs by reassociation
    # in threaded reductions at most (observed: bit-identical)
    _, again = _run_dump(tmp_path / "b", 1, 1)
    for name, arr in files.items():
        np.testing.assert_allclose(again[name], arr, rtol=1e-5, atol=1e-6,
                                   err_msg=name)


def test_bench_seeds_miopen_find_db(tmp_path, monkeypatch):
    """The committed find results land in the user find-db directory and
    never replace a find-db that is already there."""
    import glob

    sys.path.insert(0, REPO)
    try:
        import bench
    finally:
        sys.path.remove(REPO)
    shipped = glob.glob(os.path.join(bench.FIND_DB_DIR, "*.ufdb.txt"))
    assert shipped, "no committed find-db under benchmarks/miopen_find_db"
    monkeypatch.setenv("MIOPEN_USER_DB_PATH", str(tmp_path / "userdb"))
    bench.seed_miopen_find_db()
    for src in shipped:
        dst = tmp_path / "userdb" / os.path.basename(src)
        assert dst.read_bytes() == open(src, "rb").read()
    assert not glob.glob(str(tmp_path / "userdb" / "*.tmp"))
    mine = tmp_path / "userdb" / os.path.basename(shipped[0])
    mine.write_text("kept")
    bench.seed_miopen_find_db()
    assert mine.read_text() == "kept"


def test_bench_torchrun_ws8_cpu():
    """The 8-GPU scaling-run shape (dp8) end to end on CPU/gloo: 8 ranks,
    bucketed DP, max-over-ranks timing, one JSON line from rank 0."""
    env = dict(os.environ)
    env["MASTER_ADDR"] = "127.0.0.1"
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
         "--master-port", "29713", "bench.py", "--gpus", "8", "--steps", "1",
         "--warmup", "0", "--device", "cpu", "--layers", "1,1,1,1"],
        cwd=REPO, capture_output=True, text=True, timeout=1200, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    j = _last_json_line(r.stdout)
    assert j["n_gpus"] == 8
    assert j["config"]["parallelism"] == "dp8"


def test_bench_torchrun_ws2_cpu():
    """The driver launches bench via torch.distributed.run for N>1; verify the
    whole path works (gloo on CPU, 127.0.0.1 rendezvous)."""
    env = dict(os.environ)
    env["MASTER_ADDR"] = "127.0.0.1"
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29711", "bench.py", "--gpus", "2", "--steps", "2",
         "--warmup", "1", "--device", "cpu", "--layers", "1,1,1,1"],
        cwd=REPO, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    j = _last_json_line(r.stdout)
    assert j["n_gpus"] == 2
    assert j["config"]["parallelism"] == "dp2"
    assert j["config"]["global_batch"] == 2 * j["config"]["per_domain_batch"] * 3
