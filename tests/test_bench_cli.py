"""bench.py: argument handling that needs no GPU; on the GPU, the plain result line, --dump-outputs and --full."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=300)


def test_conflicting_multi_gpu_modes_are_refused():
    r = _run("--gpus", "2", "--batch", "--shard")
    assert r.returncode != 0 and "--batch runs one graph per rank" in (r.stdout + r.stderr)
    r = _run("--gpus", "2", "--replicas", "--shard")
    assert r.returncode != 0 and "--replicas runs the unsharded path" in (r.stdout + r.stderr)


def test_world_size_mismatch_is_reported():
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--no-build"], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode != 0 and "WORLD_SIZE=3" in (r.stdout + r.stderr)


def test_no_gpu_is_an_error_not_a_fallback(built):
    """Without a GPU the bench refuses to run (no CPU path behind the same metric)."""
    import torch
    if torch.cuda.is_available():
        return
    r = _run("--gpus", "1", "--no-build", "--no-cpu-baseline", "--config", "tiny")
    assert r.returncode != 0 and "needs a GPU" in (r.stdout + r.stderr)


def test_step_counts_are_checked():
    r = _run("--gpus", "1", "--steps", "0", "--no-build")
    assert r.returncode != 0 and "--steps must be >= 1" in (r.stdout + r.stderr)


def _line(r):
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    import json
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(built, tmp_path):
    """A plain run times exactly --steps steps and reports the headline only; --dump-outputs writes the last step's results
    (canonical endpoints + trussness as a caller fetches them, float arrays within 64 MB), equal to the oracle's."""
    import numpy as np
    import komb_amd
    from oracle import oracle as O
    d = _line(_run("--gpus", "1", "--config", "tiny", "--steps", "2", "--warmup", "1", "--no-build", "--dump-outputs", str(tmp_path)))
    assert d["steps"] == 2 and d["warmup"] == 1 and d["full"] is False
    assert d["metric"] == "peeled edges/sec (k-truss)" and d["unit"] == "edges/s" and d["higher_is_better"] is True and d["dtype"] == "int32"
    assert d["ms_per_step"] > 0 and abs(d["value"] - d["config"]["ne"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    for moved in ("value_resident", "kcore", "roofline", "cpu_baseline", "c2", "first_call", "corea", "runtruss_faithful"):
        assert moved not in d
    files = {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}
    assert set(files) == {"edge_index", "edge_u", "edge_v", "trussness", "truss_histogram"}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(p.stat().st_size for p in tmp_path.glob("*.npy")) <= 64 << 20
    nv, ncl, alpha, seed = 100_000, 245_000, 2.6, 42                     # bench.py CONFIGS["tiny"]
    rowptr, col = O.simplify(nv, komb_amd.gen_hug_edges(nv, ncl, alpha, seed))
    eu, ev = O.edge_list(rowptr, col)
    tr = O.trussness_native(rowptr, col, min(16, len(os.sched_getaffinity(0)))) if O.native_lib() else O.trussness(rowptr, col)
    assert len(eu) == d["config"]["ne"]
    idx = files["edge_index"].astype(np.int64)
    assert len(eu) <= 1 << 20 and np.array_equal(idx, np.arange(len(eu)))    # tiny: below the sample size, every edge is written
    assert np.array_equal(files["edge_u"], eu[idx]) and np.array_equal(files["edge_v"], ev[idx])
    assert np.array_equal(files["trussness"], tr[idx].astype(np.float32))
    assert np.array_equal(files["truss_histogram"], np.bincount(tr).astype(np.float64))


@pytest.mark.gpu
def test_full_run_reports_the_rest(built):
    """--full keeps everything else the benchmark measures beside the headline (here without the CPU baseline)."""
    d = _line(_run("--gpus", "1", "--config", "tiny", "--steps", "2", "--warmup", "1", "--no-build", "--no-cpu-baseline", "--full"))
    assert d["steps"] == 2 and d["full"] is True and d["ms_per_step"] > 0
    assert d["value_resident"] > 0 and d["kcore"]["ms"] > 0 and d["roofline"]["kernel"] and d["c2"]["kcore"]["ms"] > 0
    assert d["first_call"]["ktruss_first_ms"] > 0 and d["corea"]["vertices"] == 100_000 and d["runtruss_faithful"]["ms"] > 0
    assert d["config"]["max_coreness"] > 0 and d["config"]["max_degree"] > 0 and "cpu_baseline" not in d
