"""bench.py's N > 1 path rehearsed on one GPU: two ranks (gloo process group,
both on device 0 through LOCAL_RANK=0), the default chains mode (one chain
per rank, chain id = rank, no collective in the sweep) and --shard (one
chain split over the ranks).  The driver's 8-GPU run launches the same code
with RCCL and one device per rank; the timing here is
meaningless, the checks are on the line rank 0 prints."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _ranks(world, extra):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE=str(world),
               LOCAL_RANK="0", MVC_BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--config", "c2", "--steps",
           "3", "--warmup", "1", "--full", "--no-extras", "--no-cpu-baseline"] + extra
    procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True) for r in range(world - 1, -1, -1)]
    outs = []
    for p in procs:
        try:
            o, e = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        assert p.returncode == 0, e[-2000:]
        outs.append(o)
    lines = [ln for ln in outs[-1].strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, outs[-1][-2000:]
    for o in outs[:-1]:
        assert not [ln for ln in o.strip().splitlines() if ln.startswith("{")], "only rank 0 prints"
    return json.loads(lines[0])


def _two_ranks(extra):
    return _ranks(2, extra)


def test_bench_two_ranks_chains_mode():
    r = _two_ranks([])
    assert r["n_gpus"] == 2 and r["scaling"] == "weak"
    assert r["config"]["chains"] == 2 and r["config"]["parallelism"] == "chains2"
    # value = the sweeps of all ranks / the max-over-ranks time
    assert abs(r["value"] - 2 * r["steps"] / (r["ms_per_step"] * r["steps"] / 1e3)) <= 0.01 * r["value"]
    # the reported cross-chain reduce pooled both ranks' chains
    assert r["hyper_pooled"]["chains"] == 2
    assert r["roofline"]["bound"] in ("hbm", "mfma")


def test_bench_four_ranks_chains_mode():
    """Four ranks (the driver's 8-GPU launch has the same shape): one chain
    per rank, the line's value is all ranks' sweeps over the max-over-ranks
    time, and the pooled reduce holds four chains."""
    r = _ranks(4, [])
    assert r["n_gpus"] == 4 and r["scaling"] == "weak"
    assert r["config"]["chains"] == 4 and r["config"]["parallelism"] == "chains4"
    assert abs(r["value"] - 4 * r["steps"] / (r["ms_per_step"] * r["steps"] / 1e3)) <= 0.01 * r["value"]
    assert r["hyper_pooled"]["chains"] == 4


def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run prints the headline without the legs that need runs of
    their own (those take --full), and --dump-outputs writes the state after
    the last timed step as float64 .npy, the same from run to run."""
    import numpy as np
    dumps = []
    for tag in "ab":
        d = tmp_path / tag
        r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c2",
                            "--steps", "2", "--warmup", "1", "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["unit"] == "sweeps/s"
        assert abs(line["value"] - 1e3 / line["ms_per_step"]) <= 0.01 * line["value"]
        for moved in ("cpu_baseline", "extra", "hyper_pooled", "kernel_ms_per_sweep", "repair_last_sweep"):
            assert moved not in line
        dumps.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
    a, b = dumps
    assert sorted(a) == ["dish_counts.npy", "dish_of.npy", "hyper.npy", "table_of.npy"]
    assert a["table_of.npy"].shape == (100_000,) and a["dish_of.npy"].shape[0] == 2 and a["hyper.npy"].shape == (8,)
    for f in a:
        assert a[f].dtype == np.float64 and np.isfinite(a[f]).all()
        assert np.array_equal(a[f], b[f]), f
    assert sum(x.nbytes for x in a.values()) <= 64 << 20


def test_bench_two_ranks_shard_mode():
    r = _two_ranks(["--shard"])
    assert r["n_gpus"] == 2 and r["scaling"] == "strong"
    assert r["config"]["chains"] == 1 and r["config"]["parallelism"] == "shard2"
    assert r["hyper_pooled"]["chains"] == 1
