"""bench.py's plain run (no --full): the headline alone -- no side measurement, no CPU baseline, no HBM probe -- over exactly
--steps timed steps, and --dump-outputs: the last timed step's results as float64 .npy files, the same on every run with the
same inputs (here: two runs with different step counts)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, ITERS = 256, 300


def _plain(tmp_path, dump, steps):
    """-> (the final stdout line, the full record) of a plain run"""
    sides = tmp_path / ("bench_sides_%s.json" % os.path.basename(dump))
    env = dict(os.environ, AUVP_BENCH_SIDES=str(sides))
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--episodes", str(E), "--iters", str(ITERS), "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    line = json.loads(r.stdout.rstrip().splitlines()[-1])
    return line, json.load(open(sides))


def test_plain_run_times_the_headline_only_and_dumps_the_same_outputs_every_run(tmp_path):
    a, full = _plain(tmp_path, tmp_path / "a", 3)
    assert a["metric"] == "RRT-Dubins node expansions/s (RRT.exploring)" and a["unit"] == "expansions/s"
    assert a["higher_is_better"] is True and a["dtype"] == "f64" and a["value"] > 0
    assert a["steps"] == 3 and a["warmup"] == 1 and a["ms_per_step"] > 0
    assert abs(a["value"] - E * ITERS / (a["ms_per_step"] * 1e-3)) <= 1e-5 * a["value"]
    assert a["cpu_baseline"] is None and a["roofline"]["kernel_ms"] > 0
    assert full["expansions_per_step"] == E * ITERS
    for k in ("single_episode", "rrt_64_obstacles", "rrt_1024_replicas", "rrt_dense", "rrt_nn", "rrt_nn_long_horizon", "astar",
              "planner_rrt", "rrt_env", "config5", "shark_grid", "particle_filter", "hbm_probe", "cpu_baseline_all_cores"):
        assert k not in full, k
    assert full["cpu_baseline"] is None
    b, _ = _plain(tmp_path, tmp_path / "b", 1)
    assert b["steps"] == 1
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"summary_n_nodes.npy", "summary_best_cost.npy", "best_paths.npy", "best_path_offsets.npy", "best_path_episodes.npy"} <= set(names)
    total = 0
    for n in names:
        x = np.load(tmp_path / "a" / n)
        assert x.dtype == np.float64 and np.array_equal(x, np.load(tmp_path / "b" / n)), n
        total += os.path.getsize(tmp_path / "a" / n)
    assert total <= 64 << 20
    assert (np.load(tmp_path / "a" / "summary_status.npy") >= 0).all()
    assert (np.load(tmp_path / "a" / "summary_iters_run.npy") == ITERS).all()
    assert len(np.load(tmp_path / "a" / "summary_n_nodes.npy")) == E and np.load(tmp_path / "a" / "best_paths.npy").shape[1] == 7
