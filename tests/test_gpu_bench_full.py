"""bench.py's plain line against --full (-m gpu).  A plain run sets up, warms up, times the steps and prints the line; what the headline
figure does not need -- the twopaco CLI end to end, the CPU baseline, the vertex-hash ranges beside the address-sharded filter -- runs
with --full only."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--workload", "m1", "--scale", "0.1"]
EXTRAS = {"e2e", "e2e_back_to_back", "e2e_wall_s", "e2e_junction_occurrences_per_sec", "cpu_baseline", "ranges"}


def _line(args, env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + args, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_line_leaves_the_extras_to_full():
    env = {k: v for k, v in os.environ.items() if k != "TPC_FORCE_DIST"}
    plain = _line([], env)
    assert not EXTRAS & set(plain)
    assert plain["metric"] == "kmers_hashed_per_sec" and plain["unit"] == "k-mers/s" and plain["value"] > 0 and plain["ms_per_step"] > 0
    full = _line(["--full", "--e2e-runs", "1", "--e2e-b2b-runs", "1", "--e2e-settle", "0"], env)
    assert full["result"] == plain["result"] and plain["result"]["junction_occurrences"] > 0
    assert full["e2e"]["runs"] == 1 and full["e2e"]["junction_occurrences"] == plain["result"]["junction_occurrences"]
    assert full["e2e_back_to_back"]["runs"] == 1 and full["e2e_wall_s"] > 0
    assert full["cpu_baseline"]["value"] > 0


def test_plain_distributed_line_times_its_own_decomposition_only():
    env = dict(os.environ, TPC_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29547", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1")
    env.pop("TPC_DIST_BACKEND", None)
    line = _line([], env)
    assert line["headline_decomposition"] == "address" == line["config"]["decomposition"]
    assert not EXTRAS & set(line) and line["result"]["junctions"] > 0
