"""bench.py --dump-outputs: what the timed path computed in its last step, as float64 .npy files of at most 64 MB, the same from
run to run.  CPU: the sampling and the size cap on a stand-in context.  GPU (-m gpu): the flag end to end, twice."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("counters", "junction_positions", "junction_ids", "junction_keys")


class FakeCtx:
    """The two read-backs dump_outputs uses, with lists longer than the cap allows (emit lists in no particular order)."""

    def __init__(self, n_marked, n_keys, key_words, seed):
        rng = np.random.default_rng(seed)
        self.g = rng.permutation(np.arange(n_marked, dtype=np.uint64) * np.uint64(3))
        self.ids = rng.integers(-(1 << 40), 1 << 40, size=n_marked, dtype=np.int64)
        self.ids[::7] = (1 << 63) - 1
        self.keys = np.sort(rng.integers(0, 1 << 63, size=(n_keys, key_words), dtype=np.uint64), axis=0)
        self.n_marked = n_marked

    def emit_fetch(self):
        return self.g.copy(), self.ids.copy()

    def junction_keys(self):
        return self.keys.copy()


def _dump(ctx, d):
    bench.dump_outputs(ctx, str(d), 11, {"true": 5, "false": 6, "table": 7}, ctx.keys.shape[0], 13)
    return {n: np.load(os.path.join(str(d), n + ".npy")) for n in NAMES}


def test_dump_outputs_cap_sample_and_repeatability(tmp_path):
    ctx = FakeCtx(3_000_000, 1_500_000, 2, seed=1)
    a = _dump(ctx, tmp_path / "a")
    b = _dump(ctx, tmp_path / "b")
    total = sum(os.path.getsize(str(tmp_path / "a" / (n + ".npy"))) for n in NAMES)
    assert total <= 64 << 20
    for n in NAMES:
        assert a[n].dtype == np.float64
        assert (a[n] == b[n]).all(), n
    assert a["counters"].tolist() == [11, 1_500_000, 13, 5, 6, 7, 3_000_000]
    # a sample of the position-ordered list: rows kept whole, in order
    pos = a["junction_positions"]
    assert 0 < pos.size < ctx.n_marked and (np.diff(pos) > 0).all()
    want = dict(zip(ctx.g.tolist(), ctx.ids.tolist()))
    assert all(float(want[int(p)]) == i for p, i in zip(pos[:1000].tolist(), a["junction_ids"][:1000].tolist()))
    # keys: two exact 32-bit halves per word
    k = a["junction_keys"]
    assert k.shape[1] == 4 and 0 < k.shape[0] < ctx.keys.shape[0]
    w = k.astype(np.uint64)
    words = w[:, 0::2] | (w[:, 1::2] << np.uint64(32))
    assert np.isin(words[:, 0], ctx.keys[:, 0]).all()


def test_dump_outputs_small_lists_whole(tmp_path):
    ctx = FakeCtx(1000, 0, 1, seed=2)
    a = _dump(ctx, tmp_path)
    assert (a["junction_positions"] == np.sort(ctx.g).astype(np.float64)).all()
    assert a["junction_keys"].shape == (0, 2)


@pytest.mark.gpu
def test_bench_dump_outputs_end_to_end(tmp_path):
    """Two runs of bench.py with the same arguments dump the same arrays, and the counters are the JSON line's result."""
    lines, dumps = [], []
    for run in ("a", "b"):
        d = str(tmp_path / run)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--workload", "m1",
                            "--scale", "0.1", "--e2e-runs", "0", "--cpu-baseline", "none", "--dump-outputs", d],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
        dumps.append({n: np.load(os.path.join(d, n + ".npy")) for n in NAMES})
        assert sum(os.path.getsize(os.path.join(d, n + ".npy")) for n in NAMES) <= 64 << 20
    line, a = lines[0], dumps[0]
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    res = line["result"]
    assert a["counters"][:6].tolist() == [res["candidate_marks"], res["junctions"], res["junction_occurrences"], res["true"], res["false"], res["table"]]
    assert a["junction_keys"].shape[0] == res["junctions"] > 0
    assert a["junction_positions"].size == a["junction_ids"].size == a["counters"][6] > 0
    for n in NAMES:
        assert (dumps[0][n] == dumps[1][n]).all(), n
