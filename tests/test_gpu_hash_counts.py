"""GPU (-m gpu): every hash-function count through each first-pass kernel, against the oracle on the same text and seed.

The first pass is compiled once per count: the rolling kernels for q = 1..16 (k_part_hash2 / k_part_hash, k_q_hash2 / k_q_hash,
k_q_verify2 / k_q_verify, the direct k_insert / k_query), the closed form for q = 17..64 (csrc/tpc_pass1_anyq.hip).  Which one runs
depends on q, k and the filter geometry; the stats "insert_hash_kernel", "query_hash_kernel" and "query_verify_kernel"
(include/twopaco_hip.h) say which did, so a test cannot pass on a fallback.  Bit for bit: filter bitmap, candidate mask, mark count and,
where the second pass runs, its counters."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTERS = np.frombuffer(b"ACGTN", dtype=np.uint8)
SEED = 4711


@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


def insert_seed_table_fits(q, k):
    """tpc_partition.hip:launch_hash_q: the lean insert keeps its k x 5 x q seed table (16 bytes per entry) in LDS when it fits beside the
    bins (Bins3 control words + 128 KiB of rings: 135296 bytes), the staged text ((512 + 1 + 22) x 24), q x 160 and 128 bytes, all within
    160 KiB - 256: 80 q (k + 2) <= 15320, i.e. k <= 191.5 / q - 2."""
    return 80 * q * (k + 2) <= 15320


def text_records(k, n=64000, seed=0):
    """Codes (A0 C1 G2 T3 N4) of a 50-200 kbp text with junctions: two mutated copies of a random sequence (N runs in one, a poly-A head on
    the other, a (CA)n tract across the first tile boundary of the packed text), an unrelated record, one shorter than k, one of k + 1."""
    assert n // 2 >= 16384 + 700, n  # (room for the tract across the first tile boundary)
    rng = np.random.default_rng(1000 + 7 * k + seed)
    base = rng.integers(0, 4, n // 2).astype(np.uint8)
    recs = []
    for r in range(2):
        s = base.copy()
        hits = rng.random(s.size) < 0.02
        s[hits] = rng.integers(0, 4, int(hits.sum())).astype(np.uint8)
        recs.append(s)
    for _ in range(4):
        a = int(rng.integers(0, recs[0].size - 100))
        recs[0][a:a + int(rng.integers(1, 60))] = 4
    at = 16384 - 1 - 300  # (record 0 starts at text position 1: the tract straddles the first 16384-position tile)
    recs[0][at:at + 700] = np.resize(np.array([1, 0], dtype=np.uint8), 700)
    recs[1][:1500] = 0   # skew: a poly-A head
    recs.append(rng.integers(0, 4, 8000).astype(np.uint8))
    recs.append(rng.integers(0, 4, max(1, k - 1)).astype(np.uint8))
    recs.append(rng.integers(0, 4, k + 1).astype(np.uint8))
    return recs


def make_oracle(k, L, q, recs, seed=SEED):
    o = O.Oracle(k, L, q, O.seed_table(seed, q, L))
    for r in recs:
        o.add_record(LETTERS[r].tobytes())
    return o


def kernel_stats(ctx):
    return {n: ctx.stat(n) for n in ("insert_path", "query_path", "insert_batches", "query_batches", "insert_hash_kernel", "query_hash_kernel",
                                     "query_verify_kernel")}


def three_passes(ctx, o, ranges, tag, pass2=True):
    """Insert and query over each (lo, hi) against the oracle; after the whole range (first) also the second pass' counters.
    Returns the stats of every range."""
    out = []
    if pass2:
        o.enumerate(rounds=1)
        want2 = o.round_stats(0)
    for i, (lo, hi) in enumerate(ranges):
        o.fill_only(lo, hi)
        marks = o.check_only(lo, hi)
        ctx.filter_reset()
        ctx.pass1_insert(lo, hi)
        got = ctx.pass1_query(lo, hi)
        st = kernel_stats(ctx)
        t = tag + (lo, hi, st)
        assert (ctx.filter_download() == o.filter).all(), ("filter bitmap",) + t
        assert got == marks, ("marks", got, marks) + t
        assert (ctx.mask_download(False) == o.round_mask).all(), ("candidate mask",) + t
        if pass2 and i == 0:
            assert ctx.pass2_filter() == {"true": want2["true"], "false": want2["false"], "table": want2["table"]}, ("pass2",) + t
        out.append(st)
    return out


def rolling_ks(q):
    """Both sides of the insert seed-table bound, of the 31-letter limit of k_q_verify2, of 64 letters (k_q_hash2's seed table, two key
    words), and a k beyond 100 for q <= 4."""
    kb = 15320 // (80 * q) - 2
    assert insert_seed_table_fits(q, kb) and not insert_seed_table_fits(q, kb + 1)
    return sorted({kb, kb + 1, 31, 32, 64, 65} | ({127} if q <= 4 else set()))


@pytest.mark.parametrize("q", range(1, 17))
def test_rolling_counts_partitioned(capi, q):
    """The partitioned passes at every rolling count: the lean insert with and without its seed table (odd q > 8: a padded lane in the
    second emit batch), k_q_verify2 and k_q_verify, two and three levels, in one and in many tile batches, whole and gated ranges."""
    seen = {"insert_hash_kernel": set(), "query_hash_kernel": set(), "query_verify_kernel": set()}
    batched = False
    ctx = capi.Context(0)
    try:
        for i, k in enumerate(rolling_ks(q)):
            L, slice_bits, levels = 20 + (q + i) % 3, 8 + i % 3, 2 + (q + i) % 2
            small = i % 2 == 0
            for opt, val in (("insert_mode", 2), ("query_mode", 2), ("slice_bits", slice_bits), ("part_levels", levels), ("part_min_tiles", 1),
                             ("part_budget_bytes", 64 << 10 if small else 0)):
                ctx.set_option(opt, val)
            recs = text_records(k)
            ctx.set_params(k, L, q, capi.seed_table(q, L, seed=SEED))
            ctx.seq_upload(capi.PackedText.from_codes(recs))
            o = make_oracle(k, L, q, recs)
            size = 1 << L
            tag = (q, k, L, slice_bits, levels, small)
            for st in three_passes(ctx, o, [(0, size), (size * 3 // 16, size * 11 // 16)], tag):
                assert st["insert_path"] in (2, 3) and st["query_path"] in (2, 3), tag + (st,)
                assert st["insert_hash_kernel"] == (1 if insert_seed_table_fits(q, k) else 2), tag + (st,)
                assert st["query_hash_kernel"] in (1, 2), tag + (st,)
                assert st["query_verify_kernel"] == (1 if k <= 31 else 3), tag + (st,)
                batched = batched or (small and st["insert_batches"] > 1 and st["query_batches"] > 1)
                for n in seen:
                    seen[n].add(st[n])
            o.close()
    finally:
        ctx.close()
    print("kernels q=%d: insert_hash %s query_hash %s query_verify %s" % (q, sorted(seen["insert_hash_kernel"]), sorted(seen["query_hash_kernel"]),
                                                                        sorted(seen["query_verify_kernel"])))
    assert seen["insert_hash_kernel"] == {1, 2}, (q, seen)
    assert seen["query_verify_kernel"] == {1, 3}, (q, seen)
    assert batched, q


@pytest.mark.parametrize("q,slice_bits", [(8, 7), (9, 6), (13, 7), (16, 6)])
def test_slice_index_beyond_24_bits(capi, q, slice_bits):
    """L - slice_bits > 24: the lean kernels take a 24-bit slice index only.  The insert of q <= 8 then runs k_part_hash, that of q > 8
    (lean only) the direct kernel; the query of every q stays partitioned on k_q_hash.  Either way the oracle's results."""
    k, L = 25, 32
    recs = text_records(k, n=40000)
    ctx = capi.Context(0)
    try:
        for opt, val in (("insert_mode", 2), ("query_mode", 2), ("slice_bits", slice_bits), ("part_levels", 3)):
            ctx.set_option(opt, val)
        ctx.set_params(k, L, q, capi.seed_table(q, L, seed=SEED))
        ctx.seq_upload(capi.PackedText.from_codes(recs))
        o = make_oracle(k, L, q, recs)
        tag = (q, k, L, slice_bits, 3)
        for st in three_passes(ctx, o, [(0, 1 << L), (1 << 29, 3 << 30)], tag):
            if q <= 8:
                assert st["insert_path"] == 3 and st["insert_hash_kernel"] == 3, tag + (st,)
            else:
                assert st["insert_path"] == 1 and st["insert_hash_kernel"] == 0, tag + (st,)
            assert st["query_path"] in (2, 3) and st["query_hash_kernel"] == 2 and st["query_verify_kernel"] == 1, tag + (st,)
        o.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("q", [17, 31, 32, 33, 48, 63, 64])
def test_closed_form_counts(capi, q):
    """q = 17..64 runs the closed-form direct kernels (one 64-bit word of addresses and beyond: 32, 33, 64): filter, marks, mask and
    second-pass counters at k from 5 to 127, whole and gated ranges."""
    ctx = capi.Context(0)
    try:
        for i, k in enumerate([5, 31, 32, 64, 65, 127]):
            L = 18 + (q + i) % 4
            recs = text_records(k, n=40000, seed=q)
            ctx.set_params(k, L, q, capi.seed_table(q, L, seed=SEED))
            ctx.seq_upload(capi.PackedText.from_codes(recs))
            o = make_oracle(k, L, q, recs)
            size = 1 << L
            tag = (q, k, L)
            for st in three_passes(ctx, o, [(0, size), (size // 3, size - size // 5)], tag):
                assert st["insert_path"] == 1 and st["query_path"] == 1, tag + (st,)
                assert st["insert_hash_kernel"] == 4 and st["query_hash_kernel"] == 4 and st["query_verify_kernel"] == 0, tag + (st,)
            o.close()
    finally:
        ctx.close()


def test_closed_form_split_histogram_q64(capi):
    """k_split_anyq at q = 64 == the oracle's histogram bin for bin on a scratch filter no edge collides in (2^30 bits, k + 1 < L)."""
    k, L, q = 25, 30, 64
    recs = text_records(k, n=40000)
    o = make_oracle(k, L, q, recs)
    bins = o.split_bins()
    o.close()
    text = capi.PackedText.from_codes(recs)
    ctx = capi.Context(0)
    try:
        ctx.set_params(k, L, q, capi.seed_table(q, L, seed=SEED))
        ctx.seq_upload(text)
        keep = text.rec_length >= k
        got = ctx.pass1_split_hist(text.rec_start[keep], text.rec_length[keep])
    finally:
        ctx.close()
    assert int(bins.sum()) > 0 and (got == bins).all(), np.nonzero(got != bins)[0][:10]


def test_hash_count_refused_beyond_64(capi):
    """set_params refuses q = 65 and q = 0 with its message; the context then takes a valid count and computes the oracle's results."""
    k, L = 25, 20
    ctx = capi.Context(0)
    try:
        for bad in (65, 0):
            with pytest.raises(RuntimeError, match="q=%d unsupported" % bad):
                ctx.set_params(k, L, bad, np.zeros((bad, 5), dtype=np.uint64))
        recs = text_records(k, n=40000)
        ctx.set_params(k, L, 9, capi.seed_table(9, L, seed=SEED))
        ctx.seq_upload(capi.PackedText.from_codes(recs))
        o = make_oracle(k, L, 9, recs)
        three_passes(ctx, o, [(0, 1 << L)], (9, k, L))
        o.close()
    finally:
        ctx.close()


def knob_sweep():
    """The reduced sweep the measurement knobs run under (a fresh process each: TpcEnv reads them once): partitioned passes == the oracle;
    returns the stats of every configuration."""
    from twopaco_amd import capi
    rows = []
    for q in (1, 2, 3, 8, 9, 16):
        for k in (9, 31):
            L, size = 21, 1 << 21
            recs = text_records(k, n=40000)
            ctx = capi.Context(0)
            for opt, val in (("insert_mode", 2), ("query_mode", 2), ("slice_bits", 9)):
                ctx.set_option(opt, val)
            ctx.set_params(k, L, q, capi.seed_table(q, L, seed=SEED))
            ctx.seq_upload(capi.PackedText.from_codes(recs))
            o = make_oracle(k, L, q, recs)
            for st in three_passes(ctx, o, [(0, size), (size // 4, size // 2)], (q, k, L, os.environ.get("TPC_NO_LEAN"), os.environ.get("TPC_VERIFY_LAZY"))):
                rows.append(dict(st, q=q, k=k))
            o.close()
            ctx.close()
    return rows


def _knob_run(env_extra):
    env = dict(os.environ)
    env.update(env_extra)
    code = "import json, sys; sys.path[:0] = [%r, %r]; import test_gpu_hash_counts as t; print(json.dumps(t.knob_sweep()))" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (env_extra, r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_verify_eager_knob():
    """TPC_VERIFY_LAZY=0: every verification is k_q_verify2 eager (k <= 31) and still gives the oracle's results."""
    rows = _knob_run({"TPC_VERIFY_LAZY": "0"})
    assert len(rows) == 24
    for r in rows:
        assert r["insert_path"] in (2, 3) and r["query_path"] in (2, 3), r
        assert r["query_verify_kernel"] == 2, r
        assert r["insert_hash_kernel"] in (1, 2) and r["query_hash_kernel"] == 1, r


def test_no_lean_knob():
    """TPC_NO_LEAN=1: k_q_hash and k_q_verify for every q, k_part_hash for q <= 8 and the direct insert for q > 8 (the partitioned insert
    hashes on the lean kernel only); the oracle's results."""
    rows = _knob_run({"TPC_NO_LEAN": "1"})
    assert len(rows) == 24
    for r in rows:
        if r["q"] <= 8:
            assert r["insert_path"] in (2, 3) and r["insert_hash_kernel"] == 3, r
        else:
            assert r["insert_path"] == 1 and r["insert_hash_kernel"] == 0, r
        assert r["query_path"] in (2, 3) and (r["query_hash_kernel"], r["query_verify_kernel"]) == (2, 3), r


@pytest.mark.parametrize("q,k", [(9, 33), (16, 47), (17, 33), (64, 47)])
def test_enumerator_hash_counts_end_to_end(capi, tmp_path, q, k):
    """CreateEnumerator at q = 9, 16, 17, 64 with k > 31 in two rounds: de_bruijn.bin == the oracle's, byte for byte."""
    recs = text_records(k, n=50000)
    fa = str(tmp_path / "in.fa")
    with open(fa, "w") as f:
        for i, r in enumerate(recs):
            s = LETTERS[r].tobytes().decode()
            f.write(">r%d\n" % i)
            for j in range(0, len(s), 70):
                f.write(s[j:j + 70] + "\n")
    L = 22
    o = O.Oracle(k, L, q, O.seed_table(SEED, q, L))
    o.add_fasta(fa)
    o.enumerate(rounds=2)
    ref = str(tmp_path / "oracle.bin")
    o.write_bin(ref)
    out = str(tmp_path / "gpu.bin")
    e = capi.Enumerator([fa], k, L, q=q, rounds=2, tmpdir=str(tmp_path), out=out, seed=SEED)
    assert open(out, "rb").read() == open(ref, "rb").read(), (q, k, L)
    assert e.vertices_count() == len(o.keys) > 0, (q, k, L)
    e.close()
    o.close()

