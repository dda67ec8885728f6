"""GPU (-m gpu): the LDS instruction diet of the level-1 query hash (k_q_hash2), against the oracle.

Two switches, both process-wide options (include/twopaco_hip.h):
  qhash_pushes        6: the 3 + 3 unknown edges of a position compacted per lane (slot j takes candidate j, or j + 1 when the known
                      letter is at or below j) and pushed with every lane active; 8: the 4 + 4 candidates as predicated pushes
  qhash_roll_scalars  1: the roll selects the hashes of the leaving and the entering letter (A C G T N) from scalar registers; 0: it reads
                      them from a table in LDS
Every case inserts and queries a small text in the forms it names and compares marks, candidate mask and (L <= 32) filter bitmap with
the oracle, so the forms are compared with each other through it.  "query_hash_kernel" and "query_hash_form" say what ran: a case cannot
pass on the other kernel or the other form.

What the texts are for: a compaction that keeps the wrong candidate, or the right one under the wrong edge number, changes which Bloom
addresses are probed for a (cp, cn) pair, and a roll that selects the wrong letter's hash -- the N row included: windows roll across N
runs -- derails every position behind it in the thread's run of 16.  So every pair of the 5 x 5 letters occurs, beside N, at record
starts and ends, in periodic tracts (positions that send no probes), gated (positions that send none in this round), at k = 9 / 25 /
51 / 65, L <= 32 and L > 32 (values on one and on two registers), and at 512 bins, where in- and out-edges go in two rounds.

Ranges are [lo, hi] with both ends inclusive, as in the C-ABI: the whole hash space is (0, 2^L - 1).

A third change, one-word group descriptors in the bins' flush, was built and measured with these and dropped (profiles/r09_qhash_lds.md);
its switch and its tests (both descriptor forms, the over flag, padded last groups) left with it.  The environment knobs TPC_QHASH_* are
read once per process and are not tested here: the options are."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

LETTERS = np.frombuffer(b"ACGTN", dtype=np.uint8)
SEED = 977
TILE = 16384  # positions of a tile: one workgroup of the hash kernels
FORMS = ((6, 1), (8, 1), (6, 0), (8, 0))  # (qhash_pushes, qhash_roll_scalars)
DEFAULTS = (("qhash_pushes", 6), ("qhash_roll_scalars", 1))  # process-wide: every case puts them back


@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


def pairs_text(k, copies=2, seed=0):
    """Every (cp, cn) of the 5 x 5 letters around an N-free k-mer, `copies` times each with other neighbours in between (so that the
    planted k-mers are junctions: real second edges, not only Bloom false positives), in random text with 2 % N."""
    rng = np.random.default_rng(seed + 31 * k)
    kmers = [rng.integers(0, 4, k).astype(np.uint8) for _ in range(25)]
    parts = []
    for rep in range(copies):
        for i in range(25):
            cp, cn = (i + 7 * rep) % 5, ((i + 7 * rep) // 5 + 3 * rep) % 5
            filler = rng.integers(0, 4, 40 + int(rng.integers(0, 30))).astype(np.uint8)
            filler[rng.random(filler.size) < 0.02] = 4
            parts += [filler, np.array([cp], dtype=np.uint8), kmers[i], np.array([cn], dtype=np.uint8)]
    # the schedule above permutes the pairs per copy; make sure of all 25 in the first copy by planting them once more, plainly
    for cp in range(5):
        for cn in range(5):
            parts += [rng.integers(0, 4, 30).astype(np.uint8), np.array([cp], dtype=np.uint8), kmers[(5 * cp + cn + 11) % 25], np.array([cn], dtype=np.uint8)]
    return [np.concatenate(parts)]


def pairs_seen(recs, k):
    """The (cp, cn) pairs around N-free k-windows of the records (a record's ends count as N, as the separators do)."""
    seen = set()
    for r in recs:
        t = np.concatenate([[4], np.asarray(r, dtype=np.uint8), [4]])
        isn = (t == 4).astype(np.int64)
        run = np.concatenate([[0], np.cumsum(isn)])
        for p in range(1, len(t) - k):
            if run[p + k] - run[p] == 0:
                seen.add((int(t[p - 1]), int(t[p + k])))
    return seen


def boundary_text(k, seed=0):
    """Three tiles' worth: records that start and end at assorted places (one shorter than k, one of exactly k, one of k + 1), N runs of
    1, 2 and k letters, two mutated copies of one sequence (junctions on both sides of the N runs), and three periodic tracts (period 1,
    2 and 7, each several hundred letters: positions inside them copy their verdict and send no probes)."""
    rng = np.random.default_rng(1000 + seed + k)
    base = rng.integers(0, 4, 17000).astype(np.uint8)
    for at, n in ((500, 1), (777, 2), (1500, k), (9000, 1), (9002, 1), (16383 - k, 3)):
        base[at:at + n] = 4
    for at, unit, n in ((3000, [0], 500), (6000, [1, 2], 600), (12000, [0, 1, 3, 3, 2, 0, 1], 700)):
        base[at:at + n] = np.resize(np.array(unit, dtype=np.uint8), n)
    mut = base.copy()
    hits = rng.random(mut.size) < 0.02
    mut[hits] = rng.integers(0, 4, int(hits.sum())).astype(np.uint8)
    shorts = [rng.integers(0, 4, n).astype(np.uint8) for n in (max(1, k - 1), k, k + 1, k + 2, 3 * k)]
    return [shorts[0], base, shorts[1], shorts[2], mut, shorts[3], base[200:200 + 3 * k].copy(), shorts[4]]


def run_forms(capi, recs, k, L, q, options, ranges=None, forms=FORMS, want_b1=None, filters=True):
    """Insert and query every range in every form; marks, mask and filter against the oracle.  Returns the stats of every pass."""
    o = O.Oracle(k, L, q, O.seed_table(SEED, q, L))
    for r in recs:
        o.add_record(LETTERS[np.asarray(r, dtype=np.uint8)].tobytes())
    ranges = ranges or ((0, (1 << L) - 1),)
    ctx = capi.Context(0)
    out = []
    try:
        for opt, val in (("insert_mode", 2), ("query_mode", 2), ("part_min_tiles", 1), ("part_levels", 2)) + tuple(options):
            ctx.set_option(opt, val)
        ctx.set_params(k, L, q, capi.seed_table(q, L, seed=SEED))
        ctx.seq_upload(capi.PackedText.from_codes(recs))
        for lo, hi in ranges:
            o.fill_only(lo, hi)
            want = o.check_only(lo, hi)
            for pushes, roll in forms:
                ctx.set_option("qhash_pushes", pushes)
                ctx.set_option("qhash_roll_scalars", roll)
                ctx.filter_reset()
                ctx.pass1_insert(lo, hi)
                got = ctx.pass1_query(lo, hi)
                st = {s: ctx.stat(s) for s in ("insert_path", "query_path", "insert_hash_kernel", "query_hash_kernel", "query_hash_form", "query_b1",
                                               "query_overflow_entries", "periodic_any_query")}
                tag = (k, L, q, options, lo, hi, pushes, roll, st)
                assert st["insert_path"] == 2 and st["query_path"] == 2, tag
                assert st["query_hash_kernel"] == 1, tag  # k_q_hash2
                assert st["query_hash_form"] & 1 == (1 if pushes == 6 else 0), tag
                assert (st["query_hash_form"] >> 1) & 1 == roll, tag
                assert st["query_hash_form"] >> 2 == (0 if (lo, hi) == (0, (1 << L) - 1) else 1), tag  # the gated instantiation
                if want_b1 is not None:
                    assert st["query_b1"] == want_b1, tag
                assert got == want, ("marks", got, want) + tag
                mask = ctx.mask_download(False)
                bad = np.nonzero(mask != o.round_mask)[0]
                assert bad.size == 0, ("candidate mask", bad[:8], mask[bad[:8]], o.round_mask[bad[:8]]) + tag
                if filters:
                    assert (ctx.filter_download() == o.filter).all(), ("filter bitmap",) + tag
                out.append(st)
    finally:
        try:
            for opt, val in DEFAULTS:
                ctx.set_option(opt, val)
        finally:
            ctx.close()
            o.close()
    return out


def test_compaction_every_letter_pair(capi):
    """Every (cp, cn) of A C G T N around an N-free window, six pushes against eight."""
    k = 9
    recs = pairs_text(k)
    assert pairs_seen(recs, k) == {(a, b) for a in range(5) for b in range(5)}
    assert 2000 < sum(len(r) for r in recs) < 8000
    stats = run_forms(capi, recs, k, 22, 5, (("slice_bits", 9),), forms=FORMS)
    assert len(stats) == 4


def test_compaction_boundaries_and_periodic_tracts(capi):
    """Positions beside N runs, record starts and ends, three tiles (three workgroups), periodic tracts whose positions send no probes."""
    k = 25
    recs = boundary_text(k)
    assert 2 * TILE < sum(len(r) + 1 for r in recs) + 1 < 3 * TILE
    stats = run_forms(capi, recs, k, 22, 5, (("slice_bits", 9),), forms=FORMS)
    assert all(st["periodic_any_query"] == 1 for st in stats), stats


def test_compaction_gated_rounds(capi):
    """Four gated rounds on one context: most positions of a round send no probes, the others all six."""
    k, L = 9, 24
    recs = boundary_text(k, seed=3)
    size = 1 << L
    ranges = [(i * size // 4, (i + 1) * size // 4 - 1) for i in range(4)]
    stats = run_forms(capi, recs, k, L, 5, (("slice_bits", 10),), ranges=ranges, forms=FORMS)
    assert len(stats) == 16


# k, L, slice_bits, bins of level 1 (log2), filter compared
GEOMETRIES = [
    pytest.param(9, 22, 9, None, True, id="k9-L22"),
    pytest.param(25, 26, 8, 9, True, id="k25-L26-512bins"),         # HALF: in- and out-edges in two rounds, three pushes each
    pytest.param(51, 33, 20, None, False, id="k51-L33"),            # L > 32: values on two registers
    pytest.param(25, 33, 15, 9, False, id="k25-L33-512bins"),       # both
    pytest.param(65, 24, 10, None, True, id="k65-no-seed-table"),   # k > 64: the run is seeded by rolling
]


@pytest.mark.parametrize("k,L,slice_bits,b1,filters", GEOMETRIES)
def test_compaction_geometries(capi, k, L, slice_bits, b1, filters):
    recs = boundary_text(k, seed=k)[:4] + pairs_text(k, copies=1, seed=k)
    run_forms(capi, recs, k, L, 5, (("slice_bits", slice_bits),), forms=FORMS, want_b1=b1, filters=filters)


def test_every_switch_position_on_a_golden(capi, tmp_path):
    """Each position of the two switches once, on the golden rand6_k9_fp: marks, mask and filter of its first pass."""
    from helpers import case_files, golden_cases
    case = [c for c in golden_cases() if c["name"] == "rand6_k9_fp"][0]
    k, L, q = case["k"], case["L"], case["q"]
    o = O.Oracle(k, L, q, O.seed_table(case["seed"], q, L))
    files = case_files(case, tmp_path)
    for f in files:
        o.add_fasta(f)
    whole = (0, (1 << L) - 1)
    o.fill_only(*whole)
    want = o.check_only(*whole)
    ctx = capi.Context(0)
    try:
        for opt, val in (("insert_mode", 2), ("query_mode", 2), ("slice_bits", 8)):
            ctx.set_option(opt, val)
        ctx.set_params(k, L, q, capi.seed_table(q, L, seed=case["seed"]))
        ctx.seq_upload(capi.PackedText.from_fasta(files))
        seen = set()
        for pushes, roll in FORMS:
            ctx.set_option("qhash_pushes", pushes)
            ctx.set_option("qhash_roll_scalars", roll)
            ctx.filter_reset()
            ctx.pass1_insert(*whole)
            assert ctx.pass1_query(*whole) == want, (pushes, roll)
            assert ctx.stat("query_hash_kernel") == 1
            seen.add(ctx.stat("query_hash_form"))
            assert (ctx.mask_download(False) == o.round_mask).all() and (ctx.filter_download() == o.filter).all(), (pushes, roll)
        assert seen == {0, 1, 2, 3}, seen
    finally:
        try:
            for opt, val in DEFAULTS:
                ctx.set_option(opt, val)
        finally:
            ctx.close()
            o.close()
