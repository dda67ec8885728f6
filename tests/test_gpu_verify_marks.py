"""GPU (-m gpu): the verification's marks as write-combined lists (option "verify_marks" = 1: k_q_verify2 / k_q_verify store one verdict
per survivor, k_mark_split bins the positions by bucket, k_mark_apply ORs every bucket into its slice of the mask in LDS) against the
oracle and against the device atomics (verify_marks = 0) on the same context: mark count and candidate mask, bit for bit.

The shapes are the smallest at which the lists can go wrong: marks in the first and the last word of a bucket and a last, partial
bucket (buckets of one tile), a text shorter than a bucket, N-neighbour marks of the hash kernel in the words the apply loads, many tile
batches and a gated second range on the same context (stale lists), both verification kernels at q = 1, 5, 16, regions so small that
most entries take the atomic fallback, buckets cut into LDS sub-slices, and periodic twins that copy their verdict from the marks.
The stat "query_mark_path" says which path ran, so a case cannot pass on the other one, and "query_mark_fallback" counts the entries
that found a ring or region full."""
import numpy as np
import pytest

import periodic_cases as C
from oracle import oracle as O

pytestmark = pytest.mark.gpu

LETTERS = np.frombuffer(b"ACGTN", dtype=np.uint8)
SEED = 4711
TILE = 16384  # positions of a 512-word tile: the smallest bucket (mark_bucket_bits = 14)
TEST_OPTIONS = ("mark_bucket_bits", "mark_region_cap", "mark_slice_bits")  # process-wide: every case puts them back


@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


def starts_of(recs):
    """Text position of the first letter of every record (position 0 and the position behind every record hold a separator)."""
    out, at = [], 1
    for r in recs:
        out.append(at)
        at += len(r) + 1
    return out


def put(recs, pos, letters):
    """Overwrite the text at global position pos; the letters must lie inside one record."""
    for r, s in zip(recs, starts_of(recs)):
        if s <= pos and pos + len(letters) <= s + len(r):
            r[pos - s:pos - s + len(letters)] = letters
            return
    raise AssertionError(("not inside a record", pos, len(letters)))


def edge_text(k, total=5 * TILE - 3000, seed=0):
    """~5 tiles, not a whole number of them: two mutated copies of one sequence (true second edges), a record shorter than k, and at the
    four tile boundaries B in turn a k-mer planted to START at B - 8 (a verified mark in the last word of a bucket) or at B + 3 (the
    first word of the next); the two copies of a planted k-mer get different neighbours, which makes it a junction.  Behind the first
    two an N run two letters later: the vertex that ends at the run (it starts at the planted position + 2) is marked by the hash kernel,
    in the same word.  Returns the records, the planted positions and those N-neighbour positions."""
    rng = np.random.default_rng(77 + 13 * k + seed)
    n0 = total // 2 + 900
    n1 = total - n0 - max(1, k - 1) - 4
    base = rng.integers(0, 4, n0).astype(np.uint8)
    recs = []
    for n in (n0, n1):
        s = base[:n].copy()
        hits = rng.random(s.size) < 0.02
        s[hits] = rng.integers(0, 4, int(hits.sum())).astype(np.uint8)
        recs.append(s)
    recs.append(rng.integers(0, 4, max(1, k - 1)).astype(np.uint8))
    n_text = sum(len(r) + 1 for r in recs) + 1
    bounds = list(range(TILE, n_text, TILE))
    assert len(bounds) == 4 and n_text % TILE != 0, n_text
    kmers = (rng.integers(0, 4, k).astype(np.uint8), rng.integers(0, 4, k).astype(np.uint8))
    planted = []
    for i, b in enumerate(bounds):
        at = b - 8 if i % 2 == 0 else b + 3
        put(recs, at - 1, np.concatenate([[i // 2], kmers[i % 2], [2 + i // 2]]).astype(np.uint8))
        planted.append(at)
        if i < 2:
            put(recs, at + k + 2, np.full(3, 4, dtype=np.uint8))
    return recs, planted, [at + 2 for at in planted[:2]]


def repeat_text(k, seed=0):
    """One 2 kbp unit copied 20 times with a few substitutions each (a repeat family: thousands of marks in one bucket) between two
    mutated copies of a random sequence."""
    rng = np.random.default_rng(500 + k + seed)
    unit = rng.integers(0, 4, 2000).astype(np.uint8)
    fam = []
    for _ in range(20):
        u = unit.copy()
        hits = rng.random(u.size) < 0.015
        u[hits] = rng.integers(0, 4, int(hits.sum())).astype(np.uint8)
        fam.append(u)
        fam.append(rng.integers(0, 4, 7).astype(np.uint8))
    base = rng.integers(0, 4, 12000).astype(np.uint8)
    mut = base.copy()
    hits = rng.random(mut.size) < 0.02
    mut[hits] = rng.integers(0, 4, int(hits.sum())).astype(np.uint8)
    return [base, np.concatenate(fam), mut, rng.integers(0, 4, max(1, k - 1)).astype(np.uint8)]


def make_oracle(k, L, q, recs):
    o = O.Oracle(k, L, q, O.seed_table(SEED, q, L))
    for r in recs:
        o.add_record(LETTERS[np.asarray(r, dtype=np.uint8)].tobytes())
    return o


def open_ctx(capi, options=()):
    ctx = capi.Context(0)
    for opt, val in (("insert_mode", 2), ("query_mode", 2), ("part_min_tiles", 1), ("slice_bits", 9)) + tuple(options):
        ctx.set_option(opt, val)
    return ctx


def close_ctx(ctx):
    try:
        for opt in TEST_OPTIONS:
            ctx.set_option(opt, 0)
        ctx.set_option("verify_marks", 1)
    finally:
        ctx.close()


def check(ctx, o, ranges, tag, lists=(1, 0)):
    """Insert and query every (lo, hi); for each path of `lists` in turn: marks == check_only, mask == round_mask, the path that ran."""
    masks = []
    for lo, hi in ranges:
        o.fill_only(lo, hi)
        want = o.check_only(lo, hi)
        for path in lists:
            ctx.set_option("verify_marks", path)
            ctx.filter_reset()
            ctx.pass1_insert(lo, hi)
            got = ctx.pass1_query(lo, hi)
            t = tag + (lo, hi, path)
            assert ctx.stat("query_path") in (2, 3), t
            assert ctx.stat("query_mark_path") == path, t
            if path == 0:
                assert ctx.stat("query_mark_fallback") == 0, t
            assert got == want, ("marks", got, want) + t
            mask = ctx.mask_download(False)
            bad = np.nonzero(mask != o.round_mask)[0]
            assert bad.size == 0, ("candidate mask", bad[:8], mask[bad[:8]], o.round_mask[bad[:8]]) + t
        masks.append(o.round_mask.copy())
    return masks


@pytest.mark.parametrize("q", [1, 5, 16])
@pytest.mark.parametrize("k", [25, 31, 32, 65])
def test_bucket_edges_both_kernels(capi, k, q):
    """Buckets of one tile on ~5 tiles: marks in the first and last word of a bucket, the partial last bucket, N-neighbour marks in the
    words the apply loads; k_q_verify2 (k <= 31) and k_q_verify (k >= 32); q = 1: every survivor passes."""
    L = 21
    recs, planted, n_side = edge_text(k)
    ctx = open_ctx(capi, (("mark_bucket_bits", 14),))
    try:
        ctx.set_params(k, L, q, capi.seed_table(q, L, seed=SEED))
        ctx.seq_upload(capi.PackedText.from_codes(recs))
        o = make_oracle(k, L, q, recs)
        mask = check(ctx, o, [(0, 1 << L)], ("edges", k, q))[0]
        assert ctx.stat("query_verify_kernel") == (1 if k <= 31 else 3)
        for at in planted:  # the text does what it was built for: a mark at every planted k-mer, in the word beside the boundary
            assert (mask[at >> 5] >> (at & 31)) & 1, ("planted junction not marked", at)
            assert (at >> 5) % 512 in (0, 511), at
        # load, not zero: the hash kernel's N-neighbour mark shares its mask word with the verified mark of the planted k-mer, so an
        # apply that zeroed its slice instead of loading it would drop the former (the comparison in check() then fails)
        for at, nn in zip(planted, n_side):
            assert nn >> 5 == at >> 5 and (mask[nn >> 5] >> (nn & 31)) & 1, ("no N-neighbour mark beside the planted junction", at, nn)
        o.close()
    finally:
        close_ctx(ctx)


def test_text_shorter_than_a_bucket(capi):
    k, L, q = 25, 21, 5
    rng = np.random.default_rng(5)
    base = rng.integers(0, 4, 4000).astype(np.uint8)
    mut = base.copy()
    mut[::97] = (mut[::97] + 1) % 4
    recs = [base, mut, rng.integers(0, 4, 10).astype(np.uint8)]
    ctx = open_ctx(capi)
    try:
        ctx.set_params(k, L, q, capi.seed_table(q, L, seed=SEED))
        ctx.seq_upload(capi.PackedText.from_codes(recs))
        o = make_oracle(k, L, q, recs)
        mask = check(ctx, o, [(0, 1 << L)], ("short",))[0]
        assert mask.any()
        o.close()
    finally:
        close_ctx(ctx)


@pytest.mark.parametrize("k", [31, 32])
def test_many_batches_then_a_gated_range(capi, k):
    """A 64 KiB buffer budget: several tile batches (batches after the first mark relative to their own first tile), then a gated
    range on the same context -- verdict lists and regions of the pass before must not leak into it."""
    L, q = 21, 5
    recs, _, _ = edge_text(k, seed=1)
    ctx = open_ctx(capi, (("part_budget_bytes", 64 << 10), ("mark_bucket_bits", 14)))
    try:
        ctx.set_params(k, L, q, capi.seed_table(q, L, seed=SEED))
        ctx.seq_upload(capi.PackedText.from_codes(recs))
        o = make_oracle(k, L, q, recs)
        size = 1 << L
        whole, gated = check(ctx, o, [(0, size), (size * 3 // 16, size * 11 // 16)], ("batches", k))
        assert ctx.stat("query_batches") > 1
        assert whole.any() and gated.any() and (whole != gated).any()
        o.close()
    finally:
        close_ctx(ctx)


@pytest.mark.parametrize("k", [25, 32])
def test_region_full_takes_the_atomic_fallback(capi, k):
    """Regions of 32 entries (64 of them: one bucket of 2^17 positions holds the whole text) against a repeat family that puts
    thousands of marks into that bucket: most entries find their region full and are ORed straight into the mask."""
    L, q = 21, 5
    recs = repeat_text(k)
    ctx = open_ctx(capi, (("mark_region_cap", 32), ("mark_bucket_bits", 17)))
    try:
        ctx.set_params(k, L, q, capi.seed_table(q, L, seed=SEED))
        ctx.seq_upload(capi.PackedText.from_codes(recs))
        o = make_oracle(k, L, q, recs)
        mask = check(ctx, o, [(0, 1 << L)], ("region full", k), lists=(0, 1))[0]
        total = int(np.unpackbits(mask.view(np.uint8)).sum())
        held = 64 * 32  # what the 64 regions of the one bucket can hold
        assert total > 2 * held, "not enough marks to fill the regions"
        # the last pass of check() ran on the lists.  A list entry is a passing survivor, one per (position, edge): at least one and (the
        # edge field has three bits) at most eight per verified mark.  The regions hold `held` of them and the rest took the fallback.
        # The marks that are not verified ones come from the hash kernel: at most two beside each of the five separators (no N run).
        lost = ctx.stat("query_mark_fallback")
        assert total - held - 2 * (len(recs) + 1) <= lost <= 8 * total, (lost, total)
        o.close()
    finally:
        close_ctx(ctx)


@pytest.mark.parametrize("bucket_bits,slice_bits", [(21, 0), (14, 12), (16, 13)])
def test_buckets_cut_into_sub_slices(capi, bucket_bits, slice_bits):
    """A bucket larger than its LDS slice: 2^21-bit buckets (two 2^20-bit sub-slices, the form a batch near 2^30 positions takes), and
    the slice limit lowered so that one-tile and four-tile buckets are cut in four and in eight."""
    k, L, q = 25, 21, 5
    recs, _, _ = edge_text(k, seed=2)
    ctx = open_ctx(capi, (("mark_bucket_bits", bucket_bits), ("mark_slice_bits", slice_bits)))
    try:
        ctx.set_params(k, L, q, capi.seed_table(q, L, seed=SEED))
        ctx.seq_upload(capi.PackedText.from_codes(recs))
        o = make_oracle(k, L, q, recs)
        check(ctx, o, [(0, 1 << L)], ("sub-slices", bucket_bits, slice_bits))
        o.close()
    finally:
        close_ctx(ctx)


def test_periodic_twins_copy_from_the_marks(capi):
    """Positions inside periodic tracts send no probes and take their twin's verdict after the verification: the copy must read marks
    that k_mark_apply has already written."""
    k, L, q = 25, 21, 5
    case = C.constructed_case(k, tiles=2)
    recs = [np.asarray(r, dtype=np.uint8) for r in case["records"]]
    ctx = open_ctx(capi, (("mark_bucket_bits", 14),))
    try:
        ctx.set_params(k, L, q, capi.seed_table(q, L, seed=SEED))
        ctx.seq_upload(capi.PackedText.from_codes(recs))
        o = make_oracle(k, L, q, recs)
        mask = check(ctx, o, [(0, 1 << L)], ("periodic",))[0]
        assert ctx.stat("periodic_skip") == 1
        qs = np.asarray(case["qs"]).astype(bool)
        bits = np.unpackbits(mask.view(np.uint8), bitorder="little")[:qs.size].astype(bool)
        assert (bits & qs).any(), "no copying position carries a mark: the case does not test the copy"
        o.close()
    finally:
        close_ctx(ctx)
