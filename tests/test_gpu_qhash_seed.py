"""GPU (-m gpu): how the level-1 query hash (k_q_hash2) seeds a thread's run of 16 positions, against the oracle.

One switch, a process-wide option (include/twopaco_hip.h):
  qhash_seed_scalars  1: the hash of a run's first window is built from function 0's pre-rotated letter rows [k][5] x 16 bytes that
                      tpc_set_params leaves in device memory -- the five rows of a character are loaded at a uniform index and XORed
                      in under one-hot lane masks of the letter; 0: from the same rows in LDS, one 16-byte read per character at a per-lane index.
                      k > 64 has no such table: the run is seeded by rolling, whatever the option says.
Every case inserts and queries a three-tile text through the C-ABI in both positions of the switch and compares marks, candidate mask
and (L <= 32) filter bitmap with the oracle.  "query_hash_kernel" and "query_hash_seed" say what ran: a case cannot pass on the other
kernel or the other form, and at k = 65 the stat must not claim the table.

What can go wrong and where it shows: a row of the wrong character index, a rotation that does not wrap (k - 1 - t >= L at L = 24,
t >= L at k = 51 and 64), the high halves at L = 36, the N row (N runs of 1, 2 and k letters inside seeding windows), a partial chunk of
16 characters (k = 9, 25, 51) and a table of another k, L or seed left behind by an earlier tpc_set_params.  A wrong seed derails all 16
positions of a run, so the marks and the mask of the texts of tests/test_gpu_qhash_lds.py show it; its pairs_text has every (cp, cn) of
the 5 x 5 letters: the roll from scalar registers takes the leaving and the entering letter by the same lane masks as the seeding.

Ranges are [lo, hi] with both ends inclusive, as in the C-ABI.  The environment knob TPC_QHASH_SEED_SCALARS is read once per process
and is not tested here: the option is."""
import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_qhash_lds import LETTERS, TILE, boundary_text, pairs_seen, pairs_text

pytestmark = pytest.mark.gpu

SEED = 977
Q = 5
DEFAULTS = (("qhash_pushes", 6), ("qhash_roll_scalars", 1), ("qhash_seed_scalars", 1))  # process-wide: every case puts them back
BASE_OPTIONS = (("insert_mode", 2), ("query_mode", 2), ("part_min_tiles", 1), ("part_levels", 2))
SLICE_BITS = {24: 10, 36: 20}  # 128 + 128 bins at L = 24, the headline geometry (256 + 256) at L = 36


@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


def seed_text(k, seed=0):
    """Three tiles: the boundary text (record ends inside a tile, N runs of 1, 2 and k letters, periodic tracts) and every (cp, cn) pair."""
    recs = boundary_text(k, seed=seed) + pairs_text(k, copies=1, seed=seed)
    assert 2 * TILE < sum(len(r) + 1 for r in recs) + 1 < 3 * TILE
    assert pairs_seen(recs, k) == {(a, b) for a in range(5) for b in range(5)}
    return recs


def make_oracle(recs, k, L, seed=SEED):
    o = O.Oracle(k, L, Q, O.seed_table(seed, Q, L))
    for r in recs:
        o.add_record(LETTERS[np.asarray(r, dtype=np.uint8)].tobytes())
    return o


def query_both_forms(ctx, o, k, L, ranges=None, want_b1=None):
    """Insert and query every range with qhash_seed_scalars = 1 and 0 on a context whose parameters and text are set; marks, mask and
    (L <= 32) filter against the oracle `o`, one oracle round per range shared by the two forms."""
    whole = (0, (1 << L) - 1)
    maxk = ctx.stat("query_hash_seed_maxk")  # the longest k with a seed table
    assert maxk == 64, maxk  # the k of the cases below stand on both sides of it
    for lo, hi in ranges or (whole,):
        o.fill_only(lo, hi)
        want = o.check_only(lo, hi)
        for seeded in (1, 0):
            ctx.set_option("qhash_seed_scalars", seeded)
            ctx.filter_reset()
            ctx.pass1_insert(lo, hi)
            got = ctx.pass1_query(lo, hi)
            st = {s: ctx.stat(s) for s in ("insert_path", "query_path", "query_hash_kernel", "query_hash_form", "query_hash_seed", "query_b1",
                                           "query_overflow_entries")}
            tag = (k, L, lo, hi, seeded, st)
            assert st["insert_path"] == 2 and st["query_path"] == 2, tag
            assert st["query_hash_kernel"] == 1, tag  # k_q_hash2
            assert st["query_hash_seed"] == (seeded if k <= maxk else 0), tag
            assert st["query_hash_form"] & 3 == 3, tag  # six pushes, the roll from scalars: the defaults
            assert st["query_hash_form"] >> 2 == (0 if (lo, hi) == whole else 1), tag  # the gated instantiation
            if want_b1 is not None:
                assert st["query_b1"] == want_b1, tag
            assert got == want, ("marks", got, want) + tag
            mask = ctx.mask_download(False)
            bad = np.nonzero(mask != o.round_mask)[0]
            assert bad.size == 0, ("candidate mask", bad[:8], mask[bad[:8]], o.round_mask[bad[:8]]) + tag
            if L <= 32:
                assert (ctx.filter_download() == o.filter).all(), ("filter bitmap",) + tag


def run_case(capi, recs, k, L, slice_bits, ranges=None, want_b1=None):
    o = make_oracle(recs, k, L)
    ctx = capi.Context(0)
    try:
        for opt, val in BASE_OPTIONS + (("slice_bits", slice_bits),):
            ctx.set_option(opt, val)
        ctx.set_params(k, L, Q, capi.seed_table(Q, L, seed=SEED))
        ctx.seq_upload(capi.PackedText.from_codes(recs))
        query_both_forms(ctx, o, k, L, ranges=ranges, want_b1=want_b1)
    finally:
        try:
            for opt, val in DEFAULTS:
                ctx.set_option(opt, val)
        finally:
            ctx.close()
            o.close()


# k = 9: one partial chunk of 16; 25; 51: rotations wrap mod L; 64: the longest k with a table; 65: the rolled fallback
@pytest.mark.parametrize("L", [24, 36])
@pytest.mark.parametrize("k", [9, 25, 51, 64, 65])
def test_seed_every_k_and_L(capi, k, L):
    run_case(capi, seed_text(k, seed=k), k, L, SLICE_BITS[L])


def test_seed_gated_range(capi):
    """A range that is not the whole hash space: the gate reads the seeded value of a run's first position."""
    k, L = 25, 24
    size = 1 << L
    run_case(capi, seed_text(k, seed=5), k, L, SLICE_BITS[L], ranges=[(size // 4, 3 * size // 4 - 1)])


def test_seed_512_bins(capi):
    """512 bins at level 1: in- and out-edges of a position go in two rounds of three pushes."""
    k, L = 25, 26
    run_case(capi, seed_text(k, seed=6), k, L, 8, want_b1=9)


def test_seed_table_follows_set_params(capi):
    """tpc_set_params twice on one context, (k = 25, L = 36) and then (k = 9, L = 24) with another seed, a query after each: rows left
    over from the first call would seed the second call's runs with the wrong k, L and letters."""
    recs = seed_text(25, seed=8)
    ctx = capi.Context(0)
    try:
        for opt, val in BASE_OPTIONS:
            ctx.set_option(opt, val)
        ctx.seq_upload(capi.PackedText.from_codes(recs))
        for k, L, seed in ((25, 36, SEED), (9, 24, SEED + 1)):
            o = make_oracle(recs, k, L, seed=seed)
            try:
                ctx.set_option("slice_bits", SLICE_BITS[L])
                ctx.set_params(k, L, Q, capi.seed_table(Q, L, seed=seed))
                query_both_forms(ctx, o, k, L)
            finally:
                o.close()
    finally:
        try:
            for opt, val in DEFAULTS:
                ctx.set_option(opt, val)
        finally:
            ctx.close()
