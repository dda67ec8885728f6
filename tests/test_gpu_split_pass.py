"""GPU (-m gpu): the split pass -- k_split_emask, k_split<1..16>, k_split_anyq, tpc_pass1_split_hist -- against its definition
(tests/split_reference.py, pinned to the oracle without a device by tests/test_split_reference_cpu.py).

Every text is generated.  Where every edge is must-win for the phase count that runs, the 2^24 bins must equal the reference's
distinct_hist bin for bin under any schedule (the exact cases: every hash count, every window width, tile edges, mask layouts, both
strands).  Where edges cover each other's bits (crowded filter with q phases, sparse filter with 3) the bins must lie between the
must-win edges' histogram and all edges', and the scratch filter left behind between their bits -- with q phases it IS the union.
Every test asserts the stats "split_kernel" and "split_phases", so none passes on the other kernel or the other phase count.

Measured on an MI355X: the whole file (66 cases) 23 s of wall time, most of it the reference's per-position calls into the oracle on
the host; the slowest test is test_exact[q64] at 1.1 s (2 s of hashing for the reference included), every other one under 0.9 s.
Each tpc_pass1_split_hist call downloads 64 MiB of bins, so no test makes more than six.

Against four scratch builds with one value wrong each 36, 62, 57 and 64 of the 66 cases fail.  At k = 3 positions share
the few 4-mers there are, so one dropped position may not show in the bins; the same layouts run at k = 25 / 603, where it does."""
import numpy as np
import pytest

import split_reference as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


def open_case(capi, case, options=()):
    """(context, text, reference) with the case's text uploaded; the layout the reference assumes is the packed text's."""
    ref = S.reference(case)
    text = capi.PackedText.from_codes(ref.recs)
    assert text.length == ref.n_text and (text.rec_start == ref.rec_start).all() and (text.rec_length == ref.rec_len).all()
    ctx = capi.Context(0)
    try:
        for opt, val in options:
            ctx.set_option(opt, val)
        ctx.set_params(case["k"], case["L"], case["q"], capi.seed_table(case["q"], case["L"], seed=case.get("seed", S.SEED)))
        ctx.seq_upload(text)
    except Exception:
        ctx.close()
        raise
    return ctx, text, ref


def split(ctx, case, ref, filtered=True):
    """One tpc_pass1_split_hist; asserts the stats, returns the bins."""
    keep = ref.rec_len >= case["k"] if filtered else np.ones(ref.rec_len.size, dtype=bool)
    force = case["force_anyq"]
    if force:
        ctx.set_option("test_force_anyq", 1)   # process-wide: always reset below
    try:
        bins = ctx.pass1_split_hist(ref.rec_start[keep], ref.rec_len[keep]).astype(np.int64)
    finally:
        if force:
            ctx.set_option("test_force_anyq", 0)
    st = (ctx.stat("split_kernel"), ctx.stat("split_phases"))
    assert st == (S.kernel_of(case["q"], force), S.phases_of(case["q"], ref.n_text, case["L"])), st
    return bins


def scratch_filter(ctx, ref):
    f = ctx.filter_download()
    n = ref.filter_words()
    assert not f[n:].any()
    return f[:n]


def check_exact(bins, ref, tag):
    want = ref.distinct_hist()
    assert int(bins.sum()) == 2 * ref.n_edges, (tag, int(bins.sum()), ref.n_edges)
    assert (bins == want).all(), (tag, np.nonzero(bins != want)[0][:10])


def check_sandwich(ctx, bins, ref, phases, tag):
    """Properties 3, 5 and 6 of tests/split_reference.py, and 4 when all q phases ran."""
    lo, hi = ref.lower_hist(phases), ref.upper_hist()
    total = int(bins.sum())
    print("%s: %d edges, %d must-win, sum(bins) / 2 = %d" % (tag, ref.n_edges, int(ref.must_win(phases).sum()), total // 2))
    assert total % 2 == 0 and int(lo.sum()) <= total <= 2 * ref.n_edges, (tag, total)
    assert (lo <= bins).all() and (bins <= hi).all(), (tag, np.nonzero((lo > bins) | (bins > hi))[0][:10])
    f, union = scratch_filter(ctx, ref), ref.union_filter()
    if phases == ref.q:
        assert (f == union).all(), (tag, "filter != union", np.nonzero(f != union)[0][:10])
    else:
        must = ref.lower_filter(phases)
        assert not (must & ~f).any() and not (f & ~union).any(), tag


@pytest.mark.parametrize("name", sorted(S.EXACT))
def test_exact(capi, name):
    """Every hash count (k_split<1..16>, k_split_anyq at 17, 33, 64 and forced at 7), every window width, text totals around a tile,
    tile edges, mask layouts, no dispatched record at all: bins == distinct_hist bin for bin.  The mask layouts also with the
    unfiltered record list (the C-ABI drops the records shorter than k itself)."""
    case = S.EXACT[name]
    ctx, _, ref = open_case(capi, case)
    try:
        check_exact(split(ctx, case, ref), ref, name)
        if name.startswith(("mask", "short")):
            check_exact(split(ctx, case, ref, filtered=False), ref, name + " unfiltered")
        if ref.n_edges:
            assert (scratch_filter(ctx, ref) == ref.union_filter()).all(), name   # every edge won, so every bit of every edge is set
    finally:
        ctx.close()


@pytest.mark.parametrize("name", sorted(S.MASK_CROWDED))
def test_mask_layouts_crowded(capi, name):
    """The mask layouts under a filter small enough for q phases: the filter left behind is the union of all positions' bits, so a
    position the mask drops or adds shows there even when the bins do not tell."""
    case = S.MASK_CROWDED[name]
    ctx, _, ref = open_case(capi, case)
    try:
        for filtered in (True, False):
            check_sandwich(ctx, split(ctx, case, ref, filtered), ref, case["q"], (name, filtered))
    finally:
        ctx.close()


@pytest.mark.parametrize("name", sorted(S.CROWDED))
def test_crowded_filter_q_phases(capi, name):
    """q phases on a filter where a fifth and more of the edges find their first bit taken by another edge: the later phases decide."""
    case = S.CROWDED[name]
    ctx, _, ref = open_case(capi, case)
    try:
        bins = split(ctx, case, ref)
        assert ctx.stat("split_phases") == case["q"]
        check_sandwich(ctx, bins, ref, case["q"], name)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", sorted(S.SPARSE))
def test_sparse_filter_three_phases(capi, name):
    """3 phases of q on a filter about a tenth full: more than 1000 edges need phase 1, more than 50 need phase 2."""
    case = S.SPARSE[name]
    ctx, _, ref = open_case(capi, case)
    try:
        bins = split(ctx, case, ref)
        assert ctx.stat("split_phases") == 3
        check_sandwich(ctx, bins, ref, 3, name)
    finally:
        ctx.close()


def test_boundary_of_crowded(capi):
    """One text, q = 4, L = 18 and 19: q phases on one side of launch_split_q's `crowded`, 3 on the other."""
    for side, phases in (("crowded", 4), ("sparse", 3)):
        case = S.BOUNDARY[side]
        ctx, _, ref = open_case(capi, case)
        try:
            bins = split(ctx, case, ref)
            assert ctx.stat("split_phases") == phases, (side, ctx.stat("split_phases"))
            check_sandwich(ctx, bins, ref, phases, side)
        finally:
            ctx.close()


def test_both_strands(capi):
    """The text followed by the reverse complement of every record: the histogram of the text alone."""
    one = S.reference(S.STRANDS["one"])
    case = S.STRANDS["both"]
    ctx, _, ref = open_case(capi, case)
    try:
        bins = split(ctx, case, ref)
    finally:
        ctx.close()
    check_exact(bins, ref, "both")
    check_exact(bins, one, "one")


def test_repeat_and_after_an_insert(capi):
    """Two calls on one context give equal bins; a call after a first-pass insert -- the direct kernel's dense filter in place, or the
    partitioned insert, whose apply may still be deferred into the query that never comes -- gives the bins of a fresh context: the
    scratch filter is the pass's own."""
    case = S.EXACT["q5"]
    for mode in (0, 1, 2):
        opts = () if mode == 0 else (("insert_mode", mode), ("query_mode", mode), ("part_min_tiles", 1))
        ctx, _, ref = open_case(capi, case, opts)
        try:
            if mode:
                ctx.filter_reset()
                assert ctx.pass1_insert() > 0
                path = ctx.stat("insert_path")
                assert path == 1 if mode == 1 else path in (2, 3), (mode, path)
            check_exact(split(ctx, case, ref), ref, ("first", mode))
            check_exact(split(ctx, case, ref), ref, ("second", mode))
        finally:
            ctx.close()


@pytest.mark.parametrize("mode", [1, 2])
def test_round_after_a_split(capi, mode):
    """filter_reset, insert and query over a gated range after a split: filter, mask and marks are the oracle's -- no scratch bit
    survives into the round.  mode 1: the direct kernels, 2: the partitioned ones."""
    k, L, q = 25, 22, 5
    case = S._case(S.split_text, (k, 0), k, L, q)
    ctx, _, ref = open_case(capi, case, (("insert_mode", mode), ("query_mode", mode), ("slice_bits", 9), ("part_min_tiles", 1)))
    o = O.Oracle(k, L, q, O.seed_table(S.SEED, q, L))
    try:
        for r in ref.recs:
            o.add_record(S.LETTERS[r].tobytes())
        bins = split(ctx, case, ref)
        assert int(bins.sum()) % 2 == 0 and (bins <= ref.upper_hist()).all() and (bins >= ref.lower_hist(3)).all()
        assert scratch_filter(ctx, ref).any()
        lo, hi = (1 << L) * 3 // 16, (1 << L) * 11 // 16
        o.fill_only(lo, hi)
        marks = o.check_only(lo, hi)
        ctx.filter_reset()
        ctx.pass1_insert(lo, hi)
        got = ctx.pass1_query(lo, hi)
        paths = (ctx.stat("insert_path"), ctx.stat("query_path"))
        assert paths == (1, 1) if mode == 1 else (paths[0] in (2, 3) and paths[1] in (2, 3)), paths
        assert (ctx.filter_download() == o.filter).all(), "filter bitmap"
        assert got == marks > 0, (got, marks)
        assert (ctx.mask_download(False) == o.round_mask).all(), "candidate mask"
    finally:
        o.close()
        ctx.close()


def test_refused_on_a_sharded_context(capi):
    case = S.EXACT["mask_k25"]
    ref = S.reference(case)
    ctx = capi.Context(0)
    try:
        ctx.shard_config(0, 2)
        ctx.set_params(case["k"], case["L"], case["q"], capi.seed_table(case["q"], case["L"], seed=S.SEED))
        ctx.seq_upload(capi.PackedText.from_codes(ref.recs))
        with pytest.raises(RuntimeError, match="the split pass needs the whole filter as scratch: not available on a sharded context"):
            ctx.pass1_split_hist(ref.rec_start, ref.rec_len)
    finally:
        ctx.close()


@pytest.mark.parametrize("q", S.HOST_QS)
def test_through_the_host(capi, tmp_path, q):
    """capi.Enumerator(rounds=3) on the exact text: the planner's ranges are the oracle's, and so are the bytes."""
    import re
    case = S.EXACT["q%d" % q]
    ref = S.reference(case)
    k, L = case["k"], case["L"]
    fa = str(tmp_path / "in.fa")
    with open(fa, "w") as f:
        for i, r in enumerate(ref.recs):
            s = S.LETTERS[r].tobytes().decode()
            f.write(">r%d\n" % i)
            for j in range(0, len(s), 70):
                f.write(s[j:j + 70] + "\n")
    o = O.Oracle(k, L, q, O.seed_table(S.SEED, q, L))
    o.add_fasta(fa)
    o.enumerate(rounds=3)
    want = [(o.round_stats(r)["low"], o.round_stats(r)["high"]) for r in range(3)]
    want_bin = str(tmp_path / "oracle.bin")
    o.write_bin(want_bin)
    n_keys = len(o.keys)
    o.close()
    out = str(tmp_path / "gpu.bin")
    e = capi.Enumerator([fa], k, L, q=q, rounds=3, tmpdir=str(tmp_path), out=out, seed=S.SEED)
    try:
        got = [(int(a), int(b)) for a, b in re.findall(r"Round \d+, (\d+):(\d+)", e.log)]
        assert got == want, (q, got, want)
        assert open(out, "rb").read() == open(want_bin, "rb").read(), q
        assert e.vertices_count() == n_keys > 0
    finally:
        e.close()
