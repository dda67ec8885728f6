"""GPU (-m gpu): the entry points of the combined exchange driven directly in one process, against the oracle.

A. tpc_combine_export's set-bit lists (tpc_lists.h: a directory entry `unit << 24 | n` per (slice, window), 16-bit offsets `w << 5 | b`
   inside a 2^16-bit window) decoded in numpy, mapped back to filter addresses through the slice permutation, must be the oracle's
   filter bit for bit -- at every list density, on both export kernels (k_slice_combine below 16384 slices, the long-lived
   k_slice_export_p from there on), for 1, 4 and 16 windows per slice and 1 .. 8 destinations -- and must fit the block size
   tpc_combine_info promised.  Imported back, they give the oracle's filter and round mask.
B. tpc_pass1_query_begin followed by whatever may run before the query (another range, a new buffer budget, a filter download that
   materialises a pending insert, the export and import of the exchange): marks, mask and filter stay the oracle's."""
import numpy as np
import pytest
import torch

from lists_reference import PERM_INV, PERM_MULT, WINDOW_BITS, assert_bits_are_filter, decode_export  # noqa: F401 (the wire format, stated once)
from oracle import oracle as O

pytestmark = pytest.mark.gpu
LETTERS = np.frombuffer(b"ACGTN", dtype=np.uint8)


@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


def _random_records(n_pos, seed, n_rec=4):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4, n_pos // n_rec).astype(np.uint8) for _ in range(n_rec)]


def _skewed_records():
    """Repeats and a poly-A run (test_gpu_parity.py:test_partitioned_query_adversarial_skew): regions and bins overflow."""
    rng = np.random.default_rng(5)
    unit = rng.integers(0, 4, 700).astype(np.uint8)
    return [np.tile(unit, 400), np.zeros(200000, dtype=np.uint8), np.concatenate([unit[:300], unit[350:]])]


def _setup(capi, recs, k, L, q, seed, slice_bits, **opts):
    o = O.Oracle(k, L, q, O.seed_table(seed, q, L))
    for r in recs:
        o.add_record(LETTERS[r].tobytes())
    ctx = capi.Context(0)
    for opt, val in (("insert_mode", 2), ("query_mode", 2), ("slice_bits", slice_bits), ("part_min_tiles", 1)) + tuple(opts.items()):
        ctx.set_option(opt, val)
    ctx.set_params(k, L, q, capi.seed_table(q, L, seed=seed))
    ctx.seq_upload(capi.PackedText.from_codes(recs))
    return ctx, o


def export_and_check(ctx, o, n_dest, L):
    info = ctx.combine_info(n_dest)
    assert info["sparse"] == 1, info
    cap = info["cap_units"]
    payload = torch.zeros(n_dest * cap * 8, dtype=torch.int16, device="cuda")
    dirs = torch.zeros(info["slices"] * info["windows"], dtype=torch.int64, device="cuda")
    units = ctx.combine_export(n_dest, payload.data_ptr(), cap, dirs.data_ptr())
    assert all(u <= cap for u in units), (units, cap)
    addr = decode_export(info, n_dest, L, payload.cpu().numpy().view(np.uint16), dirs.cpu().numpy().view(np.uint64), units)
    assert_bits_are_filter(addr, o.filter)
    return info, payload, dirs


def import_and_query(ctx, o, n_dest, info, payload, dirs, marks):
    spd = info["slices"] // n_dest
    ctx.combine_import(n_dest, n_dest, payload.data_ptr(), [d * info["cap_units"] for d in range(n_dest)], dirs.data_ptr(), spd * info["windows"])
    fused = ctx.stat("fused_lookups")
    assert ctx.pass1_query() == marks
    assert ctx.stat("fused_lookups") == fused + 1  # (this query's lookup built the slices from the lists)
    assert (ctx.mask_download(False) == o.round_mask).all()
    assert (ctx.filter_download() == o.filter).all()


# (name, L, slice_bits, positions -- 0: one all-N record): about positions * 5 / (2^L / 2^16) distinct bits per 2^16-bit window
EXPORT_CASES = [
    ("empty", 22, 16, 0),
    ("m2_like", 22, 16, 2000),
    ("band", 22, 16, 32000),
    ("dense", 22, 16, 1000000),        # more than half of every window
    ("band_4win", 24, 18, 120000),
    ("dense_4win", 24, 18, 3000000),
    ("band_16win", 26, 20, 500000),
    ("persist_empty", 30, 16, 0),
    ("persist_m2_like", 30, 16, 500000),
    ("persist_band", 30, 16, 8000000),  # ~2400 bits per window: the long-lived export claimed 8.4 M units against a bound of 5.5 M
    ("persist_4win", 32, 18, 2000000),
]


@pytest.mark.parametrize("name,L,slice_bits,n_pos", EXPORT_CASES, ids=[c[0] for c in EXPORT_CASES])
def test_export_lists_are_the_filter(capi, name, L, slice_bits, n_pos):
    recs = _random_records(n_pos, seed=L + n_pos) if n_pos else [np.full(100000, 4, dtype=np.uint8)]
    ctx, o = _setup(capi, recs, 25, L, 5, 11, slice_bits)
    try:
        o.fill_only()
        marks = o.check_only()
        for n_dest in (1, 2, 4, 8):
            ctx.filter_reset()
            ctx.pass1_insert()
            assert ctx.stat("insert_batches") == 1
            info, payload, dirs = export_and_check(ctx, o, n_dest, L)
            assert info["slices"] == 1 << (L - slice_bits) and info["windows"] == max(1, 1 << (slice_bits - WINDOW_BITS))
            import_and_query(ctx, o, n_dest, info, payload, dirs, marks)
            del payload, dirs
    finally:
        ctx.close()


def test_export_carries_the_level2_overflow_entries(capi):
    """The insert's level-2 regions overflow (skewed input): the export ORs the overflow entries into their slices too."""
    ctx, o = _setup(capi, _skewed_records(), 25, 24, 5, 3, 12)
    try:
        o.fill_only()
        marks = o.check_only()
        for n_dest in (1, 4):
            ctx.filter_reset()
            ctx.pass1_insert()
            assert ctx.stat("insert_overflow_entries") > 0
            info, payload, dirs = export_and_check(ctx, o, n_dest, 24)
            import_and_query(ctx, o, n_dest, info, payload, dirs, marks)
    finally:
        ctx.close()


@pytest.mark.parametrize("why", ["blocked_entries", "too_many_dests", "batches", "three_levels"])
def test_not_sparse_is_an_answer_not_a_fault(capi, why):
    """Where the insert did not stay in 32-bit level-2 regions of one batch and two levels, or there are more destinations than level-1
    buckets, tpc_combine_info says "not sparse" and tpc_combine_export fails cleanly; the query still gets the oracle's answer."""
    from twopaco_amd import synth
    recs, _ = synth.workload("m1", scale=0.01)
    opts = {"batches": {"part_budget_bytes": 3 << 20}, "three_levels": {"part_levels": 3}}.get(why, {})
    ctx, o = _setup(capi, recs, 25, 26, 5, 11, 14, **opts)
    try:
        if why == "blocked_entries":
            ctx.set_option("insert_entry_fmt", 3)  # (process-wide)
        o.fill_only()
        marks = o.check_only()
        ctx.filter_reset()
        ctx.pass1_insert()
        n_dest = 2
        if why == "too_many_dests":
            n_dest = 2 << ctx.combine_info(1)["b1"]
        elif why == "blocked_entries":
            assert ctx.stat("insert_entry_fmt") == 3
        elif why == "batches":
            assert ctx.stat("insert_batches") > 1
        assert ctx.combine_info(n_dest)["sparse"] == 0
        payload = torch.zeros(1 << 20, dtype=torch.int16, device="cuda")
        dirs = torch.zeros(1 << 16, dtype=torch.int64, device="cuda")
        with pytest.raises(RuntimeError):
            ctx.combine_export(n_dest, payload.data_ptr(), 1 << 16, dirs.data_ptr())
        assert ctx.pass1_query() == marks
        assert (ctx.mask_download(False) == o.round_mask).all()
        assert (ctx.filter_download() == o.filter).all()
    finally:
        ctx.set_option("insert_entry_fmt", 0)
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- B. the begun query
L_B = 26
# one round over the whole range, or three gated rounds that split it (each round: insert, begin, query)
RANGES = {"whole": [(0, 1 << L_B)], "rounds": [(0, (1 << (L_B - 2)) - 1), (1 << (L_B - 2), (1 << (L_B - 1)) - 1), (1 << (L_B - 1), (1 << L_B) - 1)]}


def _begun_rounds(ctx, o, rounds, pending, between, expect_begun, begin=None):
    for i, (lo, hi) in enumerate(rounds):
        _begun_round(ctx, o, lo, hi, pending, between, begin=begin[i] if begin else None)
        assert ctx.stat("query_begun") == expect_begun, (lo, hi)


def _begun_round(ctx, o, lo, hi, pending, between, begin=None):
    o.fill_only(lo, hi)
    marks = o.check_only(lo, hi)
    ctx.filter_reset()
    ctx.pass1_insert(lo, hi)
    if not pending:
        assert (ctx.filter_download() == o.filter).all()  # (materialises the insert: the query reads the filter)
    ctx.pass1_query_begin(*(begin or (lo, hi)))
    between()
    assert ctx.pass1_query(lo, hi) == marks
    assert (ctx.mask_download(False) == o.round_mask).all()
    assert (ctx.filter_download() == o.filter).all()


@pytest.fixture(scope="module")
def m1(capi):
    from twopaco_amd import synth
    recs, _ = synth.workload("m1", scale=0.01)  # 25 tiles of 16384 positions
    ctx, o = _setup(capi, recs, 25, L_B, 5, 11, 14)
    yield ctx, o
    ctx.close()


@pytest.mark.parametrize("pending", [True, False], ids=["pending", "applied"])
@pytest.mark.parametrize("rng", ["whole", "rounds"])
def test_begun_query_same_range(m1, pending, rng):
    ctx, o = m1
    _begun_rounds(ctx, o, RANGES[rng], pending, lambda: None, 1)


@pytest.mark.parametrize("pending", [True, False], ids=["pending", "applied"])
@pytest.mark.parametrize("rng", ["whole", "rounds"])
def test_begun_query_then_another_range(m1, pending, rng):
    ctx, o = m1
    rounds = RANGES[rng]
    other = [RANGES["rounds"][0]] if rng == "whole" else rounds[1:] + rounds[:1]
    _begun_rounds(ctx, o, rounds, pending, lambda: None, 0, begin=other)


@pytest.mark.parametrize("pending", [True, False], ids=["pending", "applied"])
@pytest.mark.parametrize("rng", ["whole", "rounds"])
def test_begun_query_keeps_its_plan(m1, pending, rng):
    """The buffer budget changes between begin and query (what free-memory drift does to the automatic budget): the query finishes
    under the plan its first batch was binned with."""
    ctx, o = m1
    ctx.set_option("part_budget_bytes", 0)
    try:
        for lo, hi in RANGES[rng]:
            ctx.set_option("part_budget_bytes", 0)
            _begun_round(ctx, o, lo, hi, pending, lambda: ctx.set_option("part_budget_bytes", 3 << 20))
            assert ctx.stat("query_begun") == 1
            begun_plan = [ctx.stat(s) for s in ("query_tiles_per_batch", "query_b1", "query_b2")]
            _begun_round(ctx, o, lo, hi, pending, lambda: None)  # (planned under the small budget from the start)
            small_plan = [ctx.stat(s) for s in ("query_tiles_per_batch", "query_b1", "query_b2")]
            assert ctx.stat("query_batches") > 1
            assert begun_plan != small_plan and begun_plan[0] > small_plan[0]
    finally:
        ctx.set_option("part_budget_bytes", 0)


@pytest.mark.parametrize("pending", [True, False], ids=["pending", "applied"])
@pytest.mark.parametrize("rng", ["whole", "rounds"])
def test_begun_query_then_filter_download(m1, pending, rng):
    ctx, o = m1
    # a pending insert materialised into the buffers the begun batch owned: the query binned its first batch again
    _begun_rounds(ctx, o, RANGES[rng], pending, lambda: ctx.filter_download(), 0 if pending else 1)


@pytest.mark.parametrize("rng", ["whole", "rounds"])
def test_begun_query_then_exchange(m1, rng):
    """The order of the combined exchange (dist.py): export, begin, import, query."""
    ctx, o = m1
    for lo, hi in RANGES[rng]:
        o.fill_only(lo, hi)
        marks = o.check_only(lo, hi)
        ctx.filter_reset()
        ctx.pass1_insert(lo, hi)
        info = ctx.combine_info(1)
        cap = info["cap_units"]
        payload = torch.zeros(cap * 8, dtype=torch.int16, device="cuda")
        dirs = torch.zeros(info["slices"] * info["windows"], dtype=torch.int64, device="cuda")
        ctx.combine_export(1, payload.data_ptr(), cap, dirs.data_ptr())
        ctx.pass1_query_begin(lo, hi)
        ctx.combine_import(1, 1, payload.data_ptr(), [0], dirs.data_ptr(), info["slices"] * info["windows"])
        fused = ctx.stat("fused_lookups")
        assert ctx.pass1_query(lo, hi) == marks
        assert (ctx.mask_download(False) == o.round_mask).all()
        assert (ctx.filter_download() == o.filter).all()
        assert ctx.stat("query_begun") == 1 and ctx.stat("fused_lookups") == fused + 1


@pytest.mark.parametrize("change", [("slice_bits", 10), ("part_levels", 3)], ids=["slice_bits", "three_levels"])
def test_begun_query_that_cannot_fuse_the_pending_insert(capi, change):
    """The insert deferred its apply under one geometry, the query begins under another (the options change in between): the query
    cannot build the slices in its lookup, applies the insert first -- into the overflow list and cursor the begun batch owns, the
    insert's overflow entries included -- and must then bin its first batch again."""
    ctx, o = _setup(capi, _skewed_records(), 25, 24, 5, 3, 12)
    try:
        o.fill_only()
        marks = o.check_only()
        ctx.filter_reset()
        ctx.pass1_insert()
        assert ctx.stat("insert_overflow_entries") > 0
        ctx.set_option(*change)
        ctx.pass1_query_begin()
        fused = ctx.stat("fused_lookups")
        assert ctx.pass1_query() == marks
        assert (ctx.mask_download(False) == o.round_mask).all()
        assert (ctx.filter_download() == o.filter).all()
        assert ctx.stat("fused_lookups") == fused and ctx.stat("query_begun") == 0
    finally:
        ctx.close()


def test_begun_query_with_overflow_then_filter_download(capi):
    """Both lists in play: the begun batch has query overflow probes, the pending insert has overflow entries.  Materialising the
    insert rewrites the overflow list and cursor the begun batch owns; the query must not read them as its own."""
    ctx, o = _setup(capi, _skewed_records(), 25, 24, 5, 3, 12)
    try:
        o.fill_only()
        marks = o.check_only()
        ctx.filter_reset()
        ctx.pass1_insert()
        assert ctx.stat("insert_overflow_entries") > 0
        ctx.pass1_query_begin()
        assert (ctx.filter_download() == o.filter).all()
        assert ctx.pass1_query() == marks
        assert ctx.stat("query_overflow_entries") > 0 and ctx.stat("query_path") == 2
        assert (ctx.mask_download(False) == o.round_mask).all()
    finally:
        ctx.close()
