"""GPU (-m gpu): the set-bit list reader (csrc/tpc_lists.h: TpcListReader) and the merge of the combined exchange against their
definition in tests/lists_reference.py, through tpc_combine_merge, tpc_combine_import and its three consumers -- k_slice_combine (the
merge, and the dense apply of flush_pending_apply), k_apply_lookup6<false, true> (the fused query with 6-byte entries) and
k_apply_lookup (with 8-byte entries) -- and tpc_filter_copy_out / _in and tpc_combine_choose.  One process, device 0, no
communication library: ranks are replicated contexts, what a collective would move is moved with tensor slicing.  Every comparison
is exact.

a. tpc_combine_merge on synthetic source blocks: list lengths around every edge of the reader's loads, every slice geometry, every
   overlap of the sources, every freedom of the layout, several thousand workgroups per rank, and the "too small" refusal.
b. tpc_combine_import of blocks dealt from the oracle's filter to 1 .. 16 sources per slice, read by each of the three consumers;
   with fresh == 0; and the refusals.
c. one walk of each road of the exchange per world on real exports; tpc_filter_copy_out / _in; tpc_combine_choose."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import lists_cases as C
import lists_reference as R
from oracle import oracle as O
from test_gpu_combine_lists import LETTERS, _random_records, export_and_check

pytestmark = pytest.mark.gpu

PREFILL = 0x5A5A        # of output buffers: whatever the kernel does not own must still hold it afterwards
DECOY = 256             # entries behind an output buffer
SWITCHES = ["shuffle_lists", "gaps", "shuffle_blocks", "unaligned", "shuffle_entries"]
ALL_ON = {s: True for s in SWITCHES}
OPTIONS = (("insert_mode", 2), ("query_mode", 2), ("part_min_tiles", 1))
# The smallest slice the planner accepts for a 2^12-bit filter is 2^6 bits (tpc_qpart_plan: slice_bits >= 6, at least 2 slice
# bits): two words per slice, the non-`wide` copy loops of k_slice_combine.
SMALLEST_SLICE = (12, 6)


@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def dev16(torch, a, tail=R.UNIT):
    """uint16 entries on the device, a unit of sentinels behind them (never an empty buffer)."""
    a = np.concatenate([np.asarray(a, dtype=np.uint16), np.full(tail, R.SENTINEL, dtype=np.uint16)])
    return torch.from_numpy(a.view(np.int16)).cuda()


def dev64(torch, a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64)).cuda() if a.size else torch.zeros(1, dtype=torch.int64, device="cuda")


def dev32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def u16(t):
    return t.cpu().numpy().view(np.uint16)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def new_context(capi, L, slice_bits, recs, rank=0, world=1):
    ctx = capi.Context(0)
    for opt, val in OPTIONS + (("slice_bits", slice_bits),) + ((("replicate_filter", 1),) if world > 1 else ()):
        ctx.set_option(opt, val)
    if world > 1:
        ctx.shard_config(rank, world)
    ctx.set_params(C.K, L, C.Q, capi.seed_table(C.Q, L, seed=C.SEED))
    ctx.seq_upload(capi.PackedText.from_codes(recs))
    return ctx


def export_into(torch, ctx, n_dest):
    info = ctx.combine_info(n_dest)
    assert info["sparse"] == 1, info
    cap = info["cap_units"]
    payload = torch.zeros(n_dest * cap * R.UNIT, dtype=torch.int16, device="cuda")
    dirs = torch.zeros(info["slices"] * info["windows"], dtype=torch.int64, device="cuda")
    units = ctx.combine_export(n_dest, payload.data_ptr(), cap, dirs.data_ptr())
    return info, payload, dirs, units


# ============================================================================================================ a. tpc_combine_merge
class MergeWorld:
    """W replicated contexts over a text of one all-N record: no entries, only the geometry that the export leaves behind."""

    def __init__(self, capi, torch, W, L, slice_bits):
        self.W, self.L, self.ctxs = W, L, []
        for r in range(W):
            ctx = new_context(capi, L, slice_bits, [np.full(100000, 4, dtype=np.uint8)], r, W)
            self.ctxs.append(ctx)
            ctx.filter_reset()
            ctx.pass1_insert()
            info, _, _, units = export_into(torch, ctx, W)
            assert units == [0] * W
        self.geom = R.geometry_of(info, L)
        self.stride = info["dir_entries_per_dest"]

    def layout(self, rank, **switches):
        return R.Layout(self.W, 0, rank=rank, world=self.W, **switches)

    def slices(self, rank):
        return self.layout(rank).block_slices(self.geom, 0)

    def close(self):
        for ctx in self.ctxs:
            ctx.close()


def offsets(rng, wsize, n):
    """n distinct offsets of a window; 65535 only in the full window."""
    return np.arange(wsize) if n == wsize else np.sort(rng.choice(min(wsize, 65535), n, replace=False))


def background(rng, geom, W, slices, fill=0.5, most=40):
    """Random lists of 0 .. most entries for about `fill` of the (source, slice, window) places."""
    cells, wsize = {}, R.window_size(geom)
    for sp in slices:
        for w in range(geom["windows"]):
            for s in range(W):
                if rng.random() < fill:
                    cells[(s, int(sp), w)] = offsets(rng, wsize, int(rng.integers(0, min(most, wsize) + 1)))
    return cells


def merged_lists(cells):
    """(permuted slice, window) -> sorted distinct offsets of all sources."""
    out = {}
    for (_, sp, w), o in cells.items():
        if len(o):
            out.setdefault((sp, w), []).append(np.asarray(o, dtype=np.int64))
    return {k: np.unique(np.concatenate(v)) for k, v in out.items()}


def run_merge(torch, ctx, mw, pay, dirs, base, cap):
    out = torch.full((cap * R.UNIT + DECOY,), PREFILL, dtype=torch.int16, device="cuda")
    mdir = torch.full((mw.stride + 8,), PREFILL, dtype=torch.int64, device="cuda")
    units = ctx.combine_merge(mw.W, pay.data_ptr(), base, dirs.data_ptr(), out.data_ptr(), cap, mdir.data_ptr())
    return units, u16(out), u64(mdir)


def check_merged_block(mw, rank, want, units, out, mdir, expect):
    geom, n_win = mw.geom, mw.geom["windows"]
    need = sum((len(o) + 7) // 8 for o in want.values())
    assert units == need, "units used: without received gaps the kernel packs a slice's lists back to back"
    assert (mdir[mw.stride:] == np.uint64(PREFILL)).all(), "written behind the directory"
    assert (out[units * R.UNIT:] == PREFILL).all(), "written behind the used units"
    sp, win, vals = R.decode_block(out, mdir[:mw.stride], 0, units, geom, mw.slices(rank))
    R.assert_bits_are_filter(R.addresses(geom, sp, win, vals), expect)
    # the directory, entry by entry: the list lengths, 0 for an empty window
    n = np.zeros(mw.stride, dtype=np.int64)
    for (wsp, w), o in want.items():
        n[int(mw.layout(rank).key_of(geom, wsp)) * n_win + w] = len(o)
    assert ((mdir[:mw.stride] & np.uint64(0xFFFFFF)).astype(np.int64) == n).all()


def check_merge(torch, mw, rank, cells, too_small=False, **switches):
    """tpc_combine_merge of rank `rank` over the cells (sources 0 .. W - 1, slices of the rank's buckets) against its definition."""
    ctx, geom = mw.ctxs[rank], mw.geom
    enc = R.encode_blocks(cells, geom, mw.layout(rank, seed=rank + 1, **switches))
    assert enc["dir_stride"] == mw.stride
    pay, dirs = dev16(torch, enc["payload"]), dev64(torch, enc["dirs"])
    pay0, dirs0 = pay.clone(), dirs.clone()
    want = merged_lists(cells)
    expect = R.union_filter(cells, geom, mw.L)
    need = sum((len(o) + 7) // 8 for o in want.values())
    cap = sum(enc["units"])  # "the sum of the received units always suffices"
    assert cap >= need
    units, out, mdir = run_merge(torch, ctx, mw, pay, dirs, enc["src_base"], cap)
    check_merged_block(mw, rank, want, units, out, mdir, expect)
    if too_small and need > 0:
        small = torch.full((need * R.UNIT + DECOY,), PREFILL, dtype=torch.int16, device="cuda")
        mdir2 = torch.full((mw.stride + 8,), PREFILL, dtype=torch.int64, device="cuda")
        with pytest.raises(RuntimeError, match="too small"):
            ctx.combine_merge(mw.W, pay.data_ptr(), enc["src_base"], dirs.data_ptr(), small.data_ptr(), need - 1, mdir2.data_ptr())
        assert (u16(small)[(need - 1) * R.UNIT:] == PREFILL).all(), "written at or beyond out_cap_units"
        assert (u64(mdir2)[mw.stride:] == np.uint64(PREFILL)).all()
        units, out, mdir = run_merge(torch, ctx, mw, pay, dirs, enc["src_base"], need)  # exactly enough; the context is still usable
        check_merged_block(mw, rank, want, units, out, mdir, expect)
    assert torch.equal(pay, pay0) and torch.equal(dirs, dirs0), "the merge wrote to its input"


def forced_lengths(rng, mw, rank):
    """Every length of C.lengths that the window can hold, one per (source, window) cell, W at a time in the same window of a slice
    -- from different sources -- over a background of short random lists."""
    geom, W = mw.geom, mw.W
    wsize, n_win = R.window_size(geom), geom["windows"]
    slices = mw.slices(rank)
    cells = background(rng, geom, W, slices[:24])
    todo = sorted({n for n in C.lengths(n_win, wsize) if n <= wsize})
    for j, n in enumerate(todo + todo[::-1]):  # (twice: every length also meets other neighbours and sources)
        sp, w = int(slices[(j // W) % len(slices)]), (j // W) % n_win
        cells[((j + j // W) % W, sp, w)] = offsets(rng, wsize, n)
    return cells


# (W, L, slice_bits): 1, 4 and 16 windows, a 256-bit window, the smallest slice
MERGE_GEOMETRIES = [(2, 22, 16), (4, 22, 16), (8, 22, 16), (4, 14, 8), (4, 24, 18), (4, 26, 20), (2, 26, 20), (2,) + SMALLEST_SLICE, (8, 14, 6)]


@pytest.mark.parametrize("W,L,slice_bits", MERGE_GEOMETRIES, ids=lambda v: str(v))
def test_merge_list_lengths_and_geometries(capi, torch, W, L, slice_bits):
    mw = MergeWorld(capi, torch, W, L, slice_bits)
    try:
        assert mw.geom["slice_bits"] == slice_bits and mw.geom["windows"] == 1 << max(0, slice_bits - 16)
        for rank in range(W):
            check_merge(torch, mw, rank, forced_lengths(np.random.default_rng(L * 100 + rank), mw, rank), too_small=rank in (0, W - 1))
    finally:
        mw.close()


def overlap_cells(rng, mw, rank, pattern):
    geom, W = mw.geom, mw.W
    slices = mw.slices(rank)
    if pattern == "identical":
        one = background(rng, geom, 1, slices, fill=0.7, most=300)
        return {(s, sp, w): o for (_, sp, w), o in one.items() for s in range(W)}
    if pattern == "disjoint":  # every source its own eighth of the window
        part = R.window_size(geom) // 8
        cells = background(rng, geom, W, slices, fill=0.7, most=300)
        return {(s, sp, w): s * part + np.unique(o % part) for (s, sp, w), o in cells.items()}
    if pattern.startswith("only"):  # one source holds everything, the rest nothing
        one = background(rng, geom, 1, slices, fill=0.7, most=300)
        return {(int(pattern[4:]) % W, sp, w): o for (_, sp, w), o in one.items()}
    cells = background(rng, geom, W, slices, fill=0.7, most=300)  # random overlap: offsets from a narrow range collide
    cells = {k: np.unique(o % 400) for k, o in cells.items()}
    if pattern.startswith("empty"):
        gone = [int(x) for x in pattern[5:].split("_")]
        cells = {k: o for k, o in cells.items() if k[0] not in gone}
    return cells


@pytest.mark.parametrize("pattern", ["identical", "disjoint", "random", "only0", "only5", "empty0", "empty2", "empty7", "empty3_4", "empty0_1_2_3"])
def test_merge_overlap_of_the_sources(capi, torch, pattern):
    mw = MergeWorld(capi, torch, 8, 22, 16)
    try:
        for rank in (0, 5):
            check_merge(torch, mw, rank, overlap_cells(np.random.default_rng(len(pattern) + rank), mw, rank, pattern), too_small=True)
    finally:
        mw.close()


@pytest.mark.parametrize("L,slice_bits", [(22, 16), (26, 20)])
@pytest.mark.parametrize("switches", [(s,) for s in SWITCHES] + [tuple(SWITCHES)], ids=lambda s: "+".join(s))
def test_merge_does_not_depend_on_the_layout(capi, torch, switches, L, slice_bits):
    mw = MergeWorld(capi, torch, 4, L, slice_bits)
    try:
        for rank in (1, 3):
            check_merge(torch, mw, rank, forced_lengths(np.random.default_rng(rank), mw, rank), **{s: True for s in switches})
    finally:
        mw.close()


def test_merge_of_16384_slices(capi, torch):
    """L = 30, slice_bits = 16: a rank's share of the grid is 8192 workgroups; sparse lists, the first and the last slice among them."""
    mw = MergeWorld(capi, torch, 2, 30, 16)
    try:
        assert mw.geom["slices"] == 16384
        for rank in range(2):
            rng = np.random.default_rng(rank)
            slices = mw.slices(rank)
            some = np.concatenate([slices[:2], rng.choice(slices, 400, replace=False), slices[-2:]])
            check_merge(torch, mw, rank, background(rng, mw.geom, 2, np.unique(some), fill=0.6, most=60), too_small=rank == 1, **ALL_ON)
    finally:
        mw.close()


# ============================================================================================== b. tpc_combine_import, three consumers
@pytest.fixture(scope="module")
def texts(capi, torch):
    """name -> the text's context (not sharded), oracle, and the geometry its export establishes.  The exported lists are decoded
    once and are the oracle's filter (export_and_check); from then on the blocks come from split_bits + encode_blocks."""
    made = {}

    def get(name):
        if name not in made:
            L, slice_bits, _ = C.TEXTS[name]
            o = C.oracle_for(name)
            o.fill_only()
            ctx = new_context(capi, L, slice_bits, C.records(name))
            ctx.filter_reset()
            ctx.pass1_insert()
            info, _, _ = export_and_check(ctx, o, 1, L)
            made[name] = SimpleNamespace(name=name, ctx=ctx, o=o, L=L, filter=o.filter, marks=o.check_only(), mask=o.round_mask, info=info,
                                         geom=R.geometry_of(info, L), blocks={})
        return made[name]

    yield get
    for t in made.values():
        t.ctx.close()
        t.o.close()


def begin_round(torch, t, before=None):
    """The round up to the import: (reset or upload), insert, export -- whose lists are dropped."""
    if before is None:
        t.ctx.filter_reset()
    else:
        t.ctx.filter_upload(before)
    t.ctx.pass1_insert()
    export_into(torch, t.ctx, 1)


def blocks_of(torch, t, pair, lists_filter=None, tag=""):
    """Device blocks (kept per text, source counts and tag) whose union is lists_filter (default: the oracle's filter), dealt to the
    sources with duplicates and the forced lengths, every layout switch on."""
    key = pair + (tag,)
    if key not in t.blocks:
        f = t.filter if lists_filter is None else lists_filter
        n_src, n_owner = pair
        rng = np.random.default_rng(n_src * 31 + n_owner)
        cells = R.split_bits(f, t.geom, n_src, n_owner, rng, C.forced_cells(f, t.geom, n_src, n_owner))
        enc = R.encode_blocks(cells, t.geom, R.Layout(n_src, n_owner, seed=n_src, **ALL_ON))
        t.blocks[key] = (dev16(torch, enc["payload"]), dev64(torch, enc["dirs"]), enc["src_base"], enc["dir_stride"])
    return t.blocks[key]


def import_blocks(t, pair, blocks):
    pay, dirs, base, stride = blocks
    t.ctx.combine_import(pair[0], pair[1], pay.data_ptr(), base, dirs.data_ptr(), stride)


def check_dense_apply(t, expect=None):
    """filter_download at once: flush_pending_apply runs k_slice_combine with dense = true, no lookup rides along."""
    ctx = t.ctx
    fused = ctx.stat("fused_lookups")
    assert (ctx.filter_download() == (t.filter if expect is None else expect)).all()
    if expect is None:
        assert ctx.pass1_query() == t.marks
        assert (ctx.mask_download(False) == t.mask).all()
    assert ctx.stat("fused_lookups") == fused


def check_fused(t, fmt6):
    ctx = t.ctx
    fused = ctx.stat("fused_lookups")
    assert ctx.pass1_query() == t.marks
    assert ctx.stat("fused_lookups") == fused + 1  # (this query's lookup built the slices from the lists)
    assert (ctx.stat("query_entry_fmt") == 6) == fmt6, "the other lookup kernel ran"
    assert (ctx.mask_download(False) == t.mask).all()
    assert (ctx.filter_download() == t.filter).all()


def cases(table):
    return [pytest.param(name, pair, id="%s-%d-%d" % ((name,) + pair)) for name, pairs in table for pair in pairs]


DENSE_APPLY = [("dense8", C.PAIRS), ("sparse6", C.PAIRS), ("dense6", C.FEW_PAIRS), ("dense6_4win", C.FEW_PAIRS), ("dense8_16win", C.FEW_PAIRS),
               ("small6", C.FEW_PAIRS), ("skewed6", [(5, 1)])]


@pytest.mark.parametrize("name,pair", cases(DENSE_APPLY))
def test_import_dense_apply(torch, texts, name, pair):
    t = texts(name)
    begin_round(torch, t)
    import_blocks(t, pair, blocks_of(torch, t, pair))
    check_dense_apply(t)


@pytest.mark.parametrize("name,pair", cases(C.FMT6))
def test_import_fused_lookup_6_byte_entries(torch, texts, name, pair):
    t = texts(name)
    begin_round(torch, t)
    import_blocks(t, pair, blocks_of(torch, t, pair))
    check_fused(t, True)


@pytest.mark.parametrize("name,pair", cases(C.FMT8))
def test_import_fused_lookup_8_byte_entries(torch, texts, name, pair):
    """L - slice_bits = 6 slice bits: b2 = 3 < 4, the planner keeps the 8-byte entries."""
    t = texts(name)
    begin_round(torch, t)
    import_blocks(t, pair, blocks_of(torch, t, pair))
    check_fused(t, False)


def stale_round(torch, t, pair, tag):
    """fresh == 0: the filter holds a random subset X of the oracle's bits before the round (uploaded, no reset); the lists hold the
    oracle's bits outside X and a random part of X."""
    rng = np.random.default_rng(pair[0])
    rand = lambda: rng.integers(0, 1 << 32, t.filter.size, dtype=np.uint64).astype(np.uint32)  # noqa: E731
    X = t.filter & rand()
    lists = (t.filter & ~X) | (X & rand() & rand())
    assert (X | lists == t.filter).all() and (X & lists).any() and (X & ~lists).any()
    begin_round(torch, t, before=X)
    import_blocks(t, pair, blocks_of(torch, t, pair, lists, tag))


@pytest.mark.parametrize("pair", C.STALE_PAIRS, ids=str)
@pytest.mark.parametrize("name", ["dense8", "dense6"])
def test_import_into_a_filter_that_holds_bits_dense_apply(torch, texts, name, pair):
    t = texts(name)
    stale_round(torch, t, pair, "stale")
    check_dense_apply(t)
    # and with bits that the lists and the oracle do not hold: the old slice is ORed, not replaced
    rng = np.random.default_rng(7)
    Y = rng.integers(0, 1 << 32, t.filter.size, dtype=np.uint64).astype(np.uint32) & rng.integers(0, 1 << 32, t.filter.size, dtype=np.uint64).astype(np.uint32)
    Y[-1] = 0  # (the spare word)
    assert (Y & ~t.filter).any()
    begin_round(torch, t, before=Y)
    import_blocks(t, pair, blocks_of(torch, t, pair))
    check_dense_apply(t, expect=Y | t.filter)


@pytest.mark.parametrize("pair", C.STALE_PAIRS, ids=str)
@pytest.mark.parametrize("name,fmt6", [("dense6", True), ("sparse6", True), ("dense8", False), ("dense8_16win", False)])
def test_import_into_a_filter_that_holds_bits_fused(torch, texts, name, fmt6, pair):
    t = texts(name)
    stale_round(torch, t, pair, "stale")
    check_fused(t, fmt6)


def test_import_and_merge_refusals(capi, torch, texts):
    """Error returns before any kernel: each fails with a message, and the context then answers a correct import."""
    t = texts("sparse8")
    assert t.geom["b1"] == 3
    begin_round(torch, t)
    pay, dirs, _, stride = blocks_of(torch, t, (1, 0))
    bad = [(0, 0), (4097, 0), (3, 3), (6, 4), (16, 16)]  # no source, too many, n_owner no power of two, not dividing n_src, beyond 2^b1
    for n_src, n_owner in bad:
        with pytest.raises(RuntimeError, match="bad arguments"):
            t.ctx.combine_import(n_src, n_owner, pay.data_ptr(), [0] * n_src, dirs.data_ptr(), stride)
    with pytest.raises(RuntimeError, match="replicated"):  # merge on a context that is not replicated
        t.ctx.combine_merge(1, pay.data_ptr(), [0], dirs.data_ptr(), pay.data_ptr(), 1, dirs.data_ptr())
    import_blocks(t, (5, 1), blocks_of(torch, t, (5, 1)))
    check_dense_apply(t)
    # before any export
    ctx = new_context(capi, t.L, 16, C.records("sparse8"))
    try:
        with pytest.raises(RuntimeError, match="tpc_combine_export first"):
            ctx.combine_import(1, 0, pay.data_ptr(), [0], dirs.data_ptr(), stride)
    finally:
        ctx.close()
    mw = MergeWorld(capi, torch, 4, 22, 16)
    try:
        fresh = new_context(capi, 22, 16, [np.full(100000, 4, dtype=np.uint8)], 1, 4)
        try:
            with pytest.raises(RuntimeError, match="tpc_combine_export first"):
                run_merge(torch, fresh, mw, pay, dirs, [0] * 4, 8)
        finally:
            fresh.close()
        empty = R.encode_blocks({}, mw.geom, mw.layout(2))
        e_pay, e_dirs = dev16(torch, empty["payload"]), dev64(torch, empty["dirs"])
        for n_src in (2, 8):  # not one block per rank
            out = torch.full((64,), PREFILL, dtype=torch.int16, device="cuda")
            with pytest.raises(RuntimeError, match="one source block per rank"):
                mw.ctxs[2].combine_merge(n_src, e_pay.data_ptr(), [0] * n_src, e_dirs.data_ptr(), out.data_ptr(), 8, e_dirs.data_ptr())
        check_merge(torch, mw, 2, forced_lengths(np.random.default_rng(3), mw, 2))
    finally:
        mw.close()


# ================================================================================================ c. the roads, on real exports
def decode_dest_block(geom, W, payload, dirs, d, cap, used, stride):
    """Entries of block d of an export with n_dest = W."""
    return R.decode_block(payload, dirs[d * stride:(d + 1) * stride], d * cap, used, geom, R.Layout(W, W).block_slices(geom, d))


def walk(capi, torch, W, L, slice_bits, n_pos, roads):
    recs = _random_records(n_pos, seed=L + W)
    o = O.Oracle(C.K, L, C.Q, O.seed_table(C.SEED, C.Q, L))
    ctxs = []
    try:
        for r in recs:
            o.add_record(LETTERS[r].tobytes())
        o.fill_only()
        marks, filt, mask = o.check_only(), o.filter, o.round_mask
        ctxs = [new_context(capi, L, slice_bits, recs, r, W) for r in range(W)]
        for road in roads:
            ex = []
            for ctx in ctxs:
                ctx.filter_reset()
                ctx.pass1_insert()
                assert ctx.stat("insert_batches") == 1
                ex.append(export_into(torch, ctx, W))
            info = ex[0][0]
            geom, stride = R.geometry_of(info, L), info["dir_entries_per_dest"]
            assert all(e[0]["dir_entries_per_dest"] == stride and e[0]["slices"] == info["slices"] for e in ex)
            keep = []  # the buffers stay untouched until the query ran
            if road == "scatter":
                merged, mdirs, munits = [], [], []
                for d, ctx in enumerate(ctxs):  # block d of every rank to rank d; rank d merges
                    parts, base, at, src_addr = [], [], 0, []
                    for info_r, pay_r, dirs_r, units_r in ex:
                        cap = info_r["cap_units"]
                        parts.append(pay_r[d * cap * R.UNIT:(d * cap + units_r[d]) * R.UNIT])
                        base.append(at)
                        at += units_r[d]
                        src_addr.append(R.addresses(geom, *decode_dest_block(geom, W, u16(pay_r), u64(dirs_r), d, cap, units_r[d], stride)))
                    recv = torch.cat(parts + [torch.full((R.UNIT,), -1, dtype=torch.int16, device="cuda")])
                    rdir = torch.cat([dirs_r[d * stride:(d + 1) * stride] for _, _, dirs_r, _ in ex])
                    out = torch.full((max(at, 1) * R.UNIT + DECOY,), PREFILL, dtype=torch.int16, device="cuda")
                    mdir = torch.full((stride + 8,), PREFILL, dtype=torch.int64, device="cuda")
                    mu = ctx.combine_merge(W, recv.data_ptr(), base, rdir.data_ptr(), out.data_ptr(), at, mdir.data_ptr())
                    # the merged block, as in part a: the union of the W received blocks, every bit once, packed
                    expect = R.words_of(np.concatenate(src_addr), L)
                    h_out, h_dir = u16(out), u64(mdir)
                    sp, win, vals = R.decode_block(h_out, h_dir[:stride], 0, mu, geom, R.Layout(W, W).block_slices(geom, d))
                    R.assert_bits_are_filter(R.addresses(geom, sp, win, vals), expect)
                    assert mu == int((((h_dir[:stride] & np.uint64(0xFFFFFF)).astype(np.int64) + 7) // 8).sum())
                    assert (h_out[mu * R.UNIT:] == PREFILL).all() and (h_dir[stride:] == np.uint64(PREFILL)).all()
                    merged.append(out)
                    mdirs.append(mdir[:stride])
                    munits.append(mu)
                most = max(max(munits), 1)
                allp = torch.cat([m[:most * R.UNIT] if m.numel() >= most * R.UNIT else torch.cat([m, m.new_zeros(most * R.UNIT - m.numel())]) for m in merged])
                alld = torch.cat(mdirs)
                keep = [allp, alld]
                for ctx in ctxs:
                    ctx.combine_import(W, W, allp.data_ptr(), [r * most for r in range(W)], alld.data_ptr(), stride)
            elif road == "gather":  # all W x W export blocks, rank-major, used prefixes back to back
                most = max(max(sum(e[3]) for e in ex), 1)
                rows, base = [], []
                for r, (info_r, pay_r, dirs_r, units_r) in enumerate(ex):
                    cap, at = info_r["cap_units"], r * most
                    row = [pay_r[d * cap * R.UNIT:(d * cap + units_r[d]) * R.UNIT] for d in range(W)]
                    for d in range(W):
                        base.append(at)
                        at += units_r[d]
                    rows.append(torch.cat(row + [pay_r.new_full(((most - sum(units_r)) * R.UNIT,), -1)]))
                allp, alld = torch.cat(rows), torch.cat([e[2] for e in ex])
                keep = [allp, alld]
                for ctx in ctxs:
                    ctx.combine_import(W * W, W, allp.data_ptr(), base, alld.data_ptr(), stride)
            else:  # dense: every rank takes its own lists back, then the OR all-reduce over word ranges
                words = ctxs[0].filter_words() - 1
                chunk = words // W
                mine = []
                for ctx, (info_r, pay_r, dirs_r, _) in zip(ctxs, ex):
                    ctx.combine_import(W, W, pay_r.data_ptr(), [d * info_r["cap_units"] for d in range(W)], dirs_r.data_ptr(), stride)
                    buf = torch.zeros(words, dtype=torch.int32, device="cuda")
                    ctx.filter_copy_out(0, words, buf.data_ptr())  # (applies the imported lists)
                    mine.append(buf)
                folded = []
                for d, ctx in enumerate(ctxs):
                    parts = torch.stack([m[d * chunk:(d + 1) * chunk] for m in mine]).contiguous()
                    out = torch.zeros(chunk, dtype=torch.int32, device="cuda")
                    ctx.mask_or_blocks(parts.data_ptr(), W, chunk, out.data_ptr())
                    folded.append(out)
                allm = torch.cat(folded)
                for ctx in ctxs:
                    ctx.filter_copy_in(0, words, allm.data_ptr())
            got_marks, got_mask = 0, np.zeros_like(mask)
            for ctx in ctxs:
                fused = ctx.stat("fused_lookups")
                got_marks += ctx.pass1_query()
                assert ctx.stat("fused_lookups") == fused + (road != "dense")
                got_mask |= ctx.mask_download(False)
                assert (ctx.filter_download() == filt).all(), (road, W)
            assert got_marks == marks and (got_mask == mask).all(), (road, W)
            del keep
    finally:
        for ctx in ctxs:
            ctx.close()
        o.close()


@pytest.mark.parametrize("W", [2, 4, 8])
def test_every_road_of_the_exchange(capi, torch, W):
    walk(capi, torch, W, 24, 16, 400000, ["scatter", "gather", "dense"])


def test_scatter_road_at_16384_slices(capi, torch):
    """The exports come from the long-lived k_slice_export_p with its chunked placement: unused units between the lists."""
    walk(capi, torch, 2, 30, 16, 400000, ["scatter"])


def test_filter_copy_out_and_in(capi, torch, texts):
    t = texts("sparse8")
    ctx, words = t.ctx, t.ctx.filter_words()
    assert words == t.filter.size == (1 << (t.L - 5)) + 1
    slice_words = 1 << (t.geom["slice_bits"] - 5)

    def copy_out(word0, n):
        buf = torch.full((n + 4,), PREFILL, dtype=torch.int32, device="cuda")
        ctx.filter_copy_out(word0, n, buf.data_ptr())
        h = u32(buf)
        assert (h[n:] == PREFILL).all()
        return h[:n]

    begin_round(torch, t)
    import_blocks(t, (5, 1), blocks_of(torch, t, (5, 1)))
    fused = ctx.stat("fused_lookups")
    assert (copy_out(0, words) == t.filter).all(), "imported lists pending: copy_out applies them"
    assert ctx.stat("fused_lookups") == fused
    for word0, n in [(0, 100), (words - 100, 100), (slice_words - 7, 20), (3 * slice_words - 1, 2), (5, 0), (words, 0)]:
        assert (copy_out(word0, n) == t.filter[word0:word0 + n]).all(), (word0, n)
    ctx.filter_copy_out(0, 0, 0)
    buf = torch.zeros(8, dtype=torch.int32, device="cuda")
    for word0, n in [(words - 3, 4), (words + 1, 0), (0, words + 1)]:
        with pytest.raises(RuntimeError, match="bad arguments"):
            ctx.filter_copy_out(word0, n, buf.data_ptr())
        with pytest.raises(RuntimeError, match="bad arguments"):
            ctx.filter_copy_in(word0, n, buf.data_ptr())
    ctx.filter_reset()  # a reset pending
    assert not copy_out(0, words).any()
    ctx.filter_reset()
    ctx.pass1_insert()  # an insert pending in its regions
    assert ctx.combine_info(1)["sparse"] == 1
    assert (copy_out(slice_words - 7, 20) == t.filter[slice_words - 7:slice_words + 13]).all()
    assert (ctx.filter_download() == t.filter).all()
    # copy_in, then the download returns what was copied in
    rng = np.random.default_rng(2)
    want = t.filter.copy()
    for word0, n in [(0, 50), (slice_words - 7, 20), (words - 9, 9), (17, 0)]:
        new = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        src = dev32(torch, new) if n else buf
        ctx.filter_copy_in(word0, n, src.data_ptr())
        want[word0:word0 + n] = new
        assert (ctx.filter_download() == want).all(), (word0, n)
    ctx.filter_reset()  # copy_in with a reset pending: zeros around what was copied in
    new = rng.integers(0, 1 << 32, 64, dtype=np.uint64).astype(np.uint32)
    ctx.filter_copy_in(1000, 64, dev32(torch, new).data_ptr())
    want = np.zeros_like(t.filter)
    want[1000:1064] = new
    assert (ctx.filter_download() == want).all()


@pytest.mark.parametrize("W,L,units", [(2, 30, 1 << 20), (2, 36, 5000000), (4, 36, 5000000), (8, 36, 5000000), (8, 30, 12345), (8, 24, 1 << 22), (64, 38, 1),
                                       (4, 20, 0), (2, 10, 8)])
def test_combine_choose_is_its_formulas(capi, W, L, units):
    """The three byte counts of the comment of tpc_combine_choose, and the first smallest of them as the road.  (2, 10, 8): the
    all-gather's (W - 1) D = 128 bytes tie with the dense road's 2 (W - 1) / W 2^L / 8 = 128; the first wins."""
    D = 16.0 * units
    U = D * min(float(W), math.pow(W, 0.3))
    want = [(W - 1.0) * D, (W - 1.0) / W * (D + U), 2.0 * (W - 1.0) / W * math.ldexp(1.0, L - 3)]
    mode, got = capi.combine_choose(W, L, units)
    assert got == want
    assert mode == 1 + want.index(min(want))
    if (W, L, units) == (2, 10, 8):
        assert want[0] == want[2] == 128.0 and mode == 1
    assert capi.combine_choose(1, L, units)[0] == 1 and capi.combine_choose(0, L, units)[0] == 1
