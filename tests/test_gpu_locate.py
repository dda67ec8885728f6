"""GPU (-m gpu): the edge index and locate (csrc/tpc_locate.hip) through the C-ABI -- hit[], row[], the five run arrays, the four
per-record sums, shared[][] and both info[] -- element for element against locate_reference.py, the definition over
graph_table.event_table with dicts of canonical strings: on golden vectors from a host stream and a resident stream with the index
numbers the oracle's definition gives (locate_reference.RECORDED), with fetch windows down to one element and every bad range; and on
GENERATED inputs, hand-made streams over random texts (the text does not have to be consistent with the ids: every event is a row of its own), sized where the kernels can go wrong
and no larger: query texts of 8 191, 8 192, 8 193 and 2 x 8 192 + 1 positions (the tile is 256 x 32), a run across a tile boundary
and across a thread's 32-position boundary, test_locate_grid = 1 and 3, k = 3, 31, 33, 63 (windows of 1 to 3 packed words, n = 32
exactly and one past it), the largest k the tile halo admits and one beyond it refused, edge_k5's failed walk refused, test_edges_hash_bits = 4 (every home slot
shared: only the letters decide), a nearly full forced table and a full one refused, an event table of tests/graph_walks.py whose
spans repeat keys in the thousands, 1, 2, 33 and 65 colours and a colour map that is not monotone, no colour table, a colour build
after the edge build, every refusal's text, the other stages' arrays before and behind an edge build and two locates, and the bytes
of `graphdump --locate --gpu` and `twopaco --locate`, alone and beside --colors, against the serial program's and the oracle's.

Not tested: the refusal of buffers beyond the free device memory.  The stage's buffers grow with the text (below 2^40 positions) and
the query (below 2^32), which a device of this size holds at any size a test could build: no small input reaches the refusal.  Nor
is the refusal of a windowed text (a sharded context's, which no segment build accepts either).  The programs' batches are tested
through TWOPACO_LOCATE_BATCH, which makes graphdump cut a small query into many; twopaco's cut at 2^28 positions runs the same code, once."""
import json
import os
import subprocess

import numpy as np
import pytest

import colors_reference as C
import graph_table
import graph_walks as G
import locate_reference as R
import segments_reference as SR
from helpers import GOLDEN, golden_cases

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in golden_cases()}
MAXU = (1 << 64) - 1
GOLDEN_NAMES = ["rand6_k3", "rand6_k9_fp", "tr_k11_L28_r2", "c2_k29", "rand6_k9_a3"]      # and edge_k5, whose walk fails: test_a_failed_walk_is_refused
TILE = 8192
HALO_K = 670           # (TPC_XW_MAX - 1) * 32 - 2 of csrc/tpc_device.h: k + 1 letters fit the 22 halo words of a tile


@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


def codes_of(s):
    lut = np.full(256, 4, dtype=np.uint8)
    lut[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.arange(4, dtype=np.uint8)
    return lut[np.frombuffer(s.upper().encode(), dtype=np.uint8)]


def packed(capi, records):
    return capi.PackedText.from_codes([codes_of(r) for r in records])


def ambiguous_positions(seqs, rec_start):
    return [int(rec_start[r]) + i for r, s in enumerate(seqs) for i, ch in enumerate(s) if ch not in "ACGTN"]


def host_context(capi, seqs, data, k):
    text = packed(capi, seqs)
    ctx = capi.Context(0)
    ctx.seq_upload(text)
    ctx.segments_build(data, k, text.rec_start, text.rec_length)
    return ctx


def resident_context(capi, case, fasta, data):
    """The whole path in this process up to tpc_emit_stream, the table from the device's own copy of the stream."""
    text = capi.PackedText.from_fasta([fasta])
    ctx = capi.Context(0)
    ctx.set_params(case["k"], case["L"], case["q"], capi.seed_table(case["q"], case["L"], seed=case["seed"]))
    ctx.seq_upload(text)
    for st in case["rounds"]:
        ctx.filter_reset()
        ctx.pass1_insert(st["low"], st["high"])
        ctx.pass1_query(st["low"], st["high"])
        ctx.pass2_filter(MAXU if case["abundance"] is None else case["abundance"])
    ctx.junctions_finalize()
    ctx.emit()
    stream, _ = ctx.emit_stream(text.rec_start, text.rec_length)
    assert stream == data
    seqs = graph_table.read_fasta(fasta)
    ctx.segments_build(None, case["k"], text.rec_start, text.rec_length, ambiguous_positions(seqs, text.rec_start))
    return ctx


def check_index(ctx, index, **forced):
    info = ctx.segments_edges_build()
    entries, duplicates, skipped = index.counts()
    assert (info["entries"], info["duplicates"], info["skipped"]) == (entries, duplicates, skipped)
    slots = info["slots"]
    assert slots & (slots - 1) == 0 and (forced or slots >= 2 * (entries + duplicates)) and info["longest_probe"] < slots
    assert info["peak_bytes"] >= 16 * slots + 8 * index.n_rows
    assert ctx.kernel_ms("locate") > 0
    return info


def check_located(capi, ctx, index, records, colored):
    """Everything the device holds after a locate == the oracle's arrays; returns the oracle's."""
    want = index.locate(records)
    info = ctx.segments_locate(packed(capi, records))
    peak = info.pop("peak_bytes")
    assert info == dict(want.info, colors=index.n_colors if colored else 0)
    assert peak >= 12 * want.positions + 20 * want.info["runs"] + 32 * len(records)
    hit, row = ctx.segments_locate_fetch_hits()
    assert hit.dtype == np.uint64 and hit.size == want.positions and (hit == want.hit).all()
    assert row.dtype == np.uint32 and row.size == want.positions and (row == want.row).all()
    for got, ref in zip(ctx.segments_locate_fetch_runs(), want.runs):
        assert got.dtype == np.uint32 and got.size == ref.size and (got == ref).all()
    for got, ref in zip(ctx.segments_locate_fetch_records(0, len(records)), want.sums):
        assert got.dtype == np.uint64 and (got == ref).all()
    if colored:
        got = ctx.segments_locate_fetch_shared(0, len(records))
        assert got.shape == want.shared.shape and (got == want.shared).all()
    else:
        with pytest.raises(RuntimeError, match="segment locate: no colour table was valid at the time of the locate"):
            ctx.segments_locate_fetch_shared(0, len(records))
    assert ctx.kernel_ms("locate") > 0 and ctx.segments_error() is None
    return want


def mutated(rng, s, every):
    """s with a substitution every `every` letters."""
    a = bytearray(s.encode())
    for i in range(every // 2, len(a), every):
        a[i] = ord("ACGT"[("ACGT".index(chr(a[i])) + 1 + int(rng.integers(0, 3))) % 4]) if chr(a[i]) in "ACGT" else a[i]
    return a.decode()


def golden_queries(seqs, k, seed):
    """The genomes themselves, a reverse complement, short runs, unrelated letters, records below k + 1, an empty one, all N, poly-A."""
    rng = np.random.default_rng(seed)
    clean = "".join(ch if ch in "ACGT" else "N" for ch in seqs[0])
    return list(seqs) + [R.revcomp(clean.replace("N", "A")), mutated(rng, seqs[-1], 2 * k), "".join("ACGT"[i] for i in rng.integers(0, 4, 300)), "ACGT"[:min(k, 4)], "",
                         "N" * (k + 5), "A" * (3 * k + 40)]


# ------------------------------------------------------------------------------------------------ 1. golden vectors
@pytest.mark.parametrize("source", ["host", "resident"])
@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_golden_arrays_equal_the_oracle(capi, name, source):
    case = CASES[name]
    fasta = os.path.join(GOLDEN, case["fasta"])
    data = open(os.path.join(GOLDEN, case["bin"]), "rb").read()
    index, seqs = R.golden_index(case, GOLDEN, "sequence")
    assert index.counts() == R.RECORDED[name]
    if source == "host":
        text = capi.PackedText.from_fasta([fasta])
        ctx = capi.Context(0)
        ctx.seq_upload(text)
        ctx.segments_build(data, case["k"], text.rec_start, text.rec_length, ambiguous_positions(seqs, text.rec_start))
    else:
        ctx = resident_context(capi, case, fasta, data)
    try:
        assert ctx.segments_error() is None
        ctx.segments_colors_build(list(range(len(seqs))), len(seqs))
        check_index(ctx, index)
        own = check_located(capi, ctx, index, seqs, True)
        if case["abundance"] is None:
            assert (own.sums[1] == own.sums[0]).all() and own.info["windows"] > 0      # every edge of an input is in the graph
        else:
            assert own.info["found"] < own.info["windows"]
        other = check_located(capi, ctx, index, golden_queries(seqs, case["k"], 7), True)
        assert other.info["runs"] > 0 and (other.sums[0][-4:-1] == 0).all()
    finally:
        ctx.close()


def test_fetch_windows_down_to_one_element_and_bad_ranges(capi):
    case = CASES["rand6_k9_fp"]
    index, seqs = R.golden_index(case, GOLDEN, "sequence")
    data = open(os.path.join(GOLDEN, case["bin"]), "rb").read()
    ctx = host_context(capi, seqs, data, case["k"])
    try:
        ctx.segments_colors_build(list(range(len(seqs))), len(seqs))
        ctx.segments_edges_build()
        want = index.locate(seqs)
        ctx.segments_locate(packed(capi, seqs))
        n, b, s = want.positions, want.info["runs"], len(seqs)
        for p0, m in ((0, 1), (n - 1, 1), (n // 2, 1), (63, 130), (n, 0)):
            hit, row = ctx.segments_locate_fetch_hits(p0, m)
            assert (hit == want.hit[p0:p0 + m]).all() and (row == want.row[p0:p0 + m]).all()
        for r0, m in ((0, 1), (b - 1, 1), (b // 2, 1), (3, 17), (b, 0)):
            for got, ref in zip(ctx.segments_locate_fetch_runs(r0, m), want.runs):
                assert got.size == m and (got == ref[r0:r0 + m]).all()
        for s0, m in ((0, 1), (s - 1, 1), (1, 3), (s, 0)):
            for got, ref in zip(ctx.segments_locate_fetch_records(s0, m), want.sums):
                assert (got == ref[s0:s0 + m]).all()
            assert (ctx.segments_locate_fetch_shared(s0, m) == want.shared[s0:s0 + m]).all()
        for p0, m in ((n, 1), (n + 1, 0), (0, n + 1), (MAXU, 2)):
            with pytest.raises(RuntimeError, match="segment locate: bad position range"):
                ctx.segments_locate_fetch_hits(p0, m)
        for r0, m in ((b, 1), (b + 1, 0), (0, b + 1), (MAXU, 2)):
            with pytest.raises(RuntimeError, match="segment locate: bad run range"):
                ctx.segments_locate_fetch_runs(r0, m)
        for s0, m in ((s, 1), (s + 1, 0), (0, s + 1), (MAXU, 2)):
            with pytest.raises(RuntimeError, match="segment locate: bad record range"):
                ctx.segments_locate_fetch_records(s0, m)
            with pytest.raises(RuntimeError, match="segment locate: bad record range"):
                ctx.segments_locate_fetch_shared(s0, m)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 2. generated inputs
def letters(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


class Made:
    """A hand-made graph at any k: records of random letters, the later ones holding copies and reverse complements of the first (so
    keys repeat at larger g), one event between every two junction positions, every id of its own: every event is a row."""

    def __init__(self, k, seed, n_colors=0, color_of_seq=None, length=1500):
        rng = np.random.default_rng(seed)
        base = letters(rng, length)
        cut = min(length, 2 * k + 200)
        self.k, self.seqs = k, [base, letters(rng, 40) + base[100:100 + cut] + letters(rng, 30), R.revcomp(base[300:300 + cut]) + "N" + letters(rng, k + 60), letters(rng, k + 90)]
        sequences, ident = [], 1
        for s in self.seqs:
            last = len(s) - k
            pos = sorted(set([0, 5, min(last, 700), min(last, 707)] + list(range(0, last, 311)) + [last]))
            sequences.append((np.array(pos, dtype=np.int64), np.arange(ident, ident + len(pos), dtype=np.int64)))
            ident += len(pos)
        self.data = SR.build_stream(sequences, last_separator=True)
        self.color_of_seq = color_of_seq
        self.index = R.Index(graph_table.event_table(self.data, self.seqs, k), self.seqs, k, color_of_seq, n_colors)

    def context(self, capi):
        ctx = host_context(capi, self.seqs, self.data, self.k)
        assert ctx.segments_error() is None and ctx.segments_counts()["segments"] == self.index.n_rows
        if self.index.n_colors:
            ctx.segments_colors_build(self.color_of_seq, self.index.n_colors)
        return ctx

    def query_of(self, rng, total):
        """Records whose packed text has `total` positions: a copy of the first record lies across position 8192 when the text reaches it."""
        k, base = self.k, self.seqs[0]
        recs = [letters(rng, 50), base[20:20 + 3 * k + 100], R.revcomp(base[400:400 + 2 * k + 150]), "", mutated(rng, base[600:600 + 6 * k + 60], 2 * k), "AC"]
        used = 1 + sum(len(r) + 1 for r in recs)
        copy = min(len(base), 1200)
        if total >= TILE + 800 and used < TILE - 450:   # the long copy begins 443 positions before the tile's end: its span [311, 622) lies across it
            pad = TILE - 443 - used - 1
            recs += [letters(rng, pad), base[:copy]]
            used += pad + 1 + copy + 1
        recs.append(letters(rng, total - used - 1))
        assert 1 + sum(len(r) + 1 for r in recs) == total
        return recs


@pytest.mark.parametrize("total,grid", [(TILE - 1, 0), (TILE, 0), (TILE + 1, 0), (2 * TILE + 1, 0), (2 * TILE + 1, 1), (2 * TILE + 1, 3)])
@pytest.mark.parametrize("k", [3, 31, 33, 63])
def test_generated_texts_around_the_tile(capi, k, total, grid):
    made = Made(k, 100 + k, n_colors=3, color_of_seq=[0, 1, 2, 1])
    assert made.index.duplicates > 100
    ctx = made.context(capi)
    try:
        ctx.set_option("test_locate_grid", grid)
        check_index(ctx, made.index)
        want = check_located(capi, ctx, made.index, made.query_of(np.random.default_rng(k + total), total), True)
        assert want.positions == total - k
        if total >= TILE + 800 and k > 3:           # (136 canonical 4-mers: at k = 3 every hit lies at its key's smallest g, no run is long)
            q_first, length = want.runs[0].astype(np.int64), want.runs[1].astype(np.int64)
            across = (q_first < TILE) & (q_first + length > TILE + 64)
            assert across.any() and (q_first[across] % 32 != 0).all()
        assert want.runs[3].any() and not want.runs[3].all() and (k == 3 or want.info["found"] < want.info["windows"])
    finally:
        ctx.close()


def test_the_largest_k_of_the_halo_and_one_beyond(capi):
    made = Made(HALO_K, 5, length=2600)
    ctx = made.context(capi)
    try:
        check_index(ctx, made.index)
        want = check_located(capi, ctx, made.index, made.query_of(np.random.default_rng(6), 2 * TILE + 1), False)
        assert want.info["found"] > 0 and want.info["runs"] > 3
    finally:
        ctx.close()
    beyond = Made(HALO_K + 1, 5, length=2600)
    ctx = beyond.context(capi)
    try:
        with pytest.raises(RuntimeError, match=r"segment edges: k=671 is too large: a window of k \+ 1 letters must fit the 22 halo words of a tile \(k <= 670\)"):
            ctx.segments_edges_build()
        with pytest.raises(RuntimeError, match="segment locate: tpc_segments_edges_build first"):
            ctx.segments_locate(packed(capi, ["ACGT"]))
    finally:
        ctx.close()


def test_forced_hash_bits_and_table_sizes_change_nothing(capi):
    case = CASES["rand6_k9_fp"]
    index, seqs = R.golden_index(case, GOLDEN, "sequence")
    data = open(os.path.join(GOLDEN, case["bin"]), "rb").read()
    queries = golden_queries(seqs, case["k"], 11)
    ctx = host_context(capi, seqs, data, case["k"])
    try:
        ctx.segments_colors_build(list(range(len(seqs))), len(seqs))
        plain = check_index(ctx, index)
        check_located(capi, ctx, index, queries, True)
        ctx.set_option("test_edges_hash_bits", 4)          # 16 home slots, one tag: only the letters decide
        forced = check_index(ctx, index, hash_bits=4)
        assert forced["longest_probe"] > plain["longest_probe"] and forced["longest_probe"] >= index.counts()[0] - 16
        check_located(capi, ctx, index, queries, True)
        ctx.set_option("test_edges_hash_bits", 0)
        tight = (index.counts()[0]).bit_length()           # the smallest power of two above the entries
        assert (1 << tight) > index.counts()[0] >= 1 << (tight - 1)
        ctx.set_option("test_edges_slots_log2", tight)
        nearly_full = check_index(ctx, index, slots=tight)
        assert nearly_full["slots"] == 1 << tight and nearly_full["longest_probe"] > plain["longest_probe"]
        check_located(capi, ctx, index, queries, True)
        ctx.set_option("test_edges_slots_log2", tight - 1)
        with pytest.raises(RuntimeError, match=r"segment edges: the table of 2\^%d slots is full, \d+ of %d edges found no slot" % (tight - 1, sum(index.counts()[:2]))):
            ctx.segments_edges_build()
        with pytest.raises(RuntimeError, match="segment locate: tpc_segments_edges_build first"):
            ctx.segments_locate(packed(capi, queries))
        ctx.set_option("test_edges_slots_log2", 41)
        with pytest.raises(RuntimeError, match="segment edges: option test_edges_slots_log2 = 41 is not in 0 .. 40"):
            ctx.segments_edges_build()
        ctx.set_option("test_edges_slots_log2", 0)
        check_index(ctx, index)
    finally:
        ctx.close()


def test_spans_that_repeat_keys_in_the_thousands(capi):
    """graph_walks.lay: k = 3, every event a span of three positions over random letters -- 256 keys of four letters, thousands of spans."""
    rng = np.random.default_rng(20261201)
    seqs, sequences = G.lay(rng, [np.arange(1, 3001, dtype=np.int64), np.arange(3001, 5001, dtype=np.int64)])
    case = G.Case("repeats", seqs, sequences, n_colors=2)
    strings = [np.asarray(s, dtype=np.uint8).tobytes().decode() for s in seqs]
    index = R.Index(graph_table.event_table(case.data, strings, G.K), strings, G.K, case.color_of_seq, 2)
    entries, duplicates, _ = index.counts()
    assert entries <= 136 and duplicates > 10000          # 136 canonical 4-mers
    ctx = host_context(capi, strings, case.data, G.K)
    try:
        ctx.segments_colors_build(case.color_of_seq, 2)
        check_index(ctx, index)
        want = check_located(capi, ctx, index, [strings[1][:700], letters(rng, 500)], True)
        assert want.info["found"] > 600
    finally:
        ctx.close()


@pytest.mark.parametrize("n_colors,color_of_seq", [(1, [0, 0, 0, 0]), (2, [1, 0, 1, 1]), (33, [32, 0, 31, 32]), (65, [64, 3, 32, 0])])
def test_colours_across_presence_words_and_maps_that_are_not_monotone(capi, n_colors, color_of_seq):
    made = Made(9, 77, n_colors=n_colors, color_of_seq=color_of_seq)
    ctx = made.context(capi)
    try:
        check_index(ctx, made.index)
        want = check_located(capi, ctx, made.index, made.query_of(np.random.default_rng(3), 3000), True)
        assert want.shared.shape[1] == n_colors and want.shared.sum() >= want.info["found"] > 0
    finally:
        ctx.close()


def test_without_a_colour_table_and_with_one_built_later(capi):
    made = Made(9, 78, n_colors=3, color_of_seq=[2, 0, 1, 0])
    bare = Made(9, 78)
    queries = made.query_of(np.random.default_rng(4), 2500)
    ctx = bare.context(capi)
    try:
        check_index(ctx, bare.index)
        check_located(capi, ctx, bare.index, queries, False)
        assert ctx.segments_locate_info()["colors"] == 0
        ctx.segments_colors_build(made.color_of_seq, 3)      # after the edge build: the next locate uses it
        check_located(capi, ctx, made.index, queries, True)
        ctx.segments_colors_build([0, 0, 0, 0], 1)
        assert ctx.segments_locate_info()["colors"] == 3     # what a locate left is kept
    finally:
        ctx.close()


def test_a_failed_walk_is_refused(capi):
    """edge_k5: the serial walk ends with "The input is corrupted", and so does the device's.  The oracle's numbers for it are checked on the CPU."""
    case = CASES["edge_k5"]
    fasta = os.path.join(GOLDEN, case["fasta"])
    seqs = graph_table.read_fasta(fasta)
    text = capi.PackedText.from_fasta([fasta])
    ctx = capi.Context(0)
    try:
        ctx.seq_upload(text)
        ctx.segments_build(open(os.path.join(GOLDEN, case["bin"]), "rb").read(), case["k"], text.rec_start, text.rec_length, ambiguous_positions(seqs, text.rec_start))
        assert ctx.segments_error() is not None
        with pytest.raises(RuntimeError, match="segment edges: the segment table holds the walk's error 1 at slot 3, there are no segments to index"):
            ctx.segments_edges_build()
        with pytest.raises(RuntimeError, match="segment locate: tpc_segments_edges_build first"):
            ctx.segments_locate(text)
    finally:
        ctx.close()


def test_refusals(capi):
    made = Made(9, 79)
    text = packed(capi, made.seqs)
    ctx = capi.Context(0)
    try:
        with pytest.raises(RuntimeError, match=r"segment edges: build the segment table first \(tpc_segments_build_host / _resident\)"):
            ctx.segments_edges_build()
        with pytest.raises(RuntimeError, match="segment edges: tpc_segments_edges_build first"):
            ctx.segments_edges_info()
        with pytest.raises(RuntimeError, match="segment locate: tpc_segments_edges_build first"):
            ctx.segments_locate(text)
        with pytest.raises(RuntimeError, match="segment locate: tpc_segments_locate first"):
            ctx.segments_locate_info()
        ctx.seq_upload(text)
        ctx.segments_build(made.data, made.k, text.rec_start, text.rec_length)
        ctx.segments_edges_build()
        with pytest.raises(RuntimeError, match="segment locate: tpc_segments_locate first"):
            ctx.segments_locate_fetch_hits(0, 0)
        from twopaco_amd.capi import hip
        start, length = np.array([1, 9], dtype=np.uint64), np.array([9, 4], dtype=np.uint64)
        b, m = np.ascontiguousarray(text.bases), np.ascontiguousarray(text.nmask)
        assert hip().tpc_segments_locate(ctx._h, b.ctypes.data, m.ctypes.data, text.length, start.ctypes.data, length.ctypes.data, 2) != 0
        assert b"segment locate: the query's records must ascend and not overlap" in hip().tpc_last_error(ctx._h)
        start[1] = text.length
        assert hip().tpc_segments_locate(ctx._h, b.ctypes.data, m.ctypes.data, text.length, start.ctypes.data, length.ctypes.data, 2) != 0
        assert b"segment locate: query record 1 lies outside the query text" in hip().tpc_last_error(ctx._h)
        assert hip().tpc_segments_locate(ctx._h, None, None, text.length, None, None, 0) != 0
        assert b"segment locate: a packed query text is required" in hip().tpc_last_error(ctx._h)
        ctx.seq_upload(text)                                  # the same letters, but not the build's upload
        with pytest.raises(RuntimeError, match="segment locate: the text of tpc_seq_upload the table was built over is no longer resident"):
            ctx.segments_locate(text)
        with pytest.raises(RuntimeError, match="segment edges: the text of tpc_seq_upload the table was built over is no longer resident"):
            ctx.segments_edges_build()
        with pytest.raises(RuntimeError, match="unknown option test_edges"):
            ctx.set_option("test_edges", 1)
    finally:
        ctx.close()


def test_the_other_stages_are_unchanged_by_an_edge_build_and_two_locates(capi):
    made = Made(9, 80, n_colors=3, color_of_seq=[0, 1, 2, 0])
    ctx = made.context(capi)

    def tables():
        out = [ctx.segments_counts(), ctx.segments_colors_info(), ctx.segments_colors_fetch_presence(), ctx.segments_links_info(), ctx.segments_bubbles_info(),
               ctx.segments_distances_info(), ctx.segments_components_info(), ctx.segments_superbubbles_info(), ctx.segments_anchors_info(), ctx.segments_anchors_fetch_mates()]
        return out + list(ctx.segments_colors_fetch_rows()) + list(ctx.segments_links_fetch_rows()) + list(ctx.segments_anchors_fetch_rows()) + list(ctx.segments_fetch_events())

    try:
        ctx.segments_links_build()
        ctx.segments_bubbles_build()
        ctx.segments_distances_build()
        ctx.segments_components_build()
        ctx.segments_superbubbles_build()
        ctx.segments_anchors_build(made.color_of_seq, 3, 0)
        before = tables()
        check_index(ctx, made.index)
        for seed in (1, 2):
            check_located(capi, ctx, made.index, made.query_of(np.random.default_rng(seed), 2000), True)
        for a, b in zip(before, tables()):
            assert (a == b) if isinstance(a, dict) else (np.asarray(a) == np.asarray(b)).all()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 3. the two programs

def program_case(tmp_path):
    """rand6_k9_fp, two query files: its own genomes and generated records; the serial table and walks, checked against the oracle."""
    case = CASES["rand6_k9_fp"]
    index, seqs = R.golden_index(case, GOLDEN, "sequence")
    own = os.path.join(GOLDEN, case["fasta"])
    more = str(tmp_path / "more.fa")
    records = golden_queries(seqs, case["k"], 13)[len(seqs):]
    with open(more, "w") as f:
        for i, r in enumerate(records):
            f.write(">g%d\n%s\n" % (i, r))
    queries = ["--locate-in", own, "--locate-in", more]
    names = [n for n, _ in R.read_named(own)] + ["g%d" % i for i in range(len(records))]
    want = index.locate(list(seqs) + records)
    labels = ["%d\t%s" % (s + 1, case["fasta"]) for s in range(len(seqs))]
    tsv, walks = R.tsv(index, want, names, "sequence", labels), R.walks(index, want)
    args = [case["bin"], "-k", str(case["k"]), "-s", case["fasta"]]
    out = str(tmp_path / "serial.walks")
    r = subprocess.run([C.GRAPHDUMP] + args + ["--locate", "sequence", "--locate-walks", out] + queries, cwd=GOLDEN, capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == tsv and open(out, "rb").read() == walks
    return case, args, queries, tsv, walks, want


def test_graphdump_gpu_writes_the_serial_bytes_alone_and_beside_the_colour_table(tmp_path):
    case, args, queries, tsv, walks, want = program_case(tmp_path)
    stats, out = str(tmp_path / "stats.json"), str(tmp_path / "gpu.walks")
    env = dict(os.environ, TWOPACO_GRAPHDUMP_STATS=stats, TWOPACO_TIMING="1")
    r = subprocess.run([C.GRAPHDUMP] + args + ["--locate", "sequence", "--locate-walks", out, "--gpu", "--threads", "16"] + queries, cwd=GOLDEN, capture_output=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout == tsv and open(out, "rb").read() == walks, r.stderr[-400:]
    assert b"[timing] edge index on device:" in r.stderr and b"[timing] locate on device:" in r.stderr
    s = json.load(open(stats))
    assert s["locate_batches"] == 1 and s["path"] == "device" and s["edges_kernel_ms"] > 0 and s["locate_kernel_ms"] > 0 and s["locate_runs"] == want.info["runs"] and s["colors_kernel_ms"] > 0
    alone = subprocess.run([C.GRAPHDUMP] + args + ["--colors", "sequence"], cwd=GOLDEN, capture_output=True, timeout=300)
    table = str(tmp_path / "beside.tsv")
    r = subprocess.run([C.GRAPHDUMP] + args + ["--colors", "sequence", "--locate", "sequence", "--locate-out", table, "--locate-walks", out, "--gpu"] + queries, cwd=GOLDEN,
                       capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == alone.stdout and open(table, "rb").read() == tsv and open(out, "rb").read() == walks
    # the same queries in batches of whole records: every genome a batch of its own and the short records one (700 positions), then
    # two genomes to a batch (6 100): the sums and the runs only concatenate
    for limit, batches in ((700, 9), (6100, 5)):
        env = dict(os.environ, TWOPACO_GRAPHDUMP_STATS=stats, TWOPACO_LOCATE_BATCH=str(limit))
        r = subprocess.run([C.GRAPHDUMP] + args + ["--locate", "sequence", "--locate-walks", out, "--gpu"] + queries, cwd=GOLDEN, capture_output=True, timeout=300, env=env)
        assert r.returncode == 0 and r.stderr == b"" and r.stdout == tsv and open(out, "rb").read() == walks, limit
        s = json.load(open(stats))
        assert s["locate_batches"] == batches and s["locate_runs"] == want.info["runs"]
    # a failing walk: what the serial program says, and no file
    bad = CASES["edge_k5"]
    r = subprocess.run([C.GRAPHDUMP, bad["bin"], "-k", str(bad["k"]), "-s", bad["fasta"], "--locate", "file", "--locate-in", bad["fasta"], "--locate-out", table + ".bad", "--gpu"],
                       cwd=GOLDEN, capture_output=True, timeout=300)
    assert r.returncode == 1 and r.stdout == b"" and b"The input is corrupted" in r.stderr and not os.path.exists(table + ".bad")


def twopaco(case, extra, cwd, env=None):
    args = [C.TWOPACO, "-k", str(case["k"]), "-f", str(case["L"]), "-q", str(case["q"]), "-r", str(case["n_rounds"]), "--seed", str(case["seed"])]
    return subprocess.run(args + extra + [os.path.join(GOLDEN, case["fasta"])], cwd=cwd, capture_output=True, timeout=300, env=env)


def test_twopaco_writes_the_serial_bytes_alone_and_beside_the_colour_table(tmp_path):
    case, args, queries, tsv, walks, _ = program_case(tmp_path)
    colours = subprocess.run([C.GRAPHDUMP] + args + ["--colors", "sequence"], cwd=GOLDEN, capture_output=True, timeout=300).stdout
    tsv = tsv.replace(("\t" + case["fasta"] + "\n").encode(), ("\t" + os.path.join(GOLDEN, case["fasta"]) + "\n").encode())     # the labels are the file names as given
    colours = colours.replace(("\t" + case["fasta"] + "\n").encode(), ("\t" + os.path.join(GOLDEN, case["fasta"]) + "\n").encode())
    d = str(tmp_path / "alone")
    os.mkdir(d)
    r = twopaco(case, ["--tmpdir", d, "--locate", "sequence", "--locate-walks", os.path.join(d, "walks.tsv"), "-o", os.path.join(d, "j.bin")] + queries, d,
                env=dict(os.environ, TWOPACO_TIMING="1"))
    assert r.returncode == 0, r.stderr[-400:]
    assert sorted(os.listdir(d)) == ["de_bruijn.locate.tsv", "j.bin", "walks.tsv"]
    assert open(os.path.join(d, "j.bin"), "rb").read() == open(os.path.join(GOLDEN, case["bin"]), "rb").read()
    assert open(os.path.join(d, "de_bruijn.locate.tsv"), "rb").read() == tsv and open(os.path.join(d, "walks.tsv"), "rb").read() == walks
    err = r.stderr.decode()
    assert "edge index:" in err and "locate:" in err and "locate_kernel_ms" in err and "locate table writing:" in err
    d = str(tmp_path / "beside")
    os.mkdir(d)
    r = twopaco(case, ["--tmpdir", d, "--colors", "sequence", "--colors-out", os.path.join(d, "colors.tsv"), "--locate", "sequence", "--locate-out", os.path.join(d, "locate.tsv"),
                       "-o", os.path.join(d, "j.bin")] + queries, d)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert sorted(os.listdir(d)) == ["colors.tsv", "j.bin", "locate.tsv"]
    assert open(os.path.join(d, "locate.tsv"), "rb").read() == tsv and open(os.path.join(d, "colors.tsv"), "rb").read() == colours
    r = twopaco(case, ["--tmpdir", d, "--locate", "sequence", "--gpus", "2"] + queries, d)
    assert r.returncode == 1 and r.stderr.decode().endswith("not with --gpus above 1 for arg (--locate)\n")
    r = twopaco(case, ["--tmpdir", d, "--locate", "file", "--colors", "sequence"] + queries, d)
    assert r.returncode == 1 and b"--colors sequence does not go with --locate file" in r.stderr
