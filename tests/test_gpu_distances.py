"""GPU (-m gpu): the genome distance matrices on the device (csrc/tpc_distances.hip, the tpc_segments_distances_* group of
include/twopaco_hip.h) against their definition, restated in distances_reference.py over the serial gfa1 text (pinned to the real
reference's sha256 by tests/golden/graphdump.json): both matrices and info[] through the C-ABI on a host stream and a resident
stream, forced chunk lengths, colour counts around the presence words and the kernel's tile, thousands of colours, a weight beyond
2^17, the stages it leaves untouched, ranges, refusals, and the bytes of `graphdump --distances --gpu` and `twopaco --distances`."""
import json
import os
import subprocess

import numpy as np
import pytest

import bubbles_reference as B
import colors_reference as R
import distances_reference as D
from helpers import GOLDEN, case_files, golden_cases, sha256_file
from twopaco_amd.capi import DISTANCES_TILE as T

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in golden_cases()}
MAXU = (1 << 64) - 1
SHORT_CASE = {"name": "short", "k": B.BUBBLE_K, "L": B.BUBBLE_L, "q": B.BUBBLE_Q, "seed": B.BUBBLE_SEED, "rounds": [{"low": 0, "high": 1 << B.BUBBLE_L}], "n_rounds": 1,
              "abundance": None}
LONG_CASE = {"name": "long", "k": 25, "L": 24, "q": 5, "seed": 7, "rounds": [{"low": 0, "high": 1 << 24}], "n_rounds": 1, "abundance": None}
NAMES = ["short", "example_k11", "rand6_k3", "c2_k29", "tr_k25_L28"]
# the word boundaries of the presence bits and T - 1, T, T + 1, 2T + 1 for the tile: diagonal, off-diagonal and ragged tiles
COLOR_COUNTS = sorted(set(R.BOUNDARY_COLORS) | {T - 1, T, T + 1, 2 * T + 1})


@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


def read_fasta(path):
    return [s for _, s in B.read_fasta(path)]


def ambiguous_positions(fasta, rec_start):
    return [int(rec_start[r]) + i for r, s in enumerate(read_fasta(fasta)) for i, ch in enumerate(s) if ch not in "ACGTN"]


def host_context(capi, fasta, data, k):
    """A context used for nothing else, the table from the stream's bytes."""
    text = capi.PackedText.from_fasta([fasta])
    ctx = capi.Context(0)
    ctx.seq_upload(text)
    ctx.segments_build(data, k, text.rec_start, text.rec_length, ambiguous_positions(fasta, text.rec_start))
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
        ctx.pass2_filter()
    ctx.junctions_finalize()
    ctx.emit()
    stream, _ = ctx.emit_stream(text.rec_start, text.rec_length)
    assert stream == data
    ctx.segments_build(None, case["k"], text.rec_start, text.rec_length, ambiguous_positions(fasta, text.rec_start))
    return ctx


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """The generated inputs: FASTA, junction stream (from the CPU restatement of the pipeline, oracle/) and the serial gfa1, once."""
    d = tmp_path_factory.mktemp("distances")
    got = {"dir": str(d)}
    for name, case in (("short", SHORT_CASE), ("long", LONG_CASE)):
        fa = str(d / (name + ".fa"))
        if name == "short":
            B.few_events_fasta(fa, only_short=True)
        else:
            D.long_pair_fasta(fa)
        stream = B.oracle_stream(fa, str(d / (name + ".bin")), case["k"], case["L"], case["q"], case["seed"])
        gfa1 = R.run_graphdump([stream, "-k", str(case["k"]), "-s", fa, "-f", "gfa1"], cwd=str(d))
        assert gfa1.returncode == 0 and gfa1.stderr == b""
        got[name] = {"case": case, "fasta": fa, "stream": stream, "gfa1": gfa1.stdout}
    for c in COLOR_COUNTS:
        fa = R.boundary_fasta(str(d / ("w%d.fa" % c)), c)
        assert len(read_fasta(fa)) == c, "the generator holds 65 records"
        stream = B.oracle_stream(fa, str(d / ("w%d.bin" % c)), R.BOUNDARY_K, R.BOUNDARY_L, R.BOUNDARY_Q, R.BOUNDARY_SEED)
        gfa1 = R.run_graphdump([stream, "-k", str(R.BOUNDARY_K), "-s", fa, "-f", "gfa1"], cwd=str(d))
        assert gfa1.returncode == 0 and gfa1.stderr == b""
        got[c] = {"fasta": fa, "stream": stream, "gfa1": gfa1.stdout}
    return got


_GFA = {}


def inputs(name, made):
    """(case, fasta, stream bytes, the parsed gfa1, its text, graphdump's arguments, its directory, the files as given)"""
    if name in made:
        m = made[name]
        if name not in _GFA:
            _GFA[name] = R.Gfa1(m["gfa1"])
        return m["case"], m["fasta"], open(m["stream"], "rb").read(), _GFA[name], m["gfa1"], [m["stream"], "-k", str(m["case"]["k"]), "-s", m["fasta"]], made["dir"], [m["fasta"]]
    case = CASES[name]
    v = R.case_vector(case)
    if name not in _GFA:
        _GFA[name] = R.Gfa1(R.golden_gfa1(v))
    files = [v["args"][i + 1] for i, a in enumerate(v["args"]) if a == "-s"]
    return case, os.path.join(GOLDEN, case["fasta"]), open(os.path.join(GOLDEN, case["bin"]), "rb").read(), _GFA[name], R.golden_gfa1(v), R.colors_args(v), GOLDEN, files


_WANT = {}


def oracle(key, g, color_of_seq, n_colors, k):
    """(segments, edges) of the oracle, computed once per input and colour map and never written to."""
    key = (key, tuple(color_of_seq), n_colors)
    if key not in _WANT:
        segments, edges = D.matrices(R.table(g, color_of_seq, n_colors), k)
        segments.setflags(write=False)
        edges.setflags(write=False)
        _WANT[key] = (segments, edges)
    return _WANT[key]


def check_matrices(ctx, key, g, color_of_seq, n_colors, k, colours_built=False):
    """Everything the device holds after a distance build == the oracle's matrices of the same colour map."""
    if not colours_built:
        ctx.segments_colors_build(color_of_seq, n_colors)
    want_s, want_e = oracle(key, g, color_of_seq, n_colors, k)
    info = ctx.segments_distances_build()
    rows = len(g.row_name)
    weights = np.array(g.row_length, dtype=np.int64) - k
    assert (info["colors"], info["rows"]) == (n_colors, rows)
    assert info["planes"] == (int(weights.max()).bit_length() if rows else 0)
    assert info["peak_bytes"] >= 16 * n_colors * n_colors + 8 * n_colors * ((rows + 63) // 64)
    seg, edg = ctx.segments_distances_fetch()
    assert seg.dtype == edg.dtype == np.uint64 and seg.shape == edg.shape == (n_colors, n_colors)
    assert (seg.astype(np.int64) == want_s).all(), np.argwhere(seg.astype(np.int64) != want_s)[:5]
    assert (edg.astype(np.int64) == want_e).all(), np.argwhere(edg.astype(np.int64) != want_e)[:5]
    assert (seg == seg.T).all() and (edg == edg.T).all()
    # against the colour stage's own histogram: a row of n colours adds 1 to n diagonal entries and to n^2 entries in all
    hist, _ = ctx.segments_colors_fetch_hist()
    n = np.arange(n_colors + 1, dtype=np.int64)
    assert int(np.trace(seg.astype(np.int64))) == int((n * hist.astype(np.int64)).sum())
    assert int(seg.astype(np.int64).sum()) == int((n * n * hist.astype(np.int64)).sum())
    assert ctx.kernel_ms("distances") > 0
    return seg, edg, info


# ------------------------------------------------------------------------------------------------ 1. the matrices by their definition
@pytest.mark.parametrize("source", ["host", "resident"])
@pytest.mark.parametrize("name", NAMES)
def test_matrices_by_their_definition(capi, made, name, source):
    case, fasta, data, g, _, _, _, _ = inputs(name, made)
    n_seq = len(g.seq_name)
    ctx = host_context(capi, fasta, data, case["k"]) if source == "host" else resident_context(capi, case, fasta, data)
    assert ctx.segments_error() is None
    seg, edg, info = check_matrices(ctx, name, g, list(range(n_seq)), n_seq, case["k"])     # by sequence
    check_matrices(ctx, name, g, list(range(n_seq)), n_seq, case["k"], colours_built=True)  # a second build replaces the first
    check_matrices(ctx, name, g, [0] * n_seq, 1, case["k"])                                 # by file: one file
    if n_seq >= 2:
        # an arbitrary map: the first two sequences share colour 0, colour 1 stays empty -- a zero row and a zero column
        arbitrary = [0, 0] + list(range(2, n_seq))
        sa, ea, _ = check_matrices(ctx, name, g, arbitrary, n_seq + 1, case["k"])
        assert not sa[1].any() and not sa[:, 1].any() and not ea[1].any() and not ea[:, 1].any() and sa[0, 0] > 0
    if name == "short":
        assert 0 < info["rows"] < 64
    if name == "tr_k25_L28":
        assert info["rows"] > 64
    if name == "rand6_k3":
        assert (seg[~np.eye(n_seq, dtype=bool)] > 0).all()   # every pair of colours shares segments
    ctx.close()


@pytest.mark.parametrize("source", ["host", "resident"])
@pytest.mark.parametrize("name", NAMES + ["rand6_k9_fp"])
def test_forced_chunk_lengths(capi, made, name, source):
    """test_distances_chunk_words: one column word per chunk, then a length that leaves a partial last chunk, on every input of the
    first test and on both streams; the sums a workgroup keeps across its chunks and the zero fill past the last word are in play."""
    case, fasta, data, g, _, _, _, _ = inputs(name, made)
    n_seq = len(g.seq_name)
    words = (len(g.row_name) + 63) // 64
    ctx = host_context(capi, fasta, data, case["k"]) if source == "host" else resident_context(capi, case, fasta, data)
    # a partial last chunk needs a length cw <= 64 with 1 < cw < words and words % cw != 0
    partial = [cw for cw in range(2, min(words, 65)) if words % cw]
    if words <= 2:
        assert not partial, "one or two column words: every chunk length divides them or holds them whole"
        lengths = (1, 0)
    else:
        assert partial, (name, words)
        lengths = (1, partial[-1], partial[0], 0)
    for cw in lengths:
        ctx.set_option("test_distances_chunk_words", cw)
        check_matrices(ctx, name, g, list(range(n_seq)), n_seq, case["k"])
    if name == "rand6_k9_fp" and source == "host":
        assert words >= 8, "a few hundred rows"
        ctx.set_option("test_distances_chunk_words", 65)
        with pytest.raises(RuntimeError, match="test_distances_chunk_words = 65 is not in 0 .. 64"):
            ctx.segments_distances_build()
        ctx.set_option("test_distances_chunk_words", 0)
        check_matrices(ctx, name, g, list(range(n_seq)), n_seq, case["k"], colours_built=True)
    ctx.close()


def test_the_tile_width_is_the_kernels(capi, made):
    """The colour counts above are chosen around capi.DISTANCES_TILE; the library reports the tile its kernel was compiled with."""
    ctx = capi.Context(0)
    assert ctx.stat("distances_tile") == capi.DISTANCES_TILE == T
    ctx.close()


def test_more_colours_than_the_sizes_can_hold_are_refused(capi, made):
    """The colour stage takes up to 2^31 colours; 16 B x C^2 wraps 64 bits from 2^30 on.  Beyond 2^24 colours the stage refuses
    before it computes a size, on a table of one row so that the colour build itself fits (2 MiB of presence, 256 MiB of bins)."""
    case, fasta, data, g, _, _, _, _ = inputs("long", made)
    assert len(g.row_name) == 1
    ctx = host_context(capi, fasta, data, case["k"])
    ctx.segments_colors_build([0, 1 << 24], (1 << 24) + 1)
    with pytest.raises(RuntimeError, match="segment distances: 16777217 colours, the two matrices of 16 B x colours\\^2 are refused beyond 16777216 colours"):
        ctx.segments_distances_build()
    with pytest.raises(RuntimeError, match="tpc_segments_distances_build first"):
        ctx.segments_distances_info()
    check_matrices(ctx, "long", g, [0, 1], 2, case["k"])   # the context goes on
    ctx.close()


@pytest.mark.parametrize("c", COLOR_COUNTS)
def test_colour_counts_at_the_word_and_tile_boundaries(capi, made, c):
    assert {T - 1, T, T + 1, 2 * T + 1} <= set(COLOR_COUNTS) and 2 * T + 1 <= 65
    m = made[c]
    if c not in _GFA:
        _GFA[c] = R.Gfa1(m["gfa1"])
    g = _GFA[c]
    assert len(g.seq_name) == c
    ctx = host_context(capi, m["fasta"], open(m["stream"], "rb").read(), R.BOUNDARY_K)
    seg, _, _ = check_matrices(ctx, c, g, list(range(c)), c, R.BOUNDARY_K)
    assert seg.min() > 0 and seg[c - 1, c - 1] > 0    # one segment lies in every record: no pair is empty, the last tile's neither
    ctx.set_option("test_distances_chunk_words", 1)
    check_matrices(ctx, c, g, list(range(c)), c, R.BOUNDARY_K, colours_built=True)
    ctx.close()


def test_thousands_of_colours(capi, made):
    """4200 colours on rand6_k9_fp: the colour test's wide map (every sequence a colour of its own far from the others, everything
    between them empty) and the first two sequences sharing one.  The oracle's matrices of the compact map, placed at the colours'
    indices: P has no other column with a bit."""
    case, fasta, data, g, _, _, _, _ = inputs("rand6_k9_fp", made)
    n_seq = len(g.seq_name)
    n_colors = 700 * n_seq
    assert n_colors > 4000
    ctx = host_context(capi, fasta, data, case["k"])
    for compact in (list(range(n_seq)), [0, 0] + list(range(2, n_seq))):
        wide = [700 * c + 699 for c in compact]
        want_s, want_e = oracle("rand6_k9_fp", g, compact, n_seq, case["k"])
        ctx.segments_colors_build(wide, n_colors)
        info = ctx.segments_distances_build()
        assert info["colors"] == n_colors
        seg, edg = ctx.segments_distances_fetch()
        at = np.array(sorted(set(wide)))
        held = np.array(sorted(set(compact)))
        assert (seg[np.ix_(at, at)].astype(np.int64) == want_s[np.ix_(held, held)]).all()
        assert (edg[np.ix_(at, at)].astype(np.int64) == want_e[np.ix_(held, held)]).all()
        assert int(seg.astype(np.int64).sum()) == int(want_s.sum()) and int(edg.astype(np.int64).sum()) == int(want_e.sum())   # nothing anywhere else
        assert not seg[0].any() and not seg[:, n_colors - 2].any()
    ctx.close()


def test_a_weight_beyond_two_to_the_17(capi, made):
    """One random sequence of 200 929 bases twice, in two records of different colours: the planes of bits 16 and 17 carry a weight
    both colours share."""
    case, fasta, data, g, _, _, _, _ = inputs("long", made)
    weights = np.array(g.row_length, dtype=np.int64) - case["k"]
    assert len(g.seq_name) == 2 and int(weights.max()) >= (3 << 16) and (int(weights.max()) >> 16) & 3 == 3
    ctx = host_context(capi, fasta, data, case["k"])
    seg, edg, info = check_matrices(ctx, "long", g, [0, 1], 2, case["k"])
    assert info["planes"] == 18 and int(edg[0, 1]) >= (3 << 16) and edg[0, 1] == edg[0, 0] == edg[1, 1]
    ctx.close()


def test_no_event_at_all(capi, made):
    fa = made["short"]["fasta"]
    text = capi.PackedText.from_fasta([fa])
    ctx = capi.Context(0)
    ctx.seq_upload(text)
    ctx.segments_build(b"", B.BUBBLE_K, text.rec_start, text.rec_length)
    n_seq = len(read_fasta(fa))
    ctx.segments_colors_build(list(range(n_seq)), n_seq)
    info = ctx.segments_distances_build()
    assert (info["colors"], info["rows"], info["planes"]) == (n_seq, 0, 0)
    seg, edg = ctx.segments_distances_fetch()
    assert seg.shape == (n_seq, n_seq) and not seg.any() and not edg.any()
    ctx.close()


# ------------------------------------------------------------------------------------------------ 2. opt-in
@pytest.mark.parametrize("order", ["distances_last", "distances_before_the_links"])
def test_the_other_stages_are_unchanged(capi, made, order):
    case, fasta, data, g, _, _, _, _ = inputs("c2_k29", made)
    n_seq = len(g.seq_name)
    colours = list(range(n_seq))

    def outputs(ctx):
        name, first = ctx.segments_fetch()
        begin, end = ctx.segments_fetch_events()
        got = [name, first, begin, end, ctx.segments_fetch_sequences(0, n_seq + 1)]
        got += list(ctx.segments_colors_fetch_rows()) + [ctx.segments_colors_fetch_presence()] + list(ctx.segments_colors_fetch_hist())
        got += list(ctx.segments_links_fetch_rows()) + [ctx.segments_links_fetch_first()]
        got += list(ctx.segments_bubbles_fetch_rows()) + list(ctx.segments_bubbles_fetch_sides()) + [ctx.segments_bubbles_fetch_hist()]
        scalars = (ctx.segments_error(), ctx.segments_colors_info(), ctx.segments_links_info())
        bubbles = {key: n for key, n in ctx.segments_bubbles_info().items() if key != "peak_bytes"}
        return ctx.segments_counts(), scalars, bubbles, got

    def elsewhere(counts):
        """peak_device_bytes is what the whole device held at the segment build: it belongs to one build, not to the input"""
        return {key: n for key, n in counts.items() if key != "peak_device_bytes"}

    alone = host_context(capi, fasta, data, case["k"])
    alone.segments_colors_build(colours, n_seq)
    alone.segments_links_build()
    alone.segments_bubbles_build()
    ref = outputs(alone)
    with pytest.raises(RuntimeError, match="tpc_segments_distances_build first"):   # a context that never asked holds none
        alone.segments_distances_info()
    alone.close()
    ctx = host_context(capi, fasta, data, case["k"])
    counts = ctx.segments_counts()
    ctx.segments_colors_build(colours, n_seq)
    if order == "distances_last":
        ctx.segments_links_build()
        ctx.segments_bubbles_build()
        before = outputs(ctx)
        assert all(a.shape == b.shape and (a == b).all() for a, b in zip(before[3], ref[3]))
        check_matrices(ctx, "c2_k29", g, colours, n_seq, case["k"], colours_built=True)
    else:
        check_matrices(ctx, "c2_k29", g, colours, n_seq, case["k"], colours_built=True)
        ctx.segments_links_build()
        ctx.segments_bubbles_build()
    for _ in range(2):
        got = outputs(ctx)
        assert got[0] == counts and elsewhere(got[0]) == elsewhere(ref[0])
        assert got[1] == ref[1] and got[2] == ref[2]
        assert all(a.shape == b.shape and (a == b).all() for a, b in zip(got[3], ref[3]))
        check_matrices(ctx, "c2_k29", g, colours, n_seq, case["k"], colours_built=True)   # rebuilt: the same matrices, the others once more
    # the matrices outlive a link and a bubble build; a new colour build drops them
    ctx.segments_links_build()
    ctx.segments_bubbles_build()
    want_s, _ = oracle("c2_k29", g, colours, n_seq, case["k"])
    assert (ctx.segments_distances_fetch()[0].astype(np.int64) == want_s).all()
    ctx.segments_colors_build(colours, n_seq)
    with pytest.raises(RuntimeError, match="tpc_segments_distances_build first"):
        ctx.segments_distances_info()
    ctx.close()


# ------------------------------------------------------------------------------------------------ 3. ranges and refusals
def test_fetch_ranges(capi, made):
    case, fasta, data, g, _, _, _, _ = inputs("rand6_k9_fp", made)
    n = len(g.seq_name)
    ctx = host_context(capi, fasta, data, case["k"])
    want_s, want_e = oracle("rand6_k9_fp", g, list(range(n)), n, case["k"])
    ctx.segments_colors_build(list(range(n)), n)
    ctx.segments_distances_build()
    seg, edg = ctx.segments_distances_fetch(2, 3)     # a middle slice
    assert seg.shape == (3, n) and (seg.astype(np.int64) == want_s[2:5]).all() and (edg.astype(np.int64) == want_e[2:5]).all()
    seg, edg = ctx.segments_distances_fetch(n - 1, 1)  # the last row
    assert (seg.astype(np.int64) == want_s[n - 1:]).all() and (edg.astype(np.int64) == want_e[n - 1:]).all()
    assert all(a.size == 0 for a in ctx.segments_distances_fetch(n, 0))
    for i0, m in ((n, 1), (n + 1, 0), (0, n + 1), (MAXU, 2)):
        with pytest.raises(RuntimeError, match="bad row range"):
            ctx.segments_distances_fetch(i0, m)
    check_matrices(ctx, "rand6_k9_fp", g, list(range(n)), n, case["k"], colours_built=True)   # still usable
    ctx.close()


def test_refusals(capi, made):
    case, fasta, data, g, _, _, _, _ = inputs("c2_k29", made)
    n = len(g.seq_name)
    text = capi.PackedText.from_fasta([fasta])
    ctx = capi.Context(0)
    with pytest.raises(RuntimeError, match="segment distances: build the segment table first"):   # no table
        ctx.segments_distances_build()
    for call in (ctx.segments_distances_info, ctx.segments_distances_fetch):
        with pytest.raises(RuntimeError, match="tpc_segments_distances_build first"):
            call()
    # the context is usable: a table, then no colour table yet
    ctx.seq_upload(text)
    ctx.segments_build(data, case["k"], text.rec_start, text.rec_length, ambiguous_positions(fasta, text.rec_start))
    with pytest.raises(RuntimeError, match="segment distances: build the colour table first"):
        ctx.segments_distances_build()
    assert ctx.segments_counts()["events"] > 0 and ctx.segments_error() is None
    check_matrices(ctx, "c2_k29", g, list(range(n)), n, case["k"])
    # a new segment build drops the colours of the old one and with them the matrices
    ctx.segments_build(data, case["k"], text.rec_start, text.rec_length, ambiguous_positions(fasta, text.rec_start))
    with pytest.raises(RuntimeError, match="tpc_segments_distances_build first"):
        ctx.segments_distances_fetch(0, 0)
    with pytest.raises(RuntimeError, match="segment distances: build the colour table first"):
        ctx.segments_distances_build()
    check_matrices(ctx, "c2_k29", g, list(range(n)), n, case["k"])   # and is used again
    ctx.close()
    # a table whose walk failed
    bad = CASES["edge_k5"]
    ctx = host_context(capi, os.path.join(GOLDEN, bad["fasta"]), open(os.path.join(GOLDEN, bad["bin"]), "rb").read(), bad["k"])
    assert ctx.segments_error() is not None
    with pytest.raises(RuntimeError, match="segment distances: the segment table holds the walk's error 1 at slot 3"):
        ctx.segments_distances_build()
    with pytest.raises(RuntimeError, match="tpc_segments_distances_build first"):
        ctx.segments_distances_info()
    bad_text = capi.PackedText.from_fasta([os.path.join(GOLDEN, bad["fasta"])])
    ctx.segments_build(b"", bad["k"], bad_text.rec_start, bad_text.rec_length)
    ctx.segments_colors_build([0] * len(bad_text.rec_start), 1)
    assert ctx.segments_distances_build()["rows"] == 0
    ctx.close()


# ------------------------------------------------------------------------------------------------ 4. bytes
BYTES_NAMES = ["rand6_k9_fp", "c2_k29", "tr_k25_L28"]


@pytest.mark.parametrize("by", ["file", "sequence"])
@pytest.mark.parametrize("name", BYTES_NAMES)
def test_graphdump_gpu_writes_the_oracle_bytes(tmp_path, made, name, by):
    case, _, _, _, gfa1, args, cwd, files = inputs(name, made)
    want, want_phy, _, _, _ = D.tsv(gfa1, by, case["k"], files)
    stats, phy = str(tmp_path / "stats.json"), str(tmp_path / "d.phy")
    env = dict(os.environ, TWOPACO_GRAPHDUMP_STATS=stats)
    r = subprocess.run([R.GRAPHDUMP] + args + ["--distances", by, "--gpu", "--threads", "16", "--distances-phylip", phy], cwd=cwd, capture_output=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert r.stdout == want, name
    assert open(phy, "rb").read() == want_phy
    s = json.load(open(stats))
    assert s["path"] == "device" and s["distances_kernel_ms"] > 0 and s["colors_kernel_ms"] > 0
    out = str(tmp_path / "distances.tsv")
    r = R.run_graphdump(args + ["--distances", by, "--gpu", "--distances-out", out, "--prefix"], cwd=cwd)
    assert r.returncode == 0 and r.stdout == b"" and open(out, "rb").read() == want


def test_graphdump_gpu_beside_the_colour_and_the_bubble_table(tmp_path, made):
    """--gpu with --colors or --bubbles of the same colours: both tables as they are alone, one device context for the two."""
    case, _, _, _, gfa1, args, cwd, files = inputs("c2_k29", made)
    want, _, _, _, _ = D.tsv(gfa1, "sequence", case["k"], files)
    for flag in ("--colors", "--bubbles"):
        other = R.run_graphdump(args + [flag, "sequence"], cwd=cwd)
        assert other.returncode == 0 and other.stdout
        out = str(tmp_path / "other.tsv")
        r = R.run_graphdump(args + [flag, "sequence", flag + "-out", out, "--distances", "sequence", "--gpu"], cwd=cwd)
        assert r.returncode == 0 and r.stderr == b"", r.stderr
        assert r.stdout == want and open(out, "rb").read() == other.stdout, flag


def test_graphdump_gpu_fails_as_the_walk_fails(tmp_path):
    v = R.vector_of("edge_k5")
    out, phy = str(tmp_path / "distances.tsv"), str(tmp_path / "d.phy")
    r = R.run_graphdump(R.colors_args(v) + ["--distances", "file", "--gpu", "--distances-out", out, "--distances-phylip", phy])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode() == v["stderr"] and not os.path.exists(out) and not os.path.exists(phy)
    r = R.run_graphdump(R.colors_args(v) + ["--distances", "sequence", "--gpu"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode() == v["stderr"]


def cli(case, extra, fasta=None, cwd=GOLDEN, timeout=300, env=None):
    args = [R.TWOPACO, "-k", str(case["k"]), "-f", str(case["L"]), "-q", str(case["q"]), "-r", str(case["n_rounds"]), "--seed", str(case["seed"])]
    if case["abundance"] is not None:
        args += ["-a", str(case["abundance"])]
    return subprocess.run(args + extra + [case["fasta"] if fasta is None else fasta], cwd=cwd, capture_output=True, timeout=timeout, env=env)


@pytest.mark.parametrize("by", ["file", "sequence"])
@pytest.mark.parametrize("name", BYTES_NAMES)
def test_twopaco_writes_the_oracle_bytes_beside_everything_else(tmp_path, made, name, by):
    """--distances with --colors --links --bubbles --graph gfa1: one segment build and one colour build serve all, and every other
    file has the bytes it has without --distances."""
    case, _, data, _, gfa1, _, _, files = inputs(name, made)
    want, want_phy, _, _, _ = D.tsv(gfa1, by, case["k"], files)
    with_dir, without_dir = str(tmp_path / "with"), str(tmp_path / "without")
    others = ("graph.gfa", "links.tsv", "colors.tsv", "bubbles.tsv", "j.bin")
    for d, extra in ((without_dir, []), (with_dir, ["--distances", by, "--distances-out", os.path.join(with_dir, "distances.tsv"), "--distances-phylip", os.path.join(with_dir, "d.phy")])):
        os.mkdir(d)
        r = cli(case, ["--tmpdir", d, "--graph", "gfa1", "--graph-out", os.path.join(d, "graph.gfa"), "--links", "--links-out", os.path.join(d, "links.tsv"),
                       "--colors", by, "--colors-out", os.path.join(d, "colors.tsv"), "--bubbles", by, "--bubbles-out", os.path.join(d, "bubbles.tsv"),
                       "-o", os.path.join(d, "j.bin")] + extra)
        assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert sorted(os.listdir(without_dir)) == sorted(others) and sorted(os.listdir(with_dir)) == sorted(others + ("distances.tsv", "d.phy"))
    for f in others:
        assert open(os.path.join(with_dir, f), "rb").read() == open(os.path.join(without_dir, f), "rb").read(), f
    assert open(os.path.join(with_dir, "j.bin"), "rb").read() == data
    assert open(os.path.join(with_dir, "graph.gfa"), "rb").read() == gfa1
    assert open(os.path.join(with_dir, "distances.tsv"), "rb").read() == want
    assert open(os.path.join(with_dir, "d.phy"), "rb").read() == want_phy
    # alone
    d = str(tmp_path / "alone")
    os.mkdir(d)
    r = cli(case, ["--tmpdir", d, "--distances", by, "--distances-out", os.path.join(d, "distances.tsv"), "-o", os.path.join(d, "j.bin")])
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert open(os.path.join(d, "distances.tsv"), "rb").read() == want and sorted(os.listdir(d)) == ["distances.tsv", "j.bin"]


def test_twopaco_writes_every_table_when_no_record_reaches_k(tmp_path):
    """Two records of 5 and 7 bases at k = 9: nothing is dispatched to the device, and the graph and the four tables are still what
    serial graphdump writes from that run's junction file."""
    d = str(tmp_path)
    fasta, stream = os.path.join(d, "tiny.fa"), os.path.join(d, "j.bin")
    with open(fasta, "w") as f:
        f.write(">a\nACGTA\n>b\nGATTACA\n")
    case = {"k": 9, "L": 16, "q": 5, "n_rounds": 1, "seed": 7, "abundance": None}
    names = {"--graph": "graph.gfa", "--colors": "colors.tsv", "--links": "links.tsv", "--bubbles": "bubbles.tsv", "--distances": "distances.tsv"}
    out = {flag: os.path.join(d, f) for flag, f in names.items()}
    r = cli(case, ["--tmpdir", d, "-o", stream, "--graph", "gfa1", "--graph-out", out["--graph"], "--colors", "file", "--colors-out", out["--colors"], "--links",
                   "--links-out", out["--links"], "--bubbles", "file", "--bubbles-out", out["--bubbles"], "--distances", "file", "--distances-out", out["--distances"]],
            fasta, cwd=d)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert sorted(os.listdir(d)) == sorted(list(names.values()) + ["tiny.fa", "j.bin"])
    serial = {"--graph": ["-f", "gfa1"], "--colors": ["--colors", "file"], "--links": ["--links"], "--bubbles": ["--bubbles", "file"], "--distances": ["--distances", "file"]}
    for flag, args in serial.items():
        want = R.run_graphdump([stream, "-k", "9", "-s", fasta] + args, cwd=d)
        assert want.returncode == 0 and want.stderr == b"" and want.stdout, flag
        assert open(out[flag], "rb").read() == want.stdout, flag


def test_twopaco_default_file_timing_lines_and_refusals(tmp_path, made):
    case, fasta, _, _, gfa1, _, _, _ = inputs("short", made)
    d = str(tmp_path)
    want, _, _, _, _ = D.tsv(gfa1, "file", case["k"], [fasta])
    r = cli(case, ["--tmpdir", d, "--distances", "file"], fasta, cwd=d, env=dict(os.environ, TWOPACO_TIMING="1"))
    assert r.returncode == 0, r.stderr[-400:]
    assert sorted(os.listdir(d)) == ["de_bruijn.bin", "de_bruijn.distances.tsv"]
    err = r.stderr.decode()
    assert "segment distances:" in err and "segment distances fetch:" in err and "distances_kernel_ms" in err and "distance table writing:" in err
    assert open(os.path.join(d, "de_bruijn.distances.tsv"), "rb").read() == want
    os.unlink(os.path.join(d, "de_bruijn.bin"))
    os.unlink(os.path.join(d, "de_bruijn.distances.tsv"))
    # an input the walk refuses: the walk's message, no file
    bad = CASES["edge_k5"]
    r = cli(bad, ["--tmpdir", d, "--distances", "file", "--distances-out", os.path.join(d, "distances.tsv"), "--distances-phylip", os.path.join(d, "d.phy"),
                  "--graph", "gfa1", "--graph-out", os.path.join(d, "graph.gfa")])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: The input is corrupted\n"
    assert os.listdir(d) == []


@pytest.mark.parametrize("filter_bits", ["given", "auto"])
def test_enumerator_distances_in_process(capi, tmp_path, made, filter_bits):
    case, _, _, _, gfa1, _, _, files = inputs("c2_k29", made)
    want, want_phy, _, _, _ = D.tsv(gfa1, "sequence", case["k"], files)
    d = str(tmp_path)
    out, phy = os.path.join(d, "distances.tsv"), os.path.join(d, "d.phy")
    cwd = os.getcwd()
    os.chdir(GOLDEN)   # the colours' labels are the file names as given
    try:
        e = capi.Enumerator([case["fasta"]], case["k"], case["L"] if filter_bits == "given" else "auto", q=case["q"], rounds=case["n_rounds"], tmpdir=d, out=os.path.join(d, "j.bin"), seed=case["seed"], distances="sequence",
                            distances_out=out, distances_phylip=phy)
        e.close()
    finally:
        os.chdir(cwd)
    assert open(out, "rb").read() == want and open(phy, "rb").read() == want_phy


# ------------------------------------------------------------------------------------------------ 5. at size
def test_m2r2_device_distances_equal_the_serial_ones(tmp_path):
    """synth m2r2 at scale 0.18, k = 25, f = 32, seed 12345 (the input of test_gpu_colors.py: 62 files, two presence words per
    row): sha256 of `graphdump --distances file --gpu` == that of the serial `graphdump --distances file` over one junction stream."""
    d = str(tmp_path)
    case = {"name": "m2r2_s018", "fasta": None, "synth": {"workload": "m2r2", "seed": 12345, "scale": 0.18}}
    files = case_files(case, d)
    assert len(files) == 62
    junctions = os.path.join(d, "m2r2.bin")
    r = subprocess.run([R.TWOPACO, "-k", "25", "-f", "32", "-t", "16", "--seed", "12345", "--tmpdir", d, "-o", junctions] + files, capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr[-800:]
    seqs = []
    for f in files:
        seqs += ["-s", f]
    serial, device = os.path.join(d, "serial.tsv"), os.path.join(d, "device.tsv")
    r = subprocess.run([R.GRAPHDUMP, junctions, "-k", "25", "--distances", "file", "--distances-out", serial] + seqs, capture_output=True, timeout=900)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    r = subprocess.run([R.GRAPHDUMP, junctions, "-k", "25", "--distances", "file", "--distances-out", device, "--gpu", "--threads", "16"] + seqs, capture_output=True, timeout=900)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    head = open(serial, "rb").readline().decode().rstrip("\n").split("\t")
    assert head[:4] == ["#twopaco-distances", "1", "by=file", "k=25"] and head[4] == "colors=62"
    segments, edges = D.parse(open(serial, "rb").read())
    print("segments", head[5], "shared by all pairs at least", int(segments.min()), "edges of colour 0", int(edges[0, 0]))
    assert int(head[5].split("=")[1]) > 100_000 and segments.min() > 0 and (np.diag(edges) > 0).all()   # 244 606 segments, a core every pair shares
    assert (sha256_file(device), os.path.getsize(device)) == (sha256_file(serial), os.path.getsize(serial))
