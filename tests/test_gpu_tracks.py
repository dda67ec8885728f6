"""GPU (-m gpu): the presence tracks on the device (csrc/tpc_tracks.hip, the tpc_segments_tracks_* group of include/twopaco_hip.h)
against their definition, restated in tracks_reference.py: first_event, last_event and row of every interval, the per-colour and the
per-depth sums and info[] through the C-ABI on a host stream and a resident stream, for all colours and for each single colour; the
word-boundary input at 1 .. 65 colours and at the threshold between the thread and the wave form; the generated cases at their own
grid and under one and two workgroups (a grid turn inside a run and across run borders); a sequence without events between two that
have some; 8000 colours; the stages it leaves untouched, in both orders; ranges and refusals; and the bytes of `graphdump --tracks
--gpu` and `twopaco --tracks`."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import tracks_reference as R
from helpers import GOLDEN, case_files, golden_cases
from test_gpu_components import ambiguous_positions, cli, host_context, resident_context
from test_gpu_graph_walks import segments as case_segments

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in golden_cases()}
MAXU = (1 << 64) - 1
NAMES = ["rand6_k9_q1", "rand6_k3", "c2_k29", "example_k11", "tr_k25_L28"]
_ORACLES = {}


@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


def golden(name, by="sequence", only=None):
    """(case, fasta, stream bytes, oracle, graphdump's arguments)"""
    case = CASES[name]
    v = R.case_vector(case)
    if (name, by, only) not in _ORACLES:
        _ORACLES[(name, by, only)] = R.Tracks(R.golden_gfa1(v), case["k"], R.lengths_of([case["fasta"]]), by, only)
    return case, os.path.join(GOLDEN, case["fasta"]), open(os.path.join(GOLDEN, case["bin"]), "rb").read(), _ORACLES[(name, by, only)], R.tracks_args(v)


def check_arrays(ctx, color_of_seq, n_colors, only, rows, per_color, per_depth, selected, grid=0):
    """Everything the device holds after a track build == the reference's arrays.  grid: test_tracks_grid for this build."""
    if grid:
        ctx.set_option("test_tracks_grid", grid)
    info = ctx.segments_tracks_build(color_of_seq, n_colors, only)
    n = int(rows[0].size)
    peak = info.pop("peak_bytes")
    assert info == {"intervals": n, "selected": selected, "colors": n_colors, "only": only}
    # what the header promises: 12 B per event during the call, 12 B per interval, 48 B per colour
    assert peak >= 12 * ctx.segments_counts()["events"] + 12 * n + 48 * n_colors
    got = ctx.segments_tracks_fetch_rows()
    for a, want in zip(got, rows):
        assert a.dtype == np.uint32 and a.size == n and (a == want).all()
    got = ctx.segments_tracks_fetch_colors()
    for a, want in zip(got, per_color):
        assert a.dtype == np.uint64 and a.size == n_colors and (a == want).all()
    if only is not None:
        assert all(int(a.sum()) == int(a[only]) for a in got)          # the other colours' entries are 0
    depth = ctx.segments_tracks_fetch_depth()
    for a, want in zip(depth, per_depth):
        assert a.dtype == np.uint64 and a.size == n_colors + 1 and (a == want).all()
    assert int(depth[0].sum()) == n == int(got[0].sum()) and int(depth[1].sum()) == int(got[1].sum())
    if n_colors == 1:
        assert (got[2] == got[3]).all() and (got[2] == got[1]).all()
    assert ctx.kernel_ms("tracks") > 0 and ctx.segments_error() is None
    return got


def check_oracle(ctx, want, grid=0):
    rows, per_color, per_depth = want.arrays()
    return check_arrays(ctx, want.color_of_seq, want.n_colors, want.only, rows, per_color, per_depth, want.selected, grid)


# ------------------------------------------------------------------------------------------------ 1. the arrays by their definition
@pytest.mark.parametrize("source", ["host", "resident"])
@pytest.mark.parametrize("name", NAMES)
def test_track_arrays_by_their_definition(capi, name, source):
    case, fasta, data, want, _ = golden(name)
    ctx = host_context(capi, fasta, data, case["k"]) if source == "host" else resident_context(capi, case, fasta, data)
    assert ctx.segments_error() is None
    n_seq = len(want.seq_name)
    ctx.segments_colors_build(list(range(n_seq)), n_seq)
    edges = check_oracle(ctx, want)[1]
    check_oracle(ctx, want)   # a second build replaces the first
    for c in range(n_seq):
        check_oracle(ctx, golden(name, "sequence", c)[3])
        # edges[c] is ref_edges of the anchor table with ref = c
        assert ctx.segments_anchors_build(list(range(n_seq)), n_seq, c)["ref_edges"] == int(edges[c])
    by_file = golden(name, "file")[3]
    ctx.segments_colors_build([0] * n_seq, 1)
    check_oracle(ctx, by_file)
    check_oracle(ctx, golden(name, "file", 0)[3])
    assert by_file.count() == len(set(by_file.seq))
    if name == "rand6_k9_q1":
        assert want.count() == 3053
    ctx.close()


def test_no_event_at_all(capi):
    text = capi.PackedText.from_fasta([os.path.join(GOLDEN, "rand6.fa")])
    ctx = capi.Context(0)
    ctx.seq_upload(text)
    ctx.segments_build(b"", 9, text.rec_start, text.rec_length)
    n_seq = len(text.rec_start)
    ctx.segments_colors_build([0] * n_seq, 1)
    info = ctx.segments_tracks_build([0] * n_seq, 1)
    assert (info["intervals"], info["selected"], info["colors"], info["only"]) == (0, 0, 1, None)
    assert all(a.size == 0 for a in ctx.segments_tracks_fetch_rows()) and all(a.size == 1 and not a.any() for a in ctx.segments_tracks_fetch_colors())
    assert all(a.size == 2 and not a.any() for a in ctx.segments_tracks_fetch_depth())
    ctx.close()


# ------------------------------------------------------------------------------------------------ 2. the presence words' widths
@pytest.fixture(scope="module")
def boundary(capi, tmp_path_factory):
    """{C: (fasta, stream, gfa1, lengths)} of the first C records of colors_reference's word-boundary input, the stream from the pipeline."""
    d = tmp_path_factory.mktemp("boundary")
    got = {}
    for c in R.BOUNDARY_COLORS:
        fa = R.boundary_fasta(str(d / ("w%d.fa" % c)), c)
        out = str(d / ("w%d.bin" % c))
        e = capi.Enumerator([fa], R.BOUNDARY_K, R.BOUNDARY_L, q=R.BOUNDARY_Q, tmpdir=str(d), out=out, seed=R.BOUNDARY_SEED)
        e.close()
        gfa1 = R.run_graphdump([out, "-k", str(R.BOUNDARY_K), "-s", fa, "-f", "gfa1"], cwd=str(d))
        assert gfa1.returncode == 0 and gfa1.stderr == b""
        got[c] = (fa, out, gfa1.stdout, [len(s) for _, s in R.read_fasta(fa)])
    return got


def boundary_context(capi, boundary, c):
    fa, stream, _, _ = boundary[c]
    return host_context(capi, fa, open(stream, "rb").read(), R.BOUNDARY_K)


@pytest.mark.parametrize("c", R.BOUNDARY_COLORS)
def test_every_width_of_the_presence_words(capi, boundary, c):
    """One word, the last bit of a word, the first bit of the next, two words and three."""
    _, _, gfa1, lengths = boundary[c]
    want = R.Tracks(gfa1, R.BOUNDARY_K, lengths, "sequence")
    assert want.n_colors == c and want.count() >= c
    ctx = boundary_context(capi, boundary, c)
    ctx.segments_colors_build(list(range(c)), c)
    check_oracle(ctx, want)
    for only in sorted({0, c // 2, c - 1}):
        check_oracle(ctx, R.Tracks(gfa1, R.BOUNDARY_K, lengths, "sequence", only=only))
    check_oracle(ctx, want, grid=1)
    ctx.close()


@pytest.mark.parametrize("n_colors,step", [(256, 3), (257, 4), (512, 7), (513, 8)])
def test_the_thresholds_between_the_forms(capi, boundary, n_colors, step):
    """8 words: the last width a thread compares; 9 words: the first a wave compares.  512 colours: the last count whose sums a block
    keeps in LDS; 513: the first that goes to the global bins.  Sequence s has the colour step * s."""
    color_of_seq = [step * s for s in range(65)]
    _, _, gfa1, lengths = boundary[65]
    labels = ["colour %d" % c for c in range(n_colors)]
    want = R.Tracks(gfa1, R.BOUNDARY_K, lengths, color_of_seq=color_of_seq, labels=labels)
    assert want.n_colors == n_colors and want.count() == R.Tracks(gfa1, R.BOUNDARY_K, lengths, "sequence").count()
    ctx = boundary_context(capi, boundary, 65)
    ctx.segments_colors_build(color_of_seq, n_colors)
    check_oracle(ctx, want)
    check_oracle(ctx, want, grid=2)
    check_oracle(ctx, R.Tracks(gfa1, R.BOUNDARY_K, lengths, only=step * 64, color_of_seq=color_of_seq, labels=labels))
    ctx.close()


# ------------------------------------------------------------------------------------------------ 3. the generated cases
def generated(name):
    """(case, colour map, colours)"""
    if name in ("hot", "hot_wide"):
        c = R.hot_case(name == "hot_wide")
    elif name.startswith("different"):
        c = R.different_case(int(name[-1]))
        return c, c.bit_map, c.bit_colours
    elif name == "twins":
        c = R.twins_case()
    elif name == "gap":
        c = R.gap_case()
    else:
        c = R.pair_case(int(name[-1]))
    return c, c.color_of_seq, c.n_colors


@pytest.mark.parametrize("name", ["hot", "hot_wide", "different_1", "different_8", "twins", "pair_1", "pair_2", "gap"])
def test_generated_cases_at_their_own_grid_and_under_one_and_two_workgroups(capi, name):
    """One workgroup strides 5014 events twenty times, two ten times: a grid turn inside a run of one presence and across run borders.
    The numpy statement is pinned to the oracle over the serial gfa1 by tests/test_tracks_cpu.py."""
    c, color_of_seq, n_colors = generated(name)
    ctx = capi.Context(0)
    case_segments(capi, ctx, c)
    ctx.segments_colors_build(color_of_seq, n_colors)
    onlies = [None] + sorted({color_of_seq[0], color_of_seq[-1]})
    for only in onlies:
        rows, per_color, per_depth, selected = R.direct_of(c, only, color_of_seq, n_colors)
        for grid in (0, 1, 2):
            check_arrays(ctx, color_of_seq, n_colors, only, rows, per_color, per_depth, selected, grid)
        if only is None and name.startswith("hot"):
            assert selected == R.HOT_EVENTS
            R.check_hot(rows)
        if only is None and name.startswith("different"):
            assert rows[0].size == selected == c.w.name.size
        if only is None and name.startswith("pair"):
            assert rows[0].tolist() == [0, 40] and rows[1].tolist() == [39, 79] and int(per_depth[0][n_colors]) == 2
        if only is None and name == "gap":
            assert rows[0].tolist() == [0, 4] and rows[1].tolist() == [3, 7] and int(per_color[0][1]) == 0 and c.w.seq_event_begin.tolist() == [0, 4, 4, 8]
        if only is None and name == "twins":
            assert rows[0][:3].tolist() == [0, 5, 6] and rows[1][:3].tolist() == [4, 5, 19]
    ctx.close()


def test_eight_thousand_colours_on_the_hot_case(capi):
    """250 presence words: the wave form, on the hot key, at its own grid and under one workgroup (four events a turn)."""
    c = R.hot_case()
    n_colors = 8000
    color_of_seq = [1000 * s + 999 for s in range(8)]
    ctx = capi.Context(0)
    case_segments(capi, ctx, c)
    ctx.segments_colors_build(color_of_seq, n_colors)
    for only in (None, 999, 7999):
        rows, per_color, per_depth, selected = R.direct_of(c, only, color_of_seq, n_colors)
        check_arrays(ctx, color_of_seq, n_colors, only, rows, per_color, per_depth, selected)
        if only is None:
            R.check_hot(rows)
            check_arrays(ctx, color_of_seq, n_colors, only, rows, per_color, per_depth, selected, grid=1)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 4. opt-in
@pytest.mark.parametrize("order", ["tracks_first", "tracks_last"])
def test_the_other_tables_are_unchanged_by_a_track_build(capi, order):
    case, fasta, data, want, _ = golden("c2_k29")
    n_seq = len(want.seq_name)
    colour_map = list(range(n_seq))

    def build_others(ctx):
        ctx.segments_links_build()
        ctx.segments_distances_build()
        ctx.segments_components_build()
        ctx.segments_classes_build()
        ctx.segments_anchors_build(colour_map, n_seq, 0)

    def outputs(ctx):
        name, first = ctx.segments_fetch()
        begin, end = ctx.segments_fetch_events()
        got = [name, first, begin, end]
        got += list(ctx.segments_colors_fetch_rows()) + [ctx.segments_colors_fetch_presence()] + list(ctx.segments_colors_fetch_hist())
        got += list(ctx.segments_links_fetch_rows()) + [ctx.segments_links_fetch_first()]
        got += list(ctx.segments_distances_fetch())
        got += [ctx.segments_components_fetch_members()] + list(ctx.segments_components_fetch_rows()) + [ctx.segments_components_fetch_presence()]
        got += [ctx.segments_classes_fetch_members()] + list(ctx.segments_classes_fetch_rows()) + [ctx.segments_classes_fetch_presence()]
        got += [ctx.segments_anchors_fetch_mates()] + list(ctx.segments_anchors_fetch_rows()) + list(ctx.segments_anchors_fetch_shared())
        counts = {key: n for key, n in ctx.segments_counts().items() if key != "peak_device_bytes"}
        return counts, ctx.segments_error(), ctx.segments_colors_info(), ctx.segments_links_info(), got

    alone = host_context(capi, fasta, data, case["k"])
    alone.segments_colors_build(colour_map, n_seq)
    build_others(alone)
    ref = outputs(alone)
    with pytest.raises(RuntimeError, match="tpc_segments_tracks_build first"):    # a context that never calls the stage holds none of it
        alone.segments_tracks_info()
    alone.close()
    ctx = host_context(capi, fasta, data, case["k"])
    ctx.segments_colors_build(colour_map, n_seq)
    if order == "tracks_first":
        check_oracle(ctx, want)
        build_others(ctx)
    else:
        build_others(ctx)
        check_oracle(ctx, want)
    for _ in range(2):
        got = outputs(ctx)
        assert got[:4] == ref[:4]
        assert all(a.shape == b.shape and (a == b).all() for a, b in zip(got[4], ref[4]))
        check_oracle(ctx, golden("c2_k29", "sequence", 1)[3])
    # every other build leaves the tracks where they are; a new colour build drops them
    build_others(ctx)
    assert (ctx.segments_tracks_fetch_rows()[0] == golden("c2_k29", "sequence", 1)[3].arrays()[0][0]).all()
    ctx.segments_colors_build([0] * n_seq, 1)
    with pytest.raises(RuntimeError, match="tpc_segments_tracks_build first"):
        ctx.segments_tracks_fetch_rows(0, 0)
    check_oracle(ctx, golden("c2_k29", "file")[3])
    ctx.close()


# ------------------------------------------------------------------------------------------------ 5. ranges and refusals
def test_fetch_ranges(capi):
    case, fasta, data, want, _ = golden("c2_k29")
    ctx = host_context(capi, fasta, data, case["k"])
    n_seq = len(want.seq_name)
    ctx.segments_colors_build(list(range(n_seq)), n_seq)
    n = ctx.segments_tracks_build(list(range(n_seq)), n_seq)["intervals"]
    assert n == want.count() == 280
    rows = want.arrays()[0]
    for a, ref in zip(ctx.segments_tracks_fetch_rows(100, 71), rows):
        assert (a == ref[100:171]).all()
    for a, ref in zip(ctx.segments_tracks_fetch_rows(n - 1, 1), rows):
        assert (a == ref[n - 1:]).all()
    assert all(a.size == 0 for a in ctx.segments_tracks_fetch_rows(n, 0))
    for i0, m in ((n, 1), (n + 1, 0), (0, n + 1), (MAXU, 2)):
        with pytest.raises(RuntimeError, match="segment tracks: bad interval range"):
            ctx.segments_tracks_fetch_rows(i0, m)
    # null pointers
    L, h = capi.hip(), ctx._h
    buf = np.zeros(2 * n_seq + 8, dtype=np.uint64)
    p = buf.ctypes.data
    assert L.tpc_segments_tracks_fetch_rows(h, 0, 1, p, None, p) != 0 and b"bad interval range" in L.tpc_last_error(h)
    assert L.tpc_segments_tracks_fetch_rows(h, 0, 0, None, None, None) == 0      # nothing asked for, nothing needed
    assert L.tpc_segments_tracks_fetch_colors(h, p, p, None, p) != 0 and b"all four per-colour arrays" in L.tpc_last_error(h)
    assert L.tpc_segments_tracks_fetch_depth(h, None, p) != 0 and b"both per-depth arrays" in L.tpc_last_error(h)
    assert L.tpc_segments_tracks_info(h, None) != 0
    check_oracle(ctx, want)   # still usable
    ctx.close()


def test_refusals(capi):
    case, fasta, data, want, _ = golden("c2_k29")
    text = capi.PackedText.from_fasta([fasta])
    n_seq = len(want.seq_name)
    colour_map = list(range(n_seq))
    ctx = capi.Context(0)
    with pytest.raises(RuntimeError, match="^twopaco_hip: segment tracks: build the segment table first"):   # no table
        ctx.segments_tracks_build(colour_map, n_seq)
    for call in (ctx.segments_tracks_info, ctx.segments_tracks_fetch_rows, ctx.segments_tracks_fetch_colors, ctx.segments_tracks_fetch_depth):
        with pytest.raises(RuntimeError, match="^twopaco_hip: segment tracks: tpc_segments_tracks_build first"):
            call()
    # the context is usable: a table, then no colour table yet
    ctx.seq_upload(text)
    ctx.segments_build(data, case["k"], text.rec_start, text.rec_length, ambiguous_positions(fasta, text.rec_start))
    with pytest.raises(RuntimeError, match="^twopaco_hip: segment tracks: build the colour table first"):
        ctx.segments_tracks_build(colour_map, n_seq)
    assert ctx.segments_counts()["events"] > 0 and ctx.segments_error() is None
    ctx.segments_colors_build(colour_map, n_seq)
    check_oracle(ctx, want)
    # a colour table of another colour count; a colour beyond the colours; a one colour beyond them.  A refused build leaves no table.
    for args, text_of in (((colour_map, n_seq + 1), "the colour table holds %d colours, the caller gives %d" % (n_seq, n_seq + 1)),
                          (([0] * n_seq, 1), "the colour table holds %d colours, the caller gives 1" % n_seq),
                          ((colour_map[:-1] + [n_seq], n_seq), "sequence %d has colour %d, there are %d colours" % (n_seq - 1, n_seq, n_seq)),
                          ((colour_map, n_seq, n_seq), "the one colour is %d, there are %d colours" % (n_seq, n_seq)),
                          ((colour_map, n_seq, 0xFFFFFFFE), "the one colour is 4294967294, there are %d colours" % n_seq)):
        with pytest.raises(RuntimeError, match="^twopaco_hip: segment tracks: " + text_of):
            ctx.segments_tracks_build(*args)
        with pytest.raises(RuntimeError, match="tpc_segments_tracks_build first"):
            ctx.segments_tracks_info()
        assert ctx.segments_counts()["events"] > 0 and ctx.segments_colors_info()["colors"] == n_seq
        check_oracle(ctx, want)
    h = ctx._h
    assert capi.hip().tpc_segments_tracks_build(h, None, n_seq, 0xFFFFFFFF) != 0 and capi.hip().tpc_last_error(h).startswith(b"segment tracks: the colour of every one")
    check_oracle(ctx, want)
    # the option holds for one build, whichever way it returns
    ctx.set_option("test_tracks_grid", 1)
    with pytest.raises(RuntimeError, match="^twopaco_hip: segment tracks: the one colour"):
        ctx.segments_tracks_build(colour_map, n_seq, n_seq)
    check_oracle(ctx, want)
    # a new segment build drops the tracks of the old one (and its colours)
    ctx.segments_build(b"", case["k"], text.rec_start, text.rec_length)
    with pytest.raises(RuntimeError, match="tpc_segments_tracks_build first"):
        ctx.segments_tracks_fetch_rows(0, 0)
    with pytest.raises(RuntimeError, match="^twopaco_hip: segment tracks: build the colour table first"):
        ctx.segments_tracks_build(colour_map, n_seq)
    ctx.close()
    # a table whose walk failed
    bad = CASES["edge_k5"]
    ctx = host_context(capi, os.path.join(GOLDEN, bad["fasta"]), open(os.path.join(GOLDEN, bad["bin"]), "rb").read(), bad["k"])
    assert ctx.segments_error() is not None
    with pytest.raises(RuntimeError, match="^twopaco_hip: segment tracks: the segment table holds the walk's error 1 at slot 3"):
        ctx.segments_tracks_build([0], 1)
    with pytest.raises(RuntimeError, match="unknown option"):
        ctx.set_option("test_track_grid", 1)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 6. bytes
def serial_bytes(args, by, tmp_path, cwd, only=None):
    bed = str(tmp_path / "serial.bedgraph")
    r = R.run_graphdump(args + ["--tracks", by, "--tracks-bedgraph", bed] + ([] if only is None else ["--tracks-of", str(only)]), cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    return r.stdout, open(bed, "rb").read()


@pytest.mark.parametrize("by", ["file", "sequence"])
@pytest.mark.parametrize("name", ["rand6_k9_q1", "c2_k29", "example_k11", "boundary_65"])
def test_the_programs_write_the_serial_bytes(tmp_path, boundary, name, by):
    if name == "boundary_65":
        fa, stream, gfa1, lengths = boundary[65]
        case = {"k": R.BOUNDARY_K, "L": R.BOUNDARY_L, "q": R.BOUNDARY_Q, "seed": R.BOUNDARY_SEED, "n_rounds": 1, "abundance": None, "fasta": fa}
        args, cwd, data = [stream, "-k", str(R.BOUNDARY_K), "-s", fa], os.path.dirname(fa), open(stream, "rb").read()
        want = R.Tracks(gfa1, R.BOUNDARY_K, lengths, by)
    else:
        case, _, data, want, args = golden(name, by)
        cwd = GOLDEN
    tsv, bed_text = serial_bytes(args, by, tmp_path, cwd)
    assert tsv == want.tsv() and bed_text == want.bedgraph()
    last = want.n_colors - 1
    tsv_last, bed_last = serial_bytes(args, by, tmp_path, cwd, only=last)
    # graphdump --gpu
    stats, bed = str(tmp_path / "stats.json"), str(tmp_path / "gpu.bedgraph")
    env = dict(os.environ, TWOPACO_GRAPHDUMP_STATS=stats)
    r = subprocess.run([R.GRAPHDUMP] + args + ["--tracks", by, "--tracks-bedgraph", bed, "--gpu", "--threads", "16"], cwd=cwd, capture_output=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert r.stdout == tsv and open(bed, "rb").read() == bed_text
    s = json.load(open(stats))
    assert s["path"] == "device" and s["tracks_kernel_ms"] > 0 and s["track_intervals"] == want.count()
    r = subprocess.run([R.GRAPHDUMP] + args + ["--tracks", by, "--tracks-of", str(last), "--tracks-bedgraph", bed, "--gpu"], cwd=cwd, capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == tsv_last and open(bed, "rb").read() == bed_last
    # beside the other tables of the same colours: each what it is alone, the track table last
    flags = ("--colors", "--distances", "--components", "--anchors", "--classes")
    alone = [R.run_graphdump(args + [flag, by], cwd=cwd).stdout for flag in flags]
    extra = [x for flag in flags for x in (flag, by)]
    r = R.run_graphdump(args + ["--tracks", by, "--gpu"] + extra, cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == b"".join(alone) + tsv
    # twopaco
    d = str(tmp_path / "twopaco")
    os.mkdir(d)
    out = {key: os.path.join(d, key + ".tsv") for key in ("tracks", "bedgraph", "colors", "classes", "anchors")}
    r = cli(case, ["--tmpdir", d, "--tracks", by, "--tracks-out", out["tracks"], "--tracks-bedgraph", out["bedgraph"], "--colors", by, "--colors-out", out["colors"],
                   "--classes", by, "--classes-out", out["classes"], "--anchors", by, "--anchors-out", out["anchors"], "-o", os.path.join(d, "j.bin")], cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert open(os.path.join(d, "j.bin"), "rb").read() == data
    assert open(out["tracks"], "rb").read() == tsv and open(out["bedgraph"], "rb").read() == bed_text
    for key, text in zip(("colors", "classes", "anchors"), (alone[0], alone[4], alone[3])):
        assert open(out[key], "rb").read() == text, key
    assert sorted(os.listdir(d)) == sorted(["j.bin"] + [key + ".tsv" for key in out])
    # ... of one colour, and with the graph text rendered on the device (the table stays there: the sequences' ranges are fetched for the tracks)
    r = cli(case, ["--tmpdir", d, "--tracks", by, "--tracks-of", str(last), "--tracks-out", out["tracks"], "--tracks-bedgraph", out["bedgraph"], "--graph", "gfa1",
                   "--graph-out", os.path.join(d, "g.gfa"), "--graph-text", "device", "-o", os.path.join(d, "j.bin")], cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert open(out["tracks"], "rb").read() == tsv_last and open(out["bedgraph"], "rb").read() == bed_last


def test_twopaco_default_file_timing_lines_and_refusals(tmp_path):
    case, fasta, _, want, _ = golden("c2_k29", "file")
    d = str(tmp_path)
    r = cli(case, ["--tmpdir", d, "--tracks", "file"], fasta, cwd=d, env=dict(os.environ, TWOPACO_TIMING="1"))
    assert r.returncode == 0, r.stderr[-400:]
    assert sorted(os.listdir(d)) == ["de_bruijn.bin", "de_bruijn.tracks.tsv"]
    err = r.stderr.decode()
    assert "segment tracks:" in err and "segment tracks fetch:" in err and "tracks_kernel_ms" in err and "track table writing:" in err
    got = open(os.path.join(d, "de_bruijn.tracks.tsv"), "rb").read()
    assert got.split(b"\n")[0] == b"#twopaco-tracks\t1\tby=file\tk=29\tcolors=1\tsegments=%d\tof=all\tintervals=%d" % (want.rows, want.count())
    os.unlink(os.path.join(d, "de_bruijn.bin"))
    os.unlink(os.path.join(d, "de_bruijn.tracks.tsv"))
    r = cli(case, ["--tmpdir", d, "--tracks", "file", "--gpus", "2"], fasta, cwd=d)
    assert r.returncode == 1 and r.stderr.decode().endswith("not with --gpus above 1 for arg (--tracks)\n") and os.listdir(d) == []
    n_seq = len(want.seq_name)
    r = cli(case, ["--tmpdir", d, "--tracks", "sequence", "--tracks-of", str(n_seq)], fasta, cwd=d)
    assert r.returncode == 1 and "The track table's one colour is %d, there are %d colours" % (n_seq, n_seq) in r.stderr.decode()
    assert not os.path.exists(os.path.join(d, "de_bruijn.tracks.tsv"))


# ------------------------------------------------------------------------------------------------ 7. at size
M2R2_SCALE, M2R2_SEED = 0.05, 450


def test_m2r2_tracks_equal_the_serial_graphdump(tmp_path):
    """synth m2r2 at scale 0.05, synth seed 450, k = 25, f = 32 (the workload of test_gpu_classes.py: 62 files, two presence words):
    sha256 and size of the two files of `twopaco --tracks file` == those of the serial `graphdump --tracks file` over the junction
    stream of the same command; the text alone is checked as a tiling with the right sums."""
    d = str(tmp_path)
    case = {"name": "m2r2_tracks", "fasta": None, "synth": {"workload": "m2r2", "seed": M2R2_SEED, "scale": M2R2_SCALE}}
    files = case_files(case, d)
    assert len(files) == 62
    junctions, table, bed = os.path.join(d, "m2r2.bin"), os.path.join(d, "tracks.tsv"), os.path.join(d, "tracks.bedgraph")
    r = subprocess.run([R.TWOPACO, "-k", "25", "-f", "32", "-t", "16", "--seed", "12345", "--tmpdir", d, "-o", junctions, "--tracks", "file", "--tracks-out", table,
                        "--tracks-bedgraph", bed] + files, capture_output=True, timeout=900)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-800:]
    seqs = []
    for f in files:
        seqs += ["-s", f]
    serial, serial_bed = os.path.join(d, "serial.tsv"), os.path.join(d, "serial.bedgraph")
    r = subprocess.run([R.GRAPHDUMP, junctions, "-k", "25", "--tracks", "file", "--tracks-out", serial, "--tracks-bedgraph", serial_bed] + seqs, capture_output=True, timeout=900)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    for mine, theirs in ((table, serial), (bed, serial_bed)):
        got, ref = open(mine, "rb").read(), open(theirs, "rb").read()
        assert len(got) == len(ref) and hashlib.sha256(got).hexdigest() == hashlib.sha256(ref).hexdigest()
    got = open(table, "rb").read()
    head = dict(f.split("=") for f in got.split(b"\n", 1)[0].decode().split("\t")[2:])
    assert (head["by"], head["k"], head["colors"], head["of"]) == ("file", "25", "62", "all") and int(head["intervals"]) > 62
    count, edges = R.check_text(got, open(bed, "rb").read())
    print("intervals", count, "edges", sum(edges.values()))
