"""GPU (-m gpu): the colour classes on the device (csrc/tpc_classes.hip, the tpc_segments_classes_* group of include/twopaco_hip.h)
against their definition, restated in classes_reference.py over the serial gfa1 text (pinned to the real reference's sha256 by
tests/golden/graphdump.json): class[], every plane of the rows, presence, the per-n sets and info[] through the C-ABI on a host
stream and a resident stream; every key width in both row forms; the hot key past a grid turn; long chains, a set that is exactly
full and one that is too small (an error return from kernels that end normally); the stages it leaves untouched; ranges and
refusals; and the bytes of `graphdump --classes --gpu` and `twopaco --classes`."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import classes_reference as R
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


def golden(name, by="sequence"):
    """(case, fasta, stream bytes, oracle, graphdump's arguments)"""
    case = CASES[name]
    v = R.case_vector(case)
    if (name, by) not in _ORACLES:
        _ORACLES[(name, by)] = R.Classes(R.golden_gfa1(v), by, k=case["k"])
    return case, os.path.join(GOLDEN, case["fasta"]), open(os.path.join(GOLDEN, case["bin"]), "rb").read(), _ORACLES[(name, by)], R.classes_args(v)


def check_table(ctx, want, **options):
    """Everything the device holds after a class build == the oracle's.  options: test_classes_* for this build."""
    for key, value in options.items():
        ctx.set_option("test_classes_" + key, value)
    info = ctx.segments_classes_build()
    assert (info["classes"], info["rows"], info["largest"]) == (want.count(), want.rows, want.largest())
    colors = want.colors["colors"]
    words = (colors + 31) // 32
    # what the header promises: 4 B per row kept and 8 B per row during the call, per class 36 B and its words, the sets
    assert info["peak_bytes"] >= 12 * want.rows + want.count() * (36 + 4 * words) + 24 * (colors + 1)
    class_of = ctx.segments_classes_fetch_members()
    assert class_of.dtype == np.uint32 and class_of.size == want.rows and (class_of == want.class_of).all()
    first, segments, length, edges, occurrences = ctx.segments_classes_fetch_rows()
    assert first.dtype == np.uint32 and all(a.dtype == np.uint64 for a in (segments, length, edges, occurrences))
    for got, ref in ((first, want.first), (segments, want.segments), (length, want.length), (edges, want.edges), (occurrences, want.occurrences)):
        assert got.size == ref.size and (got.astype(np.int64) == ref).all()
    presence = ctx.segments_classes_fetch_presence()
    assert presence.dtype == np.uint32 and presence.shape == (want.count(), words)
    if want.count():
        assert (presence == R.presence_words(want.presence)).all()
        assert (np.unpackbits(presence.view(np.uint8), axis=1).sum(axis=1) == want.n_colors).all()
    sets = ctx.segments_classes_fetch_sets()
    for got, ref in zip(sets, (want.sets_classes, want.sets_segments, want.sets_edges)):
        assert got.dtype == np.uint64 and got.size == colors + 1 and (got.astype(np.int64) == ref).all()
    assert int(segments.sum()) == want.rows and int(sets[0].sum()) == want.count()
    assert ctx.kernel_ms("classes") > 0
    return info


# ------------------------------------------------------------------------------------------------ 1. the arrays by their definition
@pytest.mark.parametrize("source", ["host", "resident"])
@pytest.mark.parametrize("name", NAMES)
def test_class_arrays_by_their_definition(capi, name, source):
    case, fasta, data, want, _ = golden(name)
    ctx = host_context(capi, fasta, data, case["k"]) if source == "host" else resident_context(capi, case, fasta, data)
    assert ctx.segments_error() is None
    n_seq = len(want.g.seq_name)
    ctx.segments_colors_build(list(range(n_seq)), n_seq)
    check_table(ctx, want)
    check_table(ctx, want)   # a second build replaces the first
    hist = ctx.segments_colors_fetch_hist()[0]
    assert (ctx.segments_classes_fetch_sets()[1] == hist).all()    # the per-n segments are the colour table's histogram
    by_file = golden(name, "file")[3]
    ctx.segments_colors_build([0] * n_seq, 1)
    assert check_table(ctx, by_file)["classes"] == 1
    if name == "rand6_k9_q1":
        assert (want.count(), want.rows) == (50, 1474)
    ctx.close()


def test_no_event_at_all(capi):
    text = capi.PackedText.from_fasta([os.path.join(GOLDEN, "rand6.fa")])
    ctx = capi.Context(0)
    ctx.seq_upload(text)
    ctx.segments_build(b"", 9, text.rec_start, text.rec_length)
    ctx.segments_colors_build([0] * len(text.rec_start), 1)
    info = ctx.segments_classes_build()
    assert (info["classes"], info["rows"], info["largest"], info["collisions"]) == (0, 0, 0, 0)
    assert ctx.segments_classes_fetch_members().size == 0 and all(a.size == 0 for a in ctx.segments_classes_fetch_rows())
    assert ctx.segments_classes_fetch_presence().shape == (0, 1) and all((a == 0).all() and a.size == 2 for a in ctx.segments_classes_fetch_sets())
    ctx.close()


# ------------------------------------------------------------------------------------------------ 2. key widths, both row forms
@pytest.fixture(scope="module")
def boundary(capi, tmp_path_factory):
    """{C: (fasta, stream, gfa1)} of the first C records of colors_reference's word-boundary input, the stream from the pipeline."""
    d = tmp_path_factory.mktemp("boundary")
    got = {}
    for c in R.BOUNDARY_COLORS:
        fa = R.boundary_fasta(str(d / ("w%d.fa" % c)), c)
        out = str(d / ("w%d.bin" % c))
        e = capi.Enumerator([fa], R.BOUNDARY_K, R.BOUNDARY_L, q=R.BOUNDARY_Q, tmpdir=str(d), out=out, seed=R.BOUNDARY_SEED)
        e.close()
        gfa1 = R.run_graphdump([out, "-k", str(R.BOUNDARY_K), "-s", fa, "-f", "gfa1"], cwd=str(d))
        assert gfa1.returncode == 0 and gfa1.stderr == b""
        got[c] = (fa, out, gfa1.stdout)
    return got


def boundary_context(capi, boundary, c):
    fa, stream, _ = boundary[c]
    return host_context(capi, fa, open(stream, "rb").read(), R.BOUNDARY_K)


@pytest.mark.parametrize("c", R.BOUNDARY_COLORS)
def test_every_key_width_in_both_forms(capi, boundary, c):
    """One word, the last bit of a word, the first bit of the next, two words (the keyed slots) and three (rows in the slots)."""
    want = R.Classes(boundary[c][2], "sequence", k=R.BOUNDARY_K)
    assert want.colors["colors"] == c and want.presence.any(axis=0).all()
    ctx = boundary_context(capi, boundary, c)
    ctx.segments_colors_build(list(range(c)), c)
    check_table(ctx, want, wide=1)
    check_table(ctx, want, wide=2)
    check_table(ctx, want)
    if c == 65:
        assert (want.count(), want.rows, want.largest()) == (425, 597, 36)
    ctx.close()


@pytest.mark.parametrize("n_colors,step", [(256, 3), (257, 4)])
def test_the_threshold_between_the_forms(capi, boundary, n_colors, step):
    """8 words: the last width a thread reads; 9 words: the first a wave reads.  Sequence s has the colour step * s."""
    color_of_seq = [step * s for s in range(65)]
    want = R.Classes(boundary[65][2], k=R.BOUNDARY_K, color_of_seq=color_of_seq, n_colors=n_colors)
    assert want.presence[:, n_colors - 1 if step == 4 else 192].any() and want.count() == 425
    ctx = boundary_context(capi, boundary, 65)
    ctx.segments_colors_build(color_of_seq, n_colors)
    check_table(ctx, want)
    ctx.close()


def test_more_than_four_thousand_colours(capi):
    """8000 colours, 250 words a key, more bins of sets than a block keeps in LDS; the wave form by itself, then both forced."""
    case, fasta, data, _, _ = golden("rand6_k9_q1")
    n_seq = 6
    wide = [1000 * s + 999 for s in range(n_seq)]
    n_colors = 1000 * n_seq + 2000
    want = R.Classes(R.golden_gfa1(R.case_vector(case)), k=case["k"], color_of_seq=wide, n_colors=n_colors)
    assert want.count() == 50
    ctx = host_context(capi, fasta, data, case["k"])
    ctx.segments_colors_build(wide, n_colors)
    check_table(ctx, want)
    check_table(ctx, want, wide=1)
    check_table(ctx, want, wide=2)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 3. the hot key
@pytest.mark.parametrize("wide_map", [False, True], ids=["one_word", "three_words"])
def test_the_hot_key_past_a_grid_turn(capi, wide_map):
    """5000 rows of one class, 7 others at the first row, the last row and wave borders; four workgroups: 1024 threads stride five
    times over 5007 rows, 16 waves more than three hundred times."""
    c = R.hot_case(wide_map)
    want = R.Classes(c.gfa1(), k=c.k, color_of_seq=c.color_of_seq, n_colors=c.n_colors)
    R.check_hot(want)
    ctx = capi.Context(0)
    case_segments(capi, ctx, c)
    ctx.segments_colors_build(c.color_of_seq, c.n_colors)
    for form in (2, 1):
        info = check_table(ctx, want, grid=4, wide=form)
        assert info["largest"] == 5000
    check_table(ctx, want)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 4. chains, a full set, a set too small
@pytest.mark.parametrize("bits", [0, 1, 4])
@pytest.mark.parametrize("name", ["different_1", "different_8", "boundary_65"])
def test_chains_leave_the_tables_unchanged(capi, boundary, name, bits):
    """Only the low `bits` bits of the hash: 1, 2 or 16 home slots for hundreds of classes."""
    if name == "boundary_65":
        want = R.Classes(boundary[65][2], "sequence", k=R.BOUNDARY_K)
        ctx = boundary_context(capi, boundary, 65)
        ctx.segments_colors_build(list(range(65)), 65)
    else:
        c = R.different_case(int(name[-1]))
        want = R.Classes(c.gfa1(), k=c.k, color_of_seq=c.bit_map, n_colors=c.bit_colours)
        assert want.count() == want.rows == R.DIFFERENT_ROWS
        ctx = capi.Context(0)
        case_segments(capi, ctx, c)
        ctx.segments_colors_build(c.bit_map, c.bit_colours)
    for form in (2, 1):
        info = check_table(ctx, want, hash_bits=bits, wide=form)
        assert info["collisions"] > 0
    ctx.close()


@pytest.mark.parametrize("stride", [1, 8], ids=["keyed", "rows"])
def test_a_full_set_and_a_set_too_small(capi, stride):
    """256 classes in 2^8 slots: every slot taken, the table right.  In 2^7 slots: the error text, from kernels that end normally;
    the context stays usable and the next build, which runs without the option, gives the right table."""
    c = R.different_case(stride)
    want = R.Classes(c.gfa1(), k=c.k, color_of_seq=c.bit_map, n_colors=c.bit_colours)
    assert want.count() == 256
    ctx = capi.Context(0)
    case_segments(capi, ctx, c)
    ctx.segments_colors_build(c.bit_map, c.bit_colours)
    before = list(ctx.segments_colors_fetch_rows()) + [ctx.segments_colors_fetch_presence()]
    for form in (2, 1):
        check_table(ctx, want, slots_log2=8, wide=form)
        ctx.set_option("test_classes_slots_log2", 7)
        ctx.set_option("test_classes_wide", form)
        with pytest.raises(RuntimeError, match="segment classes: gave up after 128 probes"):
            ctx.segments_classes_build()
        with pytest.raises(RuntimeError, match="tpc_segments_classes_build first"):   # the failed build left no table
            ctx.segments_classes_info()
        assert all((a == b).all() for a, b in zip(before, list(ctx.segments_colors_fetch_rows()) + [ctx.segments_colors_fetch_presence()]))
        check_table(ctx, want)
    for name, value in (("slots_log2", 32), ("slots_log2", -1), ("hash_bits", 65), ("wide", 3)):
        ctx.set_option("test_classes_" + name, value)
        with pytest.raises(RuntimeError, match="segment classes: option test_classes_" + name):
            ctx.segments_classes_build()
        check_table(ctx, want)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 5. opt-in
def test_the_other_tables_are_unchanged_and_a_new_colour_map_gives_its_classes(capi):
    case, fasta, data, want, _ = golden("c2_k29")
    n_seq = len(want.g.seq_name)

    def build_others(ctx):
        ctx.segments_colors_build(list(range(n_seq)), n_seq)
        ctx.segments_links_build()
        ctx.segments_distances_build()
        ctx.segments_components_build()

    def outputs(ctx):
        name, first = ctx.segments_fetch()
        begin, end = ctx.segments_fetch_events()
        got = [name, first, begin, end]
        got += list(ctx.segments_colors_fetch_rows()) + [ctx.segments_colors_fetch_presence()] + list(ctx.segments_colors_fetch_hist())
        got += list(ctx.segments_links_fetch_rows()) + [ctx.segments_links_fetch_first()]
        got += list(ctx.segments_distances_fetch())
        got += [ctx.segments_components_fetch_members()] + list(ctx.segments_components_fetch_rows()) + [ctx.segments_components_fetch_presence()]
        counts = {key: n for key, n in ctx.segments_counts().items() if key != "peak_device_bytes"}
        return counts, ctx.segments_error(), ctx.segments_colors_info(), ctx.segments_links_info(), got

    alone = host_context(capi, fasta, data, case["k"])
    build_others(alone)
    ref = outputs(alone)
    with pytest.raises(RuntimeError, match="tpc_segments_classes_build first"):    # a context that never calls the stage holds none of it
        alone.segments_classes_info()
    alone.close()
    ctx = host_context(capi, fasta, data, case["k"])
    ctx.segments_colors_build(list(range(n_seq)), n_seq)
    check_table(ctx, want)              # the classes first, the other stages behind them
    ctx.segments_links_build()
    ctx.segments_distances_build()
    ctx.segments_components_build()
    for _ in range(2):
        check_table(ctx, want)
        got = outputs(ctx)
        assert got[:4] == ref[:4]
        assert all(a.shape == b.shape and (a == b).all() for a, b in zip(got[4], ref[4]))
    # the distance matrices are the sums over the classes that hold both colours
    seg, edg = ctx.segments_distances_fetch()
    want_seg, want_edg = want.matrices()
    assert (seg.astype(np.int64) == want_seg).all() and (edg.astype(np.int64) == want_edg).all()
    # a link, distance or component build leaves the classes where they are; a new colour build drops them
    ctx.segments_links_build()
    ctx.segments_distances_build()
    assert (ctx.segments_classes_fetch_members() == want.class_of).all()
    other = [s % 2 for s in range(n_seq)]
    ctx.segments_colors_build(other, 2)
    with pytest.raises(RuntimeError, match="tpc_segments_classes_build first"):
        ctx.segments_classes_fetch_members(0, 0)
    theirs = R.Classes(R.golden_gfa1(R.case_vector(case)), k=case["k"], color_of_seq=other, n_colors=2)
    assert theirs.count() != want.count()
    check_table(ctx, theirs)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 6. ranges and refusals
def test_fetch_ranges(capi):
    case, fasta, data, want, _ = golden("c2_k29")
    ctx = host_context(capi, fasta, data, case["k"])
    n_seq = len(want.g.seq_name)
    ctx.segments_colors_build(list(range(n_seq)), n_seq)
    n, rows = ctx.segments_classes_build()["classes"], want.rows
    assert n == want.count() == 7
    assert (ctx.segments_classes_fetch_members(100, 71) == want.class_of[100:171]).all()
    assert ctx.segments_classes_fetch_members(rows, 0).size == 0
    for r0, m in ((rows, 1), (rows + 1, 0), (0, rows + 1), (MAXU, 2)):
        with pytest.raises(RuntimeError, match="segment classes: bad row range"):
            ctx.segments_classes_fetch_members(r0, m)
    got = ctx.segments_classes_fetch_rows(1, 2)
    for a, ref in zip(got, (want.first, want.segments, want.length, want.edges, want.occurrences)):
        assert (a.astype(np.int64) == ref[1:3]).all()
    assert (ctx.segments_classes_fetch_presence(2, 2) == R.presence_words(want.presence)[2:4]).all()
    assert all(a.size == 0 for a in ctx.segments_classes_fetch_rows(n, 0)) and ctx.segments_classes_fetch_presence(n, 0).shape[0] == 0
    for p0, m in ((n, 1), (n + 1, 0), (0, n + 1), (MAXU, 2)):
        with pytest.raises(RuntimeError, match="segment classes: bad class range"):
            ctx.segments_classes_fetch_rows(p0, m)
        with pytest.raises(RuntimeError, match="segment classes: bad class range"):
            ctx.segments_classes_fetch_presence(p0, m)
    # null pointers with n > 0
    L, h = capi.hip(), ctx._h
    assert L.tpc_segments_classes_fetch_members(h, 0, 1, None) != 0 and b"bad row range" in L.tpc_last_error(h)
    buf = np.zeros(8, dtype=np.uint64)
    assert L.tpc_segments_classes_fetch_rows(h, 0, 1, None, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data) != 0
    assert L.tpc_segments_classes_fetch_rows(h, 0, 1, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None) != 0
    assert L.tpc_segments_classes_fetch_presence(h, 0, 1, None) != 0 and b"bad class range" in L.tpc_last_error(h)
    assert L.tpc_segments_classes_fetch_sets(h, buf.ctypes.data, None, buf.ctypes.data) != 0 and b"all three arrays" in L.tpc_last_error(h)
    assert L.tpc_segments_classes_info(h, None) != 0
    assert L.tpc_segments_classes_fetch_rows(h, 0, 0, None, None, None, None, None) == 0      # nothing asked for, nothing needed
    check_table(ctx, want)   # still usable
    ctx.close()


def test_refusals(capi):
    case, fasta, data, want, _ = golden("c2_k29")
    text = capi.PackedText.from_fasta([fasta])
    n_seq = len(want.g.seq_name)
    ctx = capi.Context(0)
    with pytest.raises(RuntimeError, match="segment classes: build the segment table first"):   # no table
        ctx.segments_classes_build()
    for call in (ctx.segments_classes_info, ctx.segments_classes_fetch_members, ctx.segments_classes_fetch_rows, ctx.segments_classes_fetch_presence):
        with pytest.raises(RuntimeError, match="tpc_segments_classes_build first"):
            call()
    # the context is usable: a table, then no colour table yet
    ctx.seq_upload(text)
    ctx.segments_build(data, case["k"], text.rec_start, text.rec_length, ambiguous_positions(fasta, text.rec_start))
    with pytest.raises(RuntimeError, match="segment classes: build the colour table first"):
        ctx.segments_classes_build()
    with pytest.raises(RuntimeError, match="tpc_segments_classes_build first"):
        ctx.segments_classes_info()
    assert ctx.segments_counts()["events"] > 0 and ctx.segments_error() is None
    ctx.segments_colors_build(list(range(n_seq)), n_seq)
    check_table(ctx, want)
    # a new segment build drops the classes of the old one (and its colours)
    ctx.segments_build(b"", case["k"], text.rec_start, text.rec_length)
    with pytest.raises(RuntimeError, match="tpc_segments_classes_build first"):
        ctx.segments_classes_fetch_members(0, 0)
    with pytest.raises(RuntimeError, match="segment classes: build the colour table first"):
        ctx.segments_classes_build()
    ctx.close()
    # a table whose walk failed
    bad = CASES["edge_k5"]
    ctx = host_context(capi, os.path.join(GOLDEN, bad["fasta"]), open(os.path.join(GOLDEN, bad["bin"]), "rb").read(), bad["k"])
    assert ctx.segments_error() is not None
    with pytest.raises(RuntimeError, match="segment classes: the segment table holds the walk's error 1 at slot 3"):
        ctx.segments_classes_build()
    with pytest.raises(RuntimeError, match="unknown option"):
        ctx.set_option("test_classes_slot_log2", 1)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 7. bytes
def serial_bytes(args, by, tmp_path, cwd):
    members = str(tmp_path / "serial_members.tsv")
    r = R.run_graphdump(args + ["--classes", by, "--classes-members", members], cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    return r.stdout, open(members, "rb").read()


@pytest.mark.parametrize("by", ["file", "sequence"])
@pytest.mark.parametrize("name", ["rand6_k9_q1", "c2_k29", "boundary_65"])
def test_the_programs_write_the_serial_bytes(tmp_path, boundary, name, by):
    if name == "boundary_65":
        fa, stream, gfa1 = boundary[65]
        case = {"k": R.BOUNDARY_K, "L": R.BOUNDARY_L, "q": R.BOUNDARY_Q, "seed": R.BOUNDARY_SEED, "n_rounds": 1, "abundance": None, "fasta": fa}
        args, cwd, data = [stream, "-k", str(R.BOUNDARY_K), "-s", fa], os.path.dirname(fa), open(stream, "rb").read()
        want = R.Classes(gfa1, by, k=R.BOUNDARY_K, files=[fa])
    else:
        case, _, data, want, args = golden(name, by)
        cwd = GOLDEN
    tsv, members_text = serial_bytes(args, by, tmp_path, cwd)
    assert tsv == want.tsv() and members_text == want.members()
    # graphdump --gpu
    stats, members = str(tmp_path / "stats.json"), str(tmp_path / "members.tsv")
    env = dict(os.environ, TWOPACO_GRAPHDUMP_STATS=stats)
    r = subprocess.run([R.GRAPHDUMP] + args + ["--classes", by, "--classes-members", members, "--gpu", "--threads", "16"], cwd=cwd, capture_output=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert r.stdout == tsv and open(members, "rb").read() == members_text
    s = json.load(open(stats))
    assert s["path"] == "device" and s["classes_kernel_ms"] > 0 and s["classes"] == want.count() and s["largest_class"] == want.largest()
    # beside the other tables of the same colours: each what it is alone, the class table last
    flags = ("--colors", "--distances", "--components")
    alone = [R.run_graphdump(args + [flag, by], cwd=cwd).stdout for flag in flags]
    extra = [x for flag in flags for x in (flag, by)]
    r = R.run_graphdump(args + ["--classes", by, "--gpu"] + extra, cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == b"".join(alone) + tsv
    # twopaco
    d = str(tmp_path / "twopaco")
    os.mkdir(d)
    out = {key: os.path.join(d, key + ".tsv") for key in ("classes", "members", "colors", "distances", "components")}
    r = cli(case, ["--tmpdir", d, "--classes", by, "--classes-out", out["classes"], "--classes-members", out["members"], "--colors", by, "--colors-out", out["colors"],
                   "--distances", by, "--distances-out", out["distances"], "--components", by, "--components-out", out["components"], "-o", os.path.join(d, "j.bin")], cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert open(os.path.join(d, "j.bin"), "rb").read() == data
    assert open(out["classes"], "rb").read() == tsv and open(out["members"], "rb").read() == members_text
    for key, text in zip(("colors", "distances", "components"), alone):
        assert open(out[key], "rb").read() == text, key
    assert sorted(os.listdir(d)) == sorted(["j.bin"] + [key + ".tsv" for key in out])


def test_twopaco_default_file_timing_lines_and_refusals(tmp_path):
    case, fasta, _, want, _ = golden("c2_k29", "file")
    d = str(tmp_path)
    r = cli(case, ["--tmpdir", d, "--classes", "file"], fasta, cwd=d, env=dict(os.environ, TWOPACO_TIMING="1"))
    assert r.returncode == 0, r.stderr[-400:]
    assert sorted(os.listdir(d)) == ["de_bruijn.bin", "de_bruijn.classes.tsv"]
    err = r.stderr.decode()
    assert "segment classes:" in err and "segment classes fetch:" in err and "classes_kernel_ms" in err and "class table writing:" in err
    got = open(os.path.join(d, "de_bruijn.classes.tsv"), "rb").read()
    assert got.split(b"\n")[0] == b"#twopaco-classes\t1\tby=file\tk=29\tcolors=1\tsegments=%d\tclasses=1" % want.rows
    os.unlink(os.path.join(d, "de_bruijn.bin"))
    os.unlink(os.path.join(d, "de_bruijn.classes.tsv"))
    r = cli(case, ["--tmpdir", d, "--classes", "file", "--gpus", "2"], fasta, cwd=d)
    assert r.returncode == 1 and r.stderr.decode().endswith("not with --gpus above 1 for arg (--classes)\n") and os.listdir(d) == []


# ------------------------------------------------------------------------------------------------ 8. at size
M2R2_SCALE, M2R2_SEED = 0.05, 450


def test_m2r2_classes_equal_the_serial_graphdump(tmp_path):
    """synth m2r2 at scale 0.05, synth seed 450, k = 25, f = 32 (the workload of test_gpu_components.py: 62 files, two words a key):
    sha256 and size of `twopaco --classes file` == those of the serial `graphdump --classes file` over the junction stream of the same
    command; and the two matrices rebuilt from the class table -- segments and edges summed over the classes that hold both colours --
    equal the distance table the same process wrote, which is what tpc_segments_distances_fetch gave it."""
    d = str(tmp_path)
    case = {"name": "m2r2_classes", "fasta": None, "synth": {"workload": "m2r2", "seed": M2R2_SEED, "scale": M2R2_SCALE}}
    files = case_files(case, d)
    assert len(files) == 62
    junctions, table, distances = os.path.join(d, "m2r2.bin"), os.path.join(d, "classes.tsv"), os.path.join(d, "distances.tsv")
    r = subprocess.run([R.TWOPACO, "-k", "25", "-f", "32", "-t", "16", "--seed", "12345", "--tmpdir", d, "-o", junctions, "--classes", "file", "--classes-out", table,
                        "--distances", "file", "--distances-out", distances] + files, capture_output=True, timeout=900)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-800:]
    seqs = []
    for f in files:
        seqs += ["-s", f]
    serial = os.path.join(d, "serial.tsv")
    r = subprocess.run([R.GRAPHDUMP, junctions, "-k", "25", "--classes", "file", "--classes-out", serial] + seqs, capture_output=True, timeout=900)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    got, ref = open(table, "rb").read(), open(serial, "rb").read()
    assert len(got) == len(ref) and hashlib.sha256(got).hexdigest() == hashlib.sha256(ref).hexdigest()
    head = dict(f.split("=") for f in ref.split(b"\n", 1)[0].decode().split("\t")[2:])
    assert (head["by"], head["k"], head["colors"]) == ("file", "25", "62") and int(head["classes"]) > 62
    rows = [line.split("\t") for line in got.decode().split("\n") if line and not line.startswith("#")]
    bits = np.array([[int(digit, 16) >> b & 1 for digit in r[7] for b in range(4)][:62] for r in rows], dtype=np.int64)
    segments, edges = np.array([int(r[2]) for r in rows]), np.array([int(r[4]) for r in rows])
    assert int(segments.sum()) == int(head["segments"])
    seg, edg = bits.T @ (bits * segments[:, None]), bits.T @ (bits * edges[:, None])
    print("segments", head["segments"], "classes", head["classes"], "largest", int(segments.max()))
    for line in open(distances).read().split("\n"):
        f = line.split("\t")
        if f[0] == "#self":
            assert (seg[int(f[1]), int(f[1])], edg[int(f[1]), int(f[1])]) == (int(f[2]), int(f[3])), line
        elif line and not line.startswith("#"):
            assert (seg[int(f[0]), int(f[1])], edg[int(f[0]), int(f[1])]) == (int(f[2]), int(f[3])), line
