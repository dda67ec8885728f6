"""GPU (-m gpu): the segment colour table on the device (csrc/tpc_colors.hip, the tpc_segments_colors_* group of
include/twopaco_hip.h) against its definition, restated in colors_reference.py over the serial gfa1 text (pinned to the real
reference's sha256 by tests/golden/graphdump.json): the arrays through the C-ABI, the word boundaries of the presence bits,
ranges and refusals, the build it leaves untouched, and the bytes of `graphdump --colors --gpu` and `twopaco --colors`."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import colors_reference as R
from helpers import GOLDEN, case_files, golden_cases, sha256_file

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in golden_cases()}
MAXU = (1 << 64) - 1


@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


def read_fasta(path):
    recs = []
    for line in open(path):
        if line.startswith(">"):
            recs.append([])
        else:
            recs[-1].append("".join(line.split()).upper())
    return ["".join(r) for r in recs]


def ambiguous_positions(seqs, rec_start):
    return [int(rec_start[r]) + i for r, s in enumerate(seqs) for i, ch in enumerate(s) if ch not in "ACGTN"]


def host_context(capi, fasta, data, k):
    """A context used for nothing else, the table from the stream's bytes."""
    text = capi.PackedText.from_fasta([fasta])
    ctx = capi.Context(0)
    ctx.seq_upload(text)
    ctx.segments_build(data, k, text.rec_start, text.rec_length, ambiguous_positions(read_fasta(fasta), text.rec_start))
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
    ctx.segments_build(None, case["k"], text.rec_start, text.rec_length, ambiguous_positions(read_fasta(fasta), text.rec_start))
    return ctx


def check_table(ctx, g, color_of_seq, n_colors, k):
    """Everything the device holds after a colours build == the oracle's table of the same colour map."""
    t = R.table(g, color_of_seq, n_colors)
    rows = len(t["name"])
    info = ctx.segments_colors_build(color_of_seq, n_colors)
    assert info == {"rows": rows, "colors": n_colors, "words": (n_colors + 31) // 32}
    first, occ, fwd, ncol = ctx.segments_colors_fetch_rows()
    name, first_bits = ctx.segments_fetch()
    begin, end = ctx.segments_fetch_events()
    assert first.dtype == occ.dtype == fwd.dtype == ncol.dtype == np.uint32
    assert (first == np.nonzero(first_bits)[0]).all()
    assert (np.abs(name[first]) == t["name"]).all()
    assert (end[first].astype(np.int64) - begin[first] + k == t["length"]).all()
    assert (occ == t["occurrences"]).all() and (fwd == t["forward"]).all() and (ncol == t["n_colors"]).all()
    presence = ctx.segments_colors_fetch_presence()
    assert presence.dtype == np.uint32 and presence.shape == (rows, (n_colors + 31) // 32)
    assert (presence == R.presence_words(t["presence"])).all()
    seg, bases = ctx.segments_colors_fetch_hist()
    assert seg.dtype == bases.dtype == np.uint64 and seg.size == bases.size == n_colors + 1
    assert (seg == t["hist_segments"]).all() and (bases == t["hist_bases"]).all()
    assert int(seg.sum()) == rows and seg[0] == 0
    assert ctx.kernel_ms("colors") > 0
    return t


# ------------------------------------------------------------------------------------------------ 1. the arrays by their definition
@pytest.mark.parametrize("source", ["host", "resident"])
@pytest.mark.parametrize("name", ["tr_k25_L28", "rand6_k3", "rand6_k9_fp", "c2_k29"])
def test_colour_arrays_by_their_definition(capi, name, source):
    case = CASES[name]
    fasta = os.path.join(GOLDEN, case["fasta"])
    data = open(os.path.join(GOLDEN, case["bin"]), "rb").read()
    g = R.Gfa1(R.golden_gfa1(R.case_vector(case)))
    n_seq = len(g.seq_name)
    ctx = host_context(capi, fasta, data, case["k"]) if source == "host" else resident_context(capi, case, fasta, data)
    assert ctx.segments_error() is None
    t = check_table(ctx, g, list(range(n_seq)), n_seq, case["k"])                 # by sequence
    check_table(ctx, g, [0] * n_seq, 1, case["k"])                                # by file: one file
    # an arbitrary map: the first two sequences share colour 0, colour 1 stays empty
    assert n_seq >= 2
    arbitrary = [0, 0] + list(range(2, n_seq))
    ta = check_table(ctx, g, arbitrary, n_seq + 1, case["k"])
    assert not ta["presence"][:, 1].any() and ta["presence"][:, 0].any()
    # more bins than a block keeps in LDS (2048): the histogram by global atomics
    wide = [1000 * s + 999 for s in range(n_seq)]
    check_table(ctx, g, wide, 1000 * n_seq + 2000, case["k"])
    if name == "tr_k25_L28":
        assert int(t["occurrences"].max()) == 4201
    if name == "rand6_k9_fp":
        assert (t["name"] >= R.FRESH).sum() == 17 and (t["n_colors"] > 1).sum() == 820
    if name == "rand6_k3":
        assert (t["occurrences"] > t["n_colors"]).sum() >= 138
    ctx.close()


# ------------------------------------------------------------------------------------------------ 2. word boundaries of presence
@pytest.fixture(scope="module")
def boundary_runs(capi, tmp_path_factory):
    """The first C records of the generated FASTA through the pipeline itself (capi.Enumerator writes the junction stream)."""
    d = tmp_path_factory.mktemp("boundary")
    got = {}
    for c in R.BOUNDARY_COLORS:
        fa = R.boundary_fasta(str(d / ("w%d.fa" % c)), c)
        out = str(d / ("w%d.bin" % c))
        e = capi.Enumerator([fa], R.BOUNDARY_K, R.BOUNDARY_L, q=R.BOUNDARY_Q, tmpdir=str(d), out=out, seed=R.BOUNDARY_SEED)
        e.close()
        got[c] = (fa, out)
    return got


@pytest.mark.parametrize("c", R.BOUNDARY_COLORS)
def test_presence_at_the_word_boundaries(capi, boundary_runs, c):
    fa, stream = boundary_runs[c]
    args = [stream, "-k", str(R.BOUNDARY_K), "-s", fa]
    gfa1 = R.run_graphdump(args + ["-f", "gfa1"], cwd=os.path.dirname(fa))
    assert gfa1.returncode == 0 and gfa1.stderr == b""
    g = R.Gfa1(gfa1.stdout)
    assert len(g.seq_name) == c
    ctx = host_context(capi, fa, open(stream, "rb").read(), R.BOUNDARY_K)
    t = check_table(ctx, g, list(range(c)), c, R.BOUNDARY_K)
    ctx.close()
    assert t["presence"][:, 32 * ((c - 1) // 32):].any() and t["presence"].all(axis=1).any()
    want, _ = R.tsv(gfa1.stdout, "sequence", R.BOUNDARY_K, [fa])
    r = R.run_graphdump(args + ["--colors", "sequence", "--gpu"], cwd=os.path.dirname(fa))
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert r.stdout == want


# ------------------------------------------------------------------------------------------------ 3. ranges and refusals
def test_fetch_ranges(capi):
    case = CASES["rand6_k9_fp"]
    g = R.Gfa1(R.golden_gfa1(R.case_vector(case)))
    ctx = host_context(capi, os.path.join(GOLDEN, case["fasta"]), open(os.path.join(GOLDEN, case["bin"]), "rb").read(), case["k"])
    n_seq = len(g.seq_name)
    t = R.table(g, list(range(n_seq)), n_seq)
    rows = len(t["name"])
    assert ctx.segments_colors_build(list(range(n_seq)), n_seq)["rows"] == rows and rows > 200
    first, occ, fwd, ncol = ctx.segments_colors_fetch_rows(133, 71)
    assert (occ == t["occurrences"][133:204]).all() and (fwd == t["forward"][133:204]).all() and (ncol == t["n_colors"][133:204]).all()
    assert (first == ctx.segments_colors_fetch_rows()[0][133:204]).all()
    assert (ctx.segments_colors_fetch_presence(133, 71) == R.presence_words(t["presence"])[133:204]).all()
    assert all(a.size == 0 for a in ctx.segments_colors_fetch_rows(rows, 0)) and ctx.segments_colors_fetch_presence(rows, 0).shape[0] == 0
    for r0, n in ((rows, 1), (rows + 1, 0), (0, rows + 1), (MAXU, 2)):
        with pytest.raises(RuntimeError, match="bad row range"):
            ctx.segments_colors_fetch_rows(r0, n)
        with pytest.raises(RuntimeError, match="bad presence range"):
            ctx.segments_colors_fetch_presence(r0, n)
    ctx.close()


def test_refusals(capi):
    case = CASES["rand6_k9_fp"]
    fasta = os.path.join(GOLDEN, case["fasta"])
    text = capi.PackedText.from_fasta([fasta])
    n_seq = len(text.rec_start)
    ctx = capi.Context(0)
    with pytest.raises(RuntimeError, match="build the segment table first"):   # no table
        ctx.segments_colors_build([0] * n_seq, 1)
    with pytest.raises(RuntimeError, match="tpc_segments_colors_build first"):
        ctx.segments_colors_fetch_rows(0, 0)
    ctx.close()
    ctx = host_context(capi, fasta, open(os.path.join(GOLDEN, case["bin"]), "rb").read(), case["k"])
    with pytest.raises(RuntimeError, match="at least one colour"):
        ctx.segments_colors_build([0] * n_seq, 0)
    with pytest.raises(RuntimeError, match="sequence 2 has colour 3, there are 3 colours"):
        ctx.segments_colors_build([0, 1, 3] + [2] * (n_seq - 3), 3)
    # sizes that would wrap in 32 bits: refused by the count, and by the memory the presence words would take (1474 rows x 2^26 words)
    with pytest.raises(RuntimeError, match="4294967295 colours, at most 2147483648"):
        ctx.segments_colors_build([0] * n_seq, 0xFFFFFFFF)
    with pytest.raises(RuntimeError, match="do not fit the free device memory"):
        ctx.segments_colors_build([0] * n_seq, 1 << 31)
    with pytest.raises(RuntimeError, match="tpc_segments_colors_build first"):   # a refused build leaves no table
        ctx.segments_colors_fetch_hist()
    ctx.segments_colors_build([0] * n_seq, 1)
    # a new segment build drops the colours of the old one
    ctx.segments_build(b"", case["k"], text.rec_start, text.rec_length)
    with pytest.raises(RuntimeError, match="tpc_segments_colors_build first"):
        ctx.segments_colors_fetch_hist()
    ctx.close()
    # a table whose walk failed
    bad = CASES["edge_k5"]
    ctx = host_context(capi, os.path.join(GOLDEN, bad["fasta"]), open(os.path.join(GOLDEN, bad["bin"]), "rb").read(), bad["k"])
    assert ctx.segments_error() is not None
    with pytest.raises(RuntimeError, match="the walk's error 1 at slot 3"):
        ctx.segments_colors_build([0] * len(read_fasta(os.path.join(GOLDEN, bad["fasta"]))), 1)
    ctx.close()


def test_an_empty_stream_gives_no_rows(capi):
    text = capi.PackedText.from_fasta([os.path.join(GOLDEN, "example.fa")])
    ctx = capi.Context(0)
    ctx.seq_upload(text)
    ctx.segments_build(b"", 11, text.rec_start, text.rec_length)
    n_seq = len(text.rec_start)
    assert ctx.segments_colors_build(list(range(n_seq)), n_seq) == {"rows": 0, "colors": n_seq, "words": 1}
    assert all(a.size == 0 for a in ctx.segments_colors_fetch_rows())
    assert ctx.segments_colors_fetch_presence().shape == (0, 1)
    seg, bases = ctx.segments_colors_fetch_hist()
    assert seg.size == n_seq + 1 and not seg.any() and not bases.any()
    ctx.close()


# ------------------------------------------------------------------------------------------------ 4. the build stays what it was
def test_the_segment_build_is_unchanged_by_a_colours_build(capi):
    case = CASES["c2_k29"]
    fasta = os.path.join(GOLDEN, case["fasta"])
    ctx = host_context(capi, fasta, open(os.path.join(GOLDEN, case["bin"]), "rb").read(), case["k"])
    n_seq = len(read_fasta(fasta))

    def state():
        name, first = ctx.segments_fetch()
        begin, end = ctx.segments_fetch_events()
        return ctx.segments_counts(), ctx.segments_error(), name, first, begin, end, ctx.segments_fetch_sequences(0, n_seq + 1)

    before = state()
    ctx.segments_colors_build(list(range(n_seq)), n_seq)
    ctx.segments_colors_build([0] * n_seq, 4000)
    after = state()
    assert before[0] == after[0] and before[1] == after[1]
    assert all((a == b).all() for a, b in zip(before[2:], after[2:]))
    ctx.close()


# ------------------------------------------------------------------------------------------------ 5. bytes
@pytest.mark.parametrize("name", ["rand6_k9_fp", "c2_k29", "tr_k25_L28"])
def test_graphdump_gpu_writes_the_serial_bytes(tmp_path, name):
    case = CASES[name]
    v = R.case_vector(case)
    gfa1 = R.golden_gfa1(v)
    stats = str(tmp_path / "stats.json")
    for by in ("file", "sequence"):
        want, t = R.tsv(gfa1, by, case["k"], [case["fasta"]])
        serial = R.run_graphdump(R.colors_args(v) + ["--colors", by])
        assert serial.returncode == 0 and serial.stdout == want
        env = dict(os.environ, TWOPACO_GRAPHDUMP_STATS=stats)
        r = subprocess.run([R.GRAPHDUMP] + R.colors_args(v) + ["--colors", by, "--gpu", "--threads", "16"], cwd=GOLDEN, capture_output=True, timeout=300, env=env)
        assert r.returncode == 0 and r.stderr == b"", r.stderr
        assert r.stdout == want, (name, by)
        s = json.load(open(stats))
        assert s["path"] == "device" and s["colors_kernel_ms"] > 0 and s["segments"] == len(t["name"]) and s["events"] == t["events"]
    out = str(tmp_path / "colors.tsv")
    r = R.run_graphdump(R.colors_args(v) + ["--colors", "sequence", "--gpu", "--colors-out", out])
    assert r.returncode == 0 and r.stdout == b"" and open(out, "rb").read() == want


def test_graphdump_gpu_fails_as_the_walk_fails(tmp_path):
    v = R.vector_of("edge_k5")
    out = str(tmp_path / "colors.tsv")
    r = R.run_graphdump(R.colors_args(v) + ["--colors", "file", "--gpu", "--colors-out", out])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode() == v["stderr"] and not os.path.exists(out)


def cli(case, extra, cwd=GOLDEN, timeout=300, env=None):
    args = [R.TWOPACO, "-k", str(case["k"]), "-f", str(case["L"]), "-q", str(case["q"]), "-r", str(case["n_rounds"]), "--seed", str(case["seed"])]
    if case["abundance"] is not None:
        args += ["-a", str(case["abundance"])]
    return subprocess.run(args + extra + [case["fasta"]], cwd=cwd, capture_output=True, timeout=timeout, env=env)


@pytest.mark.parametrize("by", ["file", "sequence"])
def test_twopaco_colors_equals_twopaco_then_serial_graphdump(tmp_path, by):
    """`twopaco --colors` == `twopaco -o` followed by the serial `graphdump --colors`; also beside --graph gfa1 (whose file
    still has the reference's sha256, and no junction file appears) and beside -o."""
    case = CASES["rand6_k9_fp"]
    v = R.vector_of("rand6_k9_fp")
    d = str(tmp_path)
    junctions = os.path.join(d, "j.bin")
    r = cli(case, ["--tmpdir", d, "-o", junctions])
    assert r.returncode == 0, r.stderr
    assert open(junctions, "rb").read() == open(os.path.join(GOLDEN, case["bin"]), "rb").read()
    serial = R.run_graphdump([junctions, "-k", str(case["k"]), "-s", case["fasta"], "--colors", by])
    assert serial.returncode == 0 and serial.stderr == b""
    want, _ = R.tsv(R.golden_gfa1(v), by, case["k"], [case["fasta"]])
    assert serial.stdout == want
    os.unlink(junctions)
    # alone, with -o
    out = os.path.join(d, "colors.tsv")
    r = cli(case, ["--tmpdir", d, "--colors", by, "--colors-out", out, "-o", junctions])
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert open(out, "rb").read() == want
    assert open(junctions, "rb").read() == open(os.path.join(GOLDEN, case["bin"]), "rb").read()
    assert sorted(os.listdir(d)) == ["colors.tsv", "j.bin"]
    os.unlink(out)
    os.unlink(junctions)
    # with --graph gfa1, host text and device text: no junction file
    for text in ("host", "device"):
        graph = os.path.join(d, "graph.gfa")
        r = cli(case, ["--tmpdir", d, "--colors", by, "--colors-out", out, "--graph", "gfa1", "--graph-out", graph, "--graph-text", text])
        assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
        assert open(out, "rb").read() == want
        assert os.path.getsize(graph) == v["stdout_bytes"] and sha256_file(graph) == v["stdout_sha256"]
        assert sorted(os.listdir(d)) == ["colors.tsv", "graph.gfa"]
        os.unlink(out)
        os.unlink(graph)
    assert not os.path.exists(os.path.join(GOLDEN, "de_bruijn.bin"))


def test_twopaco_default_file_timing_lines_and_refusals(tmp_path):
    case = dict(CASES["c2_k29"])
    case["fasta"] = os.path.join(GOLDEN, case["fasta"])
    d = str(tmp_path)
    r = cli(case, ["--tmpdir", d, "--colors", "sequence"], cwd=d, env=dict(os.environ, TWOPACO_TIMING="1"))
    assert r.returncode == 0, r.stderr[-400:]
    assert sorted(os.listdir(d)) == ["de_bruijn.bin", "de_bruijn.colors.tsv"]
    err = r.stderr.decode()
    assert "segment colours:" in err and "segment colours fetch:" in err and "colors_kernel_ms" in err
    serial = R.run_graphdump([os.path.join(d, "de_bruijn.bin"), "-k", str(case["k"]), "-s", case["fasta"], "--colors", "sequence"])
    assert serial.returncode == 0 and serial.stdout == open(os.path.join(d, "de_bruijn.colors.tsv"), "rb").read()
    os.unlink(os.path.join(d, "de_bruijn.bin"))
    os.unlink(os.path.join(d, "de_bruijn.colors.tsv"))
    r = cli(case, ["--tmpdir", d, "--colors", "file", "--gpus", "2"], cwd=d)
    assert r.returncode == 1 and r.stderr.decode().endswith("for arg (--colors)\n") and os.listdir(d) == []
    # a graph step that fails leaves no colour file behind
    r = cli(case, ["--tmpdir", d, "--colors", "file", "--colors-out", os.path.join(d, "colors.tsv"), "--graph", "gfa1", "--graph-out", os.path.join(d, "missing", "graph.gfa")], cwd=d)
    assert r.returncode == 1 and r.stderr.decode().startswith("\nError: Can't create the graph file") and os.listdir(d) == []
    # an input the walk refuses: the walk's message, no colour file
    bad = CASES["edge_k5"]
    r = cli(bad, ["--tmpdir", d, "--colors", "file", "--colors-out", os.path.join(d, "colors.tsv"), "-o", os.path.join(d, "j.bin")])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: The input is corrupted\n"
    assert os.listdir(d) == ["j.bin"]


def test_enumerator_colors_in_process(capi, tmp_path):
    case = CASES["rand6_k9_fp"]
    v = R.vector_of("rand6_k9_fp")
    before = os.getcwd()
    os.chdir(GOLDEN)
    try:
        out, graph = str(tmp_path / "colors.tsv"), str(tmp_path / "graph.gfa")
        e = capi.Enumerator([case["fasta"]], case["k"], case["L"], q=case["q"], rounds=case["n_rounds"], seed=case["seed"], tmpdir=str(tmp_path),
                            graph="gfa1", graph_out=graph, colors="sequence", colors_out=out)
        assert e.vertices_count() == case["distinct"]
        e.close()
    finally:
        os.chdir(before)
    want, _ = R.tsv(R.golden_gfa1(v), "sequence", case["k"], [case["fasta"]])
    assert open(out, "rb").read() == want and sha256_file(graph) == v["stdout_sha256"]
    assert sorted(os.listdir(str(tmp_path))) == ["colors.tsv", "graph.gfa"]


# ------------------------------------------------------------------------------------------------ 6. at size
def test_m2r2_colors_equal_twopaco_then_serial_graphdump(tmp_path):
    """synth m2r2 at scale 0.18, k = 25, f = 32, seed 12345 (the input of test_gpu_graph_flag.py: 62 files, two presence words
    per row): sha256 of `twopaco --colors file` == that of `twopaco -o` followed by the serial `graphdump --colors file`."""
    d = str(tmp_path)
    case = {"name": "m2r2_s018", "fasta": None, "synth": {"workload": "m2r2", "seed": 12345, "scale": 0.18}}
    files = case_files(case, d)
    assert len(files) == 62
    base = [R.TWOPACO, "-k", "25", "-f", "32", "-t", "16", "--seed", "12345", "--tmpdir", d]
    junctions = os.path.join(d, "m2r2.bin")
    r = subprocess.run(base + ["-o", junctions] + files, capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr[-800:]
    seqs = []
    for f in files:
        seqs += ["-s", f]
    serial = os.path.join(d, "serial.tsv")
    r = subprocess.run([R.GRAPHDUMP, junctions, "-k", "25", "--colors", "file", "--colors-out", serial] + seqs, capture_output=True, timeout=900)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    os.unlink(junctions)
    segments = named = core = hist = 0
    with open(serial, "rb") as f:
        head = f.readline().decode().rstrip("\n").split("\t")
        assert head[:3] == ["#twopaco-colors", "1", "by=file"] and head[4] == "colors=62"
        rows, events = int(head[5].split("=")[1]), int(head[6].split("=")[1])
        for line in f:
            if line.startswith(b"#hist"):
                hist += int(line.split(b"\t")[2])
            elif not line.startswith(b"#"):
                p = line.split(b"\t")
                segments += 1
                named += int(p[0]) >= R.FRESH
                core += int(p[4]) == 62
                assert len(p[5]) == 17   # 16 digits and the line end
    print("events", events, "segments", segments, "N-named", named, "in all 62", core)
    assert events > 2_000_000 and segments == rows and named > 0 and core > 0 and hist == segments
    out = os.path.join(d, "colors.tsv")
    r = subprocess.run(base + ["--colors", "file", "--colors-out", out, "-o", junctions] + files, capture_output=True, timeout=900)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-800:]
    assert (sha256_file(out), os.path.getsize(out)) == (sha256_file(serial), os.path.getsize(serial))
