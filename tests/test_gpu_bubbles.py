"""GPU (-m gpu): the simple bubbles on the device (csrc/tpc_bubbles.hip, the tpc_segments_bubbles_* group of
include/twopaco_hip.h) against their definition, restated in bubbles_reference.py over the serial gfa1 text (pinned to the real
reference's sha256 by tests/golden/graphdump.json): the side arrays, the bubble rows, the histogram and info[] through the C-ABI
on a host stream and a resident stream, the stages it leaves untouched, refusals, and the bytes of `graphdump --bubbles --gpu`
and `twopaco --bubbles`."""
import json
import os
import subprocess

import numpy as np
import pytest

import bubbles_reference as R
from helpers import GOLDEN, case_files, golden_cases, sha256_file

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in golden_cases()}
MAXU = (1 << 64) - 1
GENERATED_CASE = {"k": R.BUBBLE_K, "L": R.BUBBLE_L, "q": R.BUBBLE_Q, "seed": R.BUBBLE_SEED, "rounds": [{"low": 0, "high": 1 << R.BUBBLE_L}], "n_rounds": 1, "abundance": None}
GENERATED = {"b8": R.BUBBLE_GENOMES, "b78": R.BUBBLE_GENOMES + R.BUBBLE_HUB}
NAMES = ["b8", "b78", "c2_k29", "rand6_k27", "rand6_k3", "tr_k25_L28", "example_k11", "short"]


@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


def ambiguous_positions(fasta, rec_start):
    return [int(rec_start[r]) + i for r, (_, s) in enumerate(R.read_fasta(fasta)) for i, ch in enumerate(s) if ch not in "ACGTN"]


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
    """The generated inputs (bubbles_reference.bubble_fasta at 8 and 78 records) and the link-free records: FASTA, junction
    stream (from the CPU restatement of the pipeline, oracle/) and the serial gfa1, made once."""
    d = tmp_path_factory.mktemp("bubbles")
    got = {"dir": str(d)}
    for name in ("b8", "b78", "short"):
        fa = str(d / (name + ".fa"))
        if name == "short":
            R.few_events_fasta(fa, only_short=True)
        else:
            R.bubble_fasta(fa, GENERATED[name])
        stream = R.oracle_stream(fa, str(d / (name + ".bin")), R.BUBBLE_K, R.BUBBLE_L, R.BUBBLE_Q, R.BUBBLE_SEED)
        gfa1 = R.run_graphdump([stream, "-k", str(R.BUBBLE_K), "-s", fa, "-f", "gfa1"], cwd=str(d))
        assert gfa1.returncode == 0 and gfa1.stderr == b""
        got[name] = {"fasta": fa, "stream": stream, "gfa1": gfa1.stdout, "oracle": {}}
    return got


def inputs(name, made, by="file"):
    """(case, fasta, stream bytes, oracle, graphdump's arguments, its directory)"""
    if name in made:
        m = made[name]
        if by not in m["oracle"]:
            m["oracle"][by] = R.Bubbles(m["gfa1"], by)
        return dict(GENERATED_CASE, name=name), m["fasta"], open(m["stream"], "rb").read(), m["oracle"][by], [m["stream"], "-k", str(R.BUBBLE_K), "-s", m["fasta"]], made["dir"]
    case = CASES[name]
    v = R.case_vector(case)
    return case, os.path.join(GOLDEN, case["fasta"]), open(os.path.join(GOLDEN, case["bin"]), "rb").read(), R.golden_bubbles(v, by), R.bubbles_args(v), GOLDEN


def check_table(ctx, want):
    """Everything the device holds after a bubble build == the oracle's."""
    info = ctx.segments_bubbles_build()
    assert (info["bubbles"], info["sides"], info["arcs"]) == (want.bubbles(), want.sides, want.arcs)
    assert info["peak_bytes"] >= 12 * want.sides + 16 * want.bubbles() + 48
    deg, lo, hi = ctx.segments_bubbles_fetch_sides()
    assert deg.dtype == lo.dtype == hi.dtype == np.uint32 and deg.size == lo.size == hi.size == want.sides
    assert (deg == want.deg).all()
    # the definition reads lo / hi of the sides of degree 1 and 2 alone; they are exact for every side all the same
    assert (lo == want.lo).all() and (hi == want.hi).all()
    rows = ctx.segments_bubbles_fetch_rows()
    assert all(a.dtype == np.uint32 for a in rows)
    for got, ref in zip(rows, (want.source, want.arm_a, want.arm_b, want.sink)):
        assert got.size == ref.size and (got == ref).all()
    hist = ctx.segments_bubbles_fetch_hist()
    assert hist.dtype == np.uint64 and (hist.astype(np.int64) == want.hist).all() and int(hist.sum()) == want.sides
    assert ctx.kernel_ms("bubbles") > 0
    return info


# ------------------------------------------------------------------------------------------------ 1. the arrays by their definition
@pytest.mark.parametrize("source", ["host", "resident"])
@pytest.mark.parametrize("name", NAMES)
def test_bubble_arrays_by_their_definition(capi, made, name, source):
    case, fasta, data, want, _, _ = inputs(name, made)
    ctx = host_context(capi, fasta, data, case["k"]) if source == "host" else resident_context(capi, case, fasta, data)
    assert ctx.segments_error() is None
    links = ctx.segments_links_build()
    assert links["rows"] == want.links
    check_table(ctx, want)
    check_table(ctx, want)   # a second build replaces the first
    if name in GENERATED:
        assert want.bubbles() == 28 and int((want.source & 1).sum()) == 15
    if name == "b78":
        assert int(want.deg.max()) == 20 and want.hist[5] == 4          # the hub: many arcs meet one side
    if name == "tr_k25_L28":
        assert any(u in want.out[u] for u in range(want.sides))         # its self-loop
    if name == "rand6_k3":
        assert want.bubbles() == 0 and want.hist[4] + want.hist[5] == 273
    if name == "example_k11":
        assert want.bubbles() == 0 and want.links > 0 and all(a.size == 0 for a in ctx.segments_bubbles_fetch_rows())
    if name == "short":
        assert (want.links, want.arcs, want.bubbles()) == (0, 0, 0) and want.hist.tolist() == [want.sides, 0, 0, 0, 0, 0] and want.sides > 0
    ctx.close()


def test_no_event_at_all(capi, made):
    fa = made["short"]["fasta"]
    text = capi.PackedText.from_fasta([fa])
    ctx = capi.Context(0)
    ctx.seq_upload(text)
    ctx.segments_build(b"", R.BUBBLE_K, text.rec_start, text.rec_length)
    ctx.segments_links_build()
    info = ctx.segments_bubbles_build()
    assert (info["bubbles"], info["sides"], info["arcs"]) == (0, 0, 0)
    assert all(a.size == 0 for a in ctx.segments_bubbles_fetch_sides()) and not ctx.segments_bubbles_fetch_hist().any()
    ctx.close()


# ------------------------------------------------------------------------------------------------ 2. opt-in
@pytest.mark.parametrize("order", ["colours_last", "colours_first"])
def test_the_build_the_colours_and_the_links_are_unchanged(capi, made, order):
    case, fasta, data, want, _, _ = inputs("b78", made)
    n_seq = len(R.read_fasta(fasta))

    def outputs(ctx):
        name, first = ctx.segments_fetch()
        begin, end = ctx.segments_fetch_events()
        got = [name, first, begin, end, ctx.segments_fetch_sequences(0, n_seq + 1)]
        got += list(ctx.segments_colors_fetch_rows()) + [ctx.segments_colors_fetch_presence()] + list(ctx.segments_colors_fetch_hist())
        got += list(ctx.segments_links_fetch_rows()) + [ctx.segments_links_fetch_first()]
        return ctx.segments_counts(), ctx.segments_error(), ctx.segments_colors_info(), ctx.segments_links_info(), got

    def elsewhere(counts):
        """peak_device_bytes is what the whole device held at the segment build: it belongs to one build, not to the input"""
        return {key: n for key, n in counts.items() if key != "peak_device_bytes"}

    alone = host_context(capi, fasta, data, case["k"])
    alone.segments_colors_build(list(range(n_seq)), n_seq)
    alone.segments_links_build()
    ref = outputs(alone)
    alone.close()
    ctx = host_context(capi, fasta, data, case["k"])
    counts = ctx.segments_counts()   # of this build, before any of the three stages
    assert counts["peak_device_bytes"] > 0
    if order == "colours_last":
        ctx.segments_links_build()
        check_table(ctx, want)
        ctx.segments_colors_build(list(range(n_seq)), n_seq)
    else:
        ctx.segments_colors_build(list(range(n_seq)), n_seq)
        ctx.segments_links_build()
        check_table(ctx, want)
    for _ in range(2):
        got = outputs(ctx)
        assert got[0] == counts and elsewhere(got[0]) == elsewhere(ref[0])
        assert got[1:4] == ref[1:4]
        assert all(a.shape == b.shape and (a == b).all() for a, b in zip(got[4], ref[4]))
        check_table(ctx, want)   # rebuilt: the same table, and the others once more
    # the bubbles are still there after the colours; a new link build drops them
    assert (ctx.segments_bubbles_fetch_rows()[0] == want.source).all()
    ctx.segments_links_build()
    with pytest.raises(RuntimeError, match="tpc_segments_bubbles_build first"):
        ctx.segments_bubbles_info()
    check_table(ctx, want)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 3. ranges and refusals
def test_fetch_ranges(capi, made):
    case, fasta, data, want, _, _ = inputs("b78", made)
    ctx = host_context(capi, fasta, data, case["k"])
    ctx.segments_links_build()
    n = ctx.segments_bubbles_build()["bubbles"]
    assert n == 28
    rows = ctx.segments_bubbles_fetch_rows(5, 11)
    for got, ref in zip(rows, (want.source, want.arm_a, want.arm_b, want.sink)):
        assert (got == ref[5:16]).all()
    assert all(a.size == 0 for a in ctx.segments_bubbles_fetch_rows(n, 0))
    for b0, m in ((n, 1), (n + 1, 0), (0, n + 1), (MAXU, 2)):
        with pytest.raises(RuntimeError, match="bad row range"):
            ctx.segments_bubbles_fetch_rows(b0, m)
    sides = want.sides
    deg, lo, hi = ctx.segments_bubbles_fetch_sides(133, 71)
    assert (deg == want.deg[133:204]).all() and (lo == want.lo[133:204]).all() and (hi == want.hi[133:204]).all()
    assert all(a.size == 0 for a in ctx.segments_bubbles_fetch_sides(sides, 0))
    for c0, m in ((sides, 1), (sides + 1, 0), (0, sides + 1), (MAXU, 2)):
        with pytest.raises(RuntimeError, match="bad side range"):
            ctx.segments_bubbles_fetch_sides(c0, m)
    check_table(ctx, want)   # still usable
    ctx.close()


def test_refusals(capi, made):
    case, fasta, data, want, _, _ = inputs("b8", made)
    text = capi.PackedText.from_fasta([fasta])
    ctx = capi.Context(0)
    with pytest.raises(RuntimeError, match="segment bubbles: build the segment table first"):   # no table
        ctx.segments_bubbles_build()
    for call in (ctx.segments_bubbles_info, ctx.segments_bubbles_fetch_rows, ctx.segments_bubbles_fetch_sides, ctx.segments_bubbles_fetch_hist):
        with pytest.raises(RuntimeError, match="tpc_segments_bubbles_build first"):
            call()
    # the context is usable: a table, then no link table yet
    ctx.seq_upload(text)
    ctx.segments_build(data, case["k"], text.rec_start, text.rec_length, ambiguous_positions(fasta, text.rec_start))
    with pytest.raises(RuntimeError, match="segment bubbles: build the link table first"):
        ctx.segments_bubbles_build()
    with pytest.raises(RuntimeError, match="tpc_segments_bubbles_build first"):
        ctx.segments_bubbles_info()
    assert ctx.segments_counts()["events"] > 0 and ctx.segments_error() is None
    ctx.segments_links_build()
    check_table(ctx, want)
    # a new segment build drops the bubbles of the old one (and its links)
    ctx.segments_build(b"", case["k"], text.rec_start, text.rec_length)
    with pytest.raises(RuntimeError, match="tpc_segments_bubbles_build first"):
        ctx.segments_bubbles_fetch_rows(0, 0)
    with pytest.raises(RuntimeError, match="segment bubbles: build the link table first"):
        ctx.segments_bubbles_build()
    ctx.close()
    # a table whose walk failed
    bad = CASES["edge_k5"]
    ctx = host_context(capi, os.path.join(GOLDEN, bad["fasta"]), open(os.path.join(GOLDEN, bad["bin"]), "rb").read(), bad["k"])
    assert ctx.segments_error() is not None
    with pytest.raises(RuntimeError, match="segment bubbles: the segment table holds the walk's error 1 at slot 3"):
        ctx.segments_bubbles_build()
    with pytest.raises(RuntimeError, match="tpc_segments_bubbles_build first"):
        ctx.segments_bubbles_info()
    # and the same context goes on: what it held is what it holds, and a new table in it gets its bubbles
    assert ctx.segments_error() is not None and ctx.segments_counts()["events"] >= 0
    bad_text = capi.PackedText.from_fasta([os.path.join(GOLDEN, bad["fasta"])])
    ctx.segments_build(b"", bad["k"], bad_text.rec_start, bad_text.rec_length)
    ctx.segments_links_build()
    assert ctx.segments_bubbles_build()["bubbles"] == 0
    ctx.close()


# ------------------------------------------------------------------------------------------------ 4. bytes
@pytest.mark.parametrize("by", ["file", "sequence"])
@pytest.mark.parametrize("name", NAMES)
def test_graphdump_gpu_writes_the_oracle_bytes(tmp_path, made, name, by):
    case, fasta, _, want, args, cwd = inputs(name, made, by)
    stats = str(tmp_path / "stats.json")
    env = dict(os.environ, TWOPACO_GRAPHDUMP_STATS=stats)
    r = subprocess.run([R.GRAPHDUMP] + args + ["--bubbles", by, "--gpu", "--threads", "16"], cwd=cwd, capture_output=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert r.stdout == want.tsv(case["k"]), name
    s = json.load(open(stats))
    assert s["path"] == "device" and s["bubbles_kernel_ms"] > 0 and s["bubbles"] == want.bubbles() and s["links"] == want.links
    out = str(tmp_path / "bubbles.tsv")
    r = R.run_graphdump(args + ["--bubbles", by, "--gpu", "--bubbles-out", out, "--prefix"], cwd=cwd)
    assert r.returncode == 0 and r.stdout == b"" and open(out, "rb").read() == want.tsv(case["k"])


def test_graphdump_gpu_fails_as_the_walk_fails(tmp_path):
    v = R.vector_of("edge_k5")
    out = str(tmp_path / "bubbles.tsv")
    r = R.run_graphdump(R.bubbles_args(v) + ["--bubbles", "file", "--gpu", "--bubbles-out", out])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode() == v["stderr"] and not os.path.exists(out)
    r = R.run_graphdump(R.bubbles_args(v) + ["--bubbles", "sequence", "--gpu"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode() == v["stderr"]


def cli_input(name, fasta):
    """(fasta as twopaco is given it, its directory): a golden file by its name inside tests/golden, as the reference's vectors
    name it -- the colours' labels are the file names as given."""
    return (None, GOLDEN) if name in CASES else (fasta, os.path.dirname(fasta))


def cli(case, extra, fasta=None, cwd=GOLDEN, timeout=300, env=None):
    args = [R.TWOPACO, "-k", str(case["k"]), "-f", str(case["L"]), "-q", str(case["q"]), "-r", str(case["n_rounds"]), "--seed", str(case["seed"])]
    if case["abundance"] is not None:
        args += ["-a", str(case["abundance"])]
    return subprocess.run(args + extra + [case["fasta"] if fasta is None else fasta], cwd=cwd, capture_output=True, timeout=timeout, env=env)


@pytest.mark.parametrize("by", ["file", "sequence"])
@pytest.mark.parametrize("name", NAMES)
def test_twopaco_writes_the_oracle_bytes(tmp_path, made, name, by):
    case, fasta, data, want, _, _ = inputs(name, made, by)
    d = str(tmp_path)
    bubbles, junctions = os.path.join(d, "bubbles.tsv"), os.path.join(d, "j.bin")
    given, cwd = cli_input(name, fasta)
    r = cli(case, ["--tmpdir", d, "--bubbles", by, "--bubbles-out", bubbles, "-o", junctions], given, cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert open(junctions, "rb").read() == data
    assert open(bubbles, "rb").read() == want.tsv(case["k"])
    assert sorted(os.listdir(d)) == ["bubbles.tsv", "j.bin"]


@pytest.mark.parametrize("name", ["b78", "c2_k29"])
def test_twopaco_bubbles_beside_everything_else(tmp_path, made, name):
    """--bubbles with --graph gfa1 --graph-compact --links --colors: one segment, colour and link build serve all, and every other
    file has the bytes it has without --bubbles."""
    case, fasta, _, want, _, _ = inputs(name, made, "sequence")
    given, cwd = cli_input(name, fasta)
    with_dir, without_dir = str(tmp_path / "with"), str(tmp_path / "without")
    files = ("graph.gfa", "links.tsv", "colors.tsv")
    for d, extra in ((without_dir, []), (with_dir, ["--bubbles", "sequence", "--bubbles-out", os.path.join(with_dir, "bubbles.tsv")])):
        os.mkdir(d)
        r = cli(case, ["--tmpdir", d, "--graph", "gfa1", "--graph-compact", "--graph-out", os.path.join(d, "graph.gfa"), "--links", "--links-out", os.path.join(d, "links.tsv"),
                       "--colors", "sequence", "--colors-out", os.path.join(d, "colors.tsv")] + extra, given, cwd=cwd)
        assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert sorted(os.listdir(without_dir)) == sorted(files) and sorted(os.listdir(with_dir)) == sorted(files + ("bubbles.tsv",))
    for f in files:
        assert open(os.path.join(with_dir, f), "rb").read() == open(os.path.join(without_dir, f), "rb").read(), f
    assert open(os.path.join(with_dir, "bubbles.tsv"), "rb").read() == want.tsv(case["k"])
    # beside the plain graph rendered on the device, where no event table is fetched for the graph
    d = str(tmp_path / "device")
    os.mkdir(d)
    r = cli(case, ["--tmpdir", d, "--graph", "gfa1", "--graph-text", "device", "--graph-out", os.path.join(d, "graph.gfa"), "--bubbles", "sequence", "--bubbles-out", os.path.join(d, "bubbles.tsv")],
            given, cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert open(os.path.join(d, "bubbles.tsv"), "rb").read() == want.tsv(case["k"])
    assert sorted(os.listdir(d)) == ["bubbles.tsv", "graph.gfa"]


def test_twopaco_default_file_timing_lines_and_refusals(tmp_path, made):
    case, fasta, _, want, _, _ = inputs("b8", made)
    d = str(tmp_path)
    r = cli(case, ["--tmpdir", d, "--bubbles", "file"], fasta, cwd=d, env=dict(os.environ, TWOPACO_TIMING="1"))
    assert r.returncode == 0, r.stderr[-400:]
    assert sorted(os.listdir(d)) == ["de_bruijn.bin", "de_bruijn.bubbles.tsv"]
    err = r.stderr.decode()
    assert "segment bubbles:" in err and "segment bubbles fetch:" in err and "bubbles_kernel_ms" in err and "bubble table writing:" in err
    assert open(os.path.join(d, "de_bruijn.bubbles.tsv"), "rb").read() == want.tsv(case["k"])
    os.unlink(os.path.join(d, "de_bruijn.bin"))
    os.unlink(os.path.join(d, "de_bruijn.bubbles.tsv"))
    r = cli(case, ["--tmpdir", d, "--bubbles", "file", "--gpus", "2"], fasta, cwd=d)
    assert r.returncode == 1 and r.stderr.decode().endswith("not with --gpus above 1 for arg (--bubbles)\n") and os.listdir(d) == []
    r = cli(case, ["--tmpdir", d, "--bubbles", "file", "--colors", "sequence"], fasta, cwd=d)
    assert r.returncode == 1 and "share one set of colours" in r.stderr.decode() and r.stderr.decode().endswith("for arg (--bubbles)\n") and os.listdir(d) == []
    # an input the walk refuses: the walk's message, no file
    bad = CASES["edge_k5"]
    r = cli(bad, ["--tmpdir", d, "--bubbles", "file", "--bubbles-out", os.path.join(d, "bubbles.tsv"), "--graph", "gfa1", "--graph-out", os.path.join(d, "graph.gfa")])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: The input is corrupted\n"
    assert os.listdir(d) == []


# ------------------------------------------------------------------------------------------------ 5. at size
def test_m2r2_bubbles_equal_the_serial_graphdump(tmp_path):
    """synth m2r2 at scale 0.18, k = 25, f = 32, seed 12345 (the input of test_gpu_links.py: 62 files, tracts and
    minisatellites): sha256 of `twopaco --bubbles file` == that of the serial `graphdump --bubbles file` over the junction stream
    of the same command, and the table has rows."""
    d = str(tmp_path)
    case = {"name": "m2r2_s018", "fasta": None, "synth": {"workload": "m2r2", "seed": 12345, "scale": 0.18}}
    files = case_files(case, d)
    assert len(files) == 62
    base = [R.TWOPACO, "-k", "25", "-f", "32", "-t", "16", "--seed", "12345", "--tmpdir", d]
    junctions, bubbles = os.path.join(d, "m2r2.bin"), os.path.join(d, "bubbles.tsv")
    r = subprocess.run(base + ["-o", junctions, "--bubbles", "file", "--bubbles-out", bubbles] + files, capture_output=True, timeout=900)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-800:]
    seqs = []
    for f in files:
        seqs += ["-s", f]
    serial = os.path.join(d, "serial.tsv")
    r = subprocess.run([R.GRAPHDUMP, junctions, "-k", "25", "--bubbles", "file", "--bubbles-out", serial] + seqs, capture_output=True, timeout=900)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    head = open(serial, "rb").readline().decode().rstrip("\n").split("\t")
    assert head[:4] == ["#twopaco-bubbles", "1", "by=file", "k=25"] and head[4] == "colors=62"
    segments, links, rows = (int(head[i].split("=")[1]) for i in (5, 6, 7))
    with open(serial, "rb") as f:
        body = sum(1 for line in f if not line.startswith(b"#"))
    print("segments", segments, "links", links, "bubbles", rows)
    assert rows > 0 and body == rows and links > 100_000
    assert (sha256_file(bubbles), os.path.getsize(bubbles)) == (sha256_file(serial), os.path.getsize(serial))
