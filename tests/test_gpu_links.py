"""GPU (-m gpu): the link table on the device (csrc/tpc_links.hip, the tpc_segments_links_* group of include/twopaco_hip.h)
against its definition, restated in links_reference.py over the serial gfa1 text (pinned to the real reference's sha256 by
tests/golden/graphdump.json): the arrays and first bits through the C-ABI, long probe chains and a full link set, the hot key,
the stages it leaves untouched, refusals, and the bytes of `graphdump --links / --compact --gpu` and `twopaco --links /
--graph-compact`."""
import json
import os
import subprocess

import numpy as np
import pytest

import links_reference as R
from helpers import GOLDEN, bits_of_words, case_files, golden_cases, sha256_file

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in golden_cases()}
MAXU = (1 << 64) - 1
FEW_CASE = {"name": "few", "k": R.FEW_K, "L": R.FEW_L, "q": R.FEW_Q, "seed": R.FEW_SEED, "rounds": [{"low": 0, "high": 1 << R.FEW_L}], "n_rounds": 1, "abundance": None}


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
def few(tmp_path_factory):
    """The records with 0, 1 and 2 events: FASTA, junction stream (from the CPU restatement of the pipeline, oracle/) and the
    oracle over the serial gfa1."""
    from oracle import oracle as O
    d = tmp_path_factory.mktemp("few")
    fa = R.few_events_fasta(str(d / "few.fa"))
    o = O.Oracle(R.FEW_K, R.FEW_L, R.FEW_Q, O.seed_table(R.FEW_SEED, R.FEW_Q, R.FEW_L))
    o.add_fasta(fa)
    o.enumerate()
    stream = str(d / "few.bin")
    o.write_bin(stream)
    o.close()
    gfa1 = R.run_graphdump([stream, "-k", str(R.FEW_K), "-s", fa, "-f", "gfa1"], cwd=str(d))
    assert gfa1.returncode == 0 and gfa1.stderr == b""
    return {"fasta": fa, "stream": stream, "links": R.Links(gfa1.stdout), "dir": str(d)}


def inputs(name, few):
    """(case, fasta, stream bytes, oracle)"""
    if name == "few":
        return FEW_CASE, few["fasta"], open(few["stream"], "rb").read(), few["links"]
    case = CASES[name]
    return case, os.path.join(GOLDEN, case["fasta"]), open(os.path.join(GOLDEN, case["bin"]), "rb").read(), R.golden_links(R.case_vector(case))


def check_table(ctx, want, slots=None):
    """Everything the device holds after a links build == the oracle's."""
    info = ctx.segments_links_build()
    assert info["rows"] == want.rows() and info["occurrences"] == want.occurrences
    default = 1024
    while default < 2 * want.occurrences:
        default *= 2
    assert info["slots"] == (default if slots is None else slots) and info["peak_bytes"] >= 20 * info["slots"]
    first, count, same = ctx.segments_links_fetch_rows()
    assert first.dtype == count.dtype == same.dtype == np.uint32
    assert (first == want.first_event).all() and (count == want.count).all() and (same == want.same).all()
    events = ctx.segments_counts()["events"]
    assert events == want.events
    words = ctx.segments_links_fetch_first()
    assert words.dtype == np.uint32 and words.size == (events + 31) // 32
    assert (bits_of_words(words, events) == want.first_bits).all()
    assert not bits_of_words(words, words.size * 32)[events:].any()
    # the rows are spelled as their first occurrences
    name, _ = ctx.segments_fetch()
    if want.rows():
        assert (name[first - 1] == np.array(want.frm)).all() and (name[first] == np.array(want.to)).all()
    assert ctx.kernel_ms("links") > 0
    return info


# ------------------------------------------------------------------------------------------------ 1. the arrays by their definition
@pytest.mark.parametrize("source", ["host", "resident"])
@pytest.mark.parametrize("name", ["rand6_k3", "rand6_k9_fp", "tr_k25_L28", "c2_k29", "few"])
def test_link_arrays_and_bits_by_their_definition(capi, few, name, source):
    case, fasta, data, want = inputs(name, few)
    ctx = host_context(capi, fasta, data, case["k"]) if source == "host" else resident_context(capi, case, fasta, data)
    assert ctx.segments_error() is None
    check_table(ctx, want)
    check_table(ctx, want)   # a second build replaces the first
    if name == "rand6_k3":
        assert want.rows() == 619 and len(want.both) == 432
        _, count, same = ctx.segments_links_fetch_rows()
        assert int((same < count).sum()) == 432
    if name == "few":
        assert want.rows() >= 2 and want.occurrences < want.events
    ctx.close()


def test_a_stream_without_any_link(capi, tmp_path):
    from oracle import oracle as O
    fa = R.few_events_fasta(str(tmp_path / "short.fa"), only_short=True)
    o = O.Oracle(R.FEW_K, R.FEW_L, R.FEW_Q, O.seed_table(R.FEW_SEED, R.FEW_Q, R.FEW_L))
    o.add_fasta(fa)
    o.enumerate()
    stream = str(tmp_path / "short.bin")
    o.write_bin(stream)
    o.close()
    ctx = host_context(capi, fa, open(stream, "rb").read(), R.FEW_K)
    assert ctx.segments_counts()["events"] == 2
    info = ctx.segments_links_build()
    assert (info["rows"], info["occurrences"], info["slots"]) == (0, 0, 1024)
    assert all(a.size == 0 for a in ctx.segments_links_fetch_rows()) and not ctx.segments_links_fetch_first().any()
    ctx.close()
    # and no event at all
    text = capi.PackedText.from_fasta([fa])
    ctx = capi.Context(0)
    ctx.seq_upload(text)
    ctx.segments_build(b"", R.FEW_K, text.rec_start, text.rec_length)
    info = ctx.segments_links_build()
    assert (info["rows"], info["occurrences"]) == (0, 0) and ctx.segments_links_fetch_first().size == 0
    ctx.close()


# ------------------------------------------------------------------------------------------------ 2. probing
def test_long_probe_chains_and_a_full_set(capi):
    """rand6_k9_fp holds 1910 links.  In 2^11 slots (93 % full) the probe chains are long and the table still exact; 2^10 slots
    cannot hold them: the call ends with an error text, the context stays usable and a build at the default size is exact."""
    case, fasta, data, want = inputs("rand6_k9_fp", None)
    assert want.rows() == 1910
    ctx = host_context(capi, fasta, data, case["k"])
    ctx.set_option("test_links_slots_log2", 11)
    check_table(ctx, want, slots=2048)
    ctx.set_option("test_links_slots_log2", 10)
    with pytest.raises(RuntimeError, match="the link set of 1024 slots is full"):
        ctx.segments_links_build()
    with pytest.raises(RuntimeError, match="tpc_segments_links_build first"):   # a refused build leaves no table
        ctx.segments_links_info()
    assert ctx.segments_counts()["events"] == want.events and ctx.segments_error() is None
    ctx.set_option("test_links_slots_log2", 0)
    check_table(ctx, want)
    ctx.close()


def test_the_hot_key(capi):
    """tr_k25_L28: one self-loop link 874 times in a row, across waves and blocks: its row counts what the oracle counts."""
    case, fasta, data, want = inputs("tr_k25_L28", None)
    assert want.longest_run == 874 and want.rows() == 1328
    hot = int(np.argmax(want.count))
    assert want.count[hot] >= 874 and want.frm[hot] == want.to[hot]
    ctx = host_context(capi, fasta, data, case["k"])
    ctx.segments_links_build()
    first, count, same = ctx.segments_links_fetch_rows(hot, 1)
    assert (int(first[0]), int(count[0]), int(same[0])) == (int(want.first_event[hot]), int(want.count[hot]), int(want.same[hot]))
    # as tight as the slots get for 1328 links: 2^11
    ctx.set_option("test_links_slots_log2", 11)
    check_table(ctx, want, slots=2048)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 3. opt-in
@pytest.mark.parametrize("order", ["links_first", "colors_first"])
def test_the_build_and_the_colours_are_unchanged(capi, order):
    case, fasta, data, want = inputs("rand6_k9_fp", None)
    n_seq = len(R.read_fasta(fasta))
    alone = host_context(capi, fasta, data, case["k"])
    alone.segments_colors_build(list(range(n_seq)), n_seq)
    colours_alone = [alone.segments_colors_fetch_rows(), alone.segments_colors_fetch_presence(), alone.segments_colors_fetch_hist()]
    alone.close()
    ctx = host_context(capi, fasta, data, case["k"])

    def state():
        name, first = ctx.segments_fetch()
        begin, end = ctx.segments_fetch_events()
        return ctx.segments_counts(), ctx.segments_error(), name, first, begin, end, ctx.segments_fetch_sequences(0, n_seq + 1)

    before = state()
    if order == "links_first":
        check_table(ctx, want)
        ctx.segments_colors_build(list(range(n_seq)), n_seq)
    else:
        ctx.segments_colors_build(list(range(n_seq)), n_seq)
        check_table(ctx, want)
    after = state()
    assert before[0] == after[0] and before[1] == after[1]
    assert all((a == b).all() for a, b in zip(before[2:], after[2:]))
    colours = [ctx.segments_colors_fetch_rows(), ctx.segments_colors_fetch_presence(), ctx.segments_colors_fetch_hist()]
    for got, ref in zip(colours, colours_alone):
        got, ref = (got, ref) if isinstance(got, tuple) else ((got,), (ref,))
        assert all((a == b).all() for a, b in zip(got, ref))
    # and the links are still there after the colours
    first, count, same = ctx.segments_links_fetch_rows()
    assert (first == want.first_event).all() and (count == want.count).all() and (same == want.same).all()
    ctx.close()


# ------------------------------------------------------------------------------------------------ 4. ranges and refusals
def test_fetch_ranges(capi):
    case, fasta, data, want = inputs("rand6_k9_fp", None)
    ctx = host_context(capi, fasta, data, case["k"])
    rows = ctx.segments_links_build()["rows"]
    first, count, same = ctx.segments_links_fetch_rows(133, 71)
    assert (first == want.first_event[133:204]).all() and (count == want.count[133:204]).all() and (same == want.same[133:204]).all()
    assert all(a.size == 0 for a in ctx.segments_links_fetch_rows(rows, 0))
    for r0, n in ((rows, 1), (rows + 1, 0), (0, rows + 1), (MAXU, 2)):
        with pytest.raises(RuntimeError, match="bad row range"):
            ctx.segments_links_fetch_rows(r0, n)
    words = (want.events + 31) // 32
    whole = ctx.segments_links_fetch_first()
    assert (ctx.segments_links_fetch_first(7, 30) == whole[7:37]).all() and ctx.segments_links_fetch_first(words, 0).size == 0
    for w0, n in ((words, 1), (words + 1, 0), (0, words + 1), (MAXU, 2)):
        with pytest.raises(RuntimeError, match="bad first-bit range"):
            ctx.segments_links_fetch_first(w0, n)
    ctx.close()


def test_refusals(capi):
    case, fasta, data, want = inputs("rand6_k9_fp", None)
    text = capi.PackedText.from_fasta([fasta])
    ctx = capi.Context(0)
    with pytest.raises(RuntimeError, match="build the segment table first"):   # no table
        ctx.segments_links_build()
    for call in (ctx.segments_links_info, ctx.segments_links_fetch_rows, lambda: ctx.segments_links_fetch_first(0, 0)):
        with pytest.raises(RuntimeError, match="tpc_segments_links_build first"):
            call()
    ctx.close()
    ctx = host_context(capi, fasta, data, case["k"])
    ctx.segments_links_build()
    # a new segment build drops the links of the old one
    ctx.segments_build(b"", case["k"], text.rec_start, text.rec_length)
    with pytest.raises(RuntimeError, match="tpc_segments_links_build first"):
        ctx.segments_links_fetch_rows(0, 0)
    ctx.close()
    # a table whose walk failed
    bad = CASES["edge_k5"]
    ctx = host_context(capi, os.path.join(GOLDEN, bad["fasta"]), open(os.path.join(GOLDEN, bad["bin"]), "rb").read(), bad["k"])
    assert ctx.segments_error() is not None
    with pytest.raises(RuntimeError, match="the walk's error 1 at slot 3"):
        ctx.segments_links_build()
    with pytest.raises(RuntimeError, match="tpc_segments_links_build first"):
        ctx.segments_links_info()
    ctx.close()


# ------------------------------------------------------------------------------------------------ 5. bytes
@pytest.mark.parametrize("name", ["rand6_k3", "rand6_k9_fp", "tr_k25_L28", "c2_k29", "few"])
def test_graphdump_gpu_writes_the_serial_bytes(tmp_path, few, name):
    case, fasta, _, want = inputs(name, few)
    if name == "few":
        args, cwd = [few["stream"], "-k", str(R.FEW_K), "-s", fasta], few["dir"]
    else:
        args, cwd = R.links_args(R.case_vector(case)), GOLDEN
    stats = str(tmp_path / "stats.json")
    env = dict(os.environ, TWOPACO_GRAPHDUMP_STATS=stats)
    serial = R.run_graphdump(args + ["--links"], cwd=cwd)
    assert serial.returncode == 0 and serial.stdout == want.tsv(case["k"])
    r = subprocess.run([R.GRAPHDUMP] + args + ["--links", "--gpu", "--threads", "16"], cwd=cwd, capture_output=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert r.stdout == serial.stdout, name
    s = json.load(open(stats))
    assert s["path"] == "device" and s["links_kernel_ms"] > 0 and s["links"] == want.rows() and s["link_occurrences"] == want.occurrences
    out = str(tmp_path / "links.tsv")
    r = R.run_graphdump(args + ["--links", "--gpu", "--links-out", out], cwd=cwd)
    assert r.returncode == 0 and r.stdout == b"" and open(out, "rb").read() == serial.stdout
    for extra in ([], ["--prefix"]):
        serial = R.run_graphdump(args + ["-f", "gfa1", "--compact"] + extra, cwd=cwd)
        assert serial.returncode == 0 and (extra or serial.stdout == want.compact())
        for threads in ("1", "16"):
            r = R.run_graphdump(args + ["-f", "gfa1", "--compact", "--gpu", "--threads", threads] + extra, cwd=cwd)
            assert r.returncode == 0 and r.stderr == b"", r.stderr
            assert r.stdout == serial.stdout, (name, extra, threads)


def test_graphdump_gpu_fails_as_the_walk_fails(tmp_path):
    v = R.vector_of("edge_k5")
    out = str(tmp_path / "links.tsv")
    r = R.run_graphdump(R.links_args(v) + ["--links", "--gpu", "--links-out", out])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode() == v["stderr"] and not os.path.exists(out)
    r = R.run_graphdump(v["args"] + ["--compact", "--gpu"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode() == v["stderr"]


def cli(case, extra, fasta=None, cwd=GOLDEN, timeout=300, env=None):
    args = [R.TWOPACO, "-k", str(case["k"]), "-f", str(case["L"]), "-q", str(case["q"]), "-r", str(case["n_rounds"]), "--seed", str(case["seed"])]
    if case["abundance"] is not None:
        args += ["-a", str(case["abundance"])]
    return subprocess.run(args + extra + [case["fasta"] if fasta is None else fasta], cwd=cwd, capture_output=True, timeout=timeout, env=env)


@pytest.mark.parametrize("name", ["rand6_k3", "rand6_k9_fp", "tr_k25_L28", "c2_k29", "few"])
def test_twopaco_writes_the_serial_bytes(tmp_path, few, name):
    """`twopaco --links` and `twopaco --graph gfa1 --graph-compact` == the serial graphdump over the junction stream of the same
    command; one run serves the graph, the colours and the links."""
    case, fasta, data, want = inputs(name, few)
    d = str(tmp_path)
    links, graph, colors, junctions = (os.path.join(d, n) for n in ("links.tsv", "graph.gfa", "colors.tsv", "j.bin"))
    r = cli(case, ["--tmpdir", d, "--links", "--links-out", links, "-o", junctions], fasta)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert open(junctions, "rb").read() == data
    assert open(links, "rb").read() == want.tsv(case["k"])
    assert sorted(os.listdir(d)) == ["j.bin", "links.tsv"]
    os.unlink(links)
    os.unlink(junctions)
    r = cli(case, ["--tmpdir", d, "--graph", "gfa1", "--graph-compact", "--graph-out", graph], fasta)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert open(graph, "rb").read() == want.compact()
    assert os.listdir(d) == ["graph.gfa"]
    os.unlink(graph)
    # all three from one segment build; the compact graph beside them
    by_file = R.run_graphdump([os.path.join(GOLDEN, case["bin"]) if name != "few" else few["stream"], "-k", str(case["k"]), "-s", fasta, "--colors", "file"], cwd=os.path.dirname(fasta))
    assert by_file.returncode == 0
    r = cli(case, ["--tmpdir", d, "--links", "--links-out", links, "--colors", "file", "--colors-out", colors, "--graph", "gfa1", "--graph-compact", "--graph-out", graph], fasta,
            cwd=os.path.dirname(fasta))
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert open(links, "rb").read() == want.tsv(case["k"]) and open(graph, "rb").read() == want.compact() and open(colors, "rb").read() == by_file.stdout
    assert sorted(os.listdir(d)) == ["colors.tsv", "graph.gfa", "links.tsv"]


def test_twopaco_links_beside_the_plain_graph_and_the_device_text(tmp_path):
    case = CASES["rand6_k9_fp"]
    v = R.vector_of("rand6_k9_fp")
    want = R.golden_links(v)
    d = str(tmp_path)
    links, graph = os.path.join(d, "links.tsv"), os.path.join(d, "graph.gfa")
    for text in ("host", "device"):
        r = cli(case, ["--tmpdir", d, "--links", "--links-out", links, "--graph", "gfa1", "--graph-out", graph, "--graph-text", text])
        assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
        assert open(links, "rb").read() == want.tsv(case["k"])
        assert os.path.getsize(graph) == v["stdout_bytes"] and sha256_file(graph) == v["stdout_sha256"]   # the plain gfa1 is what it was
        assert sorted(os.listdir(d)) == ["graph.gfa", "links.tsv"]
        os.unlink(links)
        os.unlink(graph)


def test_twopaco_default_file_timing_lines_and_refusals(tmp_path):
    case = dict(CASES["c2_k29"])
    case["fasta"] = os.path.join(GOLDEN, case["fasta"])
    d = str(tmp_path)
    r = cli(case, ["--tmpdir", d, "--links"], cwd=d, env=dict(os.environ, TWOPACO_TIMING="1"))
    assert r.returncode == 0, r.stderr[-400:]
    assert sorted(os.listdir(d)) == ["de_bruijn.bin", "de_bruijn.links.tsv"]
    err = r.stderr.decode()
    assert "segment links:" in err and "segment links fetch:" in err and "links_kernel_ms" in err and "link table writing:" in err
    assert open(os.path.join(d, "de_bruijn.links.tsv"), "rb").read() == R.golden_links(R.vector_of("c2_k29")).tsv(case["k"])
    os.unlink(os.path.join(d, "de_bruijn.bin"))
    os.unlink(os.path.join(d, "de_bruijn.links.tsv"))
    r = cli(case, ["--tmpdir", d, "--links", "--gpus", "2"], cwd=d)
    assert r.returncode == 1 and r.stderr.decode().endswith("for arg (--links)\n") and os.listdir(d) == []
    # a graph step that fails leaves no link file behind
    r = cli(case, ["--tmpdir", d, "--links", "--links-out", os.path.join(d, "links.tsv"), "--graph", "gfa1", "--graph-compact", "--graph-out", os.path.join(d, "missing", "graph.gfa")], cwd=d)
    assert r.returncode == 1 and r.stderr.decode().startswith("\nError: Can't create the graph file") and os.listdir(d) == []
    # an input the walk refuses: the walk's message, neither file
    bad = CASES["edge_k5"]
    r = cli(bad, ["--tmpdir", d, "--links", "--links-out", os.path.join(d, "links.tsv"), "--graph", "gfa1", "--graph-compact", "--graph-out", os.path.join(d, "graph.gfa")])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: The input is corrupted\n"
    assert os.listdir(d) == []


def test_enumerator_links_in_process(capi, tmp_path):
    case = CASES["rand6_k9_fp"]
    want = R.golden_links(R.vector_of("rand6_k9_fp"))
    before = os.getcwd()
    os.chdir(GOLDEN)
    try:
        links, graph = str(tmp_path / "links.tsv"), str(tmp_path / "graph.gfa")
        e = capi.Enumerator([case["fasta"]], case["k"], case["L"], q=case["q"], rounds=case["n_rounds"], seed=case["seed"], tmpdir=str(tmp_path),
                            graph="gfa1", graph_out=graph, graph_compact=True, links=True, links_out=links)
        assert e.vertices_count() == case["distinct"]
        e.close()
    finally:
        os.chdir(before)
    assert open(links, "rb").read() == want.tsv(case["k"]) and open(graph, "rb").read() == want.compact()
    assert sorted(os.listdir(str(tmp_path))) == ["graph.gfa", "links.tsv"]


# ------------------------------------------------------------------------------------------------ 6. at size
def test_m2r2_links_and_compact_equal_the_serial_graphdump(tmp_path):
    """synth m2r2 at scale 0.18, k = 25, f = 32, seed 12345 (the input of test_gpu_colors.py: 62 files, 2 M+ events, tracts and
    minisatellites): sha256 of `twopaco --links` and of the compact graph == those of the serial graphdump over the junction stream
    of the same command."""
    d = str(tmp_path)
    case = {"name": "m2r2_s018", "fasta": None, "synth": {"workload": "m2r2", "seed": 12345, "scale": 0.18}}
    files = case_files(case, d)
    assert len(files) == 62
    base = [R.TWOPACO, "-k", "25", "-f", "32", "-t", "16", "--seed", "12345", "--tmpdir", d]
    junctions, links, graph = os.path.join(d, "m2r2.bin"), os.path.join(d, "links.tsv"), os.path.join(d, "graph.gfa")
    r = subprocess.run(base + ["-o", junctions, "--links", "--links-out", links, "--graph", "gfa1", "--graph-compact", "--graph-out", graph] + files, capture_output=True, timeout=900)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-800:]
    seqs = []
    for f in files:
        seqs += ["-s", f]
    serial = os.path.join(d, "serial.tsv")
    r = subprocess.run([R.GRAPHDUMP, junctions, "-k", "25", "--links", "--links-out", serial] + seqs, capture_output=True, timeout=900)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    head = open(serial, "rb").readline().decode().rstrip("\n").split("\t")
    assert head[:3] == ["#twopaco-links", "1", "k=25"]
    rows, occurrences = int(head[4].split("=")[1]), int(head[5].split("=")[1])
    hottest = both = 0
    with open(serial, "rb") as f:
        f.readline()
        for line in f:
            p = line.split(b"\t")
            hottest = max(hottest, int(p[4]))
            both += int(p[5]) < int(p[4])
    print("links", rows, "occurrences", occurrences, "hottest", hottest, "in both spellings", both)
    assert occurrences > 2_000_000 and 0 < rows < occurrences and hottest > 1
    assert (sha256_file(links), os.path.getsize(links)) == (sha256_file(serial), os.path.getsize(serial))
    serial_graph = os.path.join(d, "serial.gfa")
    with open(serial_graph, "wb") as out:
        r = subprocess.run([R.GRAPHDUMP, junctions, "-k", "25", "-f", "gfa1", "--compact"] + seqs, stdout=out, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert (sha256_file(graph), os.path.getsize(graph)) == (sha256_file(serial_graph), os.path.getsize(serial_graph))
