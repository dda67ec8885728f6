"""GPU (-m gpu): `twopaco --graph` -- genomes to the compacted graph's text in one process.  The device's event table
(csrc/tpc_segments.hip: k_seg_events, fetched with tpc_segments_fetch_events / _sequences) against its definition; the graph
file against the bytes the REAL reference graphdump wrote (tests/golden/graphdump.json), in-process and through the command
line; and against `twopaco -o` followed by the serial graphdump at a size where chunks and scans matter."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from graph_table import event_table, read_fasta, vector_parts
from helpers import GOLDEN, case_files, golden_cases, sha256_file

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ("gfa1", "gfa2", "fasta")
ALL = [v for v in json.load(open(os.path.join(GOLDEN, "graphdump.json"))) if v["case"] != "cli" and v["args"][2] in FORMATS]
VECTORS = [v for v in ALL if v["rc"] == 0]
FAILING = [v for v in ALL if v["rc"] != 0]
CASES = {c["name"]: c for c in golden_cases()}
MAXU = (1 << 64) - 1
TWOPACO = os.path.join(ROOT, "twopaco_amd", "bin", "twopaco")
GRAPHDUMP = os.path.join(ROOT, "twopaco_amd", "bin", "graphdump")


@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


@pytest.fixture()
def in_golden():
    """cwd = tests/golden with relative file names: UR:Z: carries the name as it was given."""
    before = os.getcwd()
    os.chdir(GOLDEN)
    yield
    os.chdir(before)


def no_junction_file_anywhere(*dirs):
    for d in (GOLDEN,) + dirs:
        assert not os.path.exists(os.path.join(str(d), "de_bruijn.bin")), d


# ------------------------------------------------------------------------------------------------ 1. the event table by its definition
@pytest.mark.parametrize("name", ["tr_k25_L28", "edge_k5", "c2_k29", "rand6_k3"])
def test_event_table_by_its_definition(capi, tmp_path, name):
    """begin[] / end[] / seq_event_begin[] through the C-ABI == the restatement of tests/graph_table.py, from the golden stream's
    bytes (tpc_segments_build_host) and from the stream tpc_emit_stream left on the device (tpc_segments_build_resident)."""
    case = CASES[name]
    files = case_files(case, tmp_path)
    data = open(os.path.join(GOLDEN, case["bin"]), "rb").read()
    seqs = read_fasta(files[0])
    want_name, want_first, want_begin, want_end, want_seq = event_table(data, seqs, case["k"])
    events = len(want_name)
    assert events > 0 and len(want_seq) == len(seqs) + 1 and want_seq[-1] == events
    if name == "edge_k5":
        # sequences shorter than k hold no event
        assert (np.diff(want_seq.astype(np.int64)) == 0).any()
    text = capi.PackedText.from_fasta(files)
    rec_start, rec_len = text.rec_start, text.rec_length
    amb = [int(rec_start[r]) + i for r, s in enumerate(seqs) for i, ch in enumerate(s) if ch not in "ACGTN"]

    def check(ctx):
        begin, end = ctx.segments_fetch_events()
        seq = ctx.segments_fetch_sequences(0, len(seqs) + 1)
        assert begin.dtype == end.dtype == seq.dtype == np.uint32
        assert (begin == want_begin).all() and (end == want_end).all()
        assert (seq == want_seq).all()
        got_name, got_first = ctx.segments_fetch()
        assert (got_name == want_name).all() and (got_first == want_first).all()
        # ranges
        if events > 40:
            b, e = ctx.segments_fetch_events(33, 7)
            assert (b == want_begin[33:40]).all() and (e == want_end[33:40]).all()
        b, e = ctx.segments_fetch_events(events, 0)
        assert b.size == 0 and e.size == 0
        assert (ctx.segments_fetch_sequences(1, len(seqs)) == want_seq[1:]).all()
        assert ctx.segments_counts()["events"] == events
        for e0, n in ((events, 1), (events + 1, 0), (0, events + 1), ((1 << 64) - 1, 2)):
            with pytest.raises(RuntimeError, match="bad event range"):
                ctx.segments_fetch_events(e0, n)
        for s0, n in ((len(seqs) + 1, 1), (len(seqs) + 2, 0), (0, len(seqs) + 2)):
            with pytest.raises(RuntimeError, match="bad sequence range"):
                ctx.segments_fetch_sequences(s0, n)

    ctx = capi.Context(0)
    with pytest.raises(RuntimeError):   # no table yet
        ctx.segments_fetch_sequences(0, 1)
    ctx.seq_upload(text)
    ctx.segments_build(data, case["k"], rec_start, rec_len, amb)
    check(ctx)
    ctx.close()

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
    stream, _ = ctx.emit_stream(rec_start, rec_len)
    assert stream == data
    ctx.segments_build(None, case["k"], rec_start, rec_len, amb)
    check(ctx)
    ctx.close()


def test_event_table_of_a_stream_that_ends_early(capi):
    """c2_k29's stream cut behind its first sequence, with and without the separator: the entries of the sequences the stream
    never reaches hold the event count."""
    case = CASES["c2_k29"]
    fasta = os.path.join(GOLDEN, case["fasta"])
    data = open(os.path.join(GOLDEN, case["bin"]), "rb").read()
    seqs = read_fasta(fasta)
    sep = next(i for i in range(len(data) // 12) if data[i * 12:i * 12 + 4] == b"\xff\xff\xff\xff")
    text = capi.PackedText.from_fasta([fasta])
    for cut in (sep, sep + 1):
        part = data[:cut * 12]
        want_name, want_first, want_begin, want_end, want_seq = event_table(part, seqs, case["k"])
        assert len(want_name) == sep - 1 and want_seq.tolist() == [0] + [sep - 1] * len(seqs)
        ctx = capi.Context(0)
        ctx.seq_upload(text)
        counts = ctx.segments_build(part, case["k"], text.rec_start, text.rec_length)
        assert counts["events"] == sep - 1 and ctx.segments_error() is None
        begin, end = ctx.segments_fetch_events()
        assert (begin == want_begin).all() and (end == want_end).all()
        assert (ctx.segments_fetch_sequences(0, len(seqs) + 1) == want_seq).all()
        ctx.close()


def test_event_table_of_a_stream_without_events(capi):
    """An empty stream and a stream of lone records: no event, every seq_event_begin entry 0."""
    import struct
    text = capi.PackedText.from_fasta([os.path.join(GOLDEN, "example.fa")])
    n_rec = len(text.rec_start)
    sep = struct.pack("<Iq", 0xFFFFFFFF, (1 << 63) - 1)
    for data in (b"", struct.pack("<Iq", 0, 1) + sep + struct.pack("<Iq", 0, 2)):
        ctx = capi.Context(0)
        ctx.seq_upload(text)
        counts = ctx.segments_build(data, 11, text.rec_start, text.rec_length)
        assert counts["events"] == 0
        assert (ctx.segments_fetch_sequences(0, n_rec + 1) == 0).all()
        b, e = ctx.segments_fetch_events()
        assert b.size == 0 and e.size == 0
        ctx.close()


# ------------------------------------------------------------------------------------------------ 2. the reference's bytes, one process
def enumerator_args(case):
    return dict(q=case["q"], rounds=case["n_rounds"], abundance=case["abundance"] if case["abundance"] is not None else MAXU, seed=case["seed"])


def test_vector_counts():
    assert len(VECTORS) == 95 and len(FAILING) == 20
    assert {v["case"] for v in FAILING} == {"edge_k3", "edge_k5", "edge_k5_dbg", "edge_k7_fp_r2"}


@pytest.mark.parametrize("fmt", FORMATS)
def test_graph_in_process_gives_the_reference_bytes(capi, tmp_path, in_golden, fmt):
    """All 95 vectors of the real reference with exit code 0 (this format's share here), through capi.Enumerator(graph=...)
    in this process: size and sha256 of the graph file; no junction file is written."""
    n = 0
    for v in VECTORS:
        if v["args"][2] != fmt:
            continue
        _, _, k, files, prefix = vector_parts(v)
        case = CASES[v["case"]]
        assert k == case["k"] and files == [case["fasta"]]
        out = str(tmp_path / "graph.txt")
        e = capi.Enumerator(files, k, case["L"], tmpdir=str(tmp_path), graph=fmt, graph_out=out, graph_prefix=prefix, **enumerator_args(case))
        assert e.vertices_count() == case["distinct"], v["args"]
        e.close()
        assert os.path.getsize(out) == v["stdout_bytes"], v["args"]
        assert sha256_file(out) == v["stdout_sha256"], v["args"]
        os.unlink(out)
        assert os.listdir(str(tmp_path)) == [], v["args"]
        n += 1
    assert n == {"gfa1": 38, "gfa2": 38, "fasta": 19}[fmt]
    no_junction_file_anywhere(tmp_path)


def test_graph_in_process_fails_as_the_walk_fails(capi, tmp_path, in_golden):
    """The 20 vectors the reference ends with exit code 1 (edge.fa: sequences shorter than k make the stream skip sequence ids):
    the call raises with the walk's message and no graph file is left."""
    for v in FAILING:
        _, fmt, k, files, prefix = vector_parts(v)
        case = CASES[v["case"]]
        out = str(tmp_path / "graph.txt")
        with pytest.raises(RuntimeError) as err:
            capi.Enumerator(files, k, case["L"], tmpdir=str(tmp_path), graph=fmt, graph_out=out, graph_prefix=prefix, **enumerator_args(case))
        assert v["stderr"] == "error: %s\n" % err.value, v["args"]
        assert os.listdir(str(tmp_path)) == [], v["args"]
    no_junction_file_anywhere(tmp_path)


# ------------------------------------------------------------------------------------------------ 3. the command line
def cli(case, extra, cwd=GOLDEN, timeout=300):
    args = [TWOPACO, "-k", str(case["k"]), "-f", str(case["L"]), "-q", str(case["q"]), "-r", str(case["n_rounds"]), "--seed", str(case["seed"])]
    if case["abundance"] is not None:
        args += ["-a", str(case["abundance"])]
    return subprocess.run(args + extra + [case["fasta"]], cwd=cwd, capture_output=True, timeout=timeout)


def vector_of(case_name, fmt, prefix=False):
    return [v for v in VECTORS if v["case"] == case_name and v["args"][2] == fmt and ("--prefix" in v["args"]) == prefix][0]


@pytest.mark.parametrize("case_name,fmt,prefix", [("c2_k29", "gfa1", False), ("example_k11", "gfa2", True), ("rand6_k27", "fasta", False),
                                                  ("rand6_k9_fp_r4", "gfa1", True), ("rand6_k9_a3", "gfa2", False)])
def test_cli_writes_the_reference_bytes_and_no_junction_file(tmp_path, case_name, fmt, prefix):
    """bin/twopaco --graph as a child process, cwd = tests/golden: one vector per format, then -r 4 and -a 3."""
    case, v = CASES[case_name], vector_of(case_name, fmt, prefix)
    out = str(tmp_path / "graph.txt")
    r = cli(case, ["--tmpdir", str(tmp_path), "--graph", fmt, "--graph-out", out] + (["--graph-prefix"] if prefix else []))
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    log = r.stdout.decode()
    assert "Distinct junctions = %d" % case["distinct"] in log and "True marks count: %d" % case["true_marks"] in log
    assert os.path.getsize(out) == v["stdout_bytes"] and sha256_file(out) == v["stdout_sha256"]
    assert os.listdir(str(tmp_path)) == ["graph.txt"]
    no_junction_file_anywhere(tmp_path)


def test_cli_with_outfile_writes_both(tmp_path):
    case, v = CASES["c2_k29"], vector_of("c2_k29", "gfa1")
    out, junctions = str(tmp_path / "graph.gfa"), str(tmp_path / "junctions.bin")
    r = cli(case, ["--tmpdir", str(tmp_path), "--graph", "gfa1", "--graph-out", out, "-o", junctions])
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert sha256_file(out) == v["stdout_sha256"]
    assert open(junctions, "rb").read() == open(os.path.join(GOLDEN, case["bin"]), "rb").read()
    assert sorted(os.listdir(str(tmp_path))) == ["graph.gfa", "junctions.bin"]


def test_cli_thread_counts_give_equal_bytes(tmp_path):
    case, v = CASES["c2_k29"], vector_of("c2_k29", "gfa2")
    got = []
    for threads in (1, 3, 16):
        out = str(tmp_path / ("graph_%d.txt" % threads))
        r = cli(case, ["--tmpdir", str(tmp_path), "--graph", "gfa2", "--graph-out", out, "--graph-threads", str(threads)])
        assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
        got.append(open(out, "rb").read())
    assert got[0] == got[1] == got[2] and hashlib.sha256(got[0]).hexdigest() == v["stdout_sha256"]


def test_cli_default_graph_file_and_the_walks_error(tmp_path):
    """Without --graph-out the text goes to de_bruijn.<format> in the current directory; an input the walk refuses ends the
    run with its message, exit code 1 and no graph file."""
    case = CASES["example_k11"]
    fasta = dict(case, fasta=os.path.join(GOLDEN, case["fasta"]))
    r = cli(fasta, ["--tmpdir", str(tmp_path), "--graph", "gfa1"], cwd=str(tmp_path))
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert os.listdir(str(tmp_path)) == ["de_bruijn.gfa1"]
    assert open(str(tmp_path / "de_bruijn.gfa1"), "rb").read().startswith(b"H\tVN:Z:1.0\nS\t1\t*\tUR:Z:" + fasta["fasta"].encode() + b"\n")
    os.unlink(str(tmp_path / "de_bruijn.gfa1"))
    bad = CASES["edge_k5"]
    r = cli(bad, ["--tmpdir", str(tmp_path), "--graph", "gfa1", "--graph-out", str(tmp_path / "graph.txt")])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: The input is corrupted\n"
    assert os.listdir(str(tmp_path)) == []
    no_junction_file_anywhere(tmp_path)


# ------------------------------------------------------------------------------------------------ 4. at size
def test_m2r2_graph_equals_twopaco_then_serial_graphdump(tmp_path):
    """synth m2r2 at scale 0.18, k = 25, f = 32, seed 12345 (the input of test_gpu_graphdump.py, which says why not 0.2): for
    every format the sha256 of `twopaco --graph` == that of `twopaco -o` followed by the serial graphdump."""
    d = str(tmp_path)
    case = {"name": "m2r2_s018", "fasta": None, "synth": {"workload": "m2r2", "seed": 12345, "scale": 0.18}}
    files = case_files(case, d)
    base = [TWOPACO, "-k", "25", "-f", "32", "-t", "16", "--seed", "12345", "--tmpdir", d]
    junctions = os.path.join(d, "m2r2.bin")
    r = subprocess.run(base + ["-o", junctions] + files, capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr[-800:]
    assert os.path.getsize(junctions) // 12 > 2_000_000
    seqs = []
    for f in files:
        seqs += ["-s", f]
    for fmt in FORMATS:
        serial = os.path.join(d, "serial.txt")
        with open(serial, "wb") as f:
            r = subprocess.run([GRAPHDUMP, junctions, "-f", fmt, "-k", "25"] + seqs, stdout=f, stderr=subprocess.PIPE, timeout=900)
        assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
        if fmt == "gfa1":
            events = fresh = 0
            with open(serial, "rb") as f:
                for line in f:
                    if line[:2] == b"C\t":
                        events += 1
                    elif line[:2] == b"S\t" and line[2:3].isdigit() and int(line[2:line.index(b"\t", 2)]) >= 1 << 34:
                        fresh += 1
            print("events", events, "N-named", fresh)
            assert events > 2_000_000 and fresh > 0
        want = (sha256_file(serial), os.path.getsize(serial))
        os.unlink(serial)
        out = os.path.join(d, "graph.txt")
        r = subprocess.run(base + ["--graph", fmt, "--graph-out", out] + files, capture_output=True, timeout=900)
        assert r.returncode == 0 and r.stderr == b"", r.stderr[-800:]
        assert (sha256_file(out), os.path.getsize(out)) == want and want[1] > 0, fmt
        os.unlink(out)
    assert not os.path.exists(os.path.join(d, "de_bruijn.bin"))
    no_junction_file_anywhere()


# ------------------------------------------------------------------------------------------------ 5. every table from one process
TABLES = {"colors": None, "links": None, "bubbles": None, "distances": "phylip", "components": "members", "superbubbles": "members", "anchors": "paf", "locate": "walks"}
TOGETHER = ("colors", "distances", "components", "superbubbles", "anchors", "locate")   # the largest set graphdump writes in one run


def table_args(name, by, d, query):
    """The options of one table with every file it can write, into directory d."""
    a = ["--links"] if name == "links" else ["--" + name, by]
    a += ["--%s-out" % name, os.path.join(d, name + ".tsv")]
    if TABLES[name]:
        a += ["--%s-%s" % (name, TABLES[name]), os.path.join(d, "%s.%s" % (name, TABLES[name]))]
    return a + (["--locate-in", query] if name == "locate" else [])


def read_all(d, keep):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.split(".")[0] in keep}


def all_tables_inputs(d):
    """name -> (fasta files relative to d, k, the other twopaco arguments, the locate query)."""
    with open(os.path.join(d, "short_a.fa"), "w") as f:
        f.write(">a1\nACGTACGTTG\n>a2\nGGATCCAT\n")
    with open(os.path.join(d, "short_b.fa"), "w") as f:
        f.write(">b1\nTTG\n")
    with open(os.path.join(d, "two.fa"), "w") as f:
        f.write(">r5\nACGTA\n>r7\nGATTACA\n")
    case = CASES["c2_k29"]
    with open(os.path.join(d, "c2.fa"), "wb") as f:
        f.write(open(os.path.join(GOLDEN, case["fasta"]), "rb").read())
    return {"shorter_than_k": (["short_a.fa", "short_b.fa"], 11, ["-f", "20", "--seed", "7"], "short_a.fa"),
            "two_records_k9": (["two.fa"], 9, ["-f", "20", "--seed", "7"], "two.fa"),
            "c2_k29": (["c2.fa"], case["k"], ["-f", str(case["L"]), "-q", str(case["q"]), "-r", str(case["n_rounds"]), "--seed", str(case["seed"])], "c2.fa")}


@pytest.mark.parametrize("name", ["shorter_than_k", "two_records_k9", "c2_k29"])
def test_all_tables_from_one_process_equal_the_serial_graphdump(tmp_path, name):
    """One `twopaco --graph gfa1` with all eight tables, and one `graphdump --gpu` with the largest set it writes together, by file
    and by sequence: every file byte for byte what the serial graphdump writes for that table alone.  Inputs: records all shorter
    than k in two files (nothing is dispatched: the stream is empty), two records of 5 and 7 bases at k = 9, and c2_k29 with its own file as the query."""
    d = str(tmp_path)
    files, k, args, query = all_tables_inputs(d)[name]

    def run(exe, argv, into):
        os.mkdir(os.path.join(d, into))
        return subprocess.run([exe] + argv, cwd=d, capture_output=True, timeout=300)

    # twopaco: the graph, the junction stream and all eight tables by sequence
    argv = ["-k", str(k)] + args + ["--tmpdir", d, "-o", "stream.bin", "--graph", "gfa1", "--graph-out", os.path.join("twopaco", "graph.gfa1")]
    for t in TABLES:
        argv += table_args(t, "sequence", "twopaco", query)
    r = run(TWOPACO, argv + files, "twopaco")
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-800:]
    if name == "c2_k29":
        assert open(os.path.join(d, "stream.bin"), "rb").read() == open(os.path.join(GOLDEN, CASES[name]["bin"]), "rb").read()
    else:
        assert os.path.getsize(os.path.join(d, "stream.bin")) == 0
    base = ["stream.bin", "-k", str(k)] + [a for f in files for a in ("-s", f)]

    # the serial graphdump, every table alone
    want = {}
    for by in ("file", "sequence"):
        into = "serial_" + by
        os.mkdir(os.path.join(d, into))
        for t in TABLES:
            r = subprocess.run([GRAPHDUMP] + base + table_args(t, by, into, query), cwd=d, capture_output=True, timeout=300)
            assert r.returncode == 0 and r.stderr == b"" and r.stdout == b"", (t, r.stderr[-400:])
        want[by] = read_all(os.path.join(d, into), TABLES)
        assert len(want[by]) == 13 and all(want[by][t + ".tsv"] for t in TABLES)
    r = subprocess.run([GRAPHDUMP] + base + ["-f", "gfa1"], cwd=d, capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stderr == b""
    want["sequence"]["graph.gfa1"] = r.stdout
    assert want["file"]["links.tsv"] == want["sequence"]["links.tsv"] and want["file"]["colors.tsv"] != want["sequence"]["colors.tsv"]

    assert read_all(os.path.join(d, "twopaco"), list(TABLES) + ["graph"]) == want["sequence"]

    # graphdump --gpu: the six tables it writes together
    for by in ("file", "sequence"):
        into = "gpu_" + by
        argv = list(base) + ["--gpu"]
        for t in TOGETHER:
            argv += table_args(t, by, into, query)
        r = run(GRAPHDUMP, argv, into)
        assert r.returncode == 0 and r.stderr == b"" and r.stdout == b"", r.stderr[-800:]
        got = read_all(os.path.join(d, into), TOGETHER)
        assert got == {f: b for f, b in want[by].items() if f.split(".")[0] in TOGETHER} and len(got) == 11
