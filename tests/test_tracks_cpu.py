"""CPU: the track table of the serial `graphdump --tracks` against its definition, restated in tracks_reference.py over the serial gfa1
text (itself pinned to the real reference's sha256 by tests/golden/graphdump.json): the TSV and the bedGraph byte for byte on every
golden vector whose gfa1 succeeds, in both colour modes, for all colours and for every single `--tracks-of c`, with the interval
counts; the consequences of the definition on the oracle and on the program's text alone; the statement from the FASTA alone, without
any graph, on the example vectors and the word-boundary input; the generated inputs (hot, all different, twins, two walks over the
same segments); the table beside the other tables; the flags' errors of both programs."""
import os
import subprocess

import numpy as np
import pytest

import tracks_reference as R
from helpers import GOLDEN


@pytest.fixture(scope="module", autouse=True)
def built():
    assert os.path.exists(R.GRAPHDUMP) and os.path.exists(R.TWOPACO), "run build() first"


def serial(args, by, tmp_path, only=None, cwd=GOLDEN):
    """(table from stdout, bedGraph file) of the serial graphdump."""
    bed = str(tmp_path / "tracks.bedgraph")
    r = R.run_graphdump(list(args) + ["--tracks", by, "--tracks-bedgraph", bed] + ([] if only is None else ["--tracks-of", str(only)]), cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    return r.stdout, open(bed, "rb").read()


# ------------------------------------------------------------------------------------------------ 1. golden vectors
# intervals by sequence, counted from the event-table definition; the first prefix that fits decides (a3 before the other k9)
BY_SEQUENCE = (("example_", 12), ("rand6_k9_a3", 754), ("rand6_k9_", 3053), ("rand6_k25_q3", 1378), ("rand6_k27", 1258), ("rand6_k3", 40), ("c2_k29", 280),
               ("c2_k35", 244), ("c2_k51_r2", 167), ("c2_k61", 128), ("c2_k125", 47))


def intervals_by_sequence(case):
    hits = [n for prefix, n in BY_SEQUENCE if case.startswith(prefix)]
    return hits[0] if hits else None


@pytest.mark.parametrize("by", ["file", "sequence"])
@pytest.mark.parametrize("v", R.GOOD_VECTORS, ids=[R.vector_id(v) for v in R.GOOD_VECTORS])
def test_serial_tracks_equal_the_oracle(v, by, tmp_path):
    want = R.golden_tracks(v, by)
    args = R.tracks_args(v)
    tsv, bed = serial(args, by, tmp_path)
    assert tsv == want.tsv(), R.vector_id(v)
    assert bed == want.bedgraph(), R.vector_id(v)
    count, edges = R.check_text(tsv, bed)
    assert count == want.count() > 0 and want.selected == len(want.name)
    all_genome, all_rows = R.rows_of(tsv)
    colour_of_row = [want.color_of_seq[int(line.split("\t")[0])] for line in all_rows]
    for c in range(want.n_colors):
        one = R.golden_tracks(v, by, c)
        tsv_c, bed_c = serial(args, by, tmp_path, only=c)
        assert tsv_c == one.tsv() and bed_c == one.bedgraph(), (R.vector_id(v), c)
        R.check_text(tsv_c, bed_c)
        # --tracks-of c is the filter of the all-colours rows, in the same order, and the colour's own sums
        genome_c, rows_c = R.rows_of(tsv_c)
        assert rows_c == [line for line, colour in zip(all_rows, colour_of_row) if colour == c] and genome_c == [all_genome[c]]
        # edges[c] is ref_edges of the anchor table with ref = c
        anchors = R.run_graphdump(args + ["--anchors", by, "--anchors-ref", str(c)])
        assert anchors.returncode == 0 and anchors.stderr == b""
        head = dict(f.split("=") for f in anchors.stdout.split(b"\n", 1)[0].decode().split("\t")[2:])
        assert int(head["ref_edges"]) == edges[c] == sum(e - b for b, e, s in zip(want.begin, want.end, want.seq) if want.color_of_seq[s] == c)
    if by == "file":
        with_events = len(set(want.seq))
        assert want.n_colors == 1 and want.count() == with_events and all(line[4] == 1 for line in want.lines())
        assert want.per_color[0][2] == want.per_color[0][3] == want.per_color[0][1]
    else:
        known = intervals_by_sequence(v["case"])
        assert known is None or want.count() == known, (v["case"], want.count())


def test_the_golden_counts_cover_the_vectors():
    """Counted on the oracle alone: every family of vectors the counts above name exists, so the counts cannot pass on nothing; the
    --prefix twins give the same counts."""
    for prefix, n in BY_SEQUENCE:
        named = [v for v in R.GOOD_VECTORS if v["case"].startswith(prefix) and intervals_by_sequence(v["case"]) == n]
        assert named, prefix
        assert all(R.golden_tracks(v, "sequence").count() == n for v in named), prefix
    assert len(R.GOOD_VECTORS) == 38
    twins = [v for v in R.GOOD_VECTORS if "--prefix" in v["args"]]
    assert twins and all(R.golden_tracks(v, "sequence").count() == R.golden_tracks(R.vector_of(v["case"]), "sequence").count() for v in twins)


def test_every_sequence_of_every_vector_is_tiled_from_0_to_its_length_less_k():
    for v in R.GOOD_VECTORS:
        w = R.golden_tracks(v, "sequence")
        by_seq = R.intervals_by_sequence(w)
        for s, runs in enumerate(by_seq):
            if runs:
                assert runs[0][0] == 0 and runs[-1][1] == w.seq_length[s] - w.k and all(a[1] == b[0] for a, b in zip(runs, runs[1:])), (R.vector_id(v), s)


# ------------------------------------------------------------------------------------------------ 2. from the FASTA alone
EXAMPLES = [v for v in R.GOOD_VECTORS if v["case"].startswith("example_")]


@pytest.mark.parametrize("by", ["file", "sequence"])
@pytest.mark.parametrize("v", EXAMPLES, ids=[R.vector_id(v) for v in EXAMPLES])
def test_the_fasta_alone_gives_the_intervals_of_the_examples(v, by):
    records = [s for f in R.fasta_of(v) for _, s in R.read_fasta(os.path.join(GOLDEN, f))]
    assert all(set(R.plain(s)) <= set("ACGT") for s in records)
    assert R.check_fasta_statement(R.golden_tracks(v, by), records) == len(records) > 1


def test_the_fasta_statement_covers_the_examples():
    assert len(EXAMPLES) >= 2


@pytest.fixture(scope="module")
def boundary_streams(tmp_path_factory):
    """The junction stream of the first C records of the generated FASTA, from the CPU restatement of the pipeline (oracle/)."""
    from oracle import oracle as O
    d = tmp_path_factory.mktemp("boundary")
    got = {}
    for c in R.BOUNDARY_COLORS:
        fa = R.boundary_fasta(str(d / ("w%d.fa" % c)), c)
        o = O.Oracle(R.BOUNDARY_K, R.BOUNDARY_L, R.BOUNDARY_Q, O.seed_table(R.BOUNDARY_SEED, R.BOUNDARY_Q, R.BOUNDARY_L))
        o.add_fasta(fa)
        o.enumerate()
        out = str(d / ("w%d.bin" % c))
        o.write_bin(out)
        o.close()
        got[c] = (fa, out)
    return got


@pytest.mark.parametrize("c", R.BOUNDARY_COLORS)
def test_tracks_at_the_word_boundaries(boundary_streams, c, tmp_path):
    fa, stream = boundary_streams[c]
    args = [stream, "-k", str(R.BOUNDARY_K), "-s", fa]
    cwd = os.path.dirname(fa)
    gfa1 = R.run_graphdump(args + ["-f", "gfa1"], cwd=cwd)
    assert gfa1.returncode == 0 and gfa1.stderr == b""
    records = [s for _, s in R.read_fasta(fa)]
    want = R.Tracks(gfa1.stdout, R.BOUNDARY_K, [len(s) for s in records], "sequence")
    assert want.n_colors == c
    tsv, bed = serial(args, "sequence", tmp_path, cwd=cwd)
    assert tsv == want.tsv() and bed == want.bedgraph()
    R.check_text(tsv, bed)
    # the statement without any graph: every record but the one with a run of N (record 7)
    assert R.check_fasta_statement(want, records) == c - (1 if c > 7 else 0)
    last = c - 1
    one = R.Tracks(gfa1.stdout, R.BOUNDARY_K, [len(s) for s in records], "sequence", only=last)
    assert serial(args, "sequence", tmp_path, only=last, cwd=cwd) == (one.tsv(), one.bedgraph())


# ------------------------------------------------------------------------------------------------ 3. the generated inputs
def generated(name):
    return {"hot": R.hot_case, "different": R.different_case, "twins": R.twins_case, "pair_1": lambda: R.pair_case(1), "pair_2": lambda: R.pair_case(2)}[name]()


@pytest.mark.parametrize("name", ["hot", "different", "twins", "pair_1", "pair_2"])
def test_generated_tracks_equal_the_oracle(name, tmp_path):
    case = generated(name)
    by = "file" if name == "pair_1" else "sequence"
    fa, stream = case.files(str(tmp_path))
    lengths = [int(s.size) for s in case.seqs]
    want = R.Tracks(case.gfa1(), case.k, lengths, by)
    args = [os.path.basename(stream), "-k", str(case.k), "-s", os.path.basename(fa)]
    tsv, bed = serial(args, by, tmp_path, cwd=str(tmp_path))
    assert tsv == want.tsv() and bed == want.bedgraph()
    R.check_text(tsv, bed)
    rows, per_color, per_depth = want.arrays()
    # the numpy statement, which the device tests compare with, is pinned here
    color_of_seq = [0] * len(case.seqs) if by == "file" else list(range(len(case.seqs)))
    assert want.color_of_seq == color_of_seq
    assert R.same(R.direct_of(case, None, color_of_seq, want.n_colors), (rows, per_color, per_depth))
    for only in sorted({0, 1 % want.n_colors, want.n_colors - 1}):
        one = R.Tracks(case.gfa1(), case.k, lengths, by, only=only)
        assert R.same(R.direct_of(case, only, color_of_seq, want.n_colors), one.arrays())
        assert serial(args, by, tmp_path, only=only, cwd=str(tmp_path)) == (one.tsv(), one.bedgraph())
    if name == "hot":
        assert len(want.name) == R.HOT_EVENTS and want.count() == R.HOT_INTERVALS
        R.check_hot(rows)
        wide = R.hot_case(wide=True)
        w = R.case_tracks(wide)
        R.check_hot(w.arrays()[0])
        assert R.same(R.direct_of(wide), w.arrays()) and w.n_colors == 70
    if name == "different":
        assert want.count() == len(want.name)           # every event an interval of its own
        for stride in (1, 8):                           # the maps of the device tests
            c = R.different_case(stride)
            w = R.case_tracks(case, color_of_seq=c.bit_map, n_colors=c.bit_colours)
            assert w.count() == len(w.name) and R.same(R.direct_of(case, None, c.bit_map, c.bit_colours), w.arrays())
    if name == "twins":
        first_walk = [(f, l) for f, l in want.intervals if want.seq[f] == 0]
        assert first_walk == [(0, 4), (5, 5), (6, 19)]  # split in three at the segment the last colour shares
        a, b = want.colors["presence"][want.row[4]], want.colors["presence"][want.row[5]]
        assert np.flatnonzero(a != b).tolist() == [64]
    if name == "pair_1":
        assert want.n_colors == 1 and [(f, l) for f, l in want.intervals] == [(0, 39), (40, 79)] and want.depth[1][0] == 2
    if name == "pair_2":
        assert want.n_colors == 2 and [(f, l) for f, l in want.intervals] == [(0, 39), (40, 79)] and want.depth[2][0] == 2
        assert [s[2] for s in want.per_color] == [s[1] for s in want.per_color] and all(s[3] == 0 for s in want.per_color)


def test_a_sequence_without_events_between_two_that_have_some(tmp_path):
    case = R.gap_case()
    assert case.w.seq_event_begin.tolist() == [0, 4, 4, 8]
    fa, stream = case.files(str(tmp_path))
    want = R.Tracks(case.gfa1(), case.k, [int(s.size) for s in case.seqs], "sequence")
    tsv, bed = serial([os.path.basename(stream), "-k", str(case.k), "-s", os.path.basename(fa)], "sequence", tmp_path, cwd=str(tmp_path))
    assert tsv == want.tsv() and bed == want.bedgraph()
    R.check_text(tsv, bed)
    # the sequences at both sides have the same presence at the border and still an interval each; the one between them has none
    assert want.intervals == [(0, 3), (4, 7)] and [line[0] for line in want.lines()] == [0, 2] and want.per_color[1] == [0, 0, 0, 0]
    assert [line[4] for line in want.lines()] == [2, 2] and want.n_colors == 3
    assert R.same(R.direct_of(case), want.arrays())


# ------------------------------------------------------------------------------------------------ 4. where the table goes
def test_tracks_out_and_stdout(tmp_path):
    v = R.vector_of("c2_k29")
    want = R.golden_tracks(v, "sequence")
    out, bed = str(tmp_path / "tracks.tsv"), str(tmp_path / "t.bedgraph")
    r = R.run_graphdump(R.tracks_args(v) + ["--tracks", "sequence", "--tracks-out", out, "--tracks-bedgraph", bed])
    assert r.returncode == 0 and r.stdout == b"" and r.stderr == b""
    assert open(out, "rb").read() == want.tsv() and open(bed, "rb").read() == want.bedgraph()
    assert want.count() == 280


def test_both_files_or_neither(tmp_path):
    v = R.vector_of("c2_k29")
    bed, nowhere = str(tmp_path / "t.bedgraph"), str(tmp_path / "no" / "such" / "file")
    r = R.run_graphdump(R.tracks_args(v) + ["--tracks", "sequence", "--tracks-out", nowhere, "--tracks-bedgraph", bed])
    assert r.returncode == 1 and r.stdout == b"" and b"track table" in r.stderr and not os.path.exists(bed)
    out = str(tmp_path / "tracks.tsv")
    r = R.run_graphdump(R.tracks_args(v) + ["--tracks", "sequence", "--tracks-out", out, "--tracks-bedgraph", nowhere])
    assert r.returncode == 1 and r.stdout == b"" and b"track bedGraph" in r.stderr and not os.path.exists(out)
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("by", ["file", "sequence"])
def test_beside_the_other_tables(by, tmp_path):
    """One walk for all: every other table is what it is alone, the track table comes last, wherever its flag stands."""
    v = R.vector_of("c2_k29")
    base = R.tracks_args(v)
    want = R.golden_tracks(v, by).tsv()
    flags = ("--colors", "--distances", "--components", "--superbubbles", "--anchors", "--classes")
    alone = {flag: R.run_graphdump(base + [flag, by]).stdout for flag in flags}
    for flag in flags:
        r = R.run_graphdump(base + ["--tracks", by, flag, by])
        assert r.returncode == 0 and r.stderr == b"" and r.stdout == alone[flag] + want, flag
    out = str(tmp_path / "t.tsv")
    r = R.run_graphdump(base + ["--tracks", by, "--tracks-out", out, "--classes", by, "--distances", by, "--colors", by])
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == alone["--colors"] + alone["--distances"] + alone["--classes"] and open(out, "rb").read() == want
    other = "sequence" if by == "file" else "file"
    for flag, noun in (("--colors", "colour"), ("--distances", "distance"), ("--classes", "class")):
        r = R.run_graphdump(base + [flag, other, "--tracks", by])
        assert r.returncode == 1 and r.stdout == b""
        assert r.stderr.decode().startswith("PARSE ERROR: (--tracks)\n             The track table and the %s table share one set of colours: %s %s does not go with --tracks %s\n"
                                            % (noun, flag, other, by))


# ------------------------------------------------------------------------------------------------ 5. failing walks
@pytest.mark.parametrize("case", ["edge_k5", "edge_k3"])
def test_a_failing_walk_gives_its_message_and_no_output(case, tmp_path):
    v = R.vector_of(case)
    assert v["rc"] == 1
    out, bed = str(tmp_path / "tracks.tsv"), str(tmp_path / "t.bedgraph")
    r = R.run_graphdump(R.tracks_args(v) + ["--tracks", "sequence", "--tracks-out", out, "--tracks-bedgraph", bed])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode() == v["stderr"] and not os.path.exists(out) and not os.path.exists(bed), case


# ------------------------------------------------------------------------------------------------ 6. flag errors
def test_graphdump_flag_errors():
    base = ["rand6_k3.bin", "-k", "3", "-s", "rand6.fa"]
    r = R.run_graphdump(base + ["--tracks", "xml"])
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode().startswith("PARSE ERROR: Argument: (--tracks)\n             Value 'xml' does not meet constraint: file|sequence\n")
    for flag, value in (("--tracks-out", "x.tsv"), ("--tracks-bedgraph", "x.tsv"), ("--tracks-of", "0")):
        r = R.run_graphdump(base + [flag, value])
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (%s)\n             This argument needs --tracks <file|sequence>\n" % flag)
        assert not os.path.exists(os.path.join(GOLDEN, "x.tsv"))
    r = R.run_graphdump(base + ["--tracks", "file", "--tracks-bedgraph", ""])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--tracks-bedgraph)\n             The track bedGraph needs a file name\n")
    # a colour beyond the colours: one file, six sequences; in the words --anchors-ref uses
    for by, given, colours in (("file", "1", 1), ("sequence", "6", 6), ("file", "7", 1)):
        r = R.run_graphdump(base + ["--tracks", by, "--tracks-of", given])
        assert r.returncode == 1 and r.stdout == b""
        assert r.stderr.decode().startswith("PARSE ERROR: Argument: (--tracks-of)\n             Value '%s' does not meet constraint: a colour index below %d\n" % (given, colours))
        theirs = R.run_graphdump(base + ["--anchors", by, "--anchors-ref", given]).stderr.decode()
        assert r.stderr.decode() == theirs.replace("--anchors-ref", "--tracks-of")
    for given in ("-1", "x", ""):
        r = R.run_graphdump(base + ["--tracks", "file", "--tracks-of", given])
        assert r.returncode == 1 and r.stdout == b""
        assert r.stderr.decode().startswith("PARSE ERROR: Argument: (--tracks-of)\n             Value '%s' does not meet constraint: a colour index\n" % given)
    r = R.run_graphdump(base + ["--tracks", "sequence", "--tracks-of", "5"])
    assert r.returncode == 0 and r.stderr == b"" and r.stdout.startswith(b"#twopaco-tracks\t1\tby=sequence\tk=3\tcolors=6\t") and b"\tof=5\t" in r.stdout.split(b"\n")[0]
    for args in (base + ["--tracks", "file", "-f", "gfa1"], base + ["-f", "gfa1", "--tracks", "file"]):
        r = R.run_graphdump(args)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--tracks)\n             Mutually exclusive argument already set!\n")
    for text in ("host", "device"):
        r = R.run_graphdump(base + ["--tracks", "file", "--gpu", "--text", text])
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--text)\n             The track table is formatted by the host: not with --tracks\n")
    # what --classes does not go with, --tracks does not go with either
    for flag, value, noun in (("--links", [], "link"), ("--bubbles", ["file"], "bubble")):
        for args in (base + ["--tracks", "file", flag] + value, base + [flag] + value + ["--tracks", "file"]):
            r = R.run_graphdump(args)
            assert r.returncode == 1 and r.stdout == b""
            assert r.stderr.decode().startswith("PARSE ERROR: (--tracks)\n             The track table and the %s table are written one at a time: not with %s\n" % (noun, flag))
    r = R.run_graphdump(["rand6_k3.bin", "-k", "3", "--tracks", "file"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode() == "error: Required argument missing\n for arg Argument: seqfilename\n"
    r = R.run_graphdump(base + ["--tracks"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--tracks)\n             Missing a value for this argument!\n")
    r = R.run_graphdump(["--help"])
    assert r.returncode == 0 and all(x in r.stdout for x in (b"--tracks-out <file name>", b"   --tracks <file|sequence>\n", b"--tracks-bedgraph <file name>", b"--tracks-of <integer>"))


def test_twopaco_flag_errors(tmp_path):
    """The parse errors of `twopaco` that need no device."""
    def run(args):
        return subprocess.run([R.TWOPACO] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    fa = os.path.join(GOLDEN, "rand6.fa")
    for flag, value in (("--tracks-out", "x.tsv"), ("--tracks-bedgraph", "x.tsv"), ("--tracks-of", "0")):
        r = run(["-f", "20", flag, value, fa])
        assert r.returncode == 1 and r.stderr.decode() == "\nError: This argument needs --tracks <file|sequence> for arg (%s)\n" % flag
    r = run(["-f", "20", "--tracks", "file", "--gpus", "2", fa])
    assert r.returncode == 1
    assert r.stderr.decode() == "\nError: The track table is written by one GPU only (every rank holds its own piece of the junction stream): not with --gpus above 1 for arg (--tracks)\n"
    for flag, noun in (("--colors", "colour"), ("--bubbles", "bubble"), ("--distances", "distance"), ("--classes", "class")):
        for theirs, ours in (("file", "sequence"), ("sequence", "file")):
            r = run(["-f", "20", flag, theirs, "--tracks", ours, fa])
            assert r.returncode == 1
            assert r.stderr.decode() == "\nError: The track table and the %s table share one set of colours: %s %s does not go with --tracks %s for arg (--tracks)\n" % (
                noun, flag, theirs, ours)
    r = run(["-f", "20", "--tracks", "xml", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: Value 'xml' does not meet constraint: file|sequence for arg (--tracks)\n"
    r = run(["-f", "20", "--tracks", "file", "--tracks-bedgraph", "", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: The track bedGraph needs a file name for arg (--tracks-bedgraph)\n"
    # by file, an index at or beyond the number of input files, in the words --anchors-ref uses
    for given in ("1", "9"):
        r = run(["-f", "20", "--tracks", "file", "--tracks-of", given, fa])
        assert r.returncode == 1 and r.stderr.decode() == "\nError: Value '%s' does not meet constraint: a colour index below 1 for arg (--tracks-of)\n" % given
        theirs = run(["-f", "20", "--anchors", "file", "--anchors-ref", given, fa]).stderr.decode()
        assert r.stderr.decode() == theirs.replace("--anchors-ref", "--tracks-of")
    r = run(["-f", "20", "--tracks", "file", "--tracks-of", "-1", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: Value '-1' does not meet constraint: a colour index for arg (--tracks-of)\n"
    assert os.listdir(str(tmp_path)) == []
    r = run(["--help"])
    assert r.returncode == 0 and b"[--tracks <file|sequence>] [--tracks-of <integer>] [--tracks-out <file name>] [--tracks-bedgraph <file name>]" in r.stdout
