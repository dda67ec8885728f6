"""CPU: the class table of the serial `graphdump --classes` against its definition, restated in classes_reference.py over the serial
gfa1 text (itself pinned to the real reference's sha256 by tests/golden/graphdump.json): byte for byte on every golden vector whose
gfa1 succeeds, in both colour modes, the table and the members file; on the word-boundary input of colors_reference at 1 .. 65
colours; on the generated inputs (hot, all different, twins); the consequences of the definition from the oracle and from the
program's text alone; the table beside the other tables; the flags' errors of both programs."""
import os
import subprocess

import pytest

import classes_reference as R
import colors_reference as C
import distances_reference as D
from helpers import GOLDEN


@pytest.fixture(scope="module", autouse=True)
def built():
    assert os.path.exists(R.GRAPHDUMP) and os.path.exists(R.TWOPACO), "run build() first"


def serial(args, by, tmp_path, cwd=GOLDEN):
    """(table from stdout, members file) of the serial graphdump."""
    members = str(tmp_path / "members.tsv")
    r = R.run_graphdump(list(args) + ["--classes", by, "--classes-members", members], cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    return r.stdout, open(members, "rb").read()


def check_consequences(want, tsv, members, colors_tsv):
    """What the definition implies, on the oracle and on the program's text."""
    t = want.colors
    assert int(want.segments.sum()) == want.rows and (want.segments > 0).all()
    assert (want.sets_segments == t["hist_segments"]).all()
    seg, edg = D.matrices(t, want.k)
    got_seg, got_edg = want.matrices()
    assert (got_seg == seg).all() and (got_edg == edg).all()
    assert R.check_text(tsv, members, colors_tsv) == want.count()


# ------------------------------------------------------------------------------------------------ 1. golden vectors
# classes by sequence, measured with the oracle's grouping; by file these vectors have one colour and one class.  rand6_k9_a3 cuts
# the graph by abundance: 691 rows instead of the 1474 of the other rand6_k9_* vectors, and 27 classes instead of 50
BY_SEQUENCE = (("rand6_k9_a3", 27), ("rand6_k9_", 50), ("rand6_k25_q3", 37), ("rand6_k27", 38), ("rand6_k3", 7), ("c2_", 7), ("example_", 3))


def classes_by_sequence(case):
    hits = [n for prefix, n in BY_SEQUENCE if case.startswith(prefix)]   # (the first prefix that fits: a3 before the other k9)
    return hits[0] if hits else None


@pytest.mark.parametrize("by", ["file", "sequence"])
@pytest.mark.parametrize("v", R.GOOD_VECTORS, ids=[R.vector_id(v) for v in R.GOOD_VECTORS])
def test_serial_classes_equal_the_oracle(v, by, tmp_path):
    want = R.golden_classes(v, by)
    tsv, members = serial(R.classes_args(v), by, tmp_path)
    assert tsv == want.tsv(), R.vector_id(v)
    assert members == want.members(), R.vector_id(v)
    colors_tsv = R.run_graphdump(R.classes_args(v) + ["--colors", by]).stdout
    check_consequences(want, tsv, members, colors_tsv)
    assert want.rows > 0
    if by == "file":
        assert (want.colors["colors"], want.count()) == (1, 1)
    else:
        known = classes_by_sequence(v["case"])
        assert known is None or want.count() == known, (v["case"], want.count())
        if v["case"].startswith("rand6_k9_"):
            assert (want.rows, want.colors["colors"]) == ((691, 6) if v["case"] == "rand6_k9_a3" else (1474, 6))


def test_the_golden_counts_cover_the_vectors():
    """Counted on the oracle alone: every family of vectors the counts above name exists, so the test cannot pass on an empty table."""
    for prefix, n in BY_SEQUENCE:
        named = [v for v in R.GOOD_VECTORS if v["case"].startswith(prefix) and classes_by_sequence(v["case"]) == n]
        assert named, prefix
        assert all(R.golden_classes(v, "sequence").count() == n for v in named), prefix
    assert len(R.GOOD_VECTORS) == 38


# ------------------------------------------------------------------------------------------------ 2. the word boundaries of the key
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
def test_classes_at_the_word_boundaries(boundary_streams, c, tmp_path):
    fa, stream = boundary_streams[c]
    args = [stream, "-k", str(R.BOUNDARY_K), "-s", fa]
    cwd = os.path.dirname(fa)
    gfa1 = R.run_graphdump(args + ["-f", "gfa1"], cwd=cwd)
    assert gfa1.returncode == 0 and gfa1.stderr == b""
    want = R.Classes(gfa1.stdout, "sequence", k=R.BOUNDARY_K, files=[fa])
    assert want.colors["colors"] == c
    tsv, members = serial(args, "sequence", tmp_path, cwd=cwd)
    assert tsv == want.tsv() and members == want.members()
    check_consequences(want, tsv, members, R.run_graphdump(args + ["--colors", "sequence"], cwd=cwd).stdout)
    if c == 33:
        assert (want.count(), want.rows) == (184, 318)
    if c == 65:
        assert (want.count(), want.rows, want.largest()) == (425, 597, 36) and C.presence_words(want.presence).shape[1] == 3


# ------------------------------------------------------------------------------------------------ 3. the generated inputs
@pytest.mark.parametrize("name", ["hot", "different", "twins"])
def test_generated_classes_equal_the_oracle(name, tmp_path):
    case = {"hot": R.hot_case, "different": R.different_case, "twins": R.twins_case}[name]()
    fa, stream = case.files(str(tmp_path))
    want = R.Classes(case.gfa1(), "sequence", k=case.k, files=[os.path.basename(fa)])
    args = [os.path.basename(stream), "-k", str(case.k), "-s", os.path.basename(fa)]
    tsv, members = serial(args, "sequence", tmp_path, cwd=str(tmp_path))
    assert tsv == want.tsv() and members == want.members()
    check_consequences(want, tsv, members, R.run_graphdump(args + ["--colors", "sequence"], cwd=str(tmp_path)).stdout)
    if name == "hot":
        R.check_hot(want)
        wide = R.hot_case(wide=True)
        R.check_hot(R.Classes(wide.gfa1(), k=wide.k, color_of_seq=wide.color_of_seq, n_colors=wide.n_colors))
    if name == "different":
        assert want.count() == want.rows == R.DIFFERENT_ROWS and want.colors["colors"] > 1000
        for stride in (1, 8):     # the maps of the device tests: every row a class of its own under them as well
            c = R.different_case(stride)
            w = R.Classes(case.gfa1(), k=c.k, color_of_seq=c.bit_map, n_colors=c.bit_colours)
            assert w.count() == w.rows == R.DIFFERENT_ROWS and w.colors["colors"] == c.bit_colours
    if name == "twins":
        R.check_twins(want)


# ------------------------------------------------------------------------------------------------ 4. where the table goes
def test_classes_out_and_stdout(tmp_path):
    v = R.vector_of("c2_k29")
    want = R.golden_classes(v, "sequence")
    out, members = str(tmp_path / "classes.tsv"), str(tmp_path / "m.tsv")
    r = R.run_graphdump(R.classes_args(v) + ["--classes", "sequence", "--classes-out", out, "--classes-members", members])
    assert r.returncode == 0 and r.stdout == b"" and r.stderr == b""
    assert open(out, "rb").read() == want.tsv() and open(members, "rb").read() == want.members()
    r = R.run_graphdump(R.classes_args(v) + ["--classes", "sequence", "--prefix"])
    assert r.returncode == 0 and r.stdout == want.tsv() and r.stderr == b""


@pytest.mark.parametrize("by", ["file", "sequence"])
def test_beside_the_other_tables(by, tmp_path):
    """One walk for all: every other table is what it is alone, the class table comes last, wherever its flag stands."""
    v = R.vector_of("c2_k29")
    base = R.classes_args(v)
    want = R.golden_classes(v, by).tsv()
    flags = ("--colors", "--distances", "--components", "--superbubbles", "--anchors")
    alone = {flag: R.run_graphdump(base + [flag, by]).stdout for flag in flags}
    for flag in flags:
        r = R.run_graphdump(base + ["--classes", by, flag, by])
        assert r.returncode == 0 and r.stderr == b"" and r.stdout == alone[flag] + want, flag
    out = str(tmp_path / "c.tsv")
    r = R.run_graphdump(base + ["--classes", by, "--classes-out", out, "--distances", by, "--colors", by])
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == alone["--colors"] + alone["--distances"] and open(out, "rb").read() == want
    other = "sequence" if by == "file" else "file"
    for flag, noun in (("--colors", "colour"), ("--distances", "distance"), ("--components", "component")):
        r = R.run_graphdump(base + [flag, other, "--classes", by])
        assert r.returncode == 1 and r.stdout == b""
        assert r.stderr.decode().startswith("PARSE ERROR: (--classes)\n             The class table and the %s table share one set of colours: %s %s does not go with --classes %s\n"
                                            % (noun, flag, other, by))


# ------------------------------------------------------------------------------------------------ 5. failing walks
@pytest.mark.parametrize("case", ["edge_k5", "edge_k3"])
def test_a_failing_walk_gives_its_message_and_no_output(case, tmp_path):
    v = R.vector_of(case)
    assert v["rc"] == 1
    out, members = str(tmp_path / "classes.tsv"), str(tmp_path / "members.tsv")
    r = R.run_graphdump(R.classes_args(v) + ["--classes", "sequence", "--classes-out", out, "--classes-members", members])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode() == v["stderr"] and not os.path.exists(out) and not os.path.exists(members), case


# ------------------------------------------------------------------------------------------------ 6. flag errors
def test_graphdump_flag_errors():
    base = ["rand6_k3.bin", "-k", "3", "-s", "rand6.fa"]
    r = R.run_graphdump(base + ["--classes", "xml"])
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode().startswith("PARSE ERROR: Argument: (--classes)\n             Value 'xml' does not meet constraint: file|sequence\n")
    for flag in ("--classes-out", "--classes-members"):
        r = R.run_graphdump(base + [flag, "x.tsv"])
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (%s)\n             This argument needs --classes <file|sequence>\n" % flag)
        assert not os.path.exists(os.path.join(GOLDEN, "x.tsv"))
    r = R.run_graphdump(base + ["--classes", "file", "--classes-members", ""])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--classes-members)\n             The class members need a file name\n")
    for args in (base + ["--classes", "file", "-f", "gfa1"], base + ["-f", "gfa1", "--classes", "file"]):
        r = R.run_graphdump(args)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--classes)\n             Mutually exclusive argument already set!\n")
    for text in ("host", "device"):
        r = R.run_graphdump(base + ["--classes", "file", "--gpu", "--text", text])
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--text)\n             The class table is formatted by the host: not with --classes\n")
    # what --colors does not go with, --classes does not go with either
    for flag, value, noun in (("--links", [], "link"), ("--bubbles", ["file"], "bubble")):
        for args in (base + ["--classes", "file", flag] + value, base + [flag] + value + ["--classes", "file"]):
            r = R.run_graphdump(args)
            assert r.returncode == 1 and r.stdout == b""
            assert r.stderr.decode().startswith("PARSE ERROR: (--classes)\n             The class table and the %s table are written one at a time: not with %s\n" % (noun, flag))
    r = R.run_graphdump(["rand6_k3.bin", "-k", "3", "--classes", "file"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode() == "error: Required argument missing\n for arg Argument: seqfilename\n"
    r = R.run_graphdump(base + ["--classes"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--classes)\n             Missing a value for this argument!\n")
    r = R.run_graphdump(["--help"])
    assert r.returncode == 0 and b"--classes-out <file name>" in r.stdout and b"   --classes <file|sequence>\n" in r.stdout and b"--classes-members <file name>" in r.stdout


def test_twopaco_flag_errors(tmp_path):
    """The parse errors of `twopaco` that need no device."""
    def run(args):
        return subprocess.run([R.TWOPACO] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    fa = os.path.join(GOLDEN, "rand6.fa")
    for flag in ("--classes-out", "--classes-members"):
        r = run(["-f", "20", flag, "x.tsv", fa])
        assert r.returncode == 1 and r.stderr.decode() == "\nError: This argument needs --classes <file|sequence> for arg (%s)\n" % flag
    r = run(["-f", "20", "--classes", "file", "--gpus", "2", fa])
    assert r.returncode == 1
    assert r.stderr.decode() == "\nError: The class table is written by one GPU only (every rank holds its own piece of the junction stream): not with --gpus above 1 for arg (--classes)\n"
    for flag, noun in (("--colors", "colour"), ("--bubbles", "bubble"), ("--distances", "distance"), ("--components", "component")):
        for theirs, ours in (("file", "sequence"), ("sequence", "file")):
            r = run(["-f", "20", flag, theirs, "--classes", ours, fa])
            assert r.returncode == 1
            assert r.stderr.decode() == "\nError: The class table and the %s table share one set of colours: %s %s does not go with --classes %s for arg (--classes)\n" % (
                noun, flag, theirs, ours)
    r = run(["-f", "20", "--classes", "xml", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: Value 'xml' does not meet constraint: file|sequence for arg (--classes)\n"
    r = run(["-f", "20", "--classes", "file", "--classes-members", "", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: The class members need a file name for arg (--classes-members)\n"
    assert os.listdir(str(tmp_path)) == []
    r = run(["--help"])
    assert r.returncode == 0 and b"[--classes <file|sequence>] [--classes-out <file name>] [--classes-members <file name>]" in r.stdout
