"""CPU: the genome distance table of the serial `graphdump --distances` against its definition, restated in distances_reference.py
over the serial gfa1 text (itself pinned to the real reference's sha256 by tests/golden/graphdump.json): byte for byte on every
golden vector whose gfa1 succeeds, the hot row, the PHYLIP bytes, the walk's errors, the flags' errors, the word boundaries of the
presence bits, and two identities against the colour table's histogram."""
import os
import subprocess

import numpy as np
import pytest

import bubbles_reference as B
import colors_reference as R
import distances_reference as D
from helpers import GOLDEN, golden_cases


@pytest.fixture(scope="module", autouse=True)
def built():
    assert os.path.exists(R.GRAPHDUMP) and os.path.exists(R.TWOPACO), "run build() first"


def args_of(v):
    k = int(v["args"][v["args"].index("-k") + 1])
    files = [v["args"][i + 1] for i, a in enumerate(v["args"]) if a == "-s"]
    return k, files


# ------------------------------------------------------------------------------------------------ 1. golden vectors
@pytest.mark.parametrize("v", R.GOOD_VECTORS, ids=[R.vector_id(v) for v in R.GOOD_VECTORS])
def test_serial_distances_equal_the_oracle(v):
    gfa1 = R.golden_gfa1(v)
    k, files = args_of(v)
    for by in ("sequence", "file"):
        want, _, segments, edges, t = D.tsv(gfa1, by, k, files)
        r = R.run_graphdump(R.colors_args(v) + ["--distances", by])
        assert r.returncode == 0 and r.stderr == b"", r.stderr
        assert r.stdout == want, (R.vector_id(v), by)
        assert (segments == segments.T).all() and (edges == edges.T).all()
        assert (np.diag(segments) == t["presence"].sum(axis=0)).all()


def test_there_are_38_vectors():
    assert len(R.GOOD_VECTORS) == 38


def test_the_hot_row_of_the_tracts():
    """tr_k25_L28 (tracts.fa: a poly-A tract): one segment takes 4201 of the 29895 events; it counts once per colour pair."""
    case = [c for c in golden_cases() if c["name"] == "tr_k25_L28"][0]
    v = R.case_vector(case)
    gfa1 = R.golden_gfa1(v)
    for by in ("sequence", "file"):
        want, _, segments, _, t = D.tsv(gfa1, by, case["k"], [case["fasta"]])
        r = R.run_graphdump(R.colors_args(v) + ["--distances", by])
        assert r.returncode == 0 and r.stderr == b"" and r.stdout == want, by
    assert int(t["occurrences"].max()) == 4201 and int(segments.max()) <= len(t["name"])


def test_distances_out_writes_the_same_bytes(tmp_path):
    v = R.vector_of("rand6_k9_fp")
    out = str(tmp_path / "distances.tsv")
    r = R.run_graphdump(R.colors_args(v) + ["--distances", "file", "--distances-out", out])
    assert r.returncode == 0 and r.stdout == b"" and r.stderr == b""
    assert open(out, "rb").read() == R.run_graphdump(R.colors_args(v) + ["--distances", "file"]).stdout


@pytest.mark.parametrize("by", ["file", "sequence"])
def test_beside_the_colour_or_the_bubble_table_of_the_same_colours(tmp_path, by):
    """--colors or --bubbles with the same colours: that table first, to its file or to stdout, the distance table after it."""
    v = R.vector_of("rand6_k9_fp")
    args = R.colors_args(v)
    distances = R.run_graphdump(args + ["--distances", by]).stdout
    for flag in ("--colors", "--bubbles"):
        other = R.run_graphdump(args + [flag, by]).stdout
        assert other and distances
        out = str(tmp_path / "other.tsv")
        r = R.run_graphdump(args + [flag, by, flag + "-out", out, "--distances", by])
        assert r.returncode == 0 and r.stderr == b"" and r.stdout == distances and open(out, "rb").read() == other, flag
        r = R.run_graphdump(args + ["--distances", by, flag, by])
        assert r.returncode == 0 and r.stderr == b"" and r.stdout == other + distances, flag
    # a stream the walk refuses: the walk's message and nothing else, whichever tables were asked for
    bad = R.vector_of("edge_k5")
    r = R.run_graphdump(R.colors_args(bad) + ["--colors", by, "--distances", by, "--distances-out", str(tmp_path / "d.tsv")])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode() == bad["stderr"] and not os.path.exists(str(tmp_path / "d.tsv"))


def test_both_files_or_neither(tmp_path):
    """The TSV and the PHYLIP matrix are written both or not at all: a file that cannot be created leaves the other one absent."""
    v = R.vector_of("rand6_k9_fp")
    tsv, phy = str(tmp_path / "d.tsv"), str(tmp_path / "d.phy")
    nowhere = str(tmp_path / "no" / "such" / "file")
    r = R.run_graphdump(R.colors_args(v) + ["--distances", "file", "--distances-out", tsv, "--distances-phylip", nowhere])
    assert r.returncode == 1 and r.stdout == b"" and b"PHYLIP matrix" in r.stderr and os.listdir(str(tmp_path)) == []
    r = R.run_graphdump(R.colors_args(v) + ["--distances", "file", "--distances-out", nowhere, "--distances-phylip", phy])
    assert r.returncode == 1 and r.stdout == b"" and b"distance table" in r.stderr and os.listdir(str(tmp_path)) == []
    r = R.run_graphdump(R.colors_args(v) + ["--distances", "file", "--distances-out", tsv, "--distances-phylip", phy])
    assert r.returncode == 0 and sorted(os.listdir(str(tmp_path))) == ["d.phy", "d.tsv"]


# ------------------------------------------------------------------------------------------------ 2. PHYLIP
@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    """(fasta, an empty fasta, stream): two identical records and a third one; the empty file is a colour without sequences."""
    d = tmp_path_factory.mktemp("twins")
    fa = D.twins_fasta(str(d / "twins.fa"))
    empty = str(d / "empty.fa")
    open(empty, "w").close()
    return fa, empty, B.oracle_stream(fa, str(d / "twins.bin"), 11, 20, 5, 11)


@pytest.mark.parametrize("case", ["rand6_k9_fp", "example_k11"])
def test_phylip_of_golden_vectors(case, tmp_path):
    v = R.vector_of(case)
    k, files = args_of(v)
    out = str(tmp_path / "d.phy")
    for by in ("sequence", "file"):
        want, want_phy, _, _, _ = D.tsv(R.golden_gfa1(v), by, k, files)
        r = R.run_graphdump(R.colors_args(v) + ["--distances", by, "--distances-phylip", out])
        assert r.returncode == 0 and r.stderr == b"" and r.stdout == want
        assert open(out, "rb").read() == want_phy, (case, by)


def test_phylip_with_an_empty_colour_and_two_identical_colours(twins, tmp_path):
    fa, empty, stream = twins
    cwd = os.path.dirname(fa)
    gfa1 = R.run_graphdump([stream, "-k", "11", "-s", fa, "-f", "gfa1"], cwd=cwd)
    assert gfa1.returncode == 0 and gfa1.stderr == b""
    out = str(tmp_path / "d.phy")
    # by sequence: records 0 and 1 are the same letters
    want, want_phy, segments, edges, _ = D.tsv(gfa1.stdout, "sequence", 11, [fa])
    r = R.run_graphdump([stream, "-k", "11", "-s", fa, "--distances", "sequence", "--distances-phylip", out], cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == want
    got = open(out, "rb").read()
    assert got == want_phy
    lines = got.decode().split("\n")
    assert lines[0] == "3" and lines[1].split(" ")[2] == "0.000000" and lines[2].split(" ")[1] == "0.000000"
    assert lines[1].startswith("1_" + fa + " ") and edges[0, 1] == edges[0, 0] == edges[1, 1] > 0
    assert lines[1].split(" ")[3] != "0.000000"
    # by file: the second file holds no sequence, its colour is a zero row and a zero column
    want, want_phy, segments, edges, _ = D.tsv(gfa1.stdout, "file", 11, [fa, empty])
    r = R.run_graphdump([stream, "-k", "11", "-s", fa, "-s", empty, "--distances", "file", "--distances-phylip", out], cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == want
    assert open(out, "rb").read() == want_phy
    assert segments.shape == (2, 2) and not segments[1].any() and not edges[:, 1].any()
    assert want_phy.decode().split("\n")[2] == empty + " 1.000000 0.000000"


# ------------------------------------------------------------------------------------------------ 3. failing walks
@pytest.mark.parametrize("case", ["edge_k5", "edge_k5_dbg", "edge_k7_fp_r2", "edge_k3"])
def test_a_failing_walk_gives_its_message_and_no_output(case, tmp_path):
    v = R.vector_of(case)
    assert v["rc"] == 1
    gfa1 = R.run_graphdump(v["args"])
    assert gfa1.returncode == 1 and gfa1.stderr.decode() == v["stderr"]
    out, phy = str(tmp_path / "distances.tsv"), str(tmp_path / "d.phy")
    for by in ("file", "sequence"):
        r = R.run_graphdump(R.colors_args(v) + ["--distances", by])
        assert r.returncode == 1 and r.stdout == b"" and r.stderr == gfa1.stderr, (case, by)
        r = R.run_graphdump(R.colors_args(v) + ["--distances", by, "--distances-out", out, "--distances-phylip", phy])
        assert r.returncode == 1 and r.stdout == b"" and r.stderr == gfa1.stderr and not os.path.exists(out) and not os.path.exists(phy), (case, by)


# ------------------------------------------------------------------------------------------------ 4. flag errors
def test_graphdump_flag_errors():
    base = ["rand6_k3.bin", "-k", "3", "-s", "rand6.fa"]
    r = R.run_graphdump(base + ["--distances", "xml"])
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode().startswith("PARSE ERROR: Argument: (--distances)\n             Value 'xml' does not meet constraint: file|sequence\n")
    r = R.run_graphdump(["rand6_k3.bin", "-k", "3", "--distances", "file"])
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode() == "error: Required argument missing\n for arg Argument: seqfilename\n"
    r = R.run_graphdump(base + ["--distances", "file", "-f", "gfa1"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--distances)\n")
    # the modes of two colour-carrying tables must be equal
    r = R.run_graphdump(base + ["--distances", "file", "--colors", "sequence"])
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode().startswith("PARSE ERROR: (--distances)\n             The distance table and the colour table share one set of colours: --colors sequence does not go with --distances file\n")
    r = R.run_graphdump(base + ["--bubbles", "file", "--distances", "sequence"])
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode().startswith("PARSE ERROR: (--distances)\n             The distance table and the bubble table share one set of colours: --bubbles file does not go with --distances sequence\n")
    r = R.run_graphdump(base + ["--distances", "file", "--gpu", "--text", "device"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--text)\n             The distance table is formatted by the host: not with --distances\n")
    r = R.run_graphdump(base + ["--distances", "file", "--text", "host"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--text)\n")
    r = R.run_graphdump(base + ["--distances-phylip", "x.phy"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--distances-phylip)\n             This argument needs --distances <file|sequence>\n")
    r = R.run_graphdump(base + ["--distances-out", "x.tsv"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--distances-out)\n")
    assert not os.path.exists(os.path.join(GOLDEN, "x.tsv")) and not os.path.exists(os.path.join(GOLDEN, "x.phy"))
    r = R.run_graphdump(["--help"])
    assert r.returncode == 0 and b"--distances <file|sequence>" in r.stdout and b"--distances-out <file name>" in r.stdout and b"--distances-phylip <file name>" in r.stdout


def test_twopaco_flag_errors(tmp_path):
    """The parse errors of `twopaco` that need no device."""
    def run(args):
        return subprocess.run([R.TWOPACO] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    fa = os.path.join(GOLDEN, "rand6.fa")
    r = run(["-f", "20", "--distances", "xml", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: Value 'xml' does not meet constraint: file|sequence for arg (--distances)\n"
    r = run(["-f", "20", "--distances-out", "x.tsv", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: This argument needs --distances <file|sequence> for arg (--distances-out)\n"
    r = run(["-f", "20", "--distances-phylip", "x.phy", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: This argument needs --distances <file|sequence> for arg (--distances-phylip)\n"
    r = run(["-f", "20", "--distances", "file", "--colors", "sequence", fa])
    assert r.returncode == 1 and r.stderr.decode().startswith("\nError: The distance table and the colour table share one set of colours") and r.stderr.decode().endswith(" for arg (--distances)\n")
    r = run(["-f", "20", "--distances", "file", "--bubbles", "sequence", fa])
    assert r.returncode == 1 and r.stderr.decode().startswith("\nError: The distance table and the bubble table share one set of colours")
    r = run(["-f", "20", "--distances", "file", "--gpus", "2", fa])
    assert r.returncode == 1 and r.stderr.decode().startswith("\nError: The distance table is written by one GPU only") and r.stderr.decode().endswith(" for arg (--distances)\n")
    r = run(["-f", "20", "--distances"])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: Missing a value for this argument! for arg (--distances)\n"
    assert os.listdir(str(tmp_path)) == []
    r = run(["--help"])
    assert r.returncode == 0 and b"--distances <file|sequence>" in r.stdout and b"--distances-phylip <file name>" in r.stdout


# ------------------------------------------------------------------------------------------------ 5. word boundaries of presence
@pytest.fixture(scope="module")
def boundary_streams(tmp_path_factory):
    """The junction stream of the first C records of the colour test's generated FASTA, from the CPU restatement of the pipeline."""
    d = tmp_path_factory.mktemp("boundary")
    got = {}
    for c in R.BOUNDARY_COLORS:
        fa = R.boundary_fasta(str(d / ("w%d.fa" % c)), c)
        got[c] = (fa, B.oracle_stream(fa, str(d / ("w%d.bin" % c)), R.BOUNDARY_K, R.BOUNDARY_L, R.BOUNDARY_Q, R.BOUNDARY_SEED))
    return got


@pytest.mark.parametrize("c", R.BOUNDARY_COLORS)
def test_distances_at_the_word_boundaries(boundary_streams, c):
    fa, stream = boundary_streams[c]
    args = [stream, "-k", str(R.BOUNDARY_K), "-s", fa]
    gfa1 = R.run_graphdump(args + ["-f", "gfa1"], cwd=os.path.dirname(fa))
    assert gfa1.returncode == 0 and gfa1.stderr == b""
    want, _, segments, edges, t = D.tsv(gfa1.stdout, "sequence", R.BOUNDARY_K, [fa])
    assert segments.shape == (c, c) and segments[c - 1, c - 1] > 0 and segments.min() > 0   # one segment lies in every record
    r = R.run_graphdump(args + ["--distances", "sequence"], cwd=os.path.dirname(fa))
    assert r.returncode == 0 and r.stderr == b""
    assert r.stdout == want
    assert len(r.stdout.decode().split("\n")) == 1 + 2 * c + c * (c - 1) // 2 + 1
    want_file, _, _, _, _ = D.tsv(gfa1.stdout, "file", R.BOUNDARY_K, [fa])
    r = R.run_graphdump(args + ["--distances", "file"], cwd=os.path.dirname(fa))
    assert r.returncode == 0 and r.stdout == want_file


# ------------------------------------------------------------------------------------------------ 6. the colour histogram
@pytest.mark.parametrize("case", ["rand6_k9_fp", "rand6_k3"])
def test_the_matrix_sums_equal_the_moments_of_the_colour_histogram(case):
    """A row of n colours adds 1 to n diagonal entries and to n^2 entries in all: the sum of the diagonal of `segments` is the
    first moment of the colour table's histogram and the sum of the whole matrix its second.  Both sides are the project's
    own serial outputs, --colors and --distances."""
    v = R.vector_of(case)
    col = R.run_graphdump(R.colors_args(v) + ["--colors", "sequence"])
    dst = R.run_graphdump(R.colors_args(v) + ["--distances", "sequence"])
    assert col.returncode == 0 and dst.returncode == 0
    hist = [(int(f[1]), int(f[2])) for f in (line.split("\t") for line in col.stdout.decode().split("\n")) if f[0] == "#hist"]
    segments, _ = D.parse(dst.stdout)
    assert hist and int(np.trace(segments)) == sum(n * s for n, s in hist)
    assert int(segments.sum()) == sum(n * n * s for n, s in hist)
