"""CPU: the segment colour table of the serial `graphdump --colors` against its definition, restated in colors_reference.py
over the serial gfa1 text (itself pinned to the real reference's sha256 by tests/golden/graphdump.json): byte for byte on
every golden vector whose gfa1 succeeds, the walk's errors, the flags' errors, and the word boundaries of the presence bits."""
import os
import subprocess

import numpy as np
import pytest

import colors_reference as R
from helpers import GOLDEN, golden_cases


@pytest.fixture(scope="module", autouse=True)
def built():
    assert os.path.exists(R.GRAPHDUMP) and os.path.exists(R.TWOPACO), "run build() first"


# ------------------------------------------------------------------------------------------------ 1. golden vectors
_SEEN = {}


@pytest.mark.parametrize("v", R.GOOD_VECTORS, ids=[R.vector_id(v) for v in R.GOOD_VECTORS])
def test_serial_colors_equal_the_oracle(v):
    gfa1 = R.golden_gfa1(v)
    k = int(v["args"][v["args"].index("-k") + 1])
    files = [v["args"][i + 1] for i, a in enumerate(v["args"]) if a == "-s"]
    for by in ("sequence", "file"):
        want, t = R.tsv(gfa1, by, k, files)
        r = R.run_graphdump(R.colors_args(v) + ["--colors", by])
        assert r.returncode == 0 and r.stderr == b"", r.stderr
        assert r.stdout == want, (R.vector_id(v), by)
        if by == "sequence":
            _SEEN[R.vector_id(v)] = {"rows": len(t["name"]), "multi": int((t["n_colors"] > 1).sum()),
                                     "both": int(((t["forward"] > 0) & (t["forward"] < t["occurrences"])).sum()),
                                     "named": int((t["name"] >= R.FRESH).sum()), "deep": int((t["occurrences"] > t["n_colors"]).sum()),
                                     "hot": int(t["occurrences"].max()) if len(t["name"]) else 0, "events": t["events"]}


def test_the_golden_vectors_exercise_the_table():
    """The inputs above hold what the table is about (counted by the oracle): rows in several colours, rows seen on both strands,
    'N'-named rows, rows that occur more often than they have colours, and one hot row of thousands of occurrences."""
    if len(_SEEN) != len(R.GOOD_VECTORS):   # run alone: count here
        for v in R.GOOD_VECTORS:
            test_serial_colors_equal_the_oracle(v)
    assert len(_SEEN) == 38
    s = _SEEN["rand6_k9_fp"]
    assert (s["rows"], s["multi"], s["both"], s["named"]) == (1474, 820, 15, 17), s
    s = _SEEN["rand6_k3"]
    assert s["multi"] == 138 and s["deep"] >= 138, s
    assert any(x["multi"] for x in _SEEN.values()) and any(x["both"] for x in _SEEN.values()) and any(x["named"] for x in _SEEN.values())


def test_the_hot_row_of_the_tracts():
    """tr_k25_L28 (tracts.fa: a poly-A tract): one segment takes 4201 of the 29895 events, nearly all of them consecutive.  Its
    gfa1 is pinned by the reference's vector in tests/golden/graphdump_tracts.json."""
    case = [c for c in golden_cases() if c["name"] == "tr_k25_L28"][0]
    v = R.case_vector(case)
    gfa1 = R.golden_gfa1(v)
    for by in ("sequence", "file"):
        want, t = R.tsv(gfa1, by, case["k"], [case["fasta"]])
        r = R.run_graphdump(R.colors_args(v) + ["--colors", by])
        assert r.returncode == 0 and r.stderr == b"" and r.stdout == want, by
    assert t["events"] == 29895 and int(t["occurrences"].max()) == 4201 and int(t["occurrences"].max()) > 1000
    assert (t["name"] >= R.FRESH).any()


def test_colors_out_writes_the_same_bytes(tmp_path):
    v = R.vector_of("rand6_k9_fp")
    out = str(tmp_path / "colors.tsv")
    r = R.run_graphdump(R.colors_args(v) + ["--colors", "file", "--colors-out", out])
    assert r.returncode == 0 and r.stdout == b"" and r.stderr == b""
    assert open(out, "rb").read() == R.run_graphdump(R.colors_args(v) + ["--colors", "file"]).stdout


# ------------------------------------------------------------------------------------------------ 2. failing walks
@pytest.mark.parametrize("case", ["edge_k5", "edge_k5_dbg", "edge_k7_fp_r2", "edge_k3"])
def test_a_failing_walk_gives_its_message_and_no_output(case, tmp_path):
    v = R.vector_of(case)
    assert v["rc"] == 1
    gfa1 = R.run_graphdump(v["args"])
    assert gfa1.returncode == 1 and gfa1.stderr.decode() == v["stderr"]
    out = str(tmp_path / "colors.tsv")
    for by in ("file", "sequence"):
        r = R.run_graphdump(R.colors_args(v) + ["--colors", by])
        assert r.returncode == 1 and r.stdout == b"" and r.stderr == gfa1.stderr, (case, by)
        r = R.run_graphdump(R.colors_args(v) + ["--colors", by, "--colors-out", out])
        assert r.returncode == 1 and r.stdout == b"" and r.stderr == gfa1.stderr and not os.path.exists(out), (case, by)


# ------------------------------------------------------------------------------------------------ 3. flag errors
def test_graphdump_flag_errors():
    base = ["rand6_k3.bin", "-k", "3", "-s", "rand6.fa"]
    r = R.run_graphdump(base + ["--colors", "xml"])
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode().startswith("PARSE ERROR: Argument: (--colors)\n             Value 'xml' does not meet constraint: file|sequence\n")
    r = R.run_graphdump(["rand6_k3.bin", "-k", "3", "--colors", "file"])
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode() == "error: Required argument missing\n for arg Argument: seqfilename\n"   # as gfa1 without -s
    r = R.run_graphdump(base + ["--colors", "file", "-f", "gfa1"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--colors)\n")
    r = R.run_graphdump(base + ["-f", "gfa1", "--colors", "file"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--colors)\n")
    r = R.run_graphdump(base + ["--colors-out", "x.tsv"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--colors-out)\n")
    assert not os.path.exists(os.path.join(GOLDEN, "x.tsv"))
    r = R.run_graphdump(base + ["--colors", "file", "--gpu", "--text", "device"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--text)\n             The colour table is formatted by the host: not with --colors\n")
    r = R.run_graphdump(["rand6_k3.bin", "-s", "rand6.fa", "--colors", "file"])
    assert r.returncode == 1 and "Required argument missing: kvalue" in r.stderr.decode()
    r = R.run_graphdump(["--help"])
    assert r.returncode == 0 and b"--colors <file|sequence>" in r.stdout and b"--colors-out <file name>" in r.stdout


def test_twopaco_flag_errors(tmp_path):
    """The parse errors of `twopaco` that need no device."""
    def run(args):
        return subprocess.run([R.TWOPACO] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    fa = os.path.join(GOLDEN, "rand6.fa")
    r = run(["-f", "20", "--colors", "xml", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: Value 'xml' does not meet constraint: file|sequence for arg (--colors)\n"
    r = run(["-f", "20", "--colors-out", "x.tsv", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: This argument needs --colors <file|sequence> for arg (--colors-out)\n"
    r = run(["-f", "20", "--colors", "file", "--gpus", "2", fa])
    assert r.returncode == 1 and r.stderr.decode().startswith("\nError: The colour table is written by one GPU only") and r.stderr.decode().endswith(" for arg (--colors)\n")
    r = run(["-f", "20", "--colors"])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: Missing a value for this argument! for arg (--colors)\n"
    assert os.listdir(str(tmp_path)) == []
    r = run(["--help"])
    assert r.returncode == 0 and b"--colors <file|sequence>" in r.stdout


# ------------------------------------------------------------------------------------------------ 4. word boundaries of presence
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
def test_presence_at_the_word_boundaries(boundary_streams, c):
    fa, stream = boundary_streams[c]
    args = [stream, "-k", str(R.BOUNDARY_K), "-s", fa]
    gfa1 = R.run_graphdump(args + ["-f", "gfa1"], cwd=os.path.dirname(fa))
    assert gfa1.returncode == 0 and gfa1.stderr == b""
    want, t = R.tsv(gfa1.stdout, "sequence", R.BOUNDARY_K, [fa])
    assert t["colors"] == c and len(t["name"]) > 0
    p = t["presence"]
    assert p[:, 32 * ((c - 1) // 32):].any(), "no row has a bit in the last word"
    assert p.all(axis=1).any(), "no row lies in all %d colours" % c
    if c > 8:
        assert (t["name"] >= R.FRESH).any() and ((t["forward"] > 0) & (t["forward"] < t["occurrences"])).any()
    r = R.run_graphdump(args + ["--colors", "sequence"], cwd=os.path.dirname(fa))
    assert r.returncode == 0 and r.stderr == b""
    assert r.stdout == want
    # the hex rendering, by hand: ceil(C / 4) digits, the last colour's bit in the last digit
    full = [line.split("\t")[5] for line in r.stdout.decode().split("\n") if line and line[0] != "#" and int(line.split("\t")[4]) == c]
    digits = (c + 3) // 4
    assert full and all(h == "f" * (c // 4) + ("", "1", "3", "7")[c % 4] and len(h) == digits for h in full)
    want_file, _ = R.tsv(gfa1.stdout, "file", R.BOUNDARY_K, [fa])
    r = R.run_graphdump(args + ["--colors", "file"], cwd=os.path.dirname(fa))
    assert r.returncode == 0 and r.stdout == want_file
