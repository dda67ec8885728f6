"""CPU: the link table of the serial `graphdump --links` and the compact text of `graphdump -f gfa1 --compact` against their
definition, restated in links_reference.py over the serial gfa1 text (itself pinned to the real reference's sha256 by
tests/golden/graphdump.json): byte for byte on every golden vector whose gfa1 succeeds, the compact text spelled back on its own,
records with 0, 1 and 2 events, the walk's errors and the flags' errors."""
import os
import subprocess

import pytest

import links_reference as R
from helpers import GOLDEN, golden_cases


@pytest.fixture(scope="module", autouse=True)
def built():
    assert os.path.exists(R.GRAPHDUMP) and os.path.exists(R.TWOPACO), "run build() first"


def k_of(v):
    return int(v["args"][v["args"].index("-k") + 1])


# ------------------------------------------------------------------------------------------------ 1. golden vectors
@pytest.mark.parametrize("v", R.GOOD_VECTORS, ids=[R.vector_id(v) for v in R.GOOD_VECTORS])
def test_serial_links_equal_the_oracle(v):
    want = R.golden_links(v)
    r = R.run_graphdump(R.links_args(v) + ["--links"])
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert r.stdout == want.tsv(k_of(v)), R.vector_id(v)


@pytest.mark.parametrize("v", R.GOOD_VECTORS, ids=[R.vector_id(v) for v in R.GOOD_VECTORS])
def test_serial_compact_equals_the_filtered_gfa1(v):
    want = R.golden_links(v)
    r = R.run_graphdump(v["args"] + ["--compact"])
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert r.stdout == want.compact(), R.vector_id(v)
    assert len(r.stdout) < len(R.golden_gfa1(v))


@pytest.mark.parametrize("v", [v for v in R.GOOD_VECTORS if v["case"] != "rand6_k9_a3"], ids=[R.vector_id(v) for v in R.GOOD_VECTORS if v["case"] != "rand6_k9_a3"])
def test_the_compact_text_spells_its_paths_back(v):
    """On the program's output alone, with code of this test's own.  rand6_k9_a3 is left out of this one check: with its
    abundance cut of 3 one name covers different bodies, in the reference's own gfa1 as well."""
    r = R.run_graphdump(v["args"] + ["--compact"])
    assert r.returncode == 0
    sequences = []
    for i, a in enumerate(v["args"]):
        if a == "-s":
            sequences += R.read_fasta(os.path.join(GOLDEN, v["args"][i + 1]))
    paths, steps = R.spell_back(r.stdout, k_of(v), sequences)
    assert paths == r.stdout.count(b"\nP\t")
    assert steps == R.golden_links(v).occurrences


def test_the_golden_vectors_exercise_the_table():
    """Preconditions, counted by the oracle, so that the tests above cannot go blind."""
    s = R.golden_links(R.vector_of("rand6_k3"))
    assert (s.rows(), len(s.both), len(s.lines)) == (619, 432, len(s.lines)) and s.occurrences == 17855
    assert len(s.compact()) == 91134
    s = R.golden_links(R.vector_of("rand6_k9_fp"))
    assert (s.rows(), s.occurrences, len(s.compact())) == (1910, 3776, 89470)
    s = R.golden_links(R.vector_of("c2_k29"))
    assert (s.rows(), s.occurrences, len(s.compact())) == (227, 283, 16494)
    assert any(R.golden_links(v).touches_named for v in R.GOOD_VECTORS)
    assert len(R.GOOD_VECTORS) == 38


def test_the_hot_link_of_the_tracts():
    """tr_k25_L28 (tracts.fa: a poly-A tract): one self-loop link occurs 874 times in a row.  Its gfa1 is pinned by the reference's
    vector in tests/golden/graphdump_tracts.json."""
    case = [c for c in golden_cases() if c["name"] == "tr_k25_L28"][0]
    v = R.case_vector(case)
    s = R.golden_links(v)
    assert (s.rows(), s.occurrences, s.longest_run, len(s.compact())) == (1328, 29890, 874, 245243)
    assert int(s.count.max()) >= 874
    r = R.run_graphdump(R.links_args(v) + ["--links"])
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == s.tsv(case["k"])
    r = R.run_graphdump(v["args"] + ["--compact"])
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == s.compact()
    R.spell_back(r.stdout, case["k"], R.read_fasta(os.path.join(GOLDEN, case["fasta"])))


def test_links_out_writes_the_same_bytes(tmp_path):
    v = R.vector_of("rand6_k9_fp")
    out = str(tmp_path / "links.tsv")
    r = R.run_graphdump(R.links_args(v) + ["--links", "--links-out", out])
    assert r.returncode == 0 and r.stdout == b"" and r.stderr == b""
    assert open(out, "rb").read() == R.golden_links(v).tsv(k_of(v))


# ------------------------------------------------------------------------------------------------ 2. records with 0, 1 and 2 events
@pytest.fixture(scope="module")
def few_streams(tmp_path_factory):
    """The junction streams of the generated FASTA files, from the CPU restatement of the pipeline (oracle/)."""
    from oracle import oracle as O
    d = tmp_path_factory.mktemp("few")
    got = {}
    for only_short in (False, True):
        fa = R.few_events_fasta(str(d / ("few%d.fa" % only_short)), only_short)
        o = O.Oracle(R.FEW_K, R.FEW_L, R.FEW_Q, O.seed_table(R.FEW_SEED, R.FEW_Q, R.FEW_L))
        o.add_fasta(fa)
        o.enumerate()
        out = str(d / ("few%d.bin" % only_short))
        o.write_bin(out)
        o.close()
        got[only_short] = (fa, out)
    return got


def events_per_sequence(gfa1_text):
    names = [line.split("\t")[1] for line in gfa1_text.decode().split("\n") if line.startswith("S\t") and "\t*\tUR:Z:" in line]
    n = {name: 0 for name in names}
    for line in gfa1_text.decode().split("\n"):
        if line.startswith("C\t"):
            n[line.split("\t")[3]] += 1
    return [n[name] for name in names]


@pytest.mark.parametrize("only_short", [False, True])
def test_sequences_with_0_1_and_2_events(few_streams, only_short):
    fa, stream = few_streams[only_short]
    args = [stream, "-k", str(R.FEW_K), "-s", fa]
    gfa1 = R.run_graphdump(args + ["-f", "gfa1"], cwd=os.path.dirname(fa))
    assert gfa1.returncode == 0 and gfa1.stderr == b""
    per = events_per_sequence(gfa1.stdout)
    want = R.Links(gfa1.stdout)
    if only_short:
        assert set(per) == {0, 1} and want.rows() == 0 and want.occurrences == 0
    else:
        assert {0, 1, 2} <= set(per) and want.rows() >= 2
    r = R.run_graphdump(args + ["--links"], cwd=os.path.dirname(fa))
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == want.tsv(R.FEW_K)
    if only_short:
        assert r.stdout == b"#twopaco-links\t1\tk=11\tsegments=%d\tlinks=0\toccurrences=0\n" % want.segments
    r = R.run_graphdump(args + ["-f", "gfa1", "--compact"], cwd=os.path.dirname(fa))
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == want.compact()
    if only_short:
        assert {line[:1] for line in r.stdout.decode().split("\n")[1:-1]} == {"S", "P"}
    R.spell_back(r.stdout, R.FEW_K, R.read_fasta(fa))


# ------------------------------------------------------------------------------------------------ 3. failing walks
@pytest.mark.parametrize("case", ["edge_k5", "edge_k5_dbg", "edge_k7_fp_r2", "edge_k3"])
def test_a_failing_walk_gives_its_message_and_no_output(case, tmp_path):
    v = R.vector_of(case)
    assert v["rc"] == 1
    gfa1 = R.run_graphdump(v["args"])
    assert gfa1.returncode == 1 and gfa1.stderr.decode() == v["stderr"]
    out = str(tmp_path / "links.tsv")
    r = R.run_graphdump(R.links_args(v) + ["--links"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr == gfa1.stderr, case
    r = R.run_graphdump(R.links_args(v) + ["--links", "--links-out", out])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr == gfa1.stderr and not os.path.exists(out), case
    r = R.run_graphdump(v["args"] + ["--compact"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr == gfa1.stderr, case


# ------------------------------------------------------------------------------------------------ 4. flag errors
def test_graphdump_flag_errors():
    base = ["rand6_k3.bin", "-k", "3", "-s", "rand6.fa"]
    r = R.run_graphdump(["rand6_k3.bin", "-k", "3", "--links"])
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode() == "error: Required argument missing\n for arg Argument: seqfilename\n"   # as gfa1 without -s
    for args in (base + ["--links", "-f", "gfa1"], base + ["-f", "gfa1", "--links"]):
        r = R.run_graphdump(args)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--links)\n             Mutually exclusive argument already set!\n")
    for args in (base + ["--links", "--colors", "file"], base + ["--colors", "file", "--links"]):
        r = R.run_graphdump(args)
        assert r.returncode == 1 and r.stdout == b""
        assert r.stderr.decode().startswith("PARSE ERROR: (--links)\n             The link table and the colour table are written one at a time: not with --colors\n")
    for text in ("host", "device"):
        r = R.run_graphdump(base + ["--links", "--gpu", "--text", text])
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--text)\n             The link table is formatted by the host: not with --links\n")
    r = R.run_graphdump(base + ["--links-out", "x.tsv"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--links-out)\n             This argument needs --links\n")
    assert not os.path.exists(os.path.join(GOLDEN, "x.tsv"))
    for fmt in ("gfa2", "fasta", "seq", "group", "dot"):
        r = R.run_graphdump(base + ["-f", fmt, "--compact"])
        assert r.returncode == 1 and r.stdout == b""
        assert r.stderr.decode().startswith("PARSE ERROR: (--compact)\n             The compact text is gfa1 with every link once: it needs -f gfa1\n")
    for args in (base + ["--compact"], base + ["--compact", "--links"], base + ["--compact", "--colors", "file"]):
        r = R.run_graphdump(args)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--compact)\n"), args
    r = R.run_graphdump(base + ["-f", "gfa1", "--compact", "--gpu", "--text", "device"])
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode().startswith("PARSE ERROR: (--compact)\n             The compact text is formatted by the host: not with --text device\n")
    r = R.run_graphdump(["rand6_k3.bin", "-s", "rand6.fa", "--links"])
    assert r.returncode == 1 and "Required argument missing: kvalue" in r.stderr.decode()
    r = R.run_graphdump(["--help"])
    assert r.returncode == 0 and b"--links-out <file name>" in r.stdout and b"   --links\n" in r.stdout and b"   --compact\n" in r.stdout


def test_twopaco_flag_errors(tmp_path):
    """The parse errors of `twopaco` that need no device."""
    def run(args):
        return subprocess.run([R.TWOPACO] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    fa = os.path.join(GOLDEN, "rand6.fa")
    one_gpu = " is written by one GPU only (every rank holds its own piece of the junction stream): not with --gpus above 1 for arg "
    r = run(["-f", "20", "--links-out", "x.tsv", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: This argument needs --links for arg (--links-out)\n"
    r = run(["-f", "20", "--links", "--gpus", "2", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: The link table" + one_gpu + "(--links)\n"
    r = run(["-f", "20", "--colors", "file", "--gpus", "2", fa])   # the wording it follows
    assert r.returncode == 1 and r.stderr.decode() == "\nError: The colour table" + one_gpu + "(--colors)\n"
    r = run(["-f", "20", "--graph", "gfa1", "--graph-compact", "--gpus", "2", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: The compact graph" + one_gpu + "(--graph-compact)\n"
    for args in (["--graph-compact"], ["--graph", "gfa2", "--graph-compact"], ["--graph", "fasta", "--graph-compact"], ["--links", "--graph-compact"]):
        r = run(["-f", "20"] + args + [fa])
        assert r.returncode == 1 and r.stderr.decode() == "\nError: The compact graph is gfa1 with every link once: it needs --graph gfa1 for arg (--graph-compact)\n", args
    r = run(["-f", "20", "--graph", "gfa1", "--graph-compact", "--graph-text", "device", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: The compact graph is formatted by the host: not with --graph-text device for arg (--graph-compact)\n"
    r = run(["-f", "20", "--links-out"])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: Missing a value for this argument! for arg (--links-out)\n"
    assert os.listdir(str(tmp_path)) == []
    r = run(["--help"])
    assert r.returncode == 0 and b"[--links] [--links-out <file name>] [--graph-compact]" in r.stdout
