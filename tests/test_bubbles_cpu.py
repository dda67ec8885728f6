"""CPU: the bubble table of the serial `graphdump --bubbles` against its definition, restated in bubbles_reference.py over the
serial gfa1 text (itself pinned to the real reference's sha256 by tests/golden/graphdump.json): byte for byte on every golden
vector whose gfa1 succeeds, in both colour modes; on a generated input with substitutions, deletions, insertions, three-allele
sites and a hub; on records without any link; the text spelled back on its own; the walk's errors and the flags' errors."""
import os
import subprocess

import numpy as np
import pytest

import bubbles_reference as R
from helpers import GOLDEN, golden_cases


@pytest.fixture(scope="module", autouse=True)
def built():
    assert os.path.exists(R.GRAPHDUMP) and os.path.exists(R.TWOPACO), "run build() first"


def k_of(v):
    return int(v["args"][v["args"].index("-k") + 1])


# ------------------------------------------------------------------------------------------------ 1. golden vectors
@pytest.mark.parametrize("by", ["file", "sequence"])
@pytest.mark.parametrize("v", R.GOOD_VECTORS, ids=[R.vector_id(v) for v in R.GOOD_VECTORS])
def test_serial_bubbles_equal_the_oracle(v, by):
    want = R.golden_bubbles(v, by)
    r = R.run_graphdump(R.bubbles_args(v) + ["--bubbles", by])
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert r.stdout == want.tsv(k_of(v)), R.vector_id(v)


def test_the_hot_link_of_the_tracts():
    """tr_k25_L28 (tracts.fa: a poly-A tract): a segment that is its own neighbour 874 times in a row.  A self-loop gives two arcs
    (a+ -> a+ and a- -> a-), and an arm that is a self-loop is no arm."""
    case = [c for c in golden_cases() if c["name"] == "tr_k25_L28"][0]
    v = R.case_vector(case)
    want = R.golden_bubbles(v)
    loops = [u for u in range(want.sides) if u in want.out[u]]
    assert loops and all((u ^ 1) in want.out[u ^ 1] for u in loops)
    assert not set(u >> 1 for u in loops) & set((np.concatenate([want.source, want.arm_a, want.arm_b, want.sink]) >> 1).tolist())
    r = R.run_graphdump(R.bubbles_args(v) + ["--bubbles", "file"])
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == want.tsv(case["k"])


def test_bubbles_out_writes_the_same_bytes(tmp_path):
    v = R.vector_of("c2_k29")
    out = str(tmp_path / "bubbles.tsv")
    r = R.run_graphdump(R.bubbles_args(v) + ["--bubbles", "file", "--bubbles-out", out])
    assert r.returncode == 0 and r.stdout == b"" and r.stderr == b""
    assert open(out, "rb").read() == R.golden_bubbles(v).tsv(k_of(v))


# ------------------------------------------------------------------------------------------------ 2. the generated input
@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """{records: (fasta, stream, serial gfa1)} of bubbles_reference.bubble_fasta at 8 and 78 records, the stream from the CPU
    restatement of the pipeline (oracle/)."""
    d = tmp_path_factory.mktemp("bubbles")
    got = {}
    for n in (R.BUBBLE_GENOMES, R.BUBBLE_GENOMES + R.BUBBLE_HUB):
        fa = R.bubble_fasta(str(d / ("b%d.fa" % n)), n)
        stream = R.oracle_stream(fa, str(d / ("b%d.bin" % n)), R.BUBBLE_K, R.BUBBLE_L, R.BUBBLE_Q, R.BUBBLE_SEED)
        gfa1 = R.run_graphdump([stream, "-k", str(R.BUBBLE_K), "-s", fa, "-f", "gfa1"], cwd=str(d))
        assert gfa1.returncode == 0 and gfa1.stderr == b""
        got[n] = (fa, stream, gfa1.stdout)
    return got


@pytest.mark.parametrize("by", ["file", "sequence"])
@pytest.mark.parametrize("records", [8, 78])
def test_generated_bubbles_equal_the_oracle(generated, records, by):
    fa, stream, gfa1 = generated[records]
    want = R.Bubbles(gfa1, by)
    r = R.run_graphdump([stream, "-k", str(R.BUBBLE_K), "-s", fa, "--bubbles", by], cwd=os.path.dirname(fa))
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert r.stdout == want.tsv(R.BUBBLE_K)
    assert R.check_arms_overlap(r.stdout, gfa1, R.BUBBLE_K) == want.bubbles()


@pytest.mark.parametrize("only_short", [False, True])
def test_few_events(tmp_path, only_short):
    """links_reference.few_events_fasta: records with 0, 1 and 2 events; only_short: no link at all -- no arc, no bubble, every
    side a dead end."""
    fa = R.few_events_fasta(str(tmp_path / "few.fa"), only_short)
    stream = R.oracle_stream(fa, str(tmp_path / "few.bin"), 11, 20, 5, 11)
    args = [stream, "-k", "11", "-s", fa]
    gfa1 = R.run_graphdump(args + ["-f", "gfa1"], cwd=str(tmp_path))
    assert gfa1.returncode == 0 and gfa1.stderr == b""
    want = R.Bubbles(gfa1.stdout, "sequence")
    r = R.run_graphdump(args + ["--bubbles", "sequence"], cwd=str(tmp_path))
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == want.tsv(11)
    if only_short:
        assert (want.links, want.arcs, want.bubbles()) == (0, 0, 0) and want.segments > 0
        assert want.hist.tolist() == [want.sides, 0, 0, 0, 0, 0]
        lines = r.stdout.decode().split("\n")
        assert lines[0] == "#twopaco-bubbles\t1\tby=sequence\tk=11\tcolors=3\tsegments=%d\tlinks=0\tbubbles=0" % want.segments
        assert lines[4:] == ["#sides\t0\t%d" % want.sides, ""]
    else:
        assert want.links >= 2


# ------------------------------------------------------------------------------------------------ 3. preconditions
def test_the_inputs_exercise_the_definition(generated):
    """Counted on the oracle alone, so that the tests above cannot go blind."""
    small, large = (R.Bubbles(generated[n][2], "sequence") for n in (8, 78))
    for w in (small, large):
        assert w.bubbles() == 28 and w.bubbles() >= 20
        length = w.colors["length"]
        pairs = [(int(length[a >> 1]), int(length[b >> 1])) for a, b in zip(w.arm_a.tolist(), w.arm_b.tolist())]
        # a substitution: both arms 2k + 1 = 23; two substitutions five apart: 2k + 6 = 28; deletions and insertions: unequal
        assert sum(p == (23, 23) for p in pairs) == 11 and sum(p == (28, 28) for p in pairs) == 5 and sum(p[0] != p[1] for p in pairs) == 12
        assert int((w.source & 1).sum()) == 15 and int((w.source & 1 == 0).sum()) == 13     # sources reported on both strands
        assert (w.arm_a < w.arm_b).all() and (np.diff(w.source) > 0).all()
        ends = set(w.source.tolist()) | set((w.sink ^ 1).tolist())
        assert sum(1 for s in range(w.sides) if w.deg[s] >= 3 and s not in ends) >= 12  # three alleles at one place: no bubble
        assert w.arcs == 2 * w.links and int(w.hist.sum()) == w.sides
        # the colours of the two arms of a bubble between 8 genomes: every genome holds exactly one arm
        presence = w.colors["presence"]
        for a, b in zip(w.arm_a.tolist(), w.arm_b.tolist()):
            genomes = presence[a >> 1][:8].astype(int) + presence[b >> 1][:8].astype(int)
            assert (genomes <= 1).all()
    assert (small.segments, int(small.deg.max()), small.hist.tolist()) == (141, 3, [2, 196, 72, 12, 0, 0])
    assert (large.segments, int(large.deg.max()), large.hist.tolist()) == (333, 20, [142, 394, 97, 21, 8, 4])
    assert sum(1 for n in large.g.row_name if n >= R.FRESH) == 71                        # the hub's 'N'-named neighbours
    counts = {case: R.golden_bubbles(R.vector_of(case)).bubbles() for case in ("c2_k29", "c2_k35", "rand6_k27", "rand6_k25_q3", "c2_k61", "rand6_k9_a3", "rand6_k3", "example_k11")}
    assert counts == {"c2_k29": 6, "c2_k35": 6, "rand6_k27": 4, "rand6_k25_q3": 3, "c2_k61": 3, "rand6_k9_a3": 4, "rand6_k3": 0, "example_k11": 0}
    assert R.golden_bubbles(R.vector_of("rand6_k3")).hist.tolist() == [0, 34, 0, 3, 197, 76]
    assert len(R.GOOD_VECTORS) == 38


# ------------------------------------------------------------------------------------------------ 4. the text on its own
@pytest.mark.parametrize("v", [v for v in R.GOOD_VECTORS if v["case"] != "rand6_k9_a3"], ids=[R.vector_id(v) for v in R.GOOD_VECTORS if v["case"] != "rand6_k9_a3"])
def test_the_arms_overlap_their_source_and_sink(v):
    """On the program's output and the S lines alone, with code of this test's own.  rand6_k9_a3 is left out of this one check:
    with its abundance cut of 3 one name covers different bodies, in the reference's own gfa1 as well."""
    r = R.run_graphdump(R.bubbles_args(v) + ["--bubbles", "file"])
    assert r.returncode == 0
    rows = R.check_arms_overlap(r.stdout, R.golden_gfa1(v), k_of(v))
    assert rows == int(r.stdout.decode().split("\n")[0].split("bubbles=")[1])


# ------------------------------------------------------------------------------------------------ 5. failing walks
@pytest.mark.parametrize("case", ["edge_k5", "edge_k5_dbg", "edge_k7_fp_r2", "edge_k3"])
def test_a_failing_walk_gives_its_message_and_no_output(case, tmp_path):
    v = R.vector_of(case)
    assert v["rc"] == 1
    gfa1 = R.run_graphdump(v["args"])
    assert gfa1.returncode == 1 and gfa1.stderr.decode() == v["stderr"]
    out = str(tmp_path / "bubbles.tsv")
    r = R.run_graphdump(R.bubbles_args(v) + ["--bubbles", "file"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr == gfa1.stderr, case
    r = R.run_graphdump(R.bubbles_args(v) + ["--bubbles", "sequence", "--bubbles-out", out])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr == gfa1.stderr and not os.path.exists(out), case


# ------------------------------------------------------------------------------------------------ 6. flag errors
def test_graphdump_flag_errors():
    base = ["rand6_k3.bin", "-k", "3", "-s", "rand6.fa"]
    r = R.run_graphdump(["rand6_k3.bin", "-k", "3", "--bubbles", "file"])
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode() == "error: Required argument missing\n for arg Argument: seqfilename\n"   # as gfa1 without -s
    for args in (base + ["--bubbles", "file", "-f", "gfa1"], base + ["-f", "gfa1", "--bubbles", "file"]):
        r = R.run_graphdump(args)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--bubbles)\n             Mutually exclusive argument already set!\n")
    for args in (base + ["--bubbles", "file", "--colors", "file"], base + ["--colors", "sequence", "--bubbles", "file"]):
        r = R.run_graphdump(args)
        assert r.returncode == 1 and r.stdout == b""
        assert r.stderr.decode().startswith("PARSE ERROR: (--bubbles)\n             The bubble table and the colour table are written one at a time: not with --colors\n")
    for args in (base + ["--bubbles", "file", "--links"], base + ["--links", "--bubbles", "file"]):
        r = R.run_graphdump(args)
        assert r.returncode == 1 and r.stdout == b""
        assert r.stderr.decode().startswith("PARSE ERROR: (--bubbles)\n             The bubble table and the link table are written one at a time: not with --links\n")
    for args in (base + ["--bubbles", "file", "--compact"], base + ["--compact", "--bubbles", "sequence"]):
        r = R.run_graphdump(args)
        assert r.returncode == 1 and r.stdout == b""
        assert r.stderr.decode().startswith("PARSE ERROR: (--bubbles)\n             The bubble table and the compact text are written one at a time: not with --compact\n")
    for text in ("host", "device"):
        r = R.run_graphdump(base + ["--bubbles", "file", "--gpu", "--text", text])
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--text)\n             The bubble table is formatted by the host: not with --bubbles\n")
    r = R.run_graphdump(base + ["--bubbles-out", "x.tsv"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--bubbles-out)\n             This argument needs --bubbles <file|sequence>\n")
    assert not os.path.exists(os.path.join(GOLDEN, "x.tsv"))
    r = R.run_graphdump(base + ["--bubbles", "genome"])
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode().startswith("PARSE ERROR: Argument: (--bubbles)\n             Value 'genome' does not meet constraint: file|sequence\n")
    r = R.run_graphdump(base + ["--bubbles"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--bubbles)\n             Missing a value for this argument!\n")
    r = R.run_graphdump(["rand6_k3.bin", "-s", "rand6.fa", "--bubbles", "file"])
    assert r.returncode == 1 and "Required argument missing: kvalue" in r.stderr.decode()
    r = R.run_graphdump(["--help"])
    assert r.returncode == 0 and b"--bubbles-out <file name>" in r.stdout and b"   --bubbles <file|sequence>\n" in r.stdout


def test_twopaco_flag_errors(tmp_path):
    """The parse errors of `twopaco` that need no device."""
    def run(args):
        return subprocess.run([R.TWOPACO] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    fa = os.path.join(GOLDEN, "rand6.fa")
    one_gpu = " is written by one GPU only (every rank holds its own piece of the junction stream): not with --gpus above 1 for arg "
    r = run(["-f", "20", "--bubbles-out", "x.tsv", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: This argument needs --bubbles <file|sequence> for arg (--bubbles-out)\n"
    r = run(["-f", "20", "--bubbles", "file", "--gpus", "2", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: The bubble table" + one_gpu + "(--bubbles)\n"
    r = run(["-f", "20", "--colors", "file", "--gpus", "2", fa])   # the wording it follows
    assert r.returncode == 1 and r.stderr.decode() == "\nError: The colour table" + one_gpu + "(--colors)\n"
    for colors, bubbles in (("file", "sequence"), ("sequence", "file")):
        r = run(["-f", "20", "--colors", colors, "--bubbles", bubbles, fa])
        assert r.returncode == 1
        assert r.stderr.decode() == "\nError: The bubble table and the colour table share one set of colours: --colors %s does not go with --bubbles %s for arg (--bubbles)\n" % (colors, bubbles)
    r = run(["-f", "20", "--bubbles", "genome", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: Value 'genome' does not meet constraint: file|sequence for arg (--bubbles)\n"
    r = run(["-f", "20", "--bubbles-out"])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: Missing a value for this argument! for arg (--bubbles-out)\n"
    assert os.listdir(str(tmp_path)) == []
    r = run(["--help"])
    assert r.returncode == 0 and b"[--bubbles <file|sequence>] [--bubbles-out <file name>]" in r.stdout
