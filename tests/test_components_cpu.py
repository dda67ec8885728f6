"""CPU: the component table of the serial `graphdump --components` against its definition, restated in components_reference.py over
the serial gfa1 text (itself pinned to the real reference's sha256 by tests/golden/graphdump.json): byte for byte on every golden
vector whose gfa1 succeeds, in both colour modes, the table and the members file; on the generated inputs (islands: a chain family
of 20000 links, a reversed one, two families joined by one late bridge, small components, single segments; b78; short); the text
checked on its own; the table beside the other tables; the walk's errors and the flags' errors."""
import os
import subprocess

import pytest

import components_reference as R
from helpers import GOLDEN, golden_cases


@pytest.fixture(scope="module", autouse=True)
def built():
    assert os.path.exists(R.GRAPHDUMP) and os.path.exists(R.TWOPACO), "run build() first"


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    return R.generated_inputs(str(tmp_path_factory.mktemp("components")))


def serial(args, by, tmp_path, cwd=GOLDEN):
    """(table from stdout, members file) of the serial graphdump."""
    members = str(tmp_path / "members.tsv")
    r = R.run_graphdump(list(args) + ["--components", by, "--components-members", members], cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    return r.stdout, open(members, "rb").read()


# ------------------------------------------------------------------------------------------------ 1. golden vectors
@pytest.mark.parametrize("by", ["file", "sequence"])
@pytest.mark.parametrize("v", R.GOOD_VECTORS, ids=[R.vector_id(v) for v in R.GOOD_VECTORS])
def test_serial_components_equal_the_oracle(v, by, tmp_path):
    want = R.golden_components(v, by)
    tsv, members = serial(R.components_args(v), by, tmp_path)
    assert tsv == want.tsv(), R.vector_id(v)
    assert members == want.members(), R.vector_id(v)
    assert R.check_partition(tsv, members, R.golden_gfa1(v)) == want.count()


# ------------------------------------------------------------------------------------------------ 2. the generated inputs
@pytest.mark.parametrize("by", ["file", "sequence"])
@pytest.mark.parametrize("name", ["islands", "b78", "short"])
def test_generated_components_equal_the_oracle(generated, name, by, tmp_path):
    fa, stream, gfa1, k = generated[name]
    want = R.Components(gfa1, by, k=k)
    tsv, members = serial([stream, "-k", str(k), "-s", fa], by, tmp_path, cwd=os.path.dirname(fa))
    assert tsv == want.tsv() and members == want.members()
    assert R.check_partition(tsv, members, gfa1) == want.count()


def test_the_inputs_exercise_the_union_find(generated):
    """Counted on the oracle alone, so that the tests above and the device tests cannot go blind."""
    w = R.Components(generated["islands"][2], "sequence")
    R.check_islands(w)
    assert (w.rows, w.n_links, w.count(), w.largest()) == (22495, 29831, 117, 15748)
    assert int(w.segments.sum()) == w.rows and int(w.links.sum()) == w.n_links
    assert len(R.GOOD_VECTORS) == 38


def test_known_facts(generated, tmp_path):
    # short: records without any link -- as many components as segments
    fa, stream, gfa1, k = generated["short"]
    w = R.Components(gfa1, "file", k=k)
    assert w.count() == w.rows == 2 and w.n_links == 0 and w.links.tolist() == [0, 0] and w.segments.tolist() == [1, 1]
    tsv, _ = serial([stream, "-k", str(k), "-s", fa], "file", tmp_path, cwd=os.path.dirname(fa))
    lines = tsv.decode().split("\n")
    assert lines[0] == "#twopaco-components\t1\tby=file\tk=11\tcolors=1\tsegments=2\tlinks=0\tcomponents=2"
    assert lines[2] == "#size\t0\t2\t2" and len(lines) == 6
    # rand6_k3: 4^3 k-mers, everything runs into everything -- one dense component dominates
    w = R.golden_components(R.vector_of("rand6_k3"))
    big = int(w.segments.argmax())
    assert w.segments[big] * 10 >= w.rows * 9 and w.links[big] > 2 * w.segments[big]
    # tr_k25_L28 (tracts.fa: a poly-A tract): the segment that is its own neighbour lies in a component whose links count the loop once
    case = [c for c in golden_cases() if c["name"] == "tr_k25_L28"][0]
    v = R.case_vector(case)
    w = R.Components(R.golden_gfa1(v), "file", k=case["k"])
    loops = [a for a, b in w.pairs if a == b]
    assert loops and len(set(loops)) == len(loops)
    for loop in loops:
        p = int(w.component[loop])
        inside = [(a, b) for a, b in w.pairs if w.component[a] == p]
        assert w.links[p] == len(inside) and inside.count((loop, loop)) == 1
    tsv, members = serial(R.components_args(v), "file", tmp_path)
    assert tsv == w.tsv() and members == w.members()


# ------------------------------------------------------------------------------------------------ 3. where the table goes
def test_components_out_and_stdout(tmp_path):
    v = R.vector_of("c2_k29")
    want = R.golden_components(v)
    out, members = str(tmp_path / "components.tsv"), str(tmp_path / "m.tsv")
    r = R.run_graphdump(R.components_args(v) + ["--components", "file", "--components-out", out, "--components-members", members])
    assert r.returncode == 0 and r.stdout == b"" and r.stderr == b""
    assert open(out, "rb").read() == want.tsv() and open(members, "rb").read() == want.members()
    r = R.run_graphdump(R.components_args(v) + ["--components", "file"])
    assert r.returncode == 0 and r.stdout == want.tsv() and r.stderr == b""


@pytest.mark.parametrize("by", ["file", "sequence"])
def test_beside_the_other_tables(by, tmp_path):
    """One walk for all: every other table is what it is alone, the component table comes last."""
    v = R.vector_of("c2_k29")
    base = R.components_args(v)
    want = R.golden_components(v, by).tsv()
    alone = {flag: R.run_graphdump(base + [flag, by]).stdout for flag in ("--colors", "--bubbles", "--distances")}
    for flag in ("--colors", "--bubbles", "--distances"):
        r = R.run_graphdump(base + [flag, by, "--components", by])
        assert r.returncode == 0 and r.stderr == b"" and r.stdout == alone[flag] + want, flag
    out = str(tmp_path / "c.tsv")
    r = R.run_graphdump(base + ["--components", by, "--components-out", out, "--distances", by, "--bubbles", by])
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == alone["--bubbles"] + alone["--distances"] and open(out, "rb").read() == want
    other = "sequence" if by == "file" else "file"
    for flag, noun in (("--colors", "colour"), ("--bubbles", "bubble"), ("--distances", "distance")):
        r = R.run_graphdump(base + [flag, other, "--components", by])
        assert r.returncode == 1 and r.stdout == b""
        assert r.stderr.decode().startswith("PARSE ERROR: (--components)\n             The component table and the %s table share one set of colours: %s %s does not go with --components %s\n"
                                            % (noun, flag, other, by))


# ------------------------------------------------------------------------------------------------ 4. failing walks
@pytest.mark.parametrize("case", ["edge_k5", "edge_k3"])
def test_a_failing_walk_gives_its_message_and_no_output(case, tmp_path):
    v = R.vector_of(case)
    assert v["rc"] == 1
    gfa1 = R.run_graphdump(v["args"])
    assert gfa1.returncode == 1 and gfa1.stderr.decode() == v["stderr"]
    out, members = str(tmp_path / "components.tsv"), str(tmp_path / "members.tsv")
    r = R.run_graphdump(R.components_args(v) + ["--components", "file"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr == gfa1.stderr, case
    r = R.run_graphdump(R.components_args(v) + ["--components", "sequence", "--components-out", out, "--components-members", members])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr == gfa1.stderr and not os.path.exists(out) and not os.path.exists(members), case


# ------------------------------------------------------------------------------------------------ 5. flag errors
def test_graphdump_flag_errors():
    base = ["rand6_k3.bin", "-k", "3", "-s", "rand6.fa"]
    r = R.run_graphdump(["rand6_k3.bin", "-k", "3", "--components", "file"])
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode() == "error: Required argument missing\n for arg Argument: seqfilename\n"   # as gfa1 without -s
    for args in (base + ["--components", "file", "-f", "gfa1"], base + ["-f", "gfa1", "--components", "file"]):
        r = R.run_graphdump(args)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--components)\n             Mutually exclusive argument already set!\n")
    for args in (base + ["--components", "file", "--links"], base + ["--links", "--components", "file"]):
        r = R.run_graphdump(args)
        assert r.returncode == 1 and r.stdout == b""
        assert r.stderr.decode().startswith("PARSE ERROR: (--components)\n             The component table and the link table are written one at a time: not with --links\n")
    r = R.run_graphdump(base + ["--compact", "--components", "sequence"])
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode().startswith("PARSE ERROR: (--components)\n             The component table and the compact text are written one at a time: not with --compact\n")
    for text in ("host", "device"):
        r = R.run_graphdump(base + ["--components", "file", "--gpu", "--text", text])
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--text)\n             The component table is formatted by the host: not with --components\n")
    for flag in ("--components-out", "--components-members"):
        r = R.run_graphdump(base + [flag, "x.tsv"])
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (%s)\n             This argument needs --components <file|sequence>\n" % flag)
        assert not os.path.exists(os.path.join(GOLDEN, "x.tsv"))
    r = R.run_graphdump(base + ["--components", "file", "--components-members", ""])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--components-members)\n             The component members need a file name\n")
    r = R.run_graphdump(base + ["--components", "genome"])
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode().startswith("PARSE ERROR: Argument: (--components)\n             Value 'genome' does not meet constraint: file|sequence\n")
    r = R.run_graphdump(base + ["--components"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--components)\n             Missing a value for this argument!\n")
    r = R.run_graphdump(["--help"])
    assert r.returncode == 0 and b"--components-out <file name>" in r.stdout and b"   --components <file|sequence>\n" in r.stdout and b"--components-members <file name>" in r.stdout


def test_twopaco_flag_errors(tmp_path):
    """The parse errors of `twopaco` that need no device."""
    def run(args):
        return subprocess.run([R.TWOPACO] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    fa = os.path.join(GOLDEN, "rand6.fa")
    for flag in ("--components-out", "--components-members"):
        r = run(["-f", "20", flag, "x.tsv", fa])
        assert r.returncode == 1 and r.stderr.decode() == "\nError: This argument needs --components <file|sequence> for arg (%s)\n" % flag
    r = run(["-f", "20", "--components", "file", "--gpus", "2", fa])
    assert r.returncode == 1
    assert r.stderr.decode() == "\nError: The component table is written by one GPU only (every rank holds its own piece of the junction stream): not with --gpus above 1 for arg (--components)\n"
    for flag, noun in (("--colors", "colour"), ("--bubbles", "bubble"), ("--distances", "distance")):
        for theirs, ours in (("file", "sequence"), ("sequence", "file")):
            r = run(["-f", "20", flag, theirs, "--components", ours, fa])
            assert r.returncode == 1
            assert r.stderr.decode() == "\nError: The component table and the %s table share one set of colours: %s %s does not go with --components %s for arg (--components)\n" % (
                noun, flag, theirs, ours)
    r = run(["-f", "20", "--components", "genome", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: Value 'genome' does not meet constraint: file|sequence for arg (--components)\n"
    assert os.listdir(str(tmp_path)) == []
    r = run(["--help"])
    assert r.returncode == 0 and b"[--components <file|sequence>] [--components-out <file name>] [--components-members <file name>]" in r.stdout
