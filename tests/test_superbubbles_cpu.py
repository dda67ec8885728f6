"""CPU: the superbubble table of the serial `graphdump --superbubbles` against the set definition, stated in
superbubbles_reference.py over the serial gfa1 text (itself pinned to the real reference's sha256 by tests/golden/graphdump.json):
byte for byte on every golden vector whose gfa1 succeeds, in both colour modes, the table and the members file; on the generated
input (two substitutions closer than k, three and four alleles, a nested pair, a deletion beside a substitution, an inverted repeat,
a dead end, a ring, a cluster that fills the bound exactly, a hub, a reversed record, a run of N) at max_inside 62, 8 and 2; the
cross-check against `--bubbles`; the text checked on its own; the table beside the other tables; the walk's errors and the flags'
errors."""
import os
import subprocess

import pytest

import superbubbles_reference as R
from helpers import GOLDEN


@pytest.fixture(scope="module", autouse=True)
def built():
    assert os.path.exists(R.GRAPHDUMP) and os.path.exists(R.TWOPACO), "run build() first"


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """name -> (fasta, stream, gfa1 text, k) of the generated input without (s11) and with (s81) the hub, and of the link-free records
    (made for k = 11)."""
    d = tmp_path_factory.mktemp("superbubbles")
    got = {}
    for name, n in (("s11", R.SB_RECORDS), ("s81", R.SB_RECORDS + R.SB_HUB), ("short", 0)):
        fa = str(d / (name + ".fa"))
        if name == "short":
            R.B.few_events_fasta(fa, only_short=True)
        else:
            R.superbubble_fasta(fa, n)
        k = 11 if name == "short" else R.SB_K
        stream = R.oracle_stream(fa, str(d / (name + ".bin")), k, R.SB_L, R.SB_Q, R.SB_SEED)
        gfa1 = R.run_graphdump([stream, "-k", str(k), "-s", fa, "-f", "gfa1"], cwd=str(d))
        assert gfa1.returncode == 0 and gfa1.stderr == b""
        got[name] = (fa, stream, gfa1.stdout, k)
    return got


def serial(args, by, tmp_path, cwd=GOLDEN, more=()):
    """(table from stdout, members file) of the serial graphdump."""
    members = str(tmp_path / "members.tsv")
    r = R.run_graphdump(list(args) + ["--superbubbles", by, "--superbubbles-members", members] + list(more), cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    return r.stdout, open(members, "rb").read()


# ------------------------------------------------------------------------------------------------ 1. golden vectors
@pytest.mark.parametrize("by", ["file", "sequence"])
@pytest.mark.parametrize("v", R.GOOD_VECTORS, ids=[R.vector_id(v) for v in R.GOOD_VECTORS])
def test_serial_superbubbles_equal_the_oracle(v, by, tmp_path):
    want = R.golden_superbubbles(v, by)
    tsv, members = serial(R.superbubbles_args(v), by, tmp_path)
    assert tsv == want.tsv(), R.vector_id(v)
    assert members == want.members_tsv(), R.vector_id(v)
    assert R.check_text(tsv, members, R.golden_gfa1(v), R.k_of(v), overlaps=v["case"] != "rand6_k9_a3") == want.count()
    mine, theirs = R.simple_rows(want)
    assert mine == theirs


def test_the_golden_vectors_are_all_there():
    assert len(R.GOOD_VECTORS) == 38


# ------------------------------------------------------------------------------------------------ 2. the generated input
@pytest.mark.parametrize("max_inside", [62, 8, 2])
@pytest.mark.parametrize("by", ["file", "sequence"])
@pytest.mark.parametrize("name", ["s11", "s81", "short"])
def test_generated_superbubbles_equal_the_oracle(generated, name, by, max_inside, tmp_path):
    fa, stream, gfa1, k = generated[name]
    want = R.Superbubbles(gfa1, k, by, max_inside=max_inside)
    tsv, members = serial([stream, "-k", str(k), "-s", fa], by, tmp_path, cwd=os.path.dirname(fa), more=["--superbubbles-max", str(max_inside)])
    assert tsv == want.tsv() and members == want.members_tsv()
    assert R.check_text(tsv, members, gfa1, k) == want.count()
    if max_inside == 62:   # the default bound is 62
        assert serial([stream, "-k", str(k), "-s", fa], by, tmp_path, cwd=os.path.dirname(fa)) == (tsv, members)
    if name == "short":
        assert want.count() == 0 and want.links == 0 and tsv.decode().split("\n")[0].endswith("links=0\tmax_inside=%d\tsuperbubbles=0" % max_inside)


def test_the_input_holds_every_kind(generated):
    """Counted on the oracle alone, so that the tests above and the device tests cannot go blind."""
    gfa1 = generated["s81"][2]
    full, at8, at2 = (R.Superbubbles(gfa1, R.SB_K, "sequence", max_inside=m) for m in (62, 8, 2))
    unmirrored = R.check_kinds(full, at8, at2)
    assert (full.count(), at8.count(), at2.count(), unmirrored) == (10, 9, 4, 0)
    # the cluster fills the bound exactly: 11 substitutions, 2 sides per site and 4 per pair of neighbours, 2^11 paths
    big = [r for r in full.rows if r["inside"] == 62]
    assert len(big) == 1 and big[0]["paths"] == 2048 and big[0]["n_colors"] == 8
    assert R.Superbubbles(gfa1, R.SB_K, max_inside=61).count() == 9
    # the insertion GATTA and the nested insertion of 60 letters show as min_edges != max_edges
    assert sorted(int(b - a) for a, b in zip(full.min_edges, full.max_edges) if a != b) == [3, 5, 60]
    # the cross-check against the simple bubbles: the ring is a simple bubble and no superbubble
    mine, theirs = R.simple_rows(full)
    assert mine == theirs and len(mine) == 4 and full.b.bubbles() == 5


def test_the_bubble_table_agrees(generated, tmp_path):
    """On the two programs' texts alone: the rows with inside == 2 and arcs == 4 whose members both follow the entrance are the rows of
    `--bubbles` without an arc from sink to source, in the same order (superbubbles_reference.simple_rows says why the members are
    asked as well, and test_serial_superbubbles_equal_the_oracle holds the same on every golden vector)."""
    fa, stream, gfa1, _ = generated["s81"]
    base = [stream, "-k", str(R.SB_K), "-s", fa]
    tsv, members = serial(base, "file", tmp_path, cwd=os.path.dirname(fa))
    inside = {}
    for line in members.decode().split("\n")[1:-1]:
        i, name, strand = line.split("\t")
        inside.setdefault(int(i), []).append((name, strand))
    bubbles = R.run_graphdump(base + ["--bubbles", "file"], cwd=os.path.dirname(fa))
    assert bubbles.returncode == 0
    arcs = set()
    for line in gfa1.decode().split("\n"):
        f = line.split("\t")
        if f[0] == "L":
            arcs.add((f[1], f[2], f[3], f[4]))
            arcs.add((f[3], "+-"[f[4] == "+"], f[1], "+-"[f[2] == "+"]))
    rows = [line.split("\t") for line in tsv.decode().split("\n") if line and line[0] != "#"]
    mine = [tuple(f[:4]) for i, f in enumerate(rows) if (f[4], f[5]) == ("2", "4") and all((f[0], f[1], name, strand) in arcs for name, strand in inside[i])]
    theirs = [(f[0], f[1], f[6], f[7]) for f in (line.split("\t") for line in bubbles.stdout.decode().split("\n") if line and line[0] != "#")]
    closed = [row for row in theirs if (row[2], row[3], row[0], row[1]) in arcs]
    assert len(closed) == 1 and mine == [row for row in theirs if row not in closed] and len(mine) == 4


# ------------------------------------------------------------------------------------------------ 3. where the table goes
def test_superbubbles_out_and_stdout(tmp_path):
    v = R.vector_of("c2_k29")
    want = R.golden_superbubbles(v)
    out, members = str(tmp_path / "superbubbles.tsv"), str(tmp_path / "m.tsv")
    r = R.run_graphdump(R.superbubbles_args(v) + ["--superbubbles", "file", "--superbubbles-out", out, "--superbubbles-members", members])
    assert r.returncode == 0 and r.stdout == b"" and r.stderr == b""
    assert open(out, "rb").read() == want.tsv() and open(members, "rb").read() == want.members_tsv()
    r = R.run_graphdump(R.superbubbles_args(v) + ["--superbubbles", "file"])
    assert r.returncode == 0 and r.stdout == want.tsv() and r.stderr == b""


@pytest.mark.parametrize("by", ["file", "sequence"])
def test_beside_the_other_tables(by, tmp_path):
    """One walk for all: every other table is what it is alone, the superbubble table comes last."""
    v = R.vector_of("c2_k29")
    base = R.superbubbles_args(v)
    want = R.golden_superbubbles(v, by).tsv()
    flags = ("--colors", "--bubbles", "--distances", "--components")
    alone = {flag: R.run_graphdump(base + [flag, by]).stdout for flag in flags}
    for flag in flags:
        r = R.run_graphdump(base + [flag, by, "--superbubbles", by])
        assert r.returncode == 0 and r.stderr == b"" and r.stdout == alone[flag] + want, flag
    out = str(tmp_path / "s.tsv")
    r = R.run_graphdump(base + ["--superbubbles", by, "--superbubbles-out", out, "--components", by, "--distances", by, "--bubbles", by])
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == alone["--bubbles"] + alone["--distances"] + alone["--components"] and open(out, "rb").read() == want
    other = "sequence" if by == "file" else "file"
    for flag, noun in (("--colors", "colour"), ("--bubbles", "bubble"), ("--distances", "distance"), ("--components", "component")):
        r = R.run_graphdump(base + [flag, other, "--superbubbles", by])
        assert r.returncode == 1 and r.stdout == b""
        assert r.stderr.decode().startswith("PARSE ERROR: (--superbubbles)\n             The superbubble table and the %s table share one set of colours: %s %s does not go with --superbubbles %s\n"
                                            % (noun, flag, other, by))


# ------------------------------------------------------------------------------------------------ 4. failing walks
@pytest.mark.parametrize("case", ["edge_k5", "edge_k3"])
def test_a_failing_walk_gives_its_message_and_no_output(case, tmp_path):
    v = R.vector_of(case)
    assert v["rc"] == 1
    gfa1 = R.run_graphdump(v["args"])
    assert gfa1.returncode == 1 and gfa1.stderr.decode() == v["stderr"]
    out, members = str(tmp_path / "superbubbles.tsv"), str(tmp_path / "members.tsv")
    r = R.run_graphdump(R.superbubbles_args(v) + ["--superbubbles", "file"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr == gfa1.stderr, case
    r = R.run_graphdump(R.superbubbles_args(v) + ["--superbubbles", "sequence", "--superbubbles-out", out, "--superbubbles-members", members])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr == gfa1.stderr and not os.path.exists(out) and not os.path.exists(members), case


# ------------------------------------------------------------------------------------------------ 5. flag errors
def test_graphdump_flag_errors():
    base = ["rand6_k3.bin", "-k", "3", "-s", "rand6.fa"]
    r = R.run_graphdump(["rand6_k3.bin", "-k", "3", "--superbubbles", "file"])
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode() == "error: Required argument missing\n for arg Argument: seqfilename\n"   # as gfa1 without -s
    for args in (base + ["--superbubbles", "file", "-f", "gfa1"], base + ["-f", "gfa1", "--superbubbles", "file"]):
        r = R.run_graphdump(args)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--superbubbles)\n             Mutually exclusive argument already set!\n")
    for args in (base + ["--superbubbles", "file", "--links"], base + ["--links", "--superbubbles", "file"]):
        r = R.run_graphdump(args)
        assert r.returncode == 1 and r.stdout == b""
        assert r.stderr.decode().startswith("PARSE ERROR: (--superbubbles)\n             The superbubble table and the link table are written one at a time: not with --links\n")
    r = R.run_graphdump(base + ["--compact", "--superbubbles", "sequence"])
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode().startswith("PARSE ERROR: (--superbubbles)\n             The superbubble table and the compact text are written one at a time: not with --compact\n")
    for text in ("host", "device"):
        r = R.run_graphdump(base + ["--superbubbles", "file", "--gpu", "--text", text])
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--text)\n             The superbubble table is formatted by the host: not with --superbubbles\n")
    for flag, value in (("--superbubbles-out", "x.tsv"), ("--superbubbles-members", "x.tsv"), ("--superbubbles-max", "8")):
        r = R.run_graphdump(base + [flag, value])
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (%s)\n             This argument needs --superbubbles <file|sequence>\n" % flag)
        assert not os.path.exists(os.path.join(GOLDEN, "x.tsv"))
    r = R.run_graphdump(base + ["--superbubbles", "file", "--superbubbles-members", ""])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--superbubbles-members)\n             The superbubble members need a file name\n")
    for bad in ("1", "63", "0", "-4", "x", "8x", ""):
        r = R.run_graphdump(base + ["--superbubbles", "file", "--superbubbles-max", bad])
        assert r.returncode == 1 and r.stdout == b""
        assert r.stderr.decode().startswith("PARSE ERROR: Argument: (--superbubbles-max)\n             Value '%s' does not meet constraint: an integer 2 .. 62\n" % bad), bad
    r = R.run_graphdump(base + ["--superbubbles", "genome"])
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode().startswith("PARSE ERROR: Argument: (--superbubbles)\n             Value 'genome' does not meet constraint: file|sequence\n")
    r = R.run_graphdump(base + ["--superbubbles"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--superbubbles)\n             Missing a value for this argument!\n")
    r = R.run_graphdump(["--help"])
    assert r.returncode == 0 and all(text in r.stdout for text in (b"--superbubbles-out <file name>", b"   --superbubbles <file|sequence>\n", b"--superbubbles-members <file name>",
                                                                   b"--superbubbles-max <integer>"))


def test_twopaco_flag_errors(tmp_path):
    """The parse errors of `twopaco` that need no device."""
    def run(args):
        return subprocess.run([R.TWOPACO] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    fa = os.path.join(GOLDEN, "rand6.fa")
    for flag, value in (("--superbubbles-out", "x.tsv"), ("--superbubbles-members", "x.tsv"), ("--superbubbles-max", "8")):
        r = run(["-f", "20", flag, value, fa])
        assert r.returncode == 1 and r.stderr.decode() == "\nError: This argument needs --superbubbles <file|sequence> for arg (%s)\n" % flag
    r = run(["-f", "20", "--superbubbles", "file", "--gpus", "2", fa])
    assert r.returncode == 1
    assert r.stderr.decode() == "\nError: The superbubble table is written by one GPU only (every rank holds its own piece of the junction stream): not with --gpus above 1 for arg (--superbubbles)\n"
    for flag, noun in (("--colors", "colour"), ("--bubbles", "bubble"), ("--distances", "distance"), ("--components", "component")):
        for theirs, ours in (("file", "sequence"), ("sequence", "file")):
            r = run(["-f", "20", flag, theirs, "--superbubbles", ours, fa])
            assert r.returncode == 1
            assert r.stderr.decode() == "\nError: The superbubble table and the %s table share one set of colours: %s %s does not go with --superbubbles %s for arg (--superbubbles)\n" % (
                noun, flag, theirs, ours)
    r = run(["-f", "20", "--superbubbles", "genome", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: Value 'genome' does not meet constraint: file|sequence for arg (--superbubbles)\n"
    for bad in ("1", "63", "x"):
        r = run(["-f", "20", "--superbubbles", "file", "--superbubbles-max", bad, fa])
        assert r.returncode == 1 and r.stderr.decode() == "\nError: Value '%s' does not meet constraint: an integer 2 .. 62 for arg (--superbubbles-max)\n" % bad
    r = run(["-f", "20", "--superbubbles", "file", "--superbubbles-members", "", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: The superbubble members need a file name for arg (--superbubbles-members)\n"
    assert os.listdir(str(tmp_path)) == []
    r = run(["--help"])
    assert r.returncode == 0 and b"[--superbubbles <file|sequence>] [--superbubbles-out <file name>] [--superbubbles-members <file name>] [--superbubbles-max <integer>]" in r.stdout
