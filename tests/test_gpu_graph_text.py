"""GPU (-m gpu): the graph text rendered on the device (csrc/tpc_segtext.hip, tpc_segments_text_plan / _text_fetch / _text_write
of include/twopaco_hip.h) behind `graphdump --gpu --text device` and `twopaco --graph-text device`.

The host formatter (twopaco_amd/host/graphformat.h, through capi.graph_format and through the same commands with `host`) is
the byte-for-byte oracle, and the bytes the REAL reference graphdump wrote (tests/golden/graphdump.json) tie both to the
reference."""
import hashlib
import json
import os
import random
import subprocess

import numpy as np
import pytest

from graph_table import event_table, read_fasta
from helpers import GOLDEN, case_files, golden_cases, sha256_file

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ("gfa1", "gfa2", "fasta")
ALL = [v for v in json.load(open(os.path.join(GOLDEN, "graphdump.json"))) if v["case"] != "cli" and v["args"][2] in FORMATS]
VECTORS = [v for v in ALL if v["rc"] == 0]
FAILING = [v for v in ALL if v["rc"] != 0]
CASES = {c["name"]: c for c in golden_cases()}
ABI_CASES = ["tr_k25_L28", "edge_k5", "c2_k29", "rand6_k3"]
TWOPACO = os.path.join(ROOT, "twopaco_amd", "bin", "twopaco")
GRAPHDUMP = os.path.join(ROOT, "twopaco_amd", "bin", "graphdump")


@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


def graphdump(args, stats=None, stdout=subprocess.PIPE, cwd=GOLDEN):
    env = dict(os.environ)
    env.pop("TWOPACO_GRAPHDUMP_STATS", None)
    if stats:
        if os.path.exists(stats):
            os.unlink(stats)
        env["TWOPACO_GRAPHDUMP_STATS"] = stats
    return subprocess.run([GRAPHDUMP] + args, cwd=cwd, stdout=stdout, stderr=subprocess.PIPE, timeout=600, env=env)


# ------------------------------------------------------------------------------------------------ 1. the reference's bytes through graphdump
def test_vector_counts():
    assert len(VECTORS) == 95 and len(FAILING) == 20


@pytest.mark.parametrize("fmt", FORMATS)
def test_graphdump_text_device_gives_the_reference_bytes(tmp_path, fmt):
    """All 95 vectors of the real reference that exit 0 (this format's share), `graphdump --gpu --text device`: size and sha256
    of stdout equal the reference's, stderr is empty and the stats file says the text came from the device.  No vector is
    skipped: the count is asserted."""
    stats = str(tmp_path / "stats.json")
    n = 0
    for v in VECTORS:
        if v["args"][2] != fmt:
            continue
        r = graphdump(v["args"] + ["--gpu", "--text", "device"], stats=stats)
        assert r.returncode == 0 and r.stderr == b"", (v["args"], r.stderr[-400:])
        assert len(r.stdout) == v["stdout_bytes"], v["args"]
        assert hashlib.sha256(r.stdout).hexdigest() == v["stdout_sha256"], v["args"]
        s = json.load(open(stats))
        assert s["path"] == "device" and s["text"] == "device" and s["text_kernel_ms"] > 0, (v["args"], s)
        for key in ("events", "segments", "n_named", "device_ms", "kernel_ms", "load_ms", "pack_ms", "index_ms", "format_ms", "threads", "device_bytes",
                    "stream_bytes", "text_bytes", "table_bytes"):
            assert key in s, key
        n += 1
    assert n == {"gfa1": 38, "gfa2": 38, "fasta": 19}[fmt]


def test_graphdump_text_host_says_so_in_the_stats(tmp_path):
    v = [v for v in VECTORS if v["case"] == "c2_k29" and v["args"][2] == "gfa1"][0]
    stats = str(tmp_path / "stats.json")
    for extra in (["--gpu"], ["--gpu", "--text", "host"]):
        r = graphdump(v["args"] + extra, stats=stats)
        assert r.returncode == 0 and hashlib.sha256(r.stdout).hexdigest() == v["stdout_sha256"]
        s = json.load(open(stats))
        assert s["path"] == "device" and s["text"] == "host" and s["text_kernel_ms"] == 0


def test_graphdump_text_device_fails_as_the_walk_fails():
    """The 20 vectors the reference ends with exit code 1: the same stderr, the same exit code, and an empty stdout -- the table
    is complete before the first byte is printed."""
    n = 0
    for v in FAILING:
        r = graphdump(v["args"] + ["--gpu", "--text", "device"])
        assert r.returncode == v["rc"] == 1, v["args"]
        assert r.stderr.decode() == v["stderr"], v["args"]
        assert r.stdout == b"", v["args"]
        n += 1
    assert n == 20


# ------------------------------------------------------------------------------------------------ 2. + 3. through the C-ABI
def sequence_names(path):
    """The parser's header: the first word behind '>'."""
    return [(line[1:].split() or [""])[0] for line in open(path) if line.startswith(">")]


def ambiguous(seqs, rec_start):
    """(global positions, letters) of the valid letters other than A C G T N, in text order."""
    hits = [(int(rec_start[r]) + i, ch) for r, s in enumerate(seqs) for i, ch in enumerate(s) if ch not in "ACGTN"]
    return [p for p, _ in hits], "".join(ch for _, ch in hits)


def letter_counts(name, first, begin, end, seq_event_begin, seqs, k):
    """First-sight bodies: (forward with a letter outside ACGTN, reversed with one, with an 'N')."""
    forward = reverse = n_bodies = 0
    for s in range(len(seqs)):
        for e in range(int(seq_event_begin[s]), int(seq_event_begin[s + 1])):
            if not first[e]:
                continue
            body = seqs[s][int(begin[e]):int(end[e]) + k]
            other = any(ch not in "ACGTN" for ch in body)
            forward += other and name[e] > 0
            reverse += other and name[e] <= 0
            n_bodies += "N" in body
    return int(forward), int(reverse), int(n_bodies)


def mended_fasta(path, k, out_path):
    """The records of a FASTA file that the enumerator dispatches (k letters or more), as they stand in the file."""
    records, keep = [], []
    for line in open(path):
        if line.startswith(">"):
            records.append([line])
        elif records:
            records[-1].append(line)
    for rec in records:
        if len("".join("".join(x.split()) for x in rec[1:])) >= k:
            keep.append("".join(rec))
    assert 0 < len(keep) < len(records)
    with open(out_path, "w") as f:
        f.write("".join(keep))
    return out_path


def run_to_stream(capi, ctx, case, text):
    ctx.set_params(case["k"], case["L"], case["q"], capi.seed_table(case["q"], case["L"], seed=case["seed"]))
    ctx.seq_upload(text)
    for st in case["rounds"]:
        ctx.filter_reset()
        ctx.pass1_insert(st["low"], st["high"])
        ctx.pass1_query(st["low"], st["high"])
        ctx.pass2_filter()
    ctx.junctions_finalize()
    ctx.emit()
    return ctx.emit_stream(text.rec_start, text.rec_length)[0]


class Built:
    """A context with the segment table of a case, and what the two formatters need beside it."""

    def __init__(self, capi, case_name, tmp_path):
        case = CASES[case_name]
        self.capi, self.k = capi, case["k"]
        self.files = case_files(case, tmp_path)
        self.ctx = capi.Context(0)
        if case_name == "edge_k5":
            # edge.fa's records shorter than k are never dispatched, the stream skips their sequence ids and the walk -- the
            # reference's too -- refuses it: such a table has no text (test_plan_is_refused_...).  The text of this case is that
            # of the records the enumerator dispatches, enumerated here with the case's parameters; they keep what the case is
            # in this list for (asserted below): IUPAC letters in a forward and in a reversed body, and bodies with 'N'.
            self.files = [mended_fasta(self.files[0], self.k, str(tmp_path / "edge_dispatched.fa"))]
            text = capi.PackedText.from_fasta(self.files)
            self.seqs = read_fasta(self.files[0])
            stream = run_to_stream(capi, self.ctx, case, text)
            positions, self.letters = ambiguous(self.seqs, text.rec_start)
            self.ctx.segments_build(None, self.k, text.rec_start, text.rec_length, positions)
            name, first, begin, end, seq = event_table(stream, self.seqs, self.k)
            forward, reverse, n_bodies = letter_counts(name, first, begin, end, seq, self.seqs, self.k)
            print("edge_k5, dispatched records: forward", forward, "reversed", reverse, "N bodies", n_bodies)
            assert forward >= 1 and reverse >= 1 and n_bodies >= 1
        else:
            text = capi.PackedText.from_fasta(self.files)
            self.seqs = [s for f in self.files for s in read_fasta(f)]
            positions, self.letters = ambiguous(self.seqs, text.rec_start)
            self.ctx.seq_upload(text)
            self.ctx.segments_build(open(os.path.join(GOLDEN, case["bin"]), "rb").read(), self.k, text.rec_start, text.rec_length, positions)
        assert self.ctx.segments_error() is None
        self.text = text
        self.names = [n for f in self.files for n in sequence_names(f)]
        assert len(self.names) == len(self.seqs)

    def printed_names(self, fmt, prefix):
        return ["s0_" + n for n in self.names] if prefix or fmt == "fasta" else self.names

    def host_text(self, fmt, prefix, tmp_path):
        """capi.graph_format fed with the table fetched from this context, without the header lines (an empty table gives them)."""
        name, first = self.ctx.segments_fetch()
        begin, end = self.ctx.segments_fetch_events()
        seq = self.ctx.segments_fetch_sequences(0, len(self.seqs) + 1)
        out = str(tmp_path / "host.txt")
        self.capi.graph_format(self.files, self.k, fmt, out, name, first, begin, end, seq, prefix=prefix, threads=3)
        whole = open(out, "rb").read()
        none = np.zeros(0)
        self.capi.graph_format(self.files, self.k, fmt, out, none, none, none, none, np.zeros(len(self.seqs) + 1), prefix=prefix, threads=1)
        head = open(out, "rb").read()
        os.unlink(out)
        assert whole.startswith(head)
        return whole[len(head):]

    def close(self):
        self.ctx.close()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("case_name", ABI_CASES)
def test_text_through_the_abi_equals_the_host_formatter(capi, tmp_path, case_name, fmt):
    """segments_text_plan + one whole segments_text_fetch == the host formatter on the table fetched from the same context;
    total_bytes is the length; with and without the name prefix."""
    b = Built(capi, case_name, tmp_path)
    try:
        for prefix in (False, True):
            want = b.host_text(fmt, prefix, tmp_path)
            assert len(want) > 0
            total = b.ctx.segments_text_plan(fmt, b.printed_names(fmt, prefix), b.letters)
            print(case_name, fmt, prefix, "bytes", total)
            assert total == len(want)
            got = b.ctx.segments_text_fetch(0, total)
            assert got == want
            assert b.ctx.kernel_ms("segtext") > 0
        if case_name == "tr_k25_L28":
            name, first = b.ctx.segments_fetch()
            begin, end = b.ctx.segments_fetch_events()
            longest = int((end.astype(np.int64) + b.k - begin)[first].max())
            assert longest > 160   # several lines of 80 letters in the fasta bodies
    finally:
        b.close()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("case_name", ABI_CASES)
def test_windows_concatenate_to_the_whole_text(capi, tmp_path, case_name, fmt):
    """Windows of 1, 7, 4093 and 65536 bytes and a seeded random cut list: every window may begin or end inside a number, a
    body or a path line; a range that passes the end is refused with a text and the context stays usable."""
    b = Built(capi, case_name, tmp_path)
    try:
        want = b.host_text(fmt, False, tmp_path)
        total = b.ctx.segments_text_plan(fmt, b.printed_names(fmt, False), b.letters)
        assert total == len(want)
        for window in (1, 7, 4093, 65536):
            parts = [b.ctx.segments_text_fetch(at, min(window, total - at)) for at in range(0, total, window)]
            assert b"".join(parts) == want, window
        rnd = random.Random(20240917)
        cuts = sorted({0, total} | {rnd.randrange(total + 1) for _ in range(64)})
        parts = [b.ctx.segments_text_fetch(a, z - a) for a, z in zip(cuts[:-1], cuts[1:])]
        assert b"".join(parts) == want
        assert b.ctx.segments_text_fetch(total, 0) == b""
        for at, n in ((total, 1), (0, total + 1), (total + 1, 0), ((1 << 64) - 1, 2), (total - 1, 2)):
            with pytest.raises(RuntimeError, match="bad byte range"):
                b.ctx.segments_text_fetch(at, n)
        assert b.ctx.segments_text_fetch(0, min(total, 100)) == want[:100]
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ 4. the letters are in the fixtures
@pytest.mark.parametrize("case_name,want", [("edge_k5", (2, 1, 5)), ("edge_k7_fp_r2", (3, 0, 5))])
def test_the_edge_vectors_hold_the_letters(case_name, want):
    """From tests/graph_table.py alone: first-sight bodies of the edge vectors with a letter outside ACGTN read forward, read
    reversed, and with 'N' -- the counts found when this test was written.  A fixture change that loses them fails here."""
    case = CASES[case_name]
    seqs = read_fasta(os.path.join(GOLDEN, case["fasta"]))
    name, first, begin, end, seq = event_table(open(os.path.join(GOLDEN, case["bin"]), "rb").read(), seqs, case["k"])
    assert letter_counts(name, first, begin, end, seq, seqs, case["k"]) == want


def test_the_edge_vectors_together_hold_every_kind():
    got = [0, 0, 0]
    for case_name in ("edge_k3", "edge_k5", "edge_k5_dbg", "edge_k7_fp_r2"):
        case = CASES[case_name]
        seqs = read_fasta(os.path.join(GOLDEN, case["fasta"]))
        table = event_table(open(os.path.join(GOLDEN, case["bin"]), "rb").read(), seqs, case["k"])
        got = [a + b for a, b in zip(got, letter_counts(*table, seqs, case["k"]))]
    assert got[0] > 0 and got[1] > 0 and got[2] > 0


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_plan_is_refused_without_a_good_table_and_the_context_stays_usable(capi, tmp_path):
    """Before a build; after a build whose error kind is not OK (edge_k5's own stream: "The input is corrupted"); with a format
    outside 1..3; a fetch and a write without a plan.  Each is an error text, and the same context then renders a good table."""
    bad, good = CASES["edge_k5"], CASES["c2_k29"]
    ctx = capi.Context(0)
    with pytest.raises(RuntimeError, match="build the segment table first"):
        ctx.segments_text_plan("gfa1", ["a"])
    fasta = os.path.join(GOLDEN, bad["fasta"])
    text = capi.PackedText.from_fasta([fasta])
    seqs = read_fasta(fasta)
    positions, letters = ambiguous(seqs, text.rec_start)
    ctx.seq_upload(text)
    ctx.segments_build(open(os.path.join(GOLDEN, bad["bin"]), "rb").read(), bad["k"], text.rec_start, text.rec_length, positions)
    assert ctx.segments_error() == (3, "The input is corrupted")
    with pytest.raises(RuntimeError, match="walk's error"):
        ctx.segments_text_plan("gfa1", sequence_names(fasta), letters)
    with pytest.raises(RuntimeError, match="text_plan first"):
        ctx.segments_text_fetch(0, 1)
    with open(str(tmp_path / "never.txt"), "wb") as f:
        with pytest.raises(RuntimeError, match="text_plan first"):
            ctx.segments_text_write(f.fileno())
    assert os.path.getsize(str(tmp_path / "never.txt")) == 0

    fasta = os.path.join(GOLDEN, good["fasta"])
    text = capi.PackedText.from_fasta([fasta])
    ctx.seq_upload(text)
    ctx.segments_build(open(os.path.join(GOLDEN, good["bin"]), "rb").read(), good["k"], text.rec_start, text.rec_length)
    assert ctx.segments_error() is None
    names = sequence_names(fasta)
    for fmt in (0, 4, -1, 7):
        with pytest.raises(RuntimeError, match="format"):
            ctx.segments_text_plan(fmt, names)
    with pytest.raises(RuntimeError, match="text_plan first"):   # a refused plan leaves no plan behind
        ctx.segments_text_fetch(0, 1)
    v = [v for v in VECTORS if v["case"] == "c2_k29" and v["args"][2] == "gfa2" and "--prefix" not in v["args"]][0]
    total = ctx.segments_text_plan(2, names)
    head = b"H\tVN:Z:2.0\n"
    got = head + ctx.segments_text_fetch(0, total)
    assert len(got) == v["stdout_bytes"] and hashlib.sha256(got).hexdigest() == v["stdout_sha256"]
    # the text that was uploaded is the one the table indexes: another upload drops the plan's ground
    ctx.seq_upload(capi.PackedText.from_fasta([os.path.join(GOLDEN, "example.fa")]))
    with pytest.raises(RuntimeError):
        ctx.segments_text_fetch(0, 1)
    ctx.close()


def test_text_write_to_a_file_and_small_windows(capi, tmp_path):
    """segments_text_write at an offset of a regular file, with the library's window and with windows of one tile (many of
    them in flight over the two buffers): the file holds the text behind the offset."""
    b = Built(capi, "rand6_k3", tmp_path)
    try:
        want = b.host_text("gfa2", False, tmp_path)
        total = b.ctx.segments_text_plan("gfa2", b.printed_names("gfa2", False), b.letters)
        assert total == len(want) > 100 * 8192
        for window in (0, 8192, 100000):
            path = str(tmp_path / ("w%d.txt" % window))
            with open(path, "wb") as f:
                f.write(b"head\n")
                f.flush()
                assert b.ctx.segments_text_write(f.fileno(), 5, window) == total
            assert open(path, "rb").read() == b"head\n" + want, window
        peak = b.ctx.segments_counts()["peak_device_bytes"]
        assert peak > 16 * b.ctx.segments_counts()["events"]
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ 7. a pipe
@pytest.mark.parametrize("fmt", FORMATS)
def test_graphdump_to_a_pipe_equals_to_a_file(tmp_path, fmt):
    v = [v for v in VECTORS if v["case"] == "rand6_k3" and v["args"][2] == fmt and "--prefix" not in v["args"]][0]
    args = v["args"] + ["--gpu", "--text", "device"]
    piped = graphdump(args)   # stdout is a pipe
    assert piped.returncode == 0 and piped.stderr == b""
    path = str(tmp_path / "out.txt")
    with open(path, "wb") as f:
        filed = graphdump(args, stdout=f)
    assert filed.returncode == 0 and filed.stderr == b""
    assert open(path, "rb").read() == piped.stdout
    assert len(piped.stdout) == v["stdout_bytes"] and hashlib.sha256(piped.stdout).hexdigest() == v["stdout_sha256"]
    # appended to a file that already holds something: the text goes behind it
    with open(path, "wb") as f:
        f.write(b"before\n")
    with open(path, "ab") as f:
        again = graphdump(args, stdout=f)
    assert again.returncode == 0 and open(path, "rb").read() == b"before\n" + piped.stdout


# ------------------------------------------------------------------------------------------------ 5. long bodies, long paths, at size
def twopaco(args, files, cwd, timing=False):
    env = dict(os.environ)
    env.pop("TWOPACO_TIMING", None)
    if timing:
        env["TWOPACO_TIMING"] = "1"
    return subprocess.run([TWOPACO] + args + files, cwd=cwd, capture_output=True, timeout=900, env=env)


def device_equals_host(d, base, files, check=None):
    """For every format `--graph-text device` == `--graph-text host`, compared with cmp; --graph-prefix once; -o given once,
    and then the junction file is the one a run without --graph writes."""
    host, dev = os.path.join(d, "host.txt"), os.path.join(d, "device.txt")
    plain = os.path.join(d, "plain.bin")
    r = twopaco(base + ["-o", plain], files, d)
    assert r.returncode == 0, r.stderr[-800:]
    for fmt, extra in (("gfa1", []), ("gfa2", ["--graph-prefix"]), ("fasta", []), ("gfa1", ["-o", os.path.join(d, "junctions.bin")])):
        r = twopaco(base + ["--graph", fmt, "--graph-out", host, "--graph-text", "host"] + extra, files, d)
        assert r.returncode == 0 and r.stderr == b"", r.stderr[-800:]
        if "-o" in extra:
            os.unlink(os.path.join(d, "junctions.bin"))
        r = twopaco(base + ["--graph", fmt, "--graph-out", dev, "--graph-text", "device", "--graph-threads", "2"] + extra, files, d, timing=True)
        assert r.returncode == 0, r.stderr[-800:]
        timing = r.stderr.decode()
        assert "graph text on device" in timing and "text_kernel_ms" in timing, timing[-800:]
        assert "segment table fetch" not in timing   # the four table fetches are skipped
        print(fmt, extra[:1], os.path.getsize(host), "bytes;", [line for line in timing.split("\n") if "graph text" in line or "text_kernel" in line])
        assert os.path.getsize(host) > 0
        c = subprocess.run(["cmp", host, dev], capture_output=True, timeout=600)
        assert c.returncode == 0, (fmt, extra, c.stdout[-200:])
        if "-o" in extra:
            c = subprocess.run(["cmp", plain, os.path.join(d, "junctions.bin")], capture_output=True, timeout=600)
            assert c.returncode == 0, c.stdout[-200:]
            os.unlink(os.path.join(d, "junctions.bin"))
        if check:
            check(fmt, host)
        os.unlink(host)
        os.unlink(dev)
    os.unlink(plain)
    assert not os.path.exists(os.path.join(d, "de_bruijn.bin"))


def test_one_body_of_four_megabases(tmp_path):
    """A random sequence of 4.2 Mbp at k = 31: no 31-mer repeats (the chance of one is a few in a million), so its only
    junctions are its two ends and the graph is ONE segment -- a body that many workgroups render."""
    from twopaco_amd import synth
    d = str(tmp_path)
    path = os.path.join(d, "long.fa")
    synth.write_fasta(path, [synth.random_genome(4_200_000, 777)])

    def check(fmt, host):
        if fmt == "gfa1":
            longest = max(len(line) for line in open(host, "rb") if line.startswith(b"S\t") and not line.endswith(b"\t*\tUR:Z:" + path.encode() + b"\n"))
            print("longest S line", longest)
            assert longest >= 4_000_000

    device_equals_host(d, ["-k", "31", "-f", "30", "-t", "16", "--seed", "12345", "--tmpdir", d], [path], check)


def test_a_path_line_of_a_hundred_thousand_events(tmp_path):
    """Two copies of 5 Mbp that differ by a substitution every 40 letters on average (125 000 of them): every difference opens
    and closes a bubble, and a sequence passes about one segment per difference (differences closer than k share theirs), so
    each path line lists more than 10^5 segments."""
    from twopaco_amd import synth
    d = str(tmp_path)
    a = synth.random_genome(5_000_000, 4242)
    path = os.path.join(d, "copies.fa")
    synth.write_fasta(path, [a, synth.substitute(a, 0.025, 99)])

    def check(fmt, host):
        if fmt == "gfa1":
            longest = max(line.count(b",") + 1 for line in open(host, "rb") if line.startswith(b"P\t"))
            print("longest path", longest)
            assert longest >= 100_000

    device_equals_host(d, ["-k", "25", "-f", "30", "-t", "16", "--seed", "12345", "--tmpdir", d], [path], check)


def test_m2r2_text_device_equals_text_host(tmp_path):
    """synth m2r2 at scale 0.18, k = 25, f = 32, seed 12345: the input of test_m2r2_graph_equals_twopaco_then_serial_graphdump
    (repeat families, N runs, genomes on the other strand, 7276 contigs, several million events)."""
    d = str(tmp_path)
    case = {"name": "m2r2_s018", "fasta": None, "synth": {"workload": "m2r2", "seed": 12345, "scale": 0.18}}
    files = case_files(case, d)

    def check(fmt, host):
        if fmt == "gfa1":
            events = sum(1 for line in open(host, "rb") if line[:2] == b"C\t")
            print("events", events)
            assert events > 2_000_000

    device_equals_host(d, ["-k", "25", "-f", "32", "-t", "16", "--seed", "12345", "--tmpdir", d], files, check)
