"""CPU: tests/graph_text_reference.py -- the graph text by its definition, which tests/test_gpu_graph_text_generated.py holds the
device renderer (csrc/tpc_segtext.hip) against -- pinned without a device:

  * to the REAL reference graphdump: header + reference text has the size and sha256 recorded for all 95 vectors of
    tests/golden/graphdump.json that exit 0, and for the small walks of test_graph_walks_cpu.SMALL and the zero-named variants in all
    three formats (tests/golden/graph_text_walks.json, written by this file's __main__ from oracle/_ref/graphdump_ref; the binary is run
    again where it is present);
  * to this project's serial graphdump on the same walks and on every generated case of tests/graph_text_cases.py that it can read;
  * to itself: sizes() == the len() of every event_bytes(e), their sum == len(text()), tail(n) == text()[-n:];
and the CONDITIONS of the generated cases, asserted from segments_reference.walk: which names, widths, body sizes, empty sequences and
zero-named events each case really holds, so that the GPU file reaches what it names."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import colors_reference as C
import graph_text_cases as X
import graph_text_reference as T
import test_graph_walks_cpu as W
from graph_table import event_table, read_fasta, vector_parts
from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPHDUMP_REF = os.path.join(ROOT, "oracle", "_ref", "graphdump_ref")
TEXT_GOLDEN = os.path.join(GOLDEN, "graph_text_walks.json")
VECTORS = [v for v in json.load(open(os.path.join(GOLDEN, "graphdump.json"))) if v["case"] != "cli" and v["args"][2] in T.FORMATS and v["rc"] == 0]
RECORDED = sorted(set(W.SMALL) | set(X.ZERO_VARIANTS))
GENERATED = sorted(X.BUILDERS)


def header(fmt, names, file_of):
    """The lines graphdump prints in front of the first segment."""
    if fmt == "gfa1":
        return b"H\tVN:Z:1.0\n" + b"".join(b"S\t" + n + b"\t*\tUR:Z:" + file_of[n] + b"\n" for n in names)
    return b"H\tVN:Z:2.0\n" if fmt == "gfa2" else b""


def walk_case(name):
    return X.case(name) if name in X.ZERO_VARIANTS or name in X.BUILDERS else W.small(name)


def names_of(c):
    return getattr(c, "names", None) or [b"w%d" % i for i in range(len(c.seqs))]


def whole_output(c, fmt, names=None):
    """What graphdump prints for a case written with Case.files: header and reference text."""
    names = names_of(c) if names is None else names
    fa = (c.name + ".fa").encode()
    return header(fmt, names, {n: fa for n in names}) + T.of_case(fmt, c, names).text()


def run_walk(exe, c, d, fmt):
    fa, stream = c.files(d)
    return subprocess.run([exe, os.path.basename(stream), "-k", str(c.k), "-s", os.path.basename(fa), "-f", fmt], cwd=d, capture_output=True, timeout=600)


# ---------------------------------------------------------------------------------------------------------------- the 95 reference vectors
def test_the_reference_text_is_the_real_references_on_all_95_vectors():
    """Size and sha256 of header + text for every vector that exits 0, --prefix variants included; none is skipped."""
    tables, n = {}, 0
    before = os.getcwd()
    os.chdir(GOLDEN)
    try:
        for v in VECTORS:
            bin_name, fmt, k, files, prefix = vector_parts(v)
            key = (bin_name, k, tuple(files))
            if key not in tables:
                seqs = [s for f in files for s in read_fasta(f)]
                raw = [((line[1:].split() or [""])[0], f) for f in files for line in open(f) if line.startswith(">")]
                tables[key] = (event_table(open(bin_name, "rb").read(), seqs, k), seqs, raw)
            table, seqs, raw = tables[key]
            names = [(("s0_" + n) if prefix else n).encode() for n, _ in raw]
            file_of = {name: f.encode() for name, (_, f) in zip(names, raw)}      # the file of a name's last record
            got = header(fmt, names, file_of) + T.Text(fmt, k, *table, seqs, names).text()
            assert len(got) == v["stdout_bytes"], v["args"]
            assert hashlib.sha256(got).hexdigest() == v["stdout_sha256"], v["args"]
            n += 1
    finally:
        os.chdir(before)
    assert n == len(VECTORS) == 95


# ---------------------------------------------------------------------------------------------------------------- the small walks
def test_the_recorded_walks_are_all_there():
    record = json.load(open(TEXT_GOLDEN))
    assert sorted(record) == RECORDED and len(W.SMALL) == 10 and all(sorted(record[name]) == sorted(T.FORMATS) for name in record)
    gfa1 = json.load(open(W.WALKS_GOLDEN))
    assert all(record[name]["gfa1"] == gfa1[name] for name in W.SMALL)


@pytest.mark.parametrize("fmt", T.FORMATS)
@pytest.mark.parametrize("name", RECORDED)
def test_the_reference_text_is_both_graphdumps_on_the_small_walks(tmp_path, name, fmt):
    """The ten small walks and the six zero-named variants: header + reference text == this project's serial graphdump, with an empty
    stderr, and has the size and sha256 the real reference's graphdump printed -- which is run again where it has been built."""
    c = walk_case(name)
    want = whole_output(c, fmt)
    record = json.load(open(TEXT_GOLDEN))[name][fmt]
    assert len(want) == record["stdout_bytes"] and hashlib.sha256(want).hexdigest() == record["stdout_sha256"]
    for exe in [C.GRAPHDUMP] + ([GRAPHDUMP_REF] if os.path.exists(GRAPHDUMP_REF) else []):
        d = tmp_path / os.path.basename(exe)
        d.mkdir()
        r = run_walk(exe, c, str(d), fmt)
        assert r.returncode == 0 and r.stderr == b"", (exe, r.stderr[-400:])
        assert r.stdout == want, exe


# ---------------------------------------------------------------------------------------------------------------- self-consistency
@pytest.mark.parametrize("fmt", T.FORMATS)
@pytest.mark.parametrize("name", sorted(X.WHOLE + X.ZERO_VARIANTS))
def test_sizes_are_the_lengths_of_the_bytes(name, fmt):
    t = X.case(name).text(fmt)
    per_event, total = t.sizes()
    whole = t.text()
    assert per_event.tolist() == [len(t.event_bytes(e)) for e in range(t.events)]
    assert total == len(whole) == int(per_event.sum()) and t.offset(t.events) == total
    for e in (0, t.events // 2, t.events - 1):
        assert whole[t.offset(e):t.offset(e + 1)] == t.event_bytes(e)
    for n in (0, 1, 2, 3, 4, 100, 8192, 65536, total):
        assert t.tail(n) == whole[total - min(n, total):], n


def test_the_digit_counts():
    v = [0, 1, 9, 10, 99, 100] + [10 ** d + x for d in range(3, 20) for x in (-1, 0)] + [2 ** 64 - 1]
    assert T.digits(np.array(v, dtype=np.uint64)).tolist() == [len(str(x)) for x in v]


# ---------------------------------------------------------------------------------------------------------------- the generated cases, serially
SERIAL_NAMES = {"sequences": [b"none0", b"front", b"none2", b"none3", X.LONG_NAME, b"E", b"x", b"none7"]}   # a FASTA header cannot be empty


@pytest.mark.parametrize("name", GENERATED)
def test_the_serial_graphdump_prints_the_reference_text_of_the_generated_cases(tmp_path, name):
    """Every generated case through Case.files and the serial program, all three formats (`sequences` with its empty name spelled
    E, which a FASTA header needs).  The texts of 20 MB and more are compared where the GPU file reads them: every event of `positions`,
    the events on both sides of the grid turn, and the last 64 KiB; the fasta texts of the two cases past the turn whole."""
    c = X.case(name)
    names = SERIAL_NAMES.get(name)
    if names:
        c = X.TextCase(c.name, c.seqs, c.sequences, k=c.k, names=names)
    for fmt in T.FORMATS:
        r = run_walk(C.GRAPHDUMP, c, str(tmp_path), fmt)
        assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
        t = c.text(fmt)
        if name in X.WHOLE or (fmt == "fasta" and name != "positions"):
            assert r.stdout == whole_output(c, fmt, names)
            continue
        per_event, total = t.sizes()
        assert r.stdout.endswith(t.tail(65536))
        head = len(r.stdout) - total
        assert head == len(header(fmt, c.names, dict.fromkeys(c.names, (c.name + ".fa").encode())))
        for e in list(range(t.events)) if name == "positions" else list(range(X.TURN - 4, X.TURN + 5)):
            assert r.stdout[head + t.offset(e):head + t.offset(e) + int(per_event[e])] == t.event_bytes(e), e


# ---------------------------------------------------------------------------------------------------------------- the conditions
def widths(v):
    return set(T.digits(np.abs(np.asarray(v))).tolist())


def linked(t):
    """Events that print a link line."""
    return [e for e in range(t.events) if t.links(e)]


@pytest.mark.parametrize("name", X.ZERO_VARIANTS)
def test_conditions_a_segment_named_0(name):
    """The names of every variant; behind every zero-named occurrence with a successor there is no L / E line, 0+ is in the path line and
    the segment line of 0 is the reverse complement of its letters."""
    c = X.case(name)
    w = c.w
    want = {"zero_start": [0, 8, 16, 24, 32], "zero_middle": [40, -3, 0, 56], "zero_twice": [0, -3, 0, 72], "zero_last": [32, -3, 0],
            "zero_two_sequences": [0, 24, -3, 0, 64, 0], "minus_zero": [0, 1, 24, 0]}[name]
    assert w.name.tolist() == want
    zero = np.nonzero(w.name == 0)[0]
    behind = [int(e) + 1 for e in zero if e + 1 < w.name.size and w.seq[e + 1] == w.seq[e]]
    assert (len(behind) >= 1) == (name != "zero_last")
    if name == "minus_zero":
        assert not w.forward[0] and not w.forward[3] and w.left_id[0] == 5 and w.right_id[0] == 0       # reversed into junction 0: "-0"
    gfa1, gfa2 = c.text("gfa1"), c.text("gfa2")
    for e in behind:
        assert not gfa1.links(e) and b"\nL\t" not in b"\n" + gfa1.event_lines(e) and b"\nE\t" not in b"\n" + gfa2.event_lines(e)
    assert b"L\t0\t" not in gfa1.text() and b"E\t0+" not in gfa2.text() and b"E\t0-" not in gfa2.text()
    n_links = sum(1 for e in range(1, w.name.size) if w.seq[e] == w.seq[e - 1])
    assert gfa1.text().count(b"\nL\t") == n_links - len(behind) == gfa2.text().count(b"\nE\t")
    for s in set(w.seq[zero].tolist()):
        assert b"0+" in gfa1.path_line(s).replace(b"\t", b",").split(b",") and b"0+" in gfa2.path_line(s)[:-1].replace(b"\t", b" ").split(b" ")
    e = int(zero[0])
    letters = c.seqs[int(w.seq[e])][int(w.begin[e]):int(w.end[e]) + c.k]
    body = T.reverse_complement(letters).tobytes()
    assert b"S\t0\t" + body + b"\n" in gfa1.text() and b"S\t0\t6\t" + body + b"\n" in gfa2.text() and c.text("fasta").text().startswith(b">0\n" + body + b"\n") == (e == 0)


def test_conditions_every_width_of_a_name():
    c, big = X.case("name_widths"), X.case("big_names")
    w = c.w
    have = set(w.name.tolist())
    assert set(X.SMALL_NAMES) <= have and -1 in have and {X.FRESH + i for i in (9, 10, 99, 100)} <= have
    assert widths(w.name) == set(range(1, 10)) | {11}
    assert int(np.abs(w.name[~w.fresh]).max()) == 10 ** 8 and w.table_bytes == 4 * (10 ** 8 + 1)
    t = c.text("gfa1")
    links = linked(t)
    assert set(X.SMALL_NAMES) <= {int(w.name[e]) for e in links} and set(X.SMALL_NAMES) <= {int(w.name[e - 1]) for e in links}
    e = int(np.nonzero(w.name == -1)[0][0])
    assert w.forward[e] and chr(w.letter[e]) == "R"
    wb = big.w
    assert set(X.BIG_NAMES) <= set(wb.name.tolist()) and widths(wb.name) == set(range(1, 12)) and wb.table_bytes == 4 * (10 ** 9 + 1)
    up = len(big.seqs) - 2
    assert widths(wb.name[wb.seq == up]) == set(range(1, 12)) and (wb.name[wb.seq == up] > 0).all()        # the mixed paths
    assert widths(wb.name[wb.seq == up + 1]) >= set(range(2, 9)) | {11} and (wb.name[wb.seq == up + 1][1:] < 0).all()


def test_conditions_every_width_of_a_position():
    """begin and end pass through 1 .. 8 digits, size and the sequence length through 2 .. 8: at k = 31 a segment has 32 letters or more
    and a sequence with an event too; one digit of both is what every k = 3 case prints."""
    c = X.case("positions")
    w = c.w
    size = w.end + c.k - w.begin
    totals = np.array([len(s) for s in c.seqs])
    assert widths(w.begin) == set(range(1, 9)) == widths(w.end) and widths(size) == set(range(2, 9)) == widths(totals[w.seq])
    for v in [9, 10, 99, 100, 999, 1000, 9999, 10 ** 4, 99999, 10 ** 5, 999999, 10 ** 6, 9999999, 10 ** 7]:
        assert v in w.begin and v in w.end
    assert w.first.all() and int(size[w.name > 0].max()) > 8 * 10 ** 6 and int(size[w.name < 0].max()) > 10 ** 7
    last = w.seq_event_begin[1:] - 1
    assert (w.end[last] + c.k == totals).all()                                                   # every sequence's last event: <end>$
    t = c.text("gfa2")
    e_fwd, e_rev = 5, int(w.seq_event_begin[1]) + 1                                              # links: forward behind forward; reversed behind reversed
    assert w.name[e_fwd - 1] > 0 and w.name[e_fwd] > 0 and w.name[e_rev - 1] < 0 and w.name[e_rev] < 0
    f, r = t.event_lines(e_fwd).split(b"\n")[-2].split(b"\t"), t.event_lines(e_rev).split(b"\n")[-2].split(b"\t")
    assert f[0] == r[0] == b"E" and f[4].endswith(b"$") and not f[6].endswith(b"$") and f[5] == b"0" and f[6] == b"31"         # a1 = size': $
    assert r[3] == b"0" and r[4] == b"31" and r[6].endswith(b"$") and not r[4].endswith(b"$")                                  # b1 = size: $
    assert t.event_lines(int(last[0])).split(b"\n")[-3].split(b"\t")[6] == b"%d$" % totals[0]


def test_conditions_the_fasta_wrap():
    c = X.case("wrap")
    w = c.w
    size = (w.end + c.k - w.begin).tolist()
    n = len(X.WRAP_SIZES)
    assert w.first.all() and size == [9000] + list(X.WRAP_SIZES) * 2 and (w.name[1:n + 1] > 0).all() and (w.name[n + 1:] < 0).all()
    text = c.text("fasta").text()
    assert max(len(line) for line in text.split(b"\n")) == 80 and b"\n\n" not in text
    assert text.count(b"\n") == 1 + 113 + 2 * (n + sum((s + 79) // 80 for s in X.WRAP_SIZES))
    assert all(c.text(fmt).offset(1) > X.TILE for fmt in T.FORMATS)                              # a tile edge fits in front of every wrapped body


def test_conditions_sequences():
    c = X.case("sequences")
    w = c.w
    per_seq = np.diff(w.seq_event_begin.astype(np.int64)).tolist()
    assert per_seq == [0, 329, 0, 0, 4, 1, 3, 0] and [len(n) for n in c.names] == [5, 5, 5, 5, 300, 0, 1, 5]
    for fmt in ("gfa1", "gfa2"):
        t = c.text(fmt)
        text = t.text()
        assert text.count(b"P\t" if fmt == "gfa1" else b"O\t") == 4
        at = text.index(X.LONG_NAME)
        assert at > X.TILE + 300 and text.count(X.LONG_NAME) == 5                                # 4 C / F lines and the path line; an edge fits in front
        assert (b"\nP\t\t" in text) if fmt == "gfa1" else (b"\nO\tp\t" in text)                # the empty name heads a path line
        assert b"\nP\tx\t" in text or b"\nO\txp\t" in text


def test_conditions_letters():
    one, many = X.case("letters_one"), X.case("letters_many")
    start = lambda c: np.concatenate([[0], np.cumsum([len(s) for s in c.seqs])])[:-1]
    assert X.ambiguous(one, start(one))[0].size == 1 == len(X.ambiguous(one, start(one))[1]) and 1000 <= X.ambiguous(many, start(many))[0].size <= 1100
    w = many.w
    iupac = np.frombuffer(X.IUPAC, dtype=np.uint8)
    counts = {(strand, where): 0 for strand in (True, False) for where in ("first", "last", "N")}
    for e in np.nonzero(w.first)[0]:
        letters = many.seqs[int(w.seq[e])][int(w.begin[e]):int(w.end[e]) + many.k]
        strand = bool(w.name[e] > 0)
        counts[(strand, "first")] += bool(np.isin(letters[0], iupac))
        counts[(strand, "last")] += bool(np.isin(letters[-1], iupac))
        counts[(strand, "N")] += b"NNNNN" in letters.tobytes()
    assert min(counts.values()) >= 100, counts
    assert -1 in w.name and (w.name[w.seq == 0][[0, 2, 3]] > 0).all() and (w.name[w.seq == 1] < 0).all()
    assert many.text("gfa1").total() > 10 * X.TILE
    w1 = one.w
    e = int(np.nonzero(w1.seq == 1)[0][0])                                                       # the one ambiguous letter lies in reversed bodies only
    assert (w1.name[w1.seq == 1] < 0).all() and b"Y" not in one.text("gfa1").text() and b"Y" in one.seqs[1].tobytes() and w1.begin[e] <= 4


def test_conditions_path_lines():
    c = X.case("paths")
    w = c.w
    assert np.diff(w.seq_event_begin.astype(np.int64)).tolist() == [1, 2, 3000, 1]
    long = w.name[w.seq == 2]
    assert widths(long) == set(range(1, 10)) | {11} and (long > 0).sum() > 500 and (long < 0).sum() > 500
    assert int(np.abs(w.name[~w.fresh]).max()) <= 10 ** 8
    for fmt in ("gfa1", "gfa2"):
        assert len(c.text(fmt).path_line(2)) > 2 * X.TILE + 1000                                 # it meets three tiles or more wherever it begins


def test_conditions_past_the_grid_turn():
    c = X.case("turn_events")
    w = c.w
    assert w.name.size == X.TURN + 302 and int(w.seq_event_begin[1]) == X.TURN + 300
    first = np.nonzero(w.first)[0]
    assert 20 < first.size < 80 and (first >= X.TURN).sum() >= 4 and (first < X.TURN - 2).sum() > 20
    assert c.text("fasta").total() < 1000 and len(set(w.name[X.TURN - 2:X.TURN + 3].tolist())) >= 4
    c = X.case("turn_sequences")
    w = c.w
    per_seq = np.diff(w.seq_event_begin.astype(np.int64))
    assert per_seq.size == X.TURN + 71 and per_seq[X.TURN - 1] == 0 and per_seq.sum() == X.TURN + 70 and (np.delete(per_seq, X.TURN - 1) == 1).all()
    first = np.nonzero(w.first)[0]
    assert first.size < 300 and (first > X.TURN).sum() >= 1


# ---------------------------------------------------------------------------------------------------------------- recording
if __name__ == "__main__":
    # python tests/test_graph_text_reference_cpu.py : writes tests/golden/graph_text_walks.json from the reference's own graphdump
    import tempfile
    assert os.path.exists(GRAPHDUMP_REF), "the reference's graphdump has not been built (oracle/Makefile: ref)"
    out = {}
    for name in RECORDED:
        out[name] = {}
        for fmt in T.FORMATS:
            with tempfile.TemporaryDirectory() as d:
                r = run_walk(GRAPHDUMP_REF, walk_case(name), d, fmt)
            assert r.returncode == 0 and r.stderr == b"", (name, fmt, r.stderr)
            out[name][fmt] = {"stdout_bytes": len(r.stdout), "stdout_sha256": hashlib.sha256(r.stdout).hexdigest()}
    with open(TEXT_GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", len(out), "walks in", len(T.FORMATS), "formats")
