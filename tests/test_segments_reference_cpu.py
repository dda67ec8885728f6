"""CPU: tests/segments_reference.py, the vectorised statement of the event table that tests/test_gpu_segments.py holds the kernels of
csrc/tpc_segments.hip against.  It has to agree with the sequential restatement (graph_table.event_table) on the committed golden
streams and on the synthetic cases, with what the real walks print (the reference's graphdump, recorded in
tests/golden/segments_walk.json and run again where its binary is present, and this project's graphdump), with the serial walk's
errors, and with a few tables listed by hand.  Building the synthetic cases here also runs every property their builders assert."""
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import graph_table
import segments_reference as R
import test_gpu_segments as G
from helpers import GOLDEN, golden_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPHDUMP = os.path.join(ROOT, "twopaco_amd", "bin", "graphdump")
GRAPHDUMP_REF = os.path.join(ROOT, "oracle", "_ref", "graphdump_ref")
WALK_GOLDEN = os.path.join(GOLDEN, "segments_walk.json")
COMMITTED = [c for c in golden_cases() if c.get("bin") and c.get("fasta") and os.path.exists(os.path.join(GOLDEN, c["bin"]))
             and os.path.exists(os.path.join(GOLDEN, c["fasta"]))]
# small valid synthetic streams that go through the real walks
WALKED = ("directions_signs_letters", "n_forward_reverse", "strands_real_1_first", "strands_minus_1_first", "amb_3", "no_last_separator",
          "phase_k32", "edge_65")


def same_tables(got, want):
    """got: R.Table, want: the five arrays of graph_table.event_table."""
    return all(a.shape == b.shape and (a == b).all() for a, b in zip(got[:5], want))


def strings(seqs):
    return [R.letters_of(s).tobytes().decode() for s in seqs]


# ---------------------------------------------------------------------------------------------------------------- the sequential restatement
def test_equals_the_sequential_table_on_every_golden_stream():
    """Every committed stream with a FASTA file.  Where the walk reports an error the sequential table still exists as long as every
    event lies inside its sequence (edge.fa: sequences shorter than k were skipped)."""
    checked = events = refused = 0
    for case in COMMITTED:
        data = open(os.path.join(GOLDEN, case["bin"]), "rb").read()
        seqs = graph_table.read_fasta(os.path.join(GOLDEN, case["fasta"]))
        w = R.walk(data, seqs, case["k"])
        assert w.ok.all(), case["name"]
        assert same_tables(R.event_table(data, seqs, case["k"]), graph_table.event_table(data, seqs, case["k"])), case["name"]
        checked += 1
        events += w.name.size
        refused += w.error is not None
    assert checked >= 43, checked           # a case that silently drops out cannot hide a failure
    assert events > 50000 and refused >= 1, (events, refused)


def test_equals_the_sequential_table_on_the_synthetic_cases():
    """Every small case of the GPU tests whose events all pass their checks; building them asserts their properties."""
    checked = 0
    for name in G.SMALL:
        c = G.case(name)
        if not c.w.ok.all():
            continue
        assert same_tables(R.event_table(c.data, c.seqs, c.k), graph_table.event_table(c.data, strings(c.seqs), c.k)), name
        checked += 1
    assert checked == len(G.SMALL) - 1 == 32       # all but more_separators_than_sequences


def test_the_large_cases_hold_their_properties():
    """The two large cases are built (their builders assert what they promise) in the time the issue gives the reference."""
    import time
    t0 = time.time()
    for name in G.LARGE:
        assert G.case(name).valid
    print("large cases: %.1f s" % (time.time() - t0))


# ---------------------------------------------------------------------------------------------------------------- the real walks
def run_walk(exe, c, d):
    """stdout of `exe <stream> -f gfa1 -k <k> -s <fasta>` run in d with relative file names (the header lines print the FASTA's name)."""
    with open(os.path.join(d, c.name + ".fa"), "wb") as f:
        for i, s in enumerate(c.seqs):
            f.write(b">q%d\n" % i + s.tobytes() + b"\n")
    with open(os.path.join(d, c.name + ".bin"), "wb") as f:
        f.write(c.data)
    return subprocess.run([exe, c.name + ".bin", "-f", "gfa1", "-k", str(c.k), "-s", c.name + ".fa"], cwd=d, capture_output=True, timeout=120)


def printed(n):
    """A name as the P lines print it: its magnitude and its sign, 0 and the fresh names with '+', -1 as 1-."""
    return "%d%s" % (abs(n), "-" if n < 0 else "+")


def check_gfa1(out, c):
    """The S lines with a body carry, in order, |name| of the first sights; the P line of a sequence its events' names."""
    w = c.w
    lines = out.decode().split("\n")
    assert lines[0] == "H\tVN:Z:1.0" and lines[-1] == ""
    headers = [l for l in lines if l.startswith("S\tq")]
    assert headers == ["S\tq%d\t*\tUR:Z:%s.fa" % (i, c.name) for i in range(w.n_rec)]
    bodies = [int(l.split("\t")[1]) for l in lines if l.startswith("S\t") and not l.startswith("S\tq")]
    assert bodies == np.abs(w.name[w.first]).tolist()
    paths = {l.split("\t")[1]: l.split("\t")[2:] for l in lines if l.startswith("P\t")}
    b = w.seq_event_begin
    want = {"q%d" % s: [",".join(printed(n) for n in w.name[b[s]:b[s + 1]].tolist()), "*"] for s in range(w.n_rec) if b[s + 1] > b[s]}
    assert paths == want
    assert sum(l.startswith("C\t") for l in lines) == w.name.size


@pytest.mark.parametrize("name", WALKED)
def test_equals_what_the_real_walks_print(tmp_path, name):
    """This project's serial graphdump prints the reference's recorded bytes, and those bytes spell the new reference's table; where the
    reference's own binary has been built it is run again and must give the recorded bytes too."""
    c = G.case(name)
    assert c.valid
    record = json.load(open(WALK_GOLDEN))[name]
    assert os.path.exists(GRAPHDUMP), "run build() first"
    exes = [GRAPHDUMP] + ([GRAPHDUMP_REF] if os.path.exists(GRAPHDUMP_REF) else [])
    for exe in exes:
        d = tmp_path / os.path.basename(exe)
        d.mkdir()
        r = run_walk(exe, c, str(d))
        assert r.returncode == 0 and r.stderr == b"", (exe, r.stderr)
        assert len(r.stdout) == record["stdout_bytes"] and hashlib.sha256(r.stdout).hexdigest() == record["stdout_sha256"], exe
        check_gfa1(r.stdout, c)


def test_the_recorded_walks_are_all_there():
    assert set(json.load(open(WALK_GOLDEN))) == set(WALKED)


# ---------------------------------------------------------------------------------------------------------------- errors
def rec(pos, ident):
    return struct.pack("<Iq", pos, ident)


SEP = rec(R.SEP_POS, R.SEP_ID)
TEXT = ["ACGTTGCARCGTACGGTNACCA", "GGATCCA", "AC", "TTGACCAGT"]     # k = 3
ERRORS = {
    # name: (stream, the walk's first error)
    "end_not_behind_begin": (rec(0, 1) + rec(4, 2) + rec(4, 3) + rec(9, 4), (2, R.CORRUPTED)),
    "end_past_the_sequence": (rec(0, 1) + rec(4, 2) + SEP + rec(1, 3) + rec(5, 4), (4, R.CORRUPTED)),   # 5 + 3 > 7
    "id_too_large_right": (rec(0, 1) + rec(4, 1 << 31) + rec(9, 4), (1, R.TOO_LARGE)),
    "id_too_large_left_negative": (rec(0, 1) + SEP + rec(0, -(1 << 31)) + rec(4, 2), (3, R.TOO_LARGE)),
    "id_int64_min": (rec(0, 1) + rec(4, -(1 << 63)) + rec(9, 4), (1, R.TOO_LARGE)),
    "corrupted_before_too_large": (rec(0, 1) + rec(4, 2) + rec(3, 3) + rec(9, 1 << 31), (2, R.CORRUPTED)),
    "too_large_before_corrupted": (rec(0, 1) + rec(4, 1 << 40) + rec(3, 3) + rec(9, 4), (1, R.TOO_LARGE)),
    "both_in_one_pair": (rec(0, 1) + rec(0, 1 << 31), (1, R.CORRUPTED)),
    "first_record_not_of_sequence_0": (SEP + rec(0, 1) + rec(4, 2), (1, R.CORRUPTED)),
    "two_separators": (rec(0, 1) + rec(4, 2) + SEP + SEP + rec(0, 3), (4, R.CORRUPTED)),
    "sequence_beyond_the_text": (rec(0, 1) + SEP + rec(0, 2) + SEP + rec(0, 3) + SEP + rec(0, 4) + SEP + rec(0, 4) + rec(1, 5), (9, R.CORRUPTED)),
    "large_id_in_no_event": (rec(0, 1) + rec(4, 2) + SEP + rec(0, 1 << 31), None),
    "trailing_bytes": (rec(0, 1) + rec(4, 2) + b"\x01\x02\x03", None),
    "empty": (b"", None),
}


@pytest.mark.parametrize("name", sorted(ERRORS) + ["more_separators_than_sequences", "no_record_sequences"])
def test_errors_are_the_serial_walks(tmp_path, name):
    """The first error of the new reference is the one this project's serial walk ends with (the reference's binary reads out of
    bounds on some of these streams and is not run)."""
    if name in ERRORS:
        data, want = ERRORS[name]
        c = G.Case(name, 3, TEXT, [])
        c.data, c.w = data, R.walk(data, TEXT, 3)
        assert c.w.error == want
    else:
        c = G.case(name)
        assert c.w.error is not None
    assert os.path.exists(GRAPHDUMP), "run build() first"
    r = run_walk(GRAPHDUMP, c, str(tmp_path))
    if c.w.error is None:
        assert r.returncode == 0 and r.stderr == b""
        check_gfa1(r.stdout, c)
    else:
        assert r.returncode == 1 and r.stderr.decode() == "error: %s\n" % c.w.error[1]


# ---------------------------------------------------------------------------------------------------------------- by hand
F = R.FRESH


def test_tables_listed_by_hand():
    """k = 3 over  A C G T T G C A R C G  T  A  C  G  G  T  N  A  C  C  A
                   0 1 2 3 4 5 6 7 8 9 10 11 12 13 14 15 16 17 18 19 20 21"""
    seq = TEXT[0]
    records = [(0, 0), (2, 0), (4, 0), (5, 3), (6, -3), (9, 0), (12, 7), (14, 7), (15, 2), (18, 1)]
    t = R.event_table(R.build_stream([records]), [seq], 3)
    # (0,0)-(2,0)  reverse from -0: before 2 is C, its complement G = 2; the start is the left id, so the sign stays
    # (2,0)-(4,0)  reverse: before 4 is T -> A = 0          (4,0)-(5,3)  forward from 0: behind 4 + 3 is A = 0
    # (5,3)-(6,-3) equal ids above 0, forward from 3: behind 5 + 3 is R, no code: -1
    # (6,-3)-(9,0) reverse: before 9 is R, its complement is N: fresh          (9,0)-(12,7) forward from 0: A = 0
    # (12,7)-(14,7) forward from 7: G = 2 | 7 << 3 = 58     (14,7)-(15,2) reverse from -2: before 15 is G -> C = 1 | 4 | 2 << 3 = 21, negated
    # (15,2)-(18,1) reverse: before 18 is N: fresh
    assert t.name.tolist() == [2, 0, 0, -1, F, 0, 58, -21, F + 1]
    assert t.first.tolist() == [True, True, False, True, True, False, True, True, True]
    assert t.begin.tolist() == [0, 2, 4, 5, 6, 9, 12, 14, 15] and t.end.tolist() == [2, 4, 5, 6, 9, 12, 14, 15, 18]
    assert t.seq_event_begin.tolist() == [0, 9] and t.n_named == 2 and t.error is None

    # four sequences, the separators written three ways; the third holds one record, the fourth none
    data = R.build_stream([[(0, -4), (3, 4), (4, -9)], [(1, 6), (2, -5), (4, 5)], [(0, 8)], []], ["pos", "id", "both"], last_separator=False)
    assert len(data) == 12 * 10 and data[36:48] == rec(R.SEP_POS, 5) and data[84:96] == rec(7, R.SEP_ID) and data[108:] == SEP
    t = R.event_table(data, ["GGATCCA", "GGATCCA", "ACG", "A"], 3)
    # (0,-4)-(3,4)  equal, forward from -4: behind 0 + 3 is T = 3 | 4 | 4 << 3 = 39
    # (3,4)-(4,-9)  forward from 4: behind 3 + 3 is A = 0 | 4 << 3 = 32
    # (1,6)-(2,-5)  reverse from 5: before 2 is G -> C = 1 | 5 << 3 = 41, negated
    # (2,-5)-(4,5)  equal, forward from -5: behind 2 + 3 is C = 1 | 4 | 5 << 3 = 45
    assert t.name.tolist() == [39, 32, -41, 45] and t.first.all()
    assert t.seq_event_begin.tolist() == [0, 2, 4, 4, 4] and t.error is None and t.n_named == 0
    w = R.walk(data, ["GGATCCA", "GGATCCA", "ACG", "A"], 3)
    assert w.table_bytes == 4 * 46 and w.n_separators == 3 and w.slots == 10

    # the second event ends past its sequence: name 0, the error at its right record; the others are what the rule gives
    t = R.event_table(R.build_stream([[(0, 1), (2, 2), (5, 3)], [(0, 3), (4, 2)]]), ["GGATCCA", "GGATCCA"], 3)
    assert t.error == (2, R.CORRUPTED) and t.name.tolist() == [3 | 1 << 3, 0, -(0 | 4 | 2 << 3)] and t.first.all()

    assert R.event_table(b"", [], 3)[4].tolist() == [0] and R.event_table(SEP + SEP, ["ACGT"], 3).seq_event_begin.tolist() == [0, 0]


# ---------------------------------------------------------------------------------------------------------------- recording
if __name__ == "__main__":
    # python tests/test_segments_reference_cpu.py : writes tests/golden/segments_walk.json from the reference's own graphdump
    import tempfile
    assert os.path.exists(GRAPHDUMP_REF), "the reference's graphdump has not been built (oracle/Makefile: ref)"
    out = {}
    for name in WALKED:
        with tempfile.TemporaryDirectory() as d:
            r = run_walk(GRAPHDUMP_REF, G.case(name), d)
        assert r.returncode == 0 and r.stderr == b"", (name, r.stderr)
        out[name] = {"stdout_bytes": len(r.stdout), "stdout_sha256": hashlib.sha256(r.stdout).hexdigest()}
    with open(WALK_GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", len(out), "walks")
