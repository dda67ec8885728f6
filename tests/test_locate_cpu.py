"""CPU: `graphdump --locate` without --gpu (host/graphformat.h: BuildEdgeIndex, ComputeLocate, WriteLocate, WriteLocateWalks) against
locate_reference.py -- the table and the walks file byte for byte against the definition over graph_table.event_table (statement 1),
and checked by the statement over the serial gfa1 text alone (statement 2: every run spells back on the S body it names, every window
no run covers is absent from the bodies' (k+1)-mers) -- on all the good gfa1 vectors in both colour modes with the vector's own FASTA
as the query; the numbers recorded for the index; reverse complements, unrelated letters, short runs, short, empty and all-N records,
poly-A; the flags' usage errors; the table beside the others."""
import os
import subprocess

import numpy as np
import pytest

import colors_reference as C
import graph_table
import locate_reference as R
from helpers import GOLDEN, golden_cases

CASES = {c["name"]: c for c in golden_cases()}
_INDEX = {}


def index_of(v, by):
    """(index, bin, k, files, prefix, names, letters, labels) of a gfa1 vector."""
    key = (C.vector_id(v), by)
    if key not in _INDEX:
        binf, _, k, files, prefix = graph_table.vector_parts(v)
        named = [(f, rec) for f in files for rec in R.read_named(os.path.join(GOLDEN, f))]
        letters = [rec[1] for _, rec in named]
        file_of = [files.index(f) for f, _ in named]
        color_of_seq = list(range(len(letters))) if by == "sequence" else file_of
        labels = ["%d\t%s" % (s + 1, files[file_of[s]]) for s in range(len(letters))] if by == "sequence" else list(files)
        table = graph_table.event_table(open(os.path.join(GOLDEN, binf), "rb").read(), letters, k)
        _INDEX[key] = (R.Index(table, letters, k, color_of_seq, len(labels)), binf, k, files, prefix, [rec[0] for _, rec in named], letters, labels)
    return _INDEX[key]


def graphdump(args, cwd=GOLDEN):
    return subprocess.run([C.GRAPHDUMP] + args, cwd=cwd, capture_output=True, timeout=600)


def write_fasta(path, records, names=None):
    with open(path, "w") as f:
        for i, r in enumerate(records):
            f.write(">%s some words\n" % (names[i] if names else "q%d" % i))
            for at in range(0, len(r), 70):
                f.write(r[at:at + 70] + "\n")
    return str(path)


def located(v, by, tmp_path, queries, names, extra=()):
    """graphdump --locate of the vector over query files, the bytes compared with statement 1; returns (oracle's Located, tsv, walks)."""
    index, binf, k, files, prefix, _, _, labels = index_of(v, by)
    out, walks = str(tmp_path / "locate.tsv"), str(tmp_path / "walks.tsv")
    args = [binf, "-k", str(k)] + [x for f in files for x in ("-s", f)] + (["--prefix"] if prefix else []) + ["--locate", by, "--locate-out", out, "--locate-walks", walks]
    r = graphdump(args + [x for q in queries for x in ("--locate-in", q)] + list(extra))
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    letters = [rec[1] for q in queries for rec in R.read_named(q)]
    want = index.locate(letters)
    got_tsv, got_walks = open(out, "rb").read(), open(walks, "rb").read()
    assert got_tsv == R.tsv(index, want, names, by, labels)
    assert got_walks == R.walks(index, want)
    return want, got_tsv, got_walks, r


@pytest.mark.parametrize("by", ["file", "sequence"])
@pytest.mark.parametrize("v", C.GOOD_VECTORS, ids=C.vector_id)
def test_own_genomes_byte_for_byte_and_by_the_gfa1_text(v, by, tmp_path):
    index, binf, k, files, prefix, names, letters, _ = index_of(v, by)
    want, tsv, walks, _ = located(v, by, tmp_path, [os.path.join(GOLDEN, f) for f in files], names)
    R.check_by_gfa1(C.golden_gfa1(v), k, letters, tsv, walks)
    if "_a3" not in binf:
        assert (want.sums[1] == want.sums[0]).all() and want.info["windows"] > 0       # every edge of an input is in the graph
    name = binf[:-4]
    if name in R.RECORDED:
        assert index.counts() == R.RECORDED[name]


@pytest.mark.parametrize("name", sorted(R.RECORDED))
def test_the_recorded_index_numbers(name):
    index, _ = R.golden_index(CASES[name], GOLDEN)
    assert index.counts() == R.RECORDED[name]


@pytest.mark.parametrize("name,found,windows", [("rand6_k9_a3", 16842, 17706), ("wd_k93_a3", 20453, 20735)])
def test_an_abundance_cut_loses_edges(name, found, windows, tmp_path):
    case = CASES[name]           # (wd_k93_a3 has no gfa1 vector of the reference's: the command line is made here)
    v = {"case": name, "args": [case["bin"], "-f", "gfa1", "-k", str(case["k"]), "-s", case["fasta"]]}
    _, _, _, files, _, names, _, _ = index_of(v, "file")
    want, _, _, _ = located(v, "file", tmp_path, [os.path.join(GOLDEN, f) for f in files], names)
    assert (want.info["found"], want.info["windows"]) == (found, windows)


def clean(s):
    return "".join(ch if ch in "ACGT" else "A" for ch in s)


def test_the_reverse_complement_of_a_genome(tmp_path):
    v = C.case_vector(CASES["rand6_k9_fp"])
    index, _, k, _, _, _, letters, _ = index_of(v, "sequence")
    genome = clean(letters[1])
    fa = write_fasta(tmp_path / "q.fa", [genome, R.revcomp(genome)])
    want, tsv, walks, _ = located(v, "sequence", tmp_path, [fa], ["q0", "q1"])
    R.check_by_gfa1(C.golden_gfa1(v), k, [genome, R.revcomp(genome)], tsv, walks)
    n = k + 1
    palindromes = sum(1 for p in range(len(genome) - n + 1) if genome[p:p + n] == R.revcomp(genome[p:p + n]))
    found, forward, runs = want.sums[1], want.sums[2], want.sums[3]
    assert found[0] == found[1] > 0 and runs[0] == runs[1]
    # a hit is forward in exactly one of the two unless it is a palindrome, which is forward in both
    assert int(forward[0]) + int(forward[1]) == int(found[0]) + palindromes
    first = [(int(p), int(l), int(r), int(rev), int(off)) for p, l, r, rev, off in zip(*want.runs) if p < want.rec_start[1]]
    second = [(int(p), int(l), int(r), int(rev), int(off)) for p, l, r, rev, off in zip(*want.runs) if p >= want.rec_start[1]]
    end = want.rec_start[1] + len(genome)            # the run at p of length l lies mirrored at end - p' - l - k + 1, its strand flipped unless it is a palindrome
    mirrored = sorted((want.rec_start[0] + end - p - l - k, l, r) for p, l, r, rev, off in second)
    assert sorted((p, l, r) for p, l, r, rev, off in first) == mirrored


def test_unrelated_letters_hit_at_most_a_handful():
    rng = np.random.default_rng(20261019)
    for name in ("c2_k29", "tr_k25_L28"):
        index, _ = R.golden_index(CASES[name], GOLDEN)
        assert index.k >= 21
        want = index.locate(["".join("ACGT"[i] for i in rng.integers(0, 4, 5000))])
        assert want.info["windows"] == 5000 - index.k and want.info["found"] <= 3


def test_short_runs_short_records_empty_records_and_all_n(tmp_path):
    v = C.case_vector(CASES["c2_k29"])
    index, _, k, _, _, _, letters, _ = index_of(v, "file")
    genome = clean(letters[0])[:3000]
    a = bytearray(genome.encode())
    for i in range(k, len(a), 2 * k):
        a[i] = ord("ACGT"[("ACGT".index(chr(a[i])) + 1) % 4])
    records = [a.decode(), genome[:k], genome[:k + 1], "", "N" * 100, genome[100:100 + 2 * k] + "R" + genome[500:500 + 2 * k]]
    names = ["subst", "short", "one", "empty", "enn", "iupac"]
    fa = write_fasta(tmp_path / "q.fa", records, names)
    want, tsv, walks, _ = located(v, "file", tmp_path, [fa], names)
    R.check_by_gfa1(C.golden_gfa1(v), k, records, tsv, walks)
    windows, found, _, runs = want.sums
    assert runs[0] >= len(genome) // (2 * k) - 2 and found[0] < windows[0]           # a substitution breaks k + 1 windows out of every 2 k
    assert (windows[1], windows[2], found[2], runs[2]) == (0, 1, 1, 1) and windows[3] == 0 and windows[4] == 0
    assert windows[5] == found[5] == 2 * k and runs[5] >= 2          # the letter R is an N: k + 1 windows around it are invalid


def test_poly_a_hits_one_entry_in_runs_of_one_window(tmp_path):
    v = C.case_vector(CASES["tr_k25_L28"])
    index, _, k, _, _, _, _, _ = index_of(v, "file")
    fa = write_fasta(tmp_path / "q.fa", ["A" * 3000])
    want, _, _, _ = located(v, "file", tmp_path, [fa], ["q0"])
    assert want.info["found"] == 3000 - k and want.info["runs"] == 3000 - k and len(set(want.hit.tolist()) - {R.INVALID}) == 1


def test_two_query_files_and_the_table_beside_the_colour_table(tmp_path):
    v = C.case_vector(CASES["rand6_k9_fp"])
    index, binf, k, files, _, names, letters, _ = index_of(v, "sequence")
    extra = write_fasta(tmp_path / "more.fa", [letters[0][:200], "ACGTNNACGT"])
    own = os.path.join(GOLDEN, files[0])
    _, tsv, walks, r = located(v, "sequence", tmp_path, [own, extra], names + ["q0", "q1"], extra=["--colors", "sequence"])
    alone = graphdump([binf, "-k", str(k), "-s", files[0], "--colors", "sequence"])
    assert alone.returncode == 0 and r.stdout == alone.stdout and len(r.stdout) > 0     # the colour table first, on the standard output
    to_stdout = graphdump([binf, "-k", str(k), "-s", files[0], "--locate", "sequence", "--locate-in", own, "--locate-in", extra])
    assert to_stdout.returncode == 0 and to_stdout.stdout == tsv and to_stdout.stderr == b""


@pytest.mark.parametrize("args,text", [
    (["--locate", "genome", "--locate-in", "rand6.fa"], "Value 'genome' does not meet constraint: file|sequence"),
    (["--locate", "file"], "The locate table needs a query: --locate-in <fasta file>"),
    (["--locate-in", "rand6.fa", "-f", "gfa1"], "This argument needs --locate <file|sequence>"),
    (["--locate-out", "x", "-f", "gfa1"], "This argument needs --locate <file|sequence>"),
    (["--locate-walks", "x", "-f", "gfa1"], "This argument needs --locate <file|sequence>"),
    (["--locate", "file", "--locate-in", "rand6.fa", "--locate-walks", ""], "The locate walks need a file name"),
    (["--locate", "file", "--locate-in", "rand6.fa", "-f", "gfa1"], "Mutually exclusive argument already set!"),
    (["--locate", "file", "--locate-in", "rand6.fa", "--links"], "The locate table and the link table are written one at a time: not with --links"),
    (["--locate", "file", "--locate-in", "rand6.fa", "-f", "gfa1", "--compact"], "Mutually exclusive argument already set!"),
    (["--locate", "file", "--locate-in", "rand6.fa", "--text", "host"], "The locate table is formatted by the host: not with --locate"),
    (["--locate", "file", "--locate-in", "rand6.fa", "--colors", "sequence"], "--colors sequence does not go with --locate file"),
    (["--locate", "file", "--locate-in", "rand6.fa", "--anchors", "sequence"], "--anchors sequence does not go with --locate file"),
])
def test_usage_errors(args, text):
    r = graphdump(["rand6_k9_fp.bin", "-k", "9", "-s", "rand6.fa"] + args)
    assert r.returncode != 0 and r.stdout == b"" and text in r.stderr.decode()


def test_a_query_file_that_is_missing(tmp_path):
    r = graphdump(["rand6_k9_fp.bin", "-k", "9", "-s", "rand6.fa", "--locate", "file", "--locate-in", str(tmp_path / "none.fa")])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode() == "error: Can't open file %s\n" % (tmp_path / "none.fa")
