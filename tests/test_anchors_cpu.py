"""CPU: the anchor table of the serial `graphdump --anchors` against the definition, stated twice in anchors_reference.py: over the
serial gfa1 text (part 1; itself pinned to the real reference's sha256 by tests/golden/graphdump.json) byte for byte, TSV and PAF, on
every golden vector whose gfa1 succeeds, in both colour modes, with the first and the last colour as the reference; the text checked
on its own against the FASTA letters; and on a generated family (substitutions, an inversion, a moved stretch, duplications on either
side, a whole-genome reverse complement, a genome cut into records, a run of N, an unrelated genome) also against the maximal runs
of unique (k+1)-mers read off the FASTA alone (part 2).  Then the small cases and the flags' errors."""
import os

import pytest

import anchors_reference as R
from helpers import GOLDEN


@pytest.fixture(scope="module", autouse=True)
def built():
    assert os.path.exists(R.GRAPHDUMP) and os.path.exists(R.TWOPACO), "run build() first"


def serial(args, by, tmp_path, ref=None, cwd=GOLDEN, more=()):
    """(table from stdout, PAF file) of the serial graphdump."""
    paf = str(tmp_path / "anchors.paf")
    r = R.run_graphdump(list(args) + ["--anchors", by, "--anchors-paf", paf] + ([] if ref is None else ["--anchors-ref", str(ref)]) + list(more), cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    return r.stdout, open(paf, "rb").read()


# ------------------------------------------------------------------------------------------------ 1. golden vectors
@pytest.mark.parametrize("ref", [0, "last"])
@pytest.mark.parametrize("by", ["file", "sequence"])
@pytest.mark.parametrize("v", R.GOOD_VECTORS, ids=[R.vector_id(v) for v in R.GOOD_VECTORS])
def test_serial_anchors_equal_the_oracle(v, by, ref, tmp_path):
    want = R.golden_anchors(v, by, ref)
    tsv, paf = serial(R.anchors_args(v), by, tmp_path, ref=want.ref)
    assert tsv == want.tsv(), R.vector_id(v)
    assert paf == want.paf(), R.vector_id(v)
    assert want.same_length or v["case"] == "rand6_k9_a3"
    if ref == 0:   # the default reference is colour 0
        assert serial(R.anchors_args(v), by, tmp_path) == (tsv, paf)


def test_the_golden_vectors_are_all_there():
    assert len(R.GOOD_VECTORS) == 38
    assert sum(len(R.golden_anchors(v, "sequence", 0).blocks) for v in R.GOOD_VECTORS) > 0


@pytest.mark.parametrize("by", ["file", "sequence"])
@pytest.mark.parametrize("v", [v for v in R.GOOD_VECTORS if v["case"] != "rand6_k9_a3"], ids=[R.vector_id(v) for v in R.GOOD_VECTORS if v["case"] != "rand6_k9_a3"])
def test_the_blocks_spell_the_same_letters(v, by, tmp_path):
    """(rand6_k9_a3 is left out as the bubble test leaves it out: its abundance cut lets one name cover different bodies.)"""
    for ref in (0, R.golden_anchors(v, by, "last").ref):
        tsv, _ = serial(R.anchors_args(v), by, tmp_path, ref=ref)
        assert R.check_text(tsv, R.fasta_of(v)) == len(R.golden_anchors(v, by, ref if ref == 0 else "last").blocks)


# ------------------------------------------------------------------------------------------------ 2. the generated family
@pytest.fixture(scope="module")
def family(tmp_path_factory):
    d = tmp_path_factory.mktemp("anchors")
    fastas = R.family_files(d)
    stream = R.streams_of(fastas, str(d / "family.bin"), R.FAMILY_K, R.FAMILY_L, R.FAMILY_Q, R.FAMILY_SEED)
    args = [stream, "-k", str(R.FAMILY_K)] + [x for f in fastas for x in ("-s", f)]
    gfa1 = R.run_graphdump(args + ["-f", "gfa1"], cwd=str(d))
    assert gfa1.returncode == 0 and gfa1.stderr == b""
    records = [s for f in fastas for _, s in R.read_fasta(f)]
    want = R.Anchors(gfa1.stdout, R.FAMILY_K, [len(s) for s in records], "file", 0)
    return {"dir": str(d), "fastas": fastas, "args": args, "gfa1": gfa1.stdout, "records": records, "want": want}


def test_generated_family_equals_both_oracles(family, tmp_path):
    want = family["want"]
    runs, palindrome = R.fasta_runs(family["records"], want.color_of_seq, R.FAMILY_K, 0)
    assert not palindrome, "no event holds a (k+1)-mer that is its own reverse complement"
    tsv, paf = serial(family["args"], "file", tmp_path, cwd=family["dir"])
    assert tsv == want.tsv() and paf == want.paf()
    blocks = [tuple(int(x) if i != 4 else x for i, x in enumerate(line.split("\t")[:8])) for line in tsv.decode().split("\n") if line and not line.startswith("#")]
    assert len(set(blocks)) == len(blocks) and set(blocks) == runs
    assert R.check_text(tsv, family["fastas"], cwd=family["dir"]) == len(want.blocks)


def test_the_family_holds_every_kind(family):
    """Counted on the oracle alone, so that the tests above and the device tests cannot go blind."""
    want = family["want"]
    colour = {name: c for c, name in enumerate(R.FAMILY_COLOURS)}
    assert want.n_colors == len(R.FAMILY_COLOURS) == 9 and want.labels == family["fastas"]
    lines = want.lines()
    assert any(line[4] == "-" for line in lines)
    whole = [line for line in lines if line[0] == colour["reversed"]]
    assert whole and all(line[4] == "-" for line in whole)
    assert any(len(ev) == 2 for (r, c), ev in want.count.items() if c == want.ref)
    assert want.counts_of(1, 2)
    assert want.shared[colour["unrelated"]] == [0, 0, 0, 0]
    assert len(want.blocks) >= 20
    assert any(line[8] >= 2 for line in lines)
    # the inversion shows as one reverse block between forward ones, the cut genome's blocks lie in three query sequences
    assert [line[4] for line in lines if line[0] == colour["inversion"]].count("-") >= 1
    assert len({line[5] for line in lines if line[0] == colour["cut"]}) == 3


def test_family_by_sequence_and_other_references(family, tmp_path):
    records = family["records"]
    for by, ref in (("sequence", 6), ("file", 5)):   # a third of the cut genome, the whole reverse complement
        want = R.Anchors(family["gfa1"], R.FAMILY_K, [len(s) for s in records], by, ref)
        tsv, paf = serial(family["args"], by, tmp_path, ref=ref, cwd=family["dir"])
        assert tsv == want.tsv() and paf == want.paf(), (by, ref)
        runs, _ = R.fasta_runs(records, want.color_of_seq, R.FAMILY_K, ref)
        assert {line[:8] for line in want.lines()} == runs, (by, ref)


# ------------------------------------------------------------------------------------------------ 3. small cases
@pytest.fixture(scope="module")
def few(tmp_path_factory):
    d = tmp_path_factory.mktemp("anchors_few")
    fa = R.few_events_fasta(str(d / "few.fa"))
    stream = R.oracle_stream(fa, str(d / "few.bin"), 11, 20, 5, 11)
    gfa1 = R.run_graphdump([stream, "-k", "11", "-s", fa, "-f", "gfa1"], cwd=str(d))
    assert gfa1.returncode == 0 and gfa1.stderr == b""
    return {"dir": str(d), "fa": fa, "args": [stream, "-k", "11", "-s", fa], "gfa1": gfa1.stdout, "lengths": [len(s) for _, s in R.read_fasta(fa)]}


def test_one_colour_only(few, tmp_path):
    tsv, paf = serial(few["args"], "file", tmp_path, cwd=few["dir"])
    want = R.Anchors(few["gfa1"], 11, few["lengths"], "file", 0)
    assert tsv == want.tsv() and paf == b"" and want.n_colors == 1
    text = tsv.decode()
    assert text.split("\n")[0].endswith("\tblocks=0") and "#shared" not in text and text.count("#sequence") == len(few["lengths"])


@pytest.mark.parametrize("ref", [0, 1, 3, 5])
def test_sequences_with_0_1_and_2_events(few, ref, tmp_path):
    """By sequence: records without an event (0 and 4) as the reference are a colour without events; records 3 and 5 share their head."""
    want = R.Anchors(few["gfa1"], 11, few["lengths"], "sequence", ref)
    tsv, paf = serial(few["args"], "sequence", tmp_path, ref=ref, cwd=few["dir"])
    assert tsv == want.tsv() and paf == want.paf()
    per_seq = [want.seq.count(s) for s in range(len(few["lengths"]))]
    assert per_seq == [0, 1, 1, 2, 0, 2]
    assert len(want.blocks) == (1 if ref in (3, 5) else 0)


def test_the_reference_is_the_only_colour_with_events(few, tmp_path):
    """Two files: the records above, and one whose only record has exactly k letters and so no event."""
    empty = os.path.join(few["dir"], "empty.fa")
    with open(empty, "w") as f:
        f.write(">short\nACGTTGCATGA\n")
    stream = R.streams_of([few["fa"], empty], os.path.join(few["dir"], "two.bin"), 11, 20, 5, 11)
    args = [stream, "-k", "11", "-s", few["fa"], "-s", empty]
    gfa1 = R.run_graphdump(args + ["-f", "gfa1"], cwd=few["dir"])
    assert gfa1.returncode == 0
    want = R.Anchors(gfa1.stdout, 11, few["lengths"] + [11], "file", 0)
    tsv, paf = serial(args, "file", tmp_path, cwd=few["dir"])
    assert tsv == want.tsv() and paf == b"" and want.shared[1] == [0, 0, 0, 0] and "#shared\t1\t0\t0\t0\t0\n" in tsv.decode()
    assert want.ref_edges == sum(e - b for b, e in zip(want.begin, want.end)) > 0
    # and the other way round: a reference without events
    want = R.Anchors(gfa1.stdout, 11, few["lengths"] + [11], "file", 1)
    tsv, paf = serial(args, "file", tmp_path, ref=1, cwd=few["dir"])
    assert tsv == want.tsv() and paf == b"" and want.ref_edges == 0


# ------------------------------------------------------------------------------------------------ 4. the flags
def usage_error(args, cwd):
    r = R.run_graphdump(args, cwd=cwd)
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"PARSE ERROR: "), (r.returncode, r.stderr)
    return r.stderr.decode()


def test_anchors_ref_out_of_range_is_a_usage_error(few):
    assert "(--anchors-ref)" in usage_error(few["args"] + ["--anchors", "file", "--anchors-ref", "1"], few["dir"])
    assert "(--anchors-ref)" in usage_error(few["args"] + ["--anchors", "sequence", "--anchors-ref", "6"], few["dir"])
    assert "(--anchors-ref)" in usage_error(few["args"] + ["--anchors", "sequence", "--anchors-ref", "-1"], few["dir"])
    assert "(--anchors-ref)" in usage_error(few["args"] + ["--anchors-ref", "0", "-f", "gfa1"], few["dir"])


def test_anchors_beside_other_colours_is_a_usage_error(few):
    assert "--colors sequence does not go with --anchors file" in usage_error(few["args"] + ["--anchors", "file", "--colors", "sequence"], few["dir"])
    assert "(--anchors)" in usage_error(few["args"] + ["--anchors", "file", "--links"], few["dir"])
    assert "(--anchors)" in usage_error(few["args"] + ["--anchors", "file", "-f", "gfa1"], few["dir"])
    assert "(--anchors)" in usage_error(few["args"] + ["--anchors", "genome"], few["dir"])
    assert "(--anchors-paf)" in usage_error(few["args"] + ["--anchors-paf", "x.paf", "-f", "gfa1"], few["dir"])


def test_anchors_beside_the_other_tables(family, tmp_path):
    """One walk for all: the other tables' bytes are what they are alone, the anchor table is written after them."""
    alone, _ = serial(family["args"], "file", tmp_path, cwd=family["dir"])
    out = str(tmp_path / "anchors.tsv")
    for flag in ("--colors", "--bubbles", "--superbubbles"):
        other = R.run_graphdump(family["args"] + [flag, "file"], cwd=family["dir"])
        both = R.run_graphdump(family["args"] + [flag, "file", "--anchors", "file", "--anchors-out", out], cwd=family["dir"])
        assert other.returncode == 0 and both.returncode == 0 and both.stderr == b""
        assert both.stdout == other.stdout and open(out, "rb").read() == alone, flag
