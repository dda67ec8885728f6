"""CPU: the variant table of the serial `graphdump --variants` against its definition, restated in variants_reference.py over the serial
gfa1 text (itself pinned to the real reference's sha256 by tests/golden/graphdump.json): the TSV and the VCF byte for byte on every
golden vector whose gfa1 succeeds, in both colour modes, without a reference and with every `--variants-ref c`, with the site, allele
and traversal counts; the statement from the two files and the FASTA alone; the generated input of the superbubble tests at three
bounds, a duplicated region and a hot site; the consequences of the definition; the table beside the other tables; the flags' errors
of both programs."""
import os
import subprocess

import pytest

import variants_reference as R
from helpers import GOLDEN


@pytest.fixture(scope="module", autouse=True)
def built():
    assert os.path.exists(R.GRAPHDUMP) and os.path.exists(R.TWOPACO), "run build() first"


def serial(args, by, tmp_path, ref=None, cwd=GOLDEN, more=()):
    """(table from stdout, VCF file or None) of the serial graphdump."""
    vcf = str(tmp_path / "variants.vcf")
    r = R.run_graphdump(list(args) + ["--variants", by] + ([] if ref is None else ["--variants-ref", str(ref), "--variants-vcf", vcf]) + list(more), cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    return r.stdout, None if ref is None else open(vcf, "rb").read()


# ------------------------------------------------------------------------------------------------ 1. golden vectors
# (sites, alleles, traversals), counted by the oracle; the first prefix that fits decides (a3 before the other k9).  The same in both
# colour modes: the walks do not depend on the colours.
COUNTS = (("example_", (0, 0, 0)), ("rand6_k9_a3", (13, 26, 27)), ("rand6_k9_", (43, 226, 258)), ("rand6_k25_q3", (35, 183, 193)), ("rand6_k27", (32, 166, 175)),
          ("rand6_k3", (0, 0, 0)), ("c2_k29", (29, 81, 86)), ("c2_k35", (27, 74, 78)), ("c2_k51_r2", (17, 48, 49)), ("c2_k61", (12, 33, 34)), ("c2_k125", (3, 9, 9)))


def counts_of(case):
    return [n for prefix, n in COUNTS if case.startswith(prefix)][0]


@pytest.mark.parametrize("by", ["file", "sequence"])
@pytest.mark.parametrize("v", R.GOOD_VECTORS, ids=[R.vector_id(v) for v in R.GOOD_VECTORS])
def test_serial_variants_equal_the_oracle(v, by, tmp_path):
    args = R.variants_args(v)
    none = R.golden_variants(v, by)
    cut = "_a3" in v["case"]      # an abundance cut: one name covers different bodies, the letters say nothing
    assert (none.sites(), len(none.alleles), len(none.traversals)) == counts_of(v["case"]), v["case"]
    for ref in [None] + list(range(none.n_colors)):
        want = R.golden_variants(v, by, ref)
        want.check()
        tsv, vcf = serial(args, by, tmp_path, ref)
        assert tsv == want.tsv(), (R.vector_id(v), ref)
        assert ref is None or vcf == want.vcf(), (R.vector_id(v), ref)
        alleles, records = R.check_files(tsv, vcf, want.records, cut=cut)
        assert alleles == len(want.alleles) and records == (0 if ref is None else len(want.records_of_vcf()))
        # the reference changes nothing but its own columns
        assert [a[:3] for a in want.alleles] == [a[:3] for a in none.alleles] and want.traversals == none.traversals


def test_the_golden_counts_cover_the_vectors():
    assert len(R.GOOD_VECTORS) == 38
    for prefix, n in COUNTS:
        assert [v for v in R.GOOD_VECTORS if v["case"].startswith(prefix) and counts_of(v["case"]) == n], prefix
    assert sum(1 for v in R.GOOD_VECTORS if counts_of(v["case"])[0]) >= 20


def test_consequences_on_the_golden_vectors():
    """alleles <= paths, no strays, the traversals of a site sum to its alleles' counts (Variants.check), and the simple bubbles among
    the rows have at most two alleles, with masks 1 and 2."""
    seen = 0
    for v in R.GOOD_VECTORS:
        w = R.golden_variants(v, "sequence")
        w.check()
        mine, theirs = R.simple_rows(w.sb)
        assert mine == theirs
        for b, r in enumerate(w.sb.rows):
            if (r["entrance"], r["exit"]) in mine:
                masks = [w.mask(a[0], a[2]) for a in w.alleles[w.allele_offset[b]:w.allele_offset[b + 1]]]
                assert len(masks) <= 2 and set(masks) <= {1, 2}, (R.vector_id(v), b)
                seen += len(masks)
    assert seen > 100


# ------------------------------------------------------------------------------------------------ 2. the generated inputs
@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """name -> (fasta, stream, gfa1 text, the records' letters) at k = 21: the superbubble tests' records without the hub, the
    duplicated region and the hot site."""
    d = tmp_path_factory.mktemp("variants")
    got = {}
    for name, recs in (("s11", R.superbubble_records()[:R.SB_RECORDS]), ("dup", R.duplicated_records()), ("hot", R.hot_records()), ("edge", R.edge_records())):
        fa = R.write_fasta(str(d / (name + ".fa")), recs)
        stream = R.oracle_stream(fa, str(d / (name + ".bin")), R.SB_K, R.SB_L, R.SB_Q, R.SB_SEED)
        gfa1 = R.run_graphdump([os.path.basename(stream), "-k", str(R.SB_K), "-s", os.path.basename(fa), "-f", "gfa1"], cwd=str(d))
        assert gfa1.returncode == 0 and gfa1.stderr == b""
        got[name] = (fa, stream, gfa1.stdout, [s for _, s in recs])
    return got


def oracle_of(generated, name, ref=0, max_inside=62):
    fa, stream, gfa1, records = generated[name]
    return R.Variants(gfa1, R.SB_K, [len(s) for s in records], "sequence", ref, max_inside, records=records)


def test_the_generated_input_holds_every_kind(generated):
    """On the oracle alone."""
    w = oracle_of(generated, "s11")
    w.check()
    k = w.k
    per_site = [w.allele_offset[b + 1] - w.allele_offset[b] for b in range(len(w.sb.rows))]
    assert 3 in per_site and 4 in per_site
    stop = [s for s, n in enumerate(w.seq_name) if n == "stop"][0]
    assert all(w.seq[t[0]] != stop for t in w.traversals) and any(w.seq[e] == stop for e in range(len(w.seq)))     # a colour that walks nothing
    g5 = [s for s, n in enumerate(w.seq_name) if n == "g5"][0]
    assert {t[2] for t in w.traversals if w.seq[t[0]] == g5} == {1} and {t[2] for t in w.traversals if w.seq[t[0]] != g5} == {0}
    assert any("N" in w.spelled(a[1]) for a in w.alleles)
    cluster = [b for b, r in enumerate(w.sb.rows) if r["inside"] == 62]
    assert len(cluster) == 1 and any(w.mask(t[3], t[4]) >> 61 & 1 for t in w.traversals if t[3] == cluster[0])
    assert any(w.traversals[a[1]][5] < k for a in w.alleles)                                                     # the deletion
    pairs = {(r["entrance"], r["exit"]) for r in w.sb.rows}
    nested = [(b, r) for b, r in enumerate(w.sb.rows) if any(s in r["members"] and t in r["members"] for s, t in pairs)]
    assert nested and all(per_site[b] >= 2 for b, _ in nested)
    inner = [b for b, r in enumerate(w.sb.rows) if any(r["entrance"] in o["members"] and r["exit"] in o["members"] for _, o in nested)]
    assert inner and all(per_site[b] >= 2 for b in inner)                                                          # the nested pair: two sites
    assert oracle_of(generated, "s11", max_inside=61).sb.count() == w.sb.count() - 1                               # at 61 the cluster is gone


@pytest.mark.parametrize("max_inside", [62, 8, 2])
def test_generated_variants_equal_the_oracle(generated, max_inside, tmp_path):
    fa, stream, gfa1, records = generated["s11"]
    args = [os.path.basename(stream), "-k", str(R.SB_K), "-s", os.path.basename(fa)]
    for ref in (None, 0, 5, 8):      # none, a genome, the reverse-complemented one, the one that walks nothing
        want = oracle_of(generated, "s11", ref, max_inside)
        want.check()
        tsv, vcf = serial(args, "sequence", tmp_path, ref, cwd=os.path.dirname(fa), more=["--superbubbles-max", str(max_inside)])
        assert tsv == want.tsv() and (ref is None or vcf == want.vcf()), (max_inside, ref)
        alleles, n = R.check_files(tsv, vcf, records)
        assert alleles == len(want.alleles) > 0
        assert n == (0 if ref in (None, 8) else len(want.records_of_vcf())) and (ref in (None, 8) or n > 0)
    by_bound = {62: (10, 30, 76), 8: (9, 26, 68), 2: (4, 8, 28)}
    assert (want.sites(), len(want.alleles), len(want.traversals)) == by_bound[max_inside]


def test_a_genome_that_walks_one_site_twice(generated, tmp_path):
    fa, stream, gfa1, records = generated["dup"]
    want = oracle_of(generated, "dup")
    want.check()
    assert want.sb.count() == 1 and want.ref_traversals == [2] and len(want.alleles) == 2 and [len(a[3]) for a in want.alleles] == [2, 2]
    tsv, vcf = serial([os.path.basename(stream), "-k", str(R.SB_K), "-s", os.path.basename(fa)], "sequence", tmp_path, 0, cwd=os.path.dirname(fa))
    assert tsv == want.tsv() and vcf == want.vcf()
    assert R.check_files(tsv, vcf, records) == (2, 1)
    record = vcf.decode().split("\n")[-2].split("\t")
    assert record[3:5] == ["A", "C"] and record[9:] == ["0/1", "0", "1"] and "AC=2;AN=4;NS=3" in record[7]


def test_a_hot_site(generated, tmp_path):
    fa, stream, gfa1, records = generated["hot"]
    want = oracle_of(generated, "hot")
    want.check()
    assert want.sb.count() == 1 and [len(a[3]) for a in want.alleles] == [200, 200, 200] and want.hist() == [0, 0, 0, 1]
    tsv, vcf = serial([os.path.basename(stream), "-k", str(R.SB_K), "-s", os.path.basename(fa)], "sequence", tmp_path, 0, cwd=os.path.dirname(fa))
    assert tsv == want.tsv() and vcf == want.vcf()
    assert R.check_files(tsv, vcf, records) == (3, 1)
    by_file, _ = serial([os.path.basename(stream), "-k", str(R.SB_K), "-s", os.path.basename(fa)], "file", tmp_path, 0, cwd=os.path.dirname(fa))
    assert by_file == R.Variants(gfa1, R.SB_K, [len(s) for s in records], "file", 0, records=records).tsv()


def test_walks_at_the_ends_of_their_sequences(generated, tmp_path):
    fa, stream, gfa1, records = generated["edge"]
    want = oracle_of(generated, "edge")
    want.check()
    first_of = {s: want.seq.index(s) for s in set(want.seq)}
    last_of = {s: len(want.seq) - 1 - want.seq[::-1].index(s) for s in set(want.seq)}
    assert 1 not in first_of and 0 in first_of and 2 in first_of                                  # a sequence without events between two that have some
    assert any(d == 0 and e == first_of[want.seq[e]] and x == last_of[want.seq[e]] for e, x, d, _, _, _ in want.traversals)
    assert any(d == 1 and e == last_of[want.seq[e]] and x == first_of[want.seq[e]] for e, x, d, _, _, _ in want.traversals)
    tsv, vcf = serial([os.path.basename(stream), "-k", str(R.SB_K), "-s", os.path.basename(fa)], "sequence", tmp_path, 0, cwd=os.path.dirname(fa))
    assert tsv == want.tsv() and vcf == want.vcf()
    assert R.check_files(tsv, vcf, records) == (2, 1)
    assert vcf.decode().split("\n")[-2].split("\t")[9:] == ["0", ".", "1", "0", "1"]


# ------------------------------------------------------------------------------------------------ 3. where the table goes
def test_variants_out_and_stdout(tmp_path):
    v = R.vector_of("c2_k29")
    want = R.golden_variants(v, "sequence", 1)
    out, vcf = str(tmp_path / "variants.tsv"), str(tmp_path / "v.vcf")
    r = R.run_graphdump(R.variants_args(v) + ["--variants", "sequence", "--variants-ref", "1", "--variants-out", out, "--variants-vcf", vcf])
    assert r.returncode == 0 and r.stdout == b"" and r.stderr == b""
    assert open(out, "rb").read() == want.tsv() and open(vcf, "rb").read() == want.vcf()


def test_both_files_or_neither(tmp_path):
    v = R.vector_of("c2_k29")
    vcf, nowhere = str(tmp_path / "v.vcf"), str(tmp_path / "no" / "such" / "file")
    r = R.run_graphdump(R.variants_args(v) + ["--variants", "sequence", "--variants-ref", "0", "--variants-out", nowhere, "--variants-vcf", vcf])
    assert r.returncode == 1 and r.stdout == b"" and b"variant table" in r.stderr and not os.path.exists(vcf)
    out = str(tmp_path / "variants.tsv")
    r = R.run_graphdump(R.variants_args(v) + ["--variants", "sequence", "--variants-ref", "0", "--variants-out", out, "--variants-vcf", nowhere])
    assert r.returncode == 1 and r.stdout == b"" and b"variant VCF" in r.stderr and not os.path.exists(out)
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("by", ["file", "sequence"])
def test_beside_the_other_tables(by, tmp_path):
    """One walk for all: every other table is what it is alone, the variant table comes last, wherever its flag stands."""
    v = R.vector_of("c2_k29")
    base = R.variants_args(v)
    want = R.golden_variants(v, by).tsv()
    flags = ("--colors", "--distances", "--components", "--superbubbles", "--anchors", "--classes", "--tracks")
    alone = {flag: R.run_graphdump(base + [flag, by]).stdout for flag in flags}
    for flag in flags:
        r = R.run_graphdump(base + ["--variants", by, flag, by])
        assert r.returncode == 0 and r.stderr == b"" and r.stdout == alone[flag] + want, flag
    out = str(tmp_path / "v.tsv")
    r = R.run_graphdump(base + ["--variants", by, "--variants-out", out, "--tracks", by, "--superbubbles", by, "--colors", by])
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == alone["--colors"] + alone["--superbubbles"] + alone["--tracks"] and open(out, "rb").read() == want
    # --superbubbles-max beside --variants alone, and for both tables at once
    at2 = R.golden_variants(v, by, None, 2).tsv()
    r = R.run_graphdump(base + ["--variants", by, "--superbubbles-max", "2"])
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == at2 != want
    r = R.run_graphdump(base + ["--superbubbles", by, "--variants", by, "--superbubbles-max", "2"])
    assert r.returncode == 0 and r.stdout == R.golden_superbubbles(v, by, 2).tsv() + at2
    other = "sequence" if by == "file" else "file"
    for flag, noun in (("--colors", "colour"), ("--superbubbles", "superbubble"), ("--tracks", "track")):
        r = R.run_graphdump(base + [flag, other, "--variants", by])
        assert r.returncode == 1 and r.stdout == b""
        assert r.stderr.decode().startswith("PARSE ERROR: (--variants)\n             The variant table and the %s table share one set of colours: %s %s does not go with --variants %s\n"
                                            % (noun, flag, other, by))


@pytest.mark.parametrize("case", ["edge_k5", "edge_k3"])
def test_a_failing_walk_gives_its_message_and_no_output(case, tmp_path):
    v = R.vector_of(case)
    assert v["rc"] == 1
    out, vcf = str(tmp_path / "variants.tsv"), str(tmp_path / "v.vcf")
    r = R.run_graphdump(R.variants_args(v) + ["--variants", "sequence", "--variants-ref", "0", "--variants-out", out, "--variants-vcf", vcf])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode() == v["stderr"] and not os.path.exists(out) and not os.path.exists(vcf), case


# ------------------------------------------------------------------------------------------------ 4. flag errors
def test_graphdump_flag_errors():
    base = ["rand6_k3.bin", "-k", "3", "-s", "rand6.fa"]
    r = R.run_graphdump(base + ["--variants", "xml"])
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode().startswith("PARSE ERROR: Argument: (--variants)\n             Value 'xml' does not meet constraint: file|sequence\n")
    for flag, value in (("--variants-out", "x.tsv"), ("--variants-vcf", "x.vcf"), ("--variants-ref", "0")):
        r = R.run_graphdump(base + [flag, value])
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (%s)\n             This argument needs --variants <file|sequence>\n" % flag)
        assert not os.path.exists(os.path.join(GOLDEN, value))
    # --superbubbles-max still needs one of its two tables
    r = R.run_graphdump(base + ["--superbubbles-max", "4"])
    assert r.returncode == 1 and r.stderr.decode().startswith("PARSE ERROR: (--superbubbles-max)\n             This argument needs --superbubbles <file|sequence>\n")
    r = R.run_graphdump(base + ["--variants", "file", "--variants-vcf", "x.vcf"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--variants-vcf)\n             The variant VCF needs a reference colour: --variants-ref <integer>\n")
    assert not os.path.exists(os.path.join(GOLDEN, "x.vcf"))
    r = R.run_graphdump(base + ["--variants", "file", "--variants-ref", "0", "--variants-vcf", ""])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--variants-vcf)\n             The variant VCF needs a file name\n")
    # a colour beyond the colours: one file, six sequences; in the words --anchors-ref uses
    for by, given, colours in (("file", "1", 1), ("sequence", "6", 6), ("file", "7", 1)):
        r = R.run_graphdump(base + ["--variants", by, "--variants-ref", given])
        assert r.returncode == 1 and r.stdout == b""
        assert r.stderr.decode().startswith("PARSE ERROR: Argument: (--variants-ref)\n             Value '%s' does not meet constraint: a colour index below %d\n" % (given, colours))
        theirs = R.run_graphdump(base + ["--anchors", by, "--anchors-ref", given]).stderr.decode()
        assert r.stderr.decode() == theirs.replace("--anchors-ref", "--variants-ref")
    for given in ("-1", "x", ""):
        r = R.run_graphdump(base + ["--variants", "file", "--variants-ref", given])
        assert r.returncode == 1 and r.stdout == b""
        assert r.stderr.decode().startswith("PARSE ERROR: Argument: (--variants-ref)\n             Value '%s' does not meet constraint: a colour index\n" % given)
    r = R.run_graphdump(base + ["--variants", "sequence", "--variants-ref", "5"])
    assert r.returncode == 0 and r.stderr == b"" and r.stdout.startswith(b"#twopaco-variants\t1\tby=sequence\tk=3\tcolors=6\t") and b"\tref=5\t" in r.stdout.split(b"\n")[0]
    for args in (base + ["--variants", "file", "-f", "gfa1"], base + ["-f", "gfa1", "--variants", "file"]):
        r = R.run_graphdump(args)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--variants)\n             Mutually exclusive argument already set!\n")
    for text in ("host", "device"):
        r = R.run_graphdump(base + ["--variants", "file", "--gpu", "--text", text])
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--text)\n             The variant table is formatted by the host: not with --variants\n")
    for flag, value, noun in (("--links", [], "link"), ("--bubbles", ["file"], "bubble")):
        for args in (base + ["--variants", "file", flag] + value, base + [flag] + value + ["--variants", "file"]):
            r = R.run_graphdump(args)
            assert r.returncode == 1 and r.stdout == b""
            assert r.stderr.decode().startswith("PARSE ERROR: (--variants)\n             The variant table and the %s table are written one at a time: not with %s\n" % (noun, flag))
    r = R.run_graphdump(["rand6_k3.bin", "-k", "3", "--variants", "file"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode() == "error: Required argument missing\n for arg Argument: seqfilename\n"
    r = R.run_graphdump(base + ["--variants"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("PARSE ERROR: (--variants)\n             Missing a value for this argument!\n")
    r = R.run_graphdump(["--help"])
    assert r.returncode == 0 and all(x in r.stdout for x in (b"--variants-out <file name>", b"   --variants <file|sequence>\n", b"--variants-vcf <file name>", b"--variants-ref <integer>"))


def test_twopaco_flag_errors(tmp_path):
    """The parse errors of `twopaco` that need no device."""
    def run(args):
        return subprocess.run([R.TWOPACO] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    fa = os.path.join(GOLDEN, "rand6.fa")
    for flag, value in (("--variants-out", "x.tsv"), ("--variants-vcf", "x.vcf"), ("--variants-ref", "0")):
        r = run(["-f", "20", flag, value, fa])
        assert r.returncode == 1 and r.stderr.decode() == "\nError: This argument needs --variants <file|sequence> for arg (%s)\n" % flag
    r = run(["-f", "20", "--variants", "file", "--gpus", "2", fa])
    assert r.returncode == 1
    assert r.stderr.decode() == "\nError: The variant table is written by one GPU only (every rank holds its own piece of the junction stream): not with --gpus above 1 for arg (--variants)\n"
    for flag, noun in (("--colors", "colour"), ("--bubbles", "bubble"), ("--superbubbles", "superbubble"), ("--tracks", "track")):
        for theirs, ours in (("file", "sequence"), ("sequence", "file")):
            r = run(["-f", "20", flag, theirs, "--variants", ours, fa])
            assert r.returncode == 1
            assert r.stderr.decode() == "\nError: The variant table and the %s table share one set of colours: %s %s does not go with --variants %s for arg (--variants)\n" % (
                noun, flag, theirs, ours)
    r = run(["-f", "20", "--variants", "xml", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: Value 'xml' does not meet constraint: file|sequence for arg (--variants)\n"
    r = run(["-f", "20", "--variants", "file", "--variants-vcf", "x.vcf", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: The variant VCF needs a reference colour: --variants-ref <integer> for arg (--variants-vcf)\n"
    r = run(["-f", "20", "--variants", "file", "--variants-ref", "0", "--variants-vcf", "", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: The variant VCF needs a file name for arg (--variants-vcf)\n"
    for given in ("1", "9"):
        r = run(["-f", "20", "--variants", "file", "--variants-ref", given, fa])
        assert r.returncode == 1 and r.stderr.decode() == "\nError: Value '%s' does not meet constraint: a colour index below 1 for arg (--variants-ref)\n" % given
        theirs = run(["-f", "20", "--anchors", "file", "--anchors-ref", given, fa]).stderr.decode()
        assert r.stderr.decode() == theirs.replace("--anchors-ref", "--variants-ref")
    r = run(["-f", "20", "--variants", "file", "--variants-ref", "-1", fa])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: Value '-1' does not meet constraint: a colour index for arg (--variants-ref)\n"
    assert os.listdir(str(tmp_path)) == []
    r = run(["--help"])
    assert r.returncode == 0 and b"[--variants <file|sequence>] [--variants-ref <integer>] [--variants-out <file name>] [--variants-vcf <file name>]" in r.stdout
