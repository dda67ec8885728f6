"""GPU (-m gpu): `graphdump --gpu` -- segment names, fresh names of 'N' segments and first sight computed on the device
(csrc/tpc_segments.hip, the tpc_segments_* group of include/twopaco_hip.h), the text formatted by several threads --
against the bytes the REAL reference graphdump wrote (tests/golden/graphdump.json), against the serial host walk at a size
where chunks, scans and the first-sight table matter, and the table itself against a restatement of its definition."""
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from helpers import GOLDEN, case_files, golden_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = [v for v in json.load(open(os.path.join(GOLDEN, "graphdump.json"))) if v["case"] != "cli"]
CASES = golden_cases()
SEGMENT_FORMATS = ("gfa1", "gfa2", "fasta")
CORRUPTED = "error: The input is corrupted\n"
TOO_LARGE = "error: A vertex id is too large, cannot generate GFA\n"
SEP = struct.pack("<Iq", 0xFFFFFFFF, (1 << 63) - 1)


@pytest.fixture(scope="module")
def exe():
    path = os.path.join(ROOT, "twopaco_amd", "bin", "graphdump")
    assert os.path.exists(path), "run build() first"
    return path


@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


def run(exe, args, stats=None, cwd=GOLDEN, stdout=subprocess.PIPE):
    env = dict(os.environ)
    env.pop("TWOPACO_GRAPHDUMP_STATS", None)
    if stats:
        if os.path.exists(stats):
            os.unlink(stats)
        env["TWOPACO_GRAPHDUMP_STATS"] = stats
    return subprocess.run([exe] + args, cwd=cwd, stdout=stdout, stderr=subprocess.PIPE, timeout=600, env=env)


# ------------------------------------------------------------------------------------------------ 1. the reference's bytes
@pytest.mark.parametrize("fmt", ["seq", "group", "dot", "gfa1", "gfa2", "fasta"])
def test_gpu_flag_gives_the_reference_bytes(exe, tmp_path, fmt):
    """Every vector of the real reference (all 184: a vector of seq / group / dot never opens the device, so nothing is left
    out for time) run with --gpu: exit code, stderr, stdout length and sha256 equal the reference's; for the segment formats
    the stats file proves the device path ran."""
    stats = str(tmp_path / "stats.json")
    n = 0
    for v in VECTORS:
        if v["args"][2] != fmt:
            continue
        r = run(exe, v["args"] + ["--gpu"], stats=stats)
        assert r.returncode == v["rc"], (v["args"], r.stderr)
        assert r.stderr.decode() == v["stderr"], v["args"]
        if v["rc"] == 0:
            assert len(r.stdout) == v["stdout_bytes"] and hashlib.sha256(r.stdout).hexdigest() == v["stdout_sha256"], v["args"]
            s = json.load(open(stats))
            assert s["path"] == ("device" if fmt in SEGMENT_FORMATS else "host"), v["args"]
        n += 1
    assert n >= 23


# ------------------------------------------------------------------------------------------------ 2. thread independence
@pytest.mark.parametrize("fmt", ["gfa1", "gfa2"])
def test_output_does_not_depend_on_the_thread_count(exe, tmp_path, fmt):
    v = [v for v in VECTORS if v["case"] == "c2_k29" and v["args"][2] == fmt and v["rc"] == 0][0]
    stats = str(tmp_path / "stats.json")
    outs = []
    for threads in (1, 3, 16):
        r = run(exe, v["args"] + ["--gpu", "--threads", str(threads)], stats=stats)
        assert r.returncode == 0 and r.stderr == b""
        s = json.load(open(stats))
        assert s["path"] == "device" and s["threads"] == threads
        outs.append(r.stdout)
    assert outs[0] == outs[1] == outs[2]
    assert hashlib.sha256(outs[0]).hexdigest() == v["stdout_sha256"]


# ------------------------------------------------------------------------------------------------ 3 + 6. at size
def _sha_of_run(exe, args, out_file, stats=None):
    with open(out_file, "wb") as f:
        r = run(exe, args, stats=stats, cwd=os.path.dirname(out_file), stdout=f)
    assert r.returncode == 0 and r.stderr == b"", (args, r.stderr[-400:])
    h = hashlib.sha256()
    with open(out_file, "rb") as f:
        for blk in iter(lambda: f.read(1 << 20), b""):
            h.update(blk)
    size = os.path.getsize(out_file)
    os.unlink(out_file)
    return h.hexdigest(), size


@pytest.fixture(scope="module")
def m2r2_runs(exe, tmp_path_factory):
    """synth m2r2 at scale 0.18 (62 genomes of 0.9 Mbp: repeat families, N runs, two genomes on the other strand, 7276 contigs,
    7.6 M records): bin/twopaco makes the stream, then every segment format through the serial host walk and through --gpu.
    Not scale 0.2: with this seed one of its 8092 contigs is 13 bp long, shorter than k, so the stream skips a sequence id and
    the walk -- the reference's too -- ends in "The input is corrupted"; at 0.18 the shortest contig has 43 bp."""
    d = str(tmp_path_factory.mktemp("m2r2"))
    case = {"name": "m2r2_s018", "fasta": None, "synth": {"workload": "m2r2", "seed": 12345, "scale": 0.18}}
    files = case_files(case, d)
    twopaco = os.path.join(ROOT, "twopaco_amd", "bin", "twopaco")
    out = os.path.join(d, "m2r2.bin")
    r = subprocess.run([twopaco, "-k", "25", "-f", "32", "-t", "16", "--seed", "12345", "--tmpdir", d, "-o", out] + files, capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr[-800:]
    records = os.path.getsize(out) // 12
    got = {"records": records, "formats": {}}
    seqs = []
    for f in files:
        seqs += ["-s", f]
    for fmt in SEGMENT_FORMATS:
        args = [out, "-f", fmt, "-k", "25"] + seqs
        stats = os.path.join(d, "stats_%s.json" % fmt)
        host = _sha_of_run(exe, args, os.path.join(d, "host.txt"))
        dev = _sha_of_run(exe, args + ["--gpu"], os.path.join(d, "dev.txt"), stats=stats)
        got["formats"][fmt] = {"host": host, "device": dev, "stats": json.load(open(stats))}
    for f in files:
        os.unlink(f)
    os.unlink(out)
    return got


def test_m2r2_device_equals_serial_walk(m2r2_runs):
    """A few million records: sha256 of gfa1 / gfa2 / fasta with --gpu == the serial host walk (which test 1's goldens tie to
    the real reference).  The input exercises both serial rules: 'N'-named segments and segments seen more than once."""
    assert m2r2_runs["records"] > 2_000_000
    for fmt in SEGMENT_FORMATS:
        f = m2r2_runs["formats"][fmt]
        print(fmt, f["stats"])
        assert f["device"] == f["host"] and f["host"][1] > 0, fmt
        s = f["stats"]
        assert s["path"] == "device"
        assert s["n_named"] > 0 and s["segments"] < s["events"], s
        assert s["events"] > 2_000_000 and s["threads"] == 16


def test_m2r2_footprint_has_no_filter(m2r2_runs):
    """The process holds the stream, the text, the table and a few working copies -- no Bloom filter, no partition buffers
    (8 GiB and up): peak device memory in use < 8 x (stream + text + table) + 2 GiB for the runtime and the code objects."""
    for fmt in SEGMENT_FORMATS:
        s = m2r2_runs["formats"][fmt]["stats"]
        assert s["stream_bytes"] > 0 and s["text_bytes"] > 0 and s["table_bytes"] > 0
        bound = 8 * (s["stream_bytes"] + s["text_bytes"] + s["table_bytes"]) + (2 << 30)
        print(fmt, s["device_bytes"], bound)
        assert 0 < s["device_bytes"] < bound, s


# ------------------------------------------------------------------------------------------------ 4. the table by its definition
def read_fasta(path):
    """Records as the parser gives them to graphdump: upper-cased letters, whitespace dropped."""
    recs = []
    for line in open(path):
        if line.startswith(">"):
            recs.append([])
        else:
            recs[-1].append("".join(line.split()).upper())
    return ["".join(r) for r in recs]


def read_stream(data):
    """[(sequence, pos, id, slot)] of every record: a slot is a separator when its position OR its id says so."""
    out, seq = [], 0
    for slot in range(len(data) // 12):
        pos, ident = struct.unpack_from("<Iq", data, slot * 12)
        if pos == 0xFFFFFFFF or ident == (1 << 63) - 1:
            seq += 1
        else:
            out.append((seq, pos, ident, slot))
    return out


def segment_table(data, seqs, k):
    """name[] and first[] of every event by the rule of SegmentNamer::Name / WalkSegments, restated; every event must lie inside its sequence."""
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    recs = read_stream(data)
    names, fresh = [], 1 << 34
    for (ls, lp, lid, _), (rs, rp, rid, _) in zip(recs[:-1], recs[1:]):
        if ls != rs:
            continue
        left, right = abs(lid), abs(rid)
        forward = left < right or (left == right and left > 0)
        nxt = seqs[ls][lp + k] if forward else comp.get(seqs[ls][rp - 1], "N")
        start = lid if forward else -rid
        if nxt == "N":
            names.append(fresh)
            fresh += 1
            continue
        name = "ACGT".index(nxt) if nxt in "ACGT" else -1
        if name >= 0:
            name |= (4 | abs(start) << 3) if start < 0 else start << 3
        names.append(-name if start != lid else name)   # reverse, but not between two ids of 0 (graphdump.cpp:88-91)
    seen, first = set(), []
    for n in names:
        first.append(abs(n) not in seen)
        seen.add(abs(n))
    return np.array(names, dtype=np.int64), np.array(first, dtype=bool), fresh - (1 << 34)


def ambiguous_positions(seqs, rec_start):
    return [int(rec_start[r]) + i for r, s in enumerate(seqs) for i, ch in enumerate(s) if ch not in "ACGTN"]


@pytest.mark.parametrize("name", ["tr_k25_L28", "edge_k5", "c2_k29"])
def test_segment_table_by_its_definition(capi, tmp_path, name):
    """name[] / first[] / counts through the C-ABI == the restatement above, from the golden stream's bytes; then the same
    table from the stream left RESIDENT by tpc_emit_stream after the path ran in this process."""
    case = [c for c in CASES if c["name"] == name][0]
    files = case_files(case, tmp_path)
    data = open(os.path.join(GOLDEN, case["bin"]), "rb").read()
    seqs = read_fasta(files[0])
    want_name, want_first, want_named = segment_table(data, seqs, case["k"])
    assert len(want_name) > 0
    if name == "tr_k25_L28":
        assert want_named > 0
    text = capi.PackedText.from_fasta(files)
    rec_start, rec_len = text.rec_start, text.rec_length
    assert [len(s) for s in seqs] == [int(x) for x in rec_len]
    amb = ambiguous_positions(seqs, rec_start)
    if name == "edge_k5":
        assert amb

    ctx = capi.Context(0)   # a context used for nothing else: no parameters, no filter
    ctx.seq_upload(text)
    counts = ctx.segments_build(data, case["k"], rec_start, rec_len, amb)
    # edge.fa's first sequences are shorter than k and were never dispatched: the stream steps from sequence 0 to 2, which the
    # walk reports (slot 3 holds the first record behind the two separators); the table is built all the same
    want_error = (3, "The input is corrupted") if name == "edge_k5" else None
    assert ctx.segments_error() == want_error
    got_name, got_first = ctx.segments_fetch()
    assert (got_name == want_name).all() and (got_first == want_first).all()
    assert counts["events"] == len(want_name) and counts["segments"] == int(want_first.sum()) and counts["n_named"] == want_named
    assert counts["slots"] == len(data) // 12
    # ranges
    if len(want_name) > 40:
        part_name, part_first = ctx.segments_fetch(33, 7)
        assert (part_name == want_name[33:40]).all() and (part_first == want_first[33:40]).all()
    assert ctx.kernel_ms("segments") > 0
    assert ctx.filter_words() == 0
    ctx.close()

    # resident: the whole path in this process up to tpc_emit_stream, then the table from the device's own copy of the stream
    ctx = capi.Context(0)
    ctx.set_params(case["k"], case["L"], case["q"], capi.seed_table(case["q"], case["L"], seed=case["seed"]))
    ctx.seq_upload(text)
    for st in case["rounds"]:
        ctx.filter_reset()
        ctx.pass1_insert(st["low"], st["high"])
        ctx.pass1_query(st["low"], st["high"])
        ctx.pass2_filter()
    ctx.junctions_finalize()
    ctx.emit()
    stream, _ = ctx.emit_stream(rec_start, rec_len)
    assert stream == data
    counts2 = ctx.segments_build(None, case["k"], rec_start, rec_len, amb)
    res_name, res_first = ctx.segments_fetch()
    assert ctx.segments_error() == want_error
    assert (res_name == got_name).all() and (res_first == got_first).all()
    assert {k: v for k, v in counts2.items() if k != "peak_device_bytes"} == {k: v for k, v in counts.items() if k != "peak_device_bytes"}
    ctx.close()


# ------------------------------------------------------------------------------------------------ 5. errors are findings
def _records(data):
    return read_stream(data)


def _patch(data, slot, pos=None, ident=None):
    b = bytearray(data)
    if pos is not None:
        struct.pack_into("<I", b, slot * 12, pos)
    if ident is not None:
        struct.pack_into("<q", b, slot * 12 + 4, ident)
    return bytes(b)


def _event_slots(data):
    """Slots of the right records of the events, in file order."""
    recs = _records(data)
    return [b[3] for a, b in zip(recs[:-1], recs[1:]) if a[0] == b[0]]


def _check(exe, capi, tmp_path, data, k, fasta, want_err, want_slot, label):
    """graphdump --gpu, the serial walk and the C-ABI agree on the first error of a stream."""
    path = str(tmp_path / (label + ".bin"))
    open(path, "wb").write(data)
    for fmt in SEGMENT_FORMATS:
        args = [path, "-f", fmt, "-k", str(k), "-s", fasta]
        host, dev = run(exe, args), run(exe, args + ["--gpu"])
        want_rc = 0 if want_err is None else 1
        assert host.returncode == dev.returncode == want_rc, (label, fmt, host.stderr, dev.stderr)
        assert host.stderr.decode() == dev.stderr.decode() == (want_err or ""), (label, fmt)
        if want_err is None:
            assert host.stdout == dev.stdout
    text = capi.PackedText.from_fasta([fasta])
    ctx = capi.Context(0)
    ctx.seq_upload(text)
    ctx.segments_build(data, k, text.rec_start, text.rec_length, ambiguous_positions(read_fasta(fasta), text.rec_start))
    err = ctx.segments_error()
    ctx.close()
    if want_err is None:
        assert err is None
    else:
        assert err == (want_slot, want_err[len("error: "):-1]), label


def test_errors_are_reported_as_the_serial_walk_reports_them(exe, capi, tmp_path):
    case = [c for c in CASES if c["name"] == "c2_k29"][0]
    k = case["k"]
    fasta = os.path.join(GOLDEN, case["fasta"])
    data = open(os.path.join(GOLDEN, case["bin"]), "rb").read()
    ev = _event_slots(data)
    assert len(ev) > 40
    big = 1 << 31
    early, late = ev[5], ev[30]
    _check(exe, capi, tmp_path, data, k, fasta, None, None, "untouched")
    # |id| = 2^31 in a record of an event (as its right record, then as the left record of the next pair), either sign
    _check(exe, capi, tmp_path, _patch(data, early, ident=big), k, fasta, TOO_LARGE, early, "big_right")
    _check(exe, capi, tmp_path, _patch(data, early - 1, ident=-big), k, fasta, TOO_LARGE, early - 1 if early - 1 in ev else early, "big_left")
    # ... only in a record that takes part in no event: alone in a sequence of its own behind the last one
    lone = data + SEP + struct.pack("<Iq", 0, big)
    _check(exe, capi, tmp_path, lone, k, fasta, None, None, "big_in_no_event")
    # a corrupted pair (right position not behind the left one) and a too-large id: the first in file order wins
    _check(exe, capi, tmp_path, _patch(_patch(data, early, pos=0), late, ident=big), k, fasta, CORRUPTED, early, "corrupt_then_big")
    _check(exe, capi, tmp_path, _patch(_patch(data, early, ident=big), late, pos=0), k, fasta, TOO_LARGE, early, "big_then_corrupt")
    # both in ONE pair: the corruption checks come first
    _check(exe, capi, tmp_path, _patch(data, early, pos=0, ident=big), k, fasta, CORRUPTED, early, "both_in_one_pair")
    # the other corruptions of the walk: two separators in a row, a first record that is not of sequence 0, a position past the
    # sequence's end, more sequences than the FASTA file has, trailing bytes that fill no slot (not an error)
    recs = _records(data)
    first_of_second = [r for r in recs if r[0] == 1][0][3]
    two_seps = data[:first_of_second * 12] + SEP + data[first_of_second * 12:]
    _check(exe, capi, tmp_path, two_seps, k, fasta, CORRUPTED, first_of_second + 1, "two_separators")
    _check(exe, capi, tmp_path, SEP + data, k, fasta, CORRUPTED, 1, "first_not_zero")
    _check(exe, capi, tmp_path, _patch(data, late, pos=0xFFFFFFF0), k, fasta, CORRUPTED, late, "past_the_end")
    n_seq = recs[-1][0] + 1
    extra = data + SEP + struct.pack("<Iq", 0, 5) + struct.pack("<Iq", 7, 6)
    _check(exe, capi, tmp_path, extra, k, fasta, CORRUPTED, len(data) // 12 + 2, "more_sequences_%d" % n_seq)
    _check(exe, capi, tmp_path, data + b"\x01\x02\x03\x04\x05", k, fasta, None, None, "trailing_bytes")
    _check(exe, capi, tmp_path, b"", k, fasta, None, None, "empty")


def test_bad_arguments_are_refused_with_a_text(capi):
    """What the kernels index the text with is checked before they run: a sequence outside the uploaded text and a list of
    ambiguity positions that does not ascend are errors with a text, not faults."""
    text = capi.PackedText.from_fasta([os.path.join(GOLDEN, "example.fa")])
    ctx = capi.Context(0)
    ctx.seq_upload(text)
    with pytest.raises(RuntimeError, match="segment table"):
        ctx.segments_build(b"", 11, [1 << 40], [5])   # a sequence outside the text
    with pytest.raises(RuntimeError, match="ascend"):
        ctx.segments_build(b"", 11, text.rec_start, text.rec_length, [9, 3])
    ctx.close()
