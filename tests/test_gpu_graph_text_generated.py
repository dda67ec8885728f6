"""GPU (-m gpu): the device graph text (csrc/tpc_segtext.hip: k_text_size, k_text_addpath, k_text_render) on GENERATED TABLES
(tests/graph_text_cases.py) against the text by its definition (tests/graph_text_reference.py), which
tests/test_graph_text_reference_cpu.py pins to the real reference's bytes and to the serial graphdump without a device; the same file
asserts, from segments_reference.walk, that every case holds what it is named after.

The road is segments_build from the hand-made stream, segments_text_plan, segments_text_fetch; every comparison is exact: total_bytes
== the reference's size and the bytes are equal.  "The window sizes" are 1, 15, 16, 17, 8191, 8192 and 8193 bytes and a seeded cut
list; a text above 64 KiB takes the windows of one byte only over the ranges the case is about (said where it happens), all others
over the whole.  slide() lays a TILE EDGE -- 8192 bytes behind a window's first byte -- on every byte of a range, one fetch each.

  1.  a segment named 0: no L / E line behind it (the sinks' prevId_ != 0), through the C-ABI and through `graphdump --gpu --text
      device` against the bytes recorded from the real reference.  The device printed that line until this file was written.
  2.  every width of a name: 10^d - 1 and 10^d on both strands, d = 1 .. 8; 2^34 + i across 9 -> 10 and 99 -> 100; -1; and, alone in one
      test because of its 4 GB first-sight table, 10^9 - 1 and 10^9 (every other name of this file is 10^8 at most, so the paths of
      item 7 mix 1 .. 9 and 11 digits and the path of this test all of 1 .. 11)
  3.  every width of a position, size and sequence length at k = 31 in sequences of 10^7 + 200 letters, bodies of 9 and 10 million
      letters read forward and reversed, all three formats whole (22 MB each)
  4.  the fasta wrap at bodies of 79 .. 240 letters   5.  sequences without events, of one event, printed names of 0, 1 and 300 bytes
  6.  ambiguity letters   7.  path lines of 1, 2 and 3000 events   8. + 9.  past the grid turn of 8192 x 256 threads: events, sequences
  10. segments_text_write
The refusals for want of device memory stay untested: no test provokes a fault.

Measured on an MI355X: the 22 tests 26.6 s; sequences past the turn 6.9 s (6 s of it the host building, walking and packing 2 097 223
sequences one by one), path lines 4.1 s, letters 2.2 s, events past the turn 1.7 s, names 1.6 s, the wrap 1.5 s, every graphdump variant
about 1 s for its three processes, positions 0.3 s.  DESIGN.md, the device-text section, says which one-line breaks of the kernels each
case caught."""
import hashlib
import json
import os
import subprocess
import time

import numpy as np
import pytest

import graph_text_cases as X
import graph_text_reference as T
import segments_reference as R
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPHDUMP = os.path.join(ROOT, "twopaco_amd", "bin", "graphdump")
RECORD = json.load(open(os.path.join(GOLDEN, "graph_text_walks.json")))
TILE = X.TILE
GFA = ("gfa1", "gfa2")


@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


class Device:
    """A fresh context with the case's segment table; plan(fmt) -> (total_bytes, the reference Text)."""

    def __init__(self, capi, c):
        self.c, self.t0 = c, time.time()
        lens = np.array([len(s) for s in c.seqs], dtype=np.int64)
        codes = R.codes_of(c.flat())
        ends = np.cumsum(lens)
        text = capi.PackedText.from_codes([codes[a:b] for a, b in zip((ends - lens).tolist(), ends.tolist())])
        assert (text.rec_length.astype(np.int64) == lens).all()
        at, self.letters = X.ambiguous(c, text.rec_start)
        self.ctx = capi.Context(0)
        self.ctx.seq_upload(text)
        counts = self.ctx.segments_build(c.data, c.k, text.rec_start, text.rec_length, at)
        assert self.ctx.segments_error() is None and counts["events"] == c.w.name.size and counts["n_named"] == c.w.n_named
        assert counts["segments"] == int(c.w.first.sum())

    def plan(self, fmt):
        total = self.ctx.segments_text_plan(fmt, self.c.names, self.letters)
        return total, self.c.text(fmt)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()
        print("\n%s: %.2f s" % (self.c.name, time.time() - self.t0))


def whole(d, fmt):
    """total_bytes and every byte in one fetch against the reference; returns the text."""
    total, t = d.plan(fmt)
    want = t.text()
    assert total == t.total() == len(want), (d.c.name, fmt)
    got = d.ctx.segments_text_fetch(0, total)
    if got != want:
        at = next(i for i in range(min(len(got), len(want))) if got[i] != want[i])
        raise AssertionError("%s %s: first difference at byte %d: %r != %r" % (d.c.name, fmt, at, got[max(0, at - 40):at + 40], want[max(0, at - 40):at + 40]))
    return want


def windows(ctx, want, one_byte=None):
    """The window sizes over the fetched text; one_byte: the ranges of the windows of one byte (None: everywhere)."""
    total = len(want)
    for size in X.WINDOWS:
        for lo, hi in ([(0, total)] if size > 1 or one_byte is None else one_byte):
            parts = [ctx.segments_text_fetch(at, min(size, hi - at)) for at in range(lo, hi, size)]
            assert b"".join(parts) == want[lo:hi], (size, lo, hi)
    cuts = X.cuts(total)
    assert b"".join(ctx.segments_text_fetch(a, z - a) for a, z in zip(cuts[:-1], cuts[1:])) == want
    assert ctx.segments_text_fetch(total, 0) == b""


def slide(ctx, want, lo, hi):
    """A tile edge on every byte of [lo, hi): windows that begin 8192 bytes in front of it and reach 100 bytes past it; and a window
    that begins and one that ends on the byte."""
    total = len(want)
    assert TILE <= lo < hi <= total
    for p in range(lo, hi):
        a, n = p - TILE, min(TILE + 100, total - (p - TILE))
        assert ctx.segments_text_fetch(a, n) == want[a:a + n], p
        assert ctx.segments_text_fetch(p, min(100, total - p)) == want[p:p + 100], p
        assert ctx.segments_text_fetch(p - 100, 100) == want[p - 100:p], p


# ---------------------------------------------------------------------------------------------------------------- 1. a segment named 0
@pytest.mark.parametrize("name", X.ZERO_VARIANTS)
def test_a_segment_named_0(capi, name):
    """zero_start; 0 in the middle of a sequence; twice in one; as the last event; in two sequences; and "-0", a reversed event into
    junction 0.  All formats, whole and in the window sizes.  Stated on the fetched bytes as well: no link line names 0 as its `from`,
    0+ is in the path line, the S line of 0 holds the reverse complement."""
    c = X.case(name)
    with Device(capi, c) as d:
        for fmt in T.FORMATS:
            want = whole(d, fmt)
            windows(d.ctx, want)
            got = d.ctx.segments_text_fetch(0, len(want))
            assert b"L\t0\t" not in got and b"E\t0+" not in got and b"E\t0-" not in got
            e = int(np.nonzero(c.w.name == 0)[0][0])
            body = T.reverse_complement(c.seqs[int(c.w.seq[e])][int(c.w.begin[e]):int(c.w.end[e]) + c.k]).tobytes()
            if fmt == "fasta":
                assert b">0\n" + body + b"\n" in got
            else:
                assert (b"S\t0\t" + body + b"\n" if fmt == "gfa1" else b"S\t0\t6\t" + body + b"\n") in got
                paths = [line for line in got.split(b"\n") if line[:2] in (b"P\t", b"O\t")]
                assert any(b"0+" in line.replace(b"\t", b",").replace(b" ", b",").split(b",") for line in paths)


@pytest.mark.parametrize("name", X.ZERO_VARIANTS)
def test_a_segment_named_0_through_graphdump(tmp_path, name):
    """`graphdump --gpu --text device` on the case's files: stdout has the size and sha256 the REAL reference's graphdump printed,
    stderr is empty."""
    c = X.case(name)
    fa, stream = c.files(str(tmp_path))
    for fmt in T.FORMATS:
        r = subprocess.run([GRAPHDUMP, os.path.basename(stream), "-f", fmt, "-k", str(c.k), "-s", os.path.basename(fa), "--gpu", "--text", "device"],
                           cwd=str(tmp_path), capture_output=True, timeout=300)
        assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
        assert len(r.stdout) == RECORD[name][fmt]["stdout_bytes"] and hashlib.sha256(r.stdout).hexdigest() == RECORD[name][fmt]["stdout_sha256"], (name, fmt)


# ---------------------------------------------------------------------------------------------------------------- 2. every width of a name
def test_every_width_of_a_name(capi):
    with Device(capi, X.case("name_widths")) as d:
        for fmt in T.FORMATS:
            windows(d.ctx, whole(d, fmt))


def test_names_of_ten_digits(capi):
    """10^9 - 1 and 10^9 on both strands, and two paths that mix names of 1 to 11 digits: the 4 GB first-sight table."""
    c = X.case("big_names")
    with Device(capi, c) as d:
        assert d.ctx.segments_counts()["table_bytes"] >= 4 * 10 ** 9
        for fmt in T.FORMATS:
            windows(d.ctx, whole(d, fmt))


# ---------------------------------------------------------------------------------------------------------------- 3. every width of a position
def test_every_width_of_a_position(capi):
    """begin, end, size and the sequence length through every width k = 31 allows, the `$` of every kind (asserted present in the
    reference by the CPU file), bodies of 9 and 10 million letters forward and reversed: the three texts whole."""
    c = X.case("positions", keep=False)
    with Device(capi, c) as d:
        for fmt in T.FORMATS:
            want = whole(d, fmt)
            assert len(want) > 2 * 10 ** 7
            for at in (0, len(want) // 2 - 4097, len(want) - 70000):
                assert d.ctx.segments_text_fetch(at, 70000) == want[at:at + 70000]


# ---------------------------------------------------------------------------------------------------------------- 4. the fasta wrap
def test_the_fasta_wrap(capi):
    """Bodies of 79, 80, 81, 159, 160, 161 and 240 letters forward and reversed; a tile edge on every byte of each body's last line, its
    newline and the line behind it (column 79, column 80, the newline), in fasta; the window sizes in all formats."""
    c = X.case("wrap")
    with Device(capi, c) as d:
        for fmt in T.FORMATS:
            want = whole(d, fmt)
            windows(d.ctx, want)
            if fmt == "fasta":
                t = c.text(fmt)
                for e in range(1, t.events):
                    end = t.offset(e + 1)
                    last_line = (int(t.end[e]) + c.k - int(t.begin[e]) - 1) % 80 + 2
                    slide(d.ctx, want, end - last_line - 2, min(end + 6, len(want)))


# ---------------------------------------------------------------------------------------------------------------- 5. sequences
def test_sequences_without_events_and_their_names(capi):
    """Sequences without events at the first place, in the middle, twice in a row and at the last place, one of one event; printed names
    of 0, 1 and 300 bytes in C / F and P / O lines; a tile edge on every byte of the long name's first C / F line and of its path line's
    head.  (The windows of one byte: over the sequences behind the long front sequence.)"""
    c = X.case("sequences")
    with Device(capi, c) as d:
        for fmt in GFA:
            want = whole(d, fmt)
            first = want.index(X.LONG_NAME)
            windows(d.ctx, want, one_byte=[(0, 3000), (first - 100, len(want))])
            head = want.index((b"P\t" if fmt == "gfa1" else b"O\t") + X.LONG_NAME)
            slide(d.ctx, want, first - 12, first + 312)
            slide(d.ctx, want, head - 2, head + 312)
        whole(d, "fasta")


# ---------------------------------------------------------------------------------------------------------------- 6. letters
def test_ambiguity_letters(capi):
    """IUPAC letters at the first and last letter of forward bodies (printed) and reversed bodies (N), N runs, a list of one position
    and one of about 1000; a tile edge on every byte of four bodies that hold them."""
    with Device(capi, X.case("letters_one")) as d:
        assert len(d.letters) == 1
        for fmt in T.FORMATS:
            windows(d.ctx, whole(d, fmt))
    c = X.case("letters_many")
    with Device(capi, c) as d:
        assert 1000 <= len(d.letters) <= 1100
        for fmt in T.FORMATS:
            want = whole(d, fmt)
            assert any(ch in want for ch in X.IUPAC) and b"NNNNN" in want
            t = c.text(fmt)
            windows(d.ctx, want, one_byte=[(t.offset(300), t.offset(304)), (t.offset(820), t.offset(824))])
            for e in (300, 301, 820, 821):                                                      # forward and reversed first sights
                slide(d.ctx, want, t.offset(e), t.offset(e) + (60 if fmt != "fasta" else 48))


# ---------------------------------------------------------------------------------------------------------------- 7. path lines
def test_path_lines_across_tiles(capi):
    """Path lines of 1, 2 and 3000 events (three tiles and more) of names of 1 to 9 and 11 digits on both strands.  (The windows of one
    byte: over the path lines and what lies behind them.)"""
    c = X.case("paths")
    with Device(capi, c) as d:
        for fmt in GFA:
            want = whole(d, fmt)
            t = c.text(fmt)
            line = t.path_line(2)
            at = want.index(line)
            assert len(line) > 2 * TILE
            windows(d.ctx, want, one_byte=[(0, 400), (at - 50, len(want))])


# ---------------------------------------------------------------------------------------------------------------- 8. + 9. past the grid turn
def around_the_turn(d, events):
    """total_bytes == sizes()'s total; the windows of every event of `events` and of all of them together; the last 64 KiB."""
    for fmt in GFA:
        total, t = d.plan(fmt)
        per_event, want_total = t.sizes()
        assert total == want_total > 64 * 10 ** 6, fmt
        lo, hi = t.offset(events[0]), t.offset(events[-1] + 1)
        want = b"".join(t.event_bytes(e) for e in events)
        assert hi - lo == len(want) and d.ctx.segments_text_fetch(lo, hi - lo) == want, fmt
        for e in events:
            assert d.ctx.segments_text_fetch(t.offset(e), int(per_event[e])) == t.event_bytes(e), (fmt, e)
        assert d.ctx.segments_text_fetch(total - 65536, 65536) == t.tail(65536), fmt
        assert d.ctx.segments_text_fetch(0, 65536) == b"".join(t.event_bytes(e) for e in range(3000))[:65536], fmt
    total, t = d.plan("fasta")
    want = t.text()
    assert total == len(want) and d.ctx.segments_text_fetch(0, total) == want and want.count(b">") == int(d.c.w.first.sum())


def test_past_the_grid_turn_events(capi):
    """TURN + 302 events: k_text_size's second turn sizes events TURN .. -- names first seen there among them -- and the long path line
    ends the first sequence."""
    c = X.case("turn_events", keep=False)
    with Device(capi, c) as d:
        around_the_turn(d, list(range(X.TURN - 2, X.TURN + 3)))
        total, t = d.plan("gfa1")
        end = t.offset(X.TURN + 300)                                                             # the end of the long path line
        assert d.ctx.segments_text_fetch(end - 65536, 65536) == (t.event_lines(X.TURN + 299) + t.path_line(0, last_pieces=22000))[-65536:]


def test_past_the_grid_turn_sequences(capi):
    """TURN + 71 sequences, the one at place TURN - 1 without events: k_text_addpath's second turn adds the path lines of the sequences
    from TURN on."""
    c = X.case("turn_sequences", keep=False)
    with Device(capi, c) as d:
        around_the_turn(d, list(range(X.TURN - 4, X.TURN + 5)))


# ---------------------------------------------------------------------------------------------------------------- 10. segments_text_write
def test_text_write_of_generated_cases(capi, tmp_path):
    """segments_text_write with the library's window, one tile and 100 000 bytes on the path lines (gfa2); the fasta text of the
    positions, 22 MB, with the library's window."""
    for name, fmt, sizes in (("paths", "gfa2", (0, 8192, 100000)), ("positions", "fasta", (0,))):
        c = X.case(name, keep=name == "paths")
        with Device(capi, c) as d:
            total, t = d.plan(fmt)
            want = t.text()
            assert total == len(want)
            for window in sizes:
                path = str(tmp_path / ("%s_%d.txt" % (name, window)))
                with open(path, "wb") as f:
                    f.write(b"head\n")
                    f.flush()
                    assert d.ctx.segments_text_write(f.fileno(), 5, window) == total
                assert open(path, "rb").read() == b"head\n" + want, (name, window)
                os.unlink(path)
