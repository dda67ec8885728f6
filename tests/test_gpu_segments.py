"""GPU (-m gpu): the segment and event table kernels (csrc/tpc_segments.hip) and the C-ABI's fetch paths against the walk's definition,
tests/segments_reference.py.  Integer work: exact equality throughout.

Every case is a synthetic text and a synthetic junction stream.  A sequence is drawn as its length, then strictly ascending positions
whose last + k stays inside it, then signed ids; letters are drawn, and where a case needs a letter at the position that decides an event's
name it is painted there afterwards (which event reads which position does not depend on the letters).  Each builder asserts, from the
reference alone, that the branch its case is named after occurs a stated number of times; tests/test_segments_reference_cpu.py runs every
builder and pins the reference, so the builders and their properties are checked without a device.

A case goes to a fresh Context(0): upload the text, segments_build from the stream's bytes, then every fetch path and count."""
import os
import tempfile

import numpy as np
import pytest

import segments_reference as R

pytestmark = pytest.mark.gpu

TURN = 8192 * 256                 # work items of one turn of every grid-stride loop of tpc_segments.hip (seg_grid: at most 8192 blocks of 256)
OTHER = b"RYKMSWBDHV"             # valid letters that are none of ACGTN
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
EDGE_EVENTS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 16385)
PHASE_K = (3, 25, 31, 32, 33, 93)
AMB_SIZES = (1, 2, 3, 1000)


def text_starts(lens):
    """Where host/textpack.h puts the sequences: T = N rec0 N rec1 N ..."""
    out, at = [], 1
    for n in lens:
        out.append(at)
        at += n + 1
    return out


class Case:
    """A text (seqs: the sequences the build is given), a stream (sequences: its records per sequence, which may be more than seqs) and
    the reference's walk of the two.  Never changed after it is built."""

    def __init__(self, name, k, seqs, sequences, separators="both", last_separator=True):
        self.name, self.k = name, k
        self.seqs = [R.letters_of(s).copy() for s in seqs]
        self.data = R.build_stream(sequences, separators, last_separator)
        self.w = R.walk(self.data, self.seqs, k)
        self.rec_len = [int(s.size) for s in self.seqs]
        self.rec_start = text_starts(self.rec_len)
        self.plain = all(np.isin(s, np.frombuffer(b"ACGTN", dtype=np.uint8)).all() for s in self.seqs)
        self.amb = R.ambiguous_positions(self.seqs, self.rec_start)
        self.valid = self.w.error is None

    def where_global(self):
        """Text position of every event's deciding letter (meaningless where the event fails its checks)."""
        w = self.w
        return np.asarray(self.rec_start + [0], dtype=np.int64)[np.minimum(w.seq, w.n_rec)] + w.where


def draw_sequence(rng, k, n_records, pool, spread=2):
    """(length, (pos[], id[])): the length, then ascending positions whose last + k stays inside, then signed ids out of pool."""
    length = n_records + k - 1 + int(rng.integers(0, spread * n_records + 4))
    pos = np.sort(rng.choice(length - k + 1, n_records, replace=False)).astype(np.int64)
    ids = rng.choice(np.asarray(pool, dtype=np.int64), n_records) * rng.choice(np.array([-1, 1], dtype=np.int64), n_records)
    return length, (pos, ids)


def draw_text(rng, lens, n_rate=0.0):
    out = []
    for n in lens:
        s = ACGT[rng.integers(0, 4, n)]
        s[rng.random(n) < n_rate] = ord("N")
        out.append(s)
    return out


def draw(rng, k, records_per_sequence, pool, n_rate=0.0, spread=2):
    """(seqs, sequences) of one draw per entry of records_per_sequence."""
    drawn = [draw_sequence(rng, k, n, pool, spread) for n in records_per_sequence]
    return draw_text(rng, [n for n, _ in drawn], n_rate), [r for _, r in drawn]


def is_other(letter):
    return np.isin(letter, np.frombuffer(OTHER, dtype=np.uint8))


# ---------------------------------------------------------------------------------------------------------------- the rule grid
def build_directions(name):
    """Both directions x both signs of the start x the four letters; equal ids above 0 (forward), two ids of 0 (reverse, the sign kept:
    the name is the complement's code, 0 among them), an id of 0 on one side only."""
    rng = np.random.default_rng(101)
    seqs, sequences = draw(rng, 3, rng.integers(2, 40, 14), [0, 0, 0, 1, 2, 3, 4])
    c = Case(name, 3, seqs, sequences)
    w = c.w
    assert c.valid and 100 <= w.name.size <= 600
    l, r = np.abs(w.left_id), np.abs(w.right_id)
    for forward in (True, False):
        for negative in (True, False):
            for letter in b"ACGT":
                assert int(((w.forward == forward) & ((w.start < 0) == negative) & (w.letter == letter)).sum()) >= 2, (forward, negative, letter)
    same = (l == r) & (l > 0)
    assert same.sum() >= 3 and w.forward[same].all()
    zero = (l == 0) & (r == 0)
    assert zero.sum() >= 8 and not w.forward[zero].any()
    assert set(w.name[zero].tolist()) == {0, 1, 2, 3}          # -0 is the left id: the reference does not negate these
    assert ((l == 0) & (r > 0)).sum() >= 3 and ((l > 0) & (r == 0)).sum() >= 3
    assert (w.name < 0).sum() >= 10 and (w.name > 0).sum() >= 10 and not w.fresh.any()
    return c


def build_n(name):
    """'N' at the deciding position, forward and reverse: fresh names 2^34, 2^34 + 1, ... in file order, each a first sight."""
    rng = np.random.default_rng(102)
    seqs, sequences = draw(rng, 3, rng.integers(2, 30, 10), range(1, 7), n_rate=0.15)
    c = Case(name, 3, seqs, sequences)
    w = c.w
    assert c.valid and (w.fresh & w.forward).sum() >= 3 and (w.fresh & ~w.forward).sum() >= 3
    assert (w.name[w.fresh] == R.FRESH + np.arange(w.n_named)).all() and w.first[w.fresh].all()
    assert (w.letter[w.fresh] == ord("N")).all() and (~w.fresh).sum() >= 20
    return c


def build_amb(name, n_amb):
    """Letters that are none of ACGTN: read forward the name is -1 (the amb[] search hits), read reverse a fresh name.  The list has
    n_amb entries (about, for 1000) and the hits include its first and its last one.  With 1000: 'N' at the deciding position right
    beside a listed letter -- the near misses of the search."""
    rng = np.random.default_rng(110 + n_amb)
    k = 5
    seqs, sequences = draw(rng, k, rng.integers(20, 60, 30) if n_amb > 3 else rng.integers(5, 30, 6), range(1, 9))
    c0 = Case(name, k, seqs, sequences)
    w, g = c0.w, c0.where_global()
    fwd = np.nonzero(w.forward)[0]
    lo, hi = fwd[np.argmin(g[fwd])], fwd[np.argmax(g[fwd])]
    assert g[lo] < g[hi]

    def paint(e, letter, shift=0):
        """The letter at the deciding position of event e (+ shift), if that lies strictly between the two outermost hits."""
        s, at = int(w.seq[e]), int(w.where[e]) + shift
        if 0 <= at < seqs[s].size and g[lo] < c0.rec_start[s] + at < g[hi]:
            seqs[s][at] = letter

    seqs[w.seq[lo]][w.where[lo]] = OTHER[0]
    if n_amb >= 2:
        seqs[w.seq[hi]][w.where[hi]] = OTHER[1]
    rev = [e for e in np.nonzero(~w.forward)[0] if g[lo] < g[e] < g[hi] and not (w.forward & (g == g[e])).any()]
    if n_amb == 3:
        paint(rev[len(rev) // 2], OTHER[2])
    if n_amb > 3:
        for e in rev[::7]:
            paint(e, OTHER[int(rng.integers(0, len(OTHER)))])
        inner = [e for e in fwd if g[lo] + 1 < g[e] < g[hi] - 1]
        for e in inner[::5]:
            paint(e, OTHER[int(rng.integers(0, len(OTHER)))])
        for i, e in enumerate(inner[2::5]):                     # N where the name is decided, a listed letter on one or both sides
            paint(e, ord("N"))
            if i % 3 != 0:
                paint(e, OTHER[3], -1)
            if i % 3 != 1:
                paint(e, OTHER[4], +1)
        have = int(sum(is_other(s).sum() for s in seqs))
        for s, n in enumerate(c0.rec_len):                      # fill up with listed letters anywhere between the outermost two
            at = np.nonzero((c0.rec_start[s] + np.arange(n) > g[lo]) & (c0.rec_start[s] + np.arange(n) < g[hi]) & ~is_other(seqs[s]) & (seqs[s] != ord("N")))[0]
            take = rng.choice(at, min(at.size, max(0, (1000 - have) * n // sum(c0.rec_len) + 1)), replace=False)
            seqs[s][take] = np.frombuffer(OTHER, dtype=np.uint8)[rng.integers(0, len(OTHER), take.size)]
    c = Case(name, k, seqs, sequences)
    w, g = c.w, c.where_global()
    assert c.valid and not c.plain
    assert (c.amb.size == n_amb) if n_amb <= 3 else (900 <= c.amb.size <= 1100), c.amb.size
    hit = w.forward & is_other(w.letter)
    assert hit.sum() >= (1 if n_amb <= 3 else 20) and (w.name[hit] == -1).all()
    assert c.amb[0] in g[hit] and c.amb[-1] in g[hit]
    if n_amb >= 3:
        back = ~w.forward & is_other(w.letter)
        assert back.sum() >= (1 if n_amb == 3 else 5) and w.fresh[back].all()
    if n_amb > 3:
        near = w.forward & (w.letter == ord("N")) & (np.isin(g - 1, c.amb) | np.isin(g + 1, c.amb))
        assert near.sum() >= 10 and w.fresh[near].all()
        assert (w.forward & (w.letter == ord("N")) & np.isin(g - 1, c.amb) & ~np.isin(g + 1, c.amb)).sum() >= 2
        assert (w.forward & (w.letter == ord("N")) & ~np.isin(g - 1, c.amb) & np.isin(g + 1, c.amb)).sum() >= 2
    return c


def build_strands(name, real_first):
    """One segment met on both strands (name 18 and -18), and the real name 1 (start 0, letter C) against the -1 of a letter that is
    none of ACGTN: first[] goes by magnitude, whichever comes first."""
    k = 3
    rng = np.random.default_rng(120)
    #         records                  deciding position, letter there, the name
    rows = [([(0, 2), (4, 9)], 3, "G", 18),        # forward from 2: G = 2 | 2 << 3
            ([(1, -9), (5, -2)], 4, "C", -18),     # the same segment from the other side: reverse from -(-2), the complement of C
            ([(0, 0), (3, 4)], 3, "C", 1),         # forward from 0
            ([(0, 3), (2, -3)], 3, "R", -1),       # equal ids above 0: forward; R has no code
            ([(0, 5), (3, 6)], 3, "Y", -1),
            ([(0, 0), (2, 0)], 1, "G", 1)]         # two ids of 0: reverse, the complement of G, sign kept
    if not real_first:
        rows = [rows[1], rows[0], rows[3], rows[2], rows[4], rows[5]]
    seqs = draw_text(rng, [10] * len(rows))
    for s, (_, at, letter, _) in zip(seqs, rows):
        s[at] = ord(letter)
    c = Case(name, k, seqs, [r for r, _, _, _ in rows])
    w = c.w
    assert c.valid and w.name.tolist() == [n for _, _, _, n in rows]
    assert w.first.tolist() == [True, False, True, False, False, False]
    assert (w.name[2] == 1) == real_first and (w.name[0] == 18) == real_first
    return c


def build_separators(name, last_separator):
    """Separators written three ways in one stream -- position field only (carrying an ordinary id), id field only (carrying an
    ordinary position), both -- between sequences with one record and with events; behind the last record, sequences with no record
    and shorter than k (anywhere else the walk refuses them: build_no_record) -- or, without a last separator, the stream ends in a record."""
    rng = np.random.default_rng(130)
    k = 5
    per = [int(x) for x in rng.choice([1, 1, 1, 2, 5, 20], 45)] + [6] + ([0, 0, 0, 0, 0] if last_separator else [])
    seqs, sequences = draw(rng, k, per, range(1, 12))
    for s in (-1, -3, -4) if last_separator else ():                                       # shorter than k: such a sequence can hold no record
        seqs[s] = seqs[s][:int(rng.integers(0, k))]
    n_sep = len(per) - (0 if last_separator else 1)
    kinds = [("pos", "id", "both")[int(x)] for x in rng.integers(0, 3, n_sep)]
    c = Case(name, k, seqs, sequences, kinds, last_separator)
    w = c.w
    slots = np.frombuffer(c.data, dtype=R.SLOT)
    p, i = slots["pos"] == R.SEP_POS, slots["id"] == R.SEP_ID
    assert (p & ~i).sum() >= 5 and (~p & i).sum() >= 5 and (p & i).sum() >= 5 and (p | i).sum() == n_sep == w.n_separators
    assert set(slots["id"][p & ~i].tolist()) == {5} and set(slots["pos"][~p & i].tolist()) == {7}
    assert (p | i)[-1] == last_separator
    assert c.valid and w.name.size == sum(max(n - 1, 0) for n in per) >= 50
    assert sum(n == 1 for n in per) >= 5 and sum(n == 0 for n in per) == (5 if last_separator else 0) and sum(n < k for n in c.rec_len) == (3 if last_separator else 0)
    # records on both sides of each kind of separator: read as a record, such a slot would close or open an event
    for kind in (p & ~i, ~p & i):
        at = np.nonzero(kind)[0]
        assert sum(1 for a in at if 0 < a < slots.size - 1 and not (p | i)[a - 1] and not (p | i)[a + 1]) >= 1
    return c


def build_no_record(name):
    """Sequences with no record, some of them shorter than k, between sequences with records: the walk wants every record's sequence
    to be the one after the previous record's and reports the first that is not; every event is still what the rule gives."""
    rng = np.random.default_rng(135)
    k = 5
    per = [6, 0, 4, 1, 0, 0, 9, 0, 3]
    seqs, sequences = draw(rng, k, per, range(1, 12))
    for s in (1, 5):
        seqs[s] = seqs[s][:int(rng.integers(0, k))]
    c = Case(name, k, seqs, sequences, ["pos", "id", "both", "both", "id", "pos", "both", "id", "pos"])
    w = c.w
    assert w.error == (6 + 1 + 1, R.CORRUPTED) and w.ok.all() and w.name.size == 5 + 3 + 8 + 2
    assert w.seq_event_begin.tolist() == [0, 5, 5, 8, 8, 8, 8, 16, 16, 18]
    return c


def build_more_sequences(name):
    """A thousand sequences and a stream of a few slots: seq_event_begin[] is longer than the stream."""
    rng = np.random.default_rng(140)
    k = 3
    lens = [20, 20] + [int(x) for x in rng.integers(0, 30, 998)]
    sequences = [[(0, 4), (5, -7), (9, 2)], [(2, 1), (3, 1)]]
    c = Case(name, k, draw_text(rng, lens), sequences, last_separator=False)
    w = c.w
    assert c.valid and w.slots == 6 and w.n_rec == 1000 and w.name.size == 3
    assert w.seq_event_begin.tolist() == [0, 2] + [3] * 999
    return c


def build_more_separators(name):
    """More separators than sequences: the walk's "corrupted" at the first event of a sequence beyond the given ones (a lone record
    there is no event and no error); every event before it is what the rule gives."""
    rng = np.random.default_rng(150)
    k = 3
    seqs, sequences = draw(rng, k, [8, 1, 12, 1, 4, 3], range(1, 9))
    c = Case(name, k, seqs[:3], sequences)
    w = c.w
    beyond = int(np.argmax(w.seq >= 3))
    assert w.n_separators == 6 > w.n_rec == 3
    assert w.error == (int(w.right_slot[beyond]), R.CORRUPTED) and beyond == 7 + 11 and w.seq[beyond] == 4
    assert w.ok[:beyond].all() and not w.ok[beyond:].any() and (w.name[beyond:] == 0).all() and w.name.size == beyond + 3 + 2
    assert w.seq_event_begin.tolist() == [0, 7, 7, 18]
    return c


def build_phase(name, k):
    """Deciding positions on every phase of the 32-base text word, forward and reverse, and on the other side of a word boundary."""
    rng = np.random.default_rng(160 + k)
    seqs, sequences = draw(rng, k, rng.integers(50, 120, 6), range(1, 10), n_rate=0.03)
    c = Case(name, k, seqs, sequences)
    w, g = c.w, c.where_global()
    assert c.valid and w.fresh.sum() >= 3
    assert set((g[w.forward] % 32).tolist()) == set(range(32)) == set((g[~w.forward] % 32).tolist())
    begin = np.asarray(c.rec_start, dtype=np.int64)[w.seq] + w.begin
    assert (w.forward & (g >> 5 != begin >> 5)).sum() >= 5 and (w.forward & (g >> 5 == begin >> 5)).sum() >= (5 if k < 32 else 0)
    return c


# ---------------------------------------------------------------------------------------------------------------- event-count edges
def build_edge(name, n_events, last_first):
    """n_events events in (up to) three sequences, names out of a small pool; the last event is the first sight of its name, or a
    duplicate of an event of the first sequence."""
    rng = np.random.default_rng(200 + n_events)
    k = 3
    per = [n_events + 1] if n_events < 3 else [n_events // 3 + 1, n_events // 3 + 1, n_events - 2 * (n_events // 3) + 1]
    seqs, sequences = draw(rng, k, per, range(1, max(4, n_events // 8)))
    pos, ids = sequences[-1]
    if last_first:
        ids[-2:] = (1000000, 1000001)
    else:
        w0 = R.walk(R.build_stream(sequences), seqs, k)
        j = int(np.nonzero(w0.forward[:per[0] - 1])[0][0])      # an earlier forward event of the first sequence ...
        ids[-2:] = (w0.left_id[j], w0.right_id[j])              # ... its two ids and its letter again: the same name
        seqs[-1][pos[-2] + k] = w0.letter[j]
    c = Case(name, k, seqs, sequences)
    w = c.w
    assert c.valid and w.name.size == n_events and not w.fresh.any()
    assert bool(w.first[-1]) == last_first
    assert n_events < 31 or (0 < w.first.sum() < n_events)
    return c


# ---------------------------------------------------------------------------------------------------------------- wide names
WIDE_IDS = (1 << 28, (1 << 28) + 1, 1 << 29, (1 << 29) + 5)
WIDE_TOP = 1 << 30                   # never a start: every id it is paired with is smaller


def build_wide(name):
    """Ids of 2^28 .. 2^29 + 5 in both signs: |name| crosses 2^31 and 2^32 and the first-sight table takes 16 GiB.  One event per
    sequence (records at 2 and 7 of 12 letters, k = 3: forward reads letter 5, reverse letter 6)."""
    rng = np.random.default_rng(300)
    k, big = 3, WIDE_IDS[-1]
    pairs = []                       # (left id, right id, the deciding letter or None)
    for b in WIDE_IDS:
        for sign in (1, -1):
            pairs += [(sign * b, WIDE_TOP, None), (-WIDE_TOP, sign * b, None)]
    pairs = [p for p in pairs if abs(p[0]) != big and abs(p[1]) != big]
    pairs += [(-big, WIDE_TOP, "T"),                            # forward from -(2^29 + 5), code 3: the largest name of all, once
              (-WIDE_TOP, big, "T"),                            # reverse from -(2^29 + 5) as well: the complement's code 0 keeps it smaller
              (5, 9, "G"), (big, WIDE_TOP, "G"),                # names 42 and 42 + 2^32: the same below bit 32
              (-WIDE_TOP, -big, "A")]                           # reverse from 2^29 + 5: code 3, so that |name| 42 + 2^32 is met once
    small = list(range(0, 20)) + list(WIDE_IDS[:3])
    for _ in range(300 - len(pairs)):
        a, b = (int(x) * int(s) for x, s in zip(rng.choice(small, 2), rng.choice([-1, 1], 2)))
        pairs.append((a, b, None))
    order = rng.permutation(len(pairs))
    pairs = [pairs[i] for i in order]
    seqs = draw_text(rng, [12] * len(pairs))
    for s, (a, b, letter) in zip(seqs, pairs):
        if letter:
            forward = abs(a) < abs(b) or (abs(a) == abs(b) and abs(a) > 0)
            s[5 if forward else 6] = ord(letter)
    c = Case(name, k, seqs, [[(2, a), (7, b)] for a, b, _ in pairs])
    w = c.w
    mag = np.abs(w.name)
    assert c.valid and w.name.size == 300 and not w.fresh.any()
    assert set(WIDE_IDS) | {-x for x in WIDE_IDS} <= set(w.left_id.tolist()) | set(w.right_id.tolist())
    top = 3 | 4 | big << 3
    assert mag.max() == top == (1 << 32) + 47 and (mag == top).sum() == 1 and w.table_bytes == 4 * (top + 1)
    assert ((mag >= 1 << 31) & (mag < 1 << 32)).sum() >= 8 and (mag >= 1 << 32).sum() >= 6 and (mag < 1 << 13).sum() >= 100
    a, b = np.nonzero(mag == 42)[0], np.nonzero(mag == 42 + (1 << 32))[0]
    assert (w.name[a] == 42).any() and b.size == 1 and w.name[b[0]] > 0 and w.first[a[0]] and w.first[b[0]]   # equal in their low 32 bits, both first sights
    assert (w.name < -(1 << 32)).any() and (w.name > 1 << 32).any()
    assert 0 < w.first.sum() < 300
    return c


# ---------------------------------------------------------------------------------------------------------------- beyond one grid
BIG_EVENTS = TURN + 1933             # 1933 = 30 x 64 + 13


def build_big(name):
    """A little over 2,097,152 events: every grid-stride loop of the five kernels turns over.  The first TURN events draw their ids from
    one pool; the sequences behind them add a second pool, so names of the second pool are first seen in the loops' second turn, and
    names of the first are seen first in the first turn and again in the second.  The largest |name| is the last event's alone."""
    rng = np.random.default_rng(2097)
    k = 25
    pool_a, pool_b = np.arange(1, 60), np.arange(100, 160)
    per, events = [], 0
    while events < TURN:
        n = int(rng.integers(300, 1100))
        if rng.random() < 0.01:
            n = 1                                                # a sequence without events (without a record the walk would refuse the next)
        n = min(n, TURN - events + 1)
        per.append(n)
        events += max(n - 1, 0)
    assert events == TURN
    head = len(per)
    per += [701, 1, 701, 1, BIG_EVENTS - TURN - 1400 + 1]
    drawn = [draw_sequence(rng, k, n, pool_a if s < head else np.concatenate([pool_a, pool_b]), spread=1) for s, n in enumerate(per)]
    seqs, sequences = draw_text(rng, [n for n, _ in drawn], n_rate=0.004), [r for _, r in drawn]
    pos, ids = sequences[-1]
    ids[-2:] = (-5000, 6000)                                     # forward from -5000, letter T: 7 | 5000 << 3
    seqs[-1][pos[-2] + k] = ord("T")
    c = Case(name, k, seqs, sequences)
    w = c.w
    n = w.name.size
    assert c.valid and n == BIG_EVENTS and n % 64 != 0 and n > TURN and w.slots > TURN + 3000 and 2000 <= w.n_rec <= 4000
    assert 24e6 < len(c.data) < 28e6 and 2e6 < sum(c.rec_len) < 6e6
    mag = np.abs(w.name)
    plain = np.where(w.fresh, 0, mag)
    assert plain.max() == (7 | 5000 << 3) == plain[-1] and (plain == plain[-1]).sum() == 1 and w.table_bytes == 4 * (plain[-1] + 1)
    late_first = np.nonzero(w.first & ~w.fresh)[0]
    late_first = late_first[late_first >= TURN]
    assert late_first.size >= 50                                                  # first sights in the second turn ...
    again = [e for e in late_first if (mag[e + 1:] == mag[e]).any()]
    assert len(again) >= 10                                                       # ... some of them with duplicates behind them
    early = np.unique(mag[:TURN][~w.fresh[:TURN]])
    assert np.isin(mag[TURN:], early).sum() >= 500                                # first turn's names again in the second
    assert (w.first[:TURN] & ~w.fresh[:TURN]).sum() >= 400
    for part in np.array_split(w.fresh, 16):
        assert part.sum() >= 100                                                  # 'N'-named events through the whole stream
    assert w.fresh[TURN:].sum() >= 2
    b = w.seq_event_begin.astype(np.int64)
    empty = b[1:] == b[:-1]
    assert (empty & (b[:-1] < TURN) & (b[:-1] > 0)).sum() >= 3 and (empty & (b[:-1] > TURN)).sum() >= 2
    return c


# ---------------------------------------------------------------------------------------------------------------- the cases
SPECS = {"directions_signs_letters": (build_directions, ()), "n_forward_reverse": (build_n, ()),
         "strands_real_1_first": (build_strands, (True,)), "strands_minus_1_first": (build_strands, (False,)),
         "separators_three_ways": (build_separators, (True,)), "no_last_separator": (build_separators, (False,)),
         "no_record_sequences": (build_no_record, ()), "more_sequences_than_slots": (build_more_sequences, ()), "more_separators_than_sequences": (build_more_separators, ())}
SPECS.update({"amb_%d" % n: (build_amb, (n,)) for n in AMB_SIZES})
SPECS.update({"phase_k%d" % k: (build_phase, (k,)) for k in PHASE_K})
SPECS.update({"edge_%d" % n: (build_edge, (n, i % 2 == 0)) for i, n in enumerate(EDGE_EVENTS)})
LARGE = {"wide_names": (build_wide, ()), "beyond_one_grid": (build_big, ())}
SMALL = list(SPECS)
SPECS.update(LARGE)
_BUILT = {}


def case(name):
    """Built once, shared by every test, never changed."""
    if name not in _BUILT:
        fn, args = SPECS[name]
        _BUILT[name] = fn(name, *args)
    return _BUILT[name]


def test_the_edge_cases_end_both_ways():
    firsts = [SPECS["edge_%d" % n][1][1] for n in EDGE_EVENTS]
    assert sum(firsts) == len(firsts) - sum(firsts) == 7


# ---------------------------------------------------------------------------------------------------------------- the device
@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


def packed_text(capi, c):
    """The case's text as the host packs it: from codes where it holds ACGTN only, else through a FASTA file and the parser."""
    if c.plain:
        text = capi.PackedText.from_codes([R.codes_of(s) for s in c.seqs])
    else:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, c.name + ".fa")
            with open(path, "wb") as f:
                for i, s in enumerate(c.seqs):
                    f.write(b">q%d\n" % i + s.tobytes() + b"\n")
            text = capi.PackedText.from_fasta([path])
    assert [int(x) for x in text.rec_start] == c.rec_start and [int(x) for x in text.rec_length] == c.rec_len
    return text


def built(capi, c):
    """(context, counts) of the case's table on a fresh context."""
    text = packed_text(capi, c)
    ctx = capi.Context(0)
    ctx.seq_upload(text)
    return ctx, ctx.segments_build(c.data, c.k, text.rec_start, text.rec_length, c.amb)


def check_table(ctx, counts, c):
    w = c.w
    n = w.name.size
    assert ctx.segments_error() == w.error
    name, first = ctx.segments_fetch()
    begin, end = ctx.segments_fetch_events()
    assert name.size == n and (name == w.name).all(), np.nonzero(name != w.name)[0][:10]
    assert (first == w.first).all(), np.nonzero(first != w.first)[0][:10]
    assert (begin[w.ok] == w.begin[w.ok]).all() and (end[w.ok] == w.end[w.ok]).all()
    assert (ctx.segments_fetch_sequences(0, w.n_rec + 1) == w.seq_event_begin).all()
    want = {"events": n, "segments": int(w.first.sum()), "n_named": w.n_named, "slots": w.slots, "table_bytes": w.table_bytes}
    assert {key: counts[key] for key in want} == want


@pytest.mark.parametrize("name", SMALL)
def test_table_equals_the_definition(capi, name):
    c = case(name)
    ctx, counts = built(capi, c)
    try:
        check_table(ctx, counts, c)
    finally:
        ctx.close()


@pytest.mark.parametrize("n_events", EDGE_EVENTS)
def test_ranges_off_the_word_boundaries(capi, n_events):
    """name[] / first[] / begin[] / end[] on ranges that begin and end inside the 32-bit words of first[] and inside the 64-event
    ballots, down to one event and none."""
    c = case("edge_%d" % n_events)
    w = c.w
    ctx, _ = built(capi, c)
    try:
        cuts = sorted({x for x in (0, 1, 5, 31, 32, 33, 63, 64, 65, 100, n_events - 33, n_events - 1, n_events) if 0 <= x <= n_events})
        for e0 in cuts:
            for e1 in cuts:
                if e0 <= e1:
                    name, first = ctx.segments_fetch(e0, e1 - e0)
                    begin, end = ctx.segments_fetch_events(e0, e1 - e0)
                    assert (name == w.name[e0:e1]).all() and (first == w.first[e0:e1]).all(), (e0, e1)
                    assert (begin == w.begin[e0:e1]).all() and (end == w.end[e0:e1]).all(), (e0, e1)
        with pytest.raises(RuntimeError, match="bad name range"):
            ctx.segments_fetch(1, n_events)
    finally:
        ctx.close()


def test_inner_ranges_of_the_sequence_table(capi):
    c = case("more_sequences_than_slots")
    w = c.w
    ctx, _ = built(capi, c)
    try:
        for s0, n in ((0, 1), (1, 1), (1, 3), (2, 998), (7, 500), (999, 2), (1000, 1), (1001, 0), (0, 0)):
            assert (ctx.segments_fetch_sequences(s0, n) == w.seq_event_begin[s0:s0 + n]).all(), (s0, n)
        with pytest.raises(RuntimeError, match="bad sequence range"):
            ctx.segments_fetch_sequences(1000, 2)
    finally:
        ctx.close()


def test_wide_names(capi):
    """|name| beyond 2^31 and 2^32: 64-bit name arithmetic, 64-bit table indices, the block maximum's top bits.  The first-sight
    table is 16 GiB; a build that refuses it fails here with its own text."""
    c = case("wide_names")
    ctx, counts = built(capi, c)
    try:
        check_table(ctx, counts, c)
        assert counts["table_bytes"] == 4 * ((1 << 32) + 48)
    finally:
        ctx.close()


def test_beyond_one_grid(capi):
    c = case("beyond_one_grid")
    ctx, counts = built(capi, c)
    try:
        check_table(ctx, counts, c)
        w = c.w
        name, first = ctx.segments_fetch(TURN - 70, 141)          # across the turn, off the word boundaries
        assert (name == w.name[TURN - 70:TURN + 71]).all() and (first == w.first[TURN - 70:TURN + 71]).all()
        tail = ctx.segments_fetch(BIG_EVENTS - 13, 13)
        assert (tail[0] == w.name[-13:]).all() and (tail[1] == w.first[-13:]).all()
    finally:
        ctx.close()
