"""GENERATED TABLES for the device graph text (csrc/tpc_segtext.hip): hand-made junction streams whose ids, positions and letters decide
every name, width and body the text prints.  Builders only -- numpy, segments_reference and graph_walks; no device and none of the
project's Python.  tests/test_graph_text_reference_cpu.py runs every builder and asserts, from segments_reference.walk, that a case
holds what it is named after; tests/test_gpu_graph_text_generated.py renders them on the device against tests/graph_text_reference.py.

A name is decided by one event's two junction ids and its deciding letter (segments_reference): |name| = code | 4 (start < 0) |
|start| << 3, so event_for(name) gives the ids and the letter of any name but |name| in 4 .. 7 (a start of -0 is 0).  A sequence
without events is a sequence of ONE record: one without records makes the next record's sequence id skip one, which the walk refuses
as corrupted."""
import os

import numpy as np

import graph_text_reference as T
import graph_walks as G
import segments_reference as R

TURN = G.TURN
FRESH = R.FRESH
WINDOWS = (1, 15, 16, 17, 8191, 8192, 8193)
TILE = 8192
IUPAC = b"RYKMSWBDHV"


class TextCase(G.Case):
    """A graph_walks.Case at any k with printed sequence names; serial: the serial graphdump can read it from files()."""

    def __init__(self, name, seqs, sequences, k=G.K, names=None, data=None, serial=True, all_a=False):
        super().__init__(name, seqs, sequences, n_colors=1, data=data)
        self.k, self.serial, self.all_a = k, serial, all_a          # all_a: every letter is A (of_ids), said by the builder, checked by flat()
        self.names = [b"w%d" % i for i in range(len(seqs))] if names is None else [n.encode() if isinstance(n, str) else n for n in names]
        self._text = {}

    def files(self, directory):
        fa, stream = os.path.join(directory, self.name + ".fa"), os.path.join(directory, self.name + ".bin")
        with open(fa, "wb") as f:
            for n, s in zip(self.names, self.seqs):
                f.write(b">" + n + b"\n" + np.asarray(s, dtype=np.uint8).tobytes() + b"\n")
        with open(stream, "wb") as f:
            f.write(self.data)
        return fa, stream

    def text(self, fmt):
        return text_of(self, fmt)

    def flat(self):
        """All letters in one array.  An all-A case may hold millions of sequences: they are views of one array (case_of_ids), and that
        array is returned after a check that it is theirs and holds nothing but A."""
        if not self.all_a:
            return np.concatenate(self.seqs)
        base = self.seqs[0].base
        assert base is not None and all(s.base is base for s in (self.seqs[0], self.seqs[len(self.seqs) // 2], self.seqs[-1]))
        assert base.size == sum(map(len, self.seqs)) and (base == ord("A")).all()
        return base


def of_ids(name, groups):
    """graph_walks.case_of_ids as a TextCase: all A, the ids alone decide."""
    plain = G.case_of_ids(name, groups)
    return TextCase(name, plain.seqs, None, data=plain.data, all_a=True)


def ambiguous(c, rec_start):
    """(ascending global text positions, their letters) of the case's letters that are none of ACGTN, sequence s at rec_start[s]."""
    if c.all_a:
        return np.zeros(0, dtype=np.int64), b""
    flat = c.flat()
    return R.ambiguous_positions(c.seqs, rec_start), flat[~np.isin(flat, np.frombuffer(b"ACGTN", dtype=np.uint8))].tobytes()


def text_of(c, fmt):
    """The case's reference text in a format, built once; the formats share one table."""
    if fmt not in c._text:
        c._text[fmt] = next(iter(c._text.values())).in_format(fmt) if c._text else T.of_case(fmt, c)
    return c._text[fmt]


def event_for(name):
    """(left id, right id, forward, the raw deciding letter) of an event with this signed name; the id that is not the start is |start| + 1."""
    m = abs(name)
    assert m < 4 or m > 7
    code, mag = m & 3, m >> 3
    start = -mag if m & 4 else mag
    if name >= 0:                                          # forward: start is the left id, and the name keeps its sign
        return start, mag + 1, True, "ACGT"[code]
    return mag + 1, -start, False, "TGCA"[code]           # reversed: start is minus the right id; the letter read is complemented


def make(name, rng, specs, k=G.K, names=None, paint=(), put=(), serial=True):
    """specs: (positions, ids, length) per sequence; letters drawn from ACGT; paint = [(sequence, event, raw letter)] sets the deciding
    letter of an event, put = [(sequence, position, raw letter)] any letter."""
    seqs, sequences = [], []
    for pos, ids, length in specs:
        seqs.append(G.LETTERS[rng.integers(0, 4, length)])
        sequences.append((np.asarray(pos, dtype=np.int64), np.asarray(ids, dtype=np.int64)))
    for s, e, letter in paint:
        pos, ids = sequences[s]
        l, r = abs(int(ids[e])), abs(int(ids[e + 1]))
        forward = l < r or (l == r and l > 0)
        seqs[s][int(pos[e]) + k if forward else int(pos[e + 1]) - 1] = ord(letter)
    for s, at, letter in put:
        seqs[s][at] = letter if isinstance(letter, int) else ord(letter)
    return TextCase(name, seqs, sequences, k=k, names=names, serial=serial)


def laid(ids):
    """graph_walks.lay's layout of one walk: record i at 3 i, 3 n letters."""
    return G.GAP * np.arange(len(ids)), ids, G.GAP * len(ids)


def by_names(name, rng, targets, k=G.K, extra=()):
    """Every target name twice: as the first event of a sequence of two events (it is then the `from` of a link line) and as the second
    (the `to`); the other event's far id is 2 or 3, so no name is larger than the largest target.  extra: further specs, unpainted."""
    specs, paint = [], []
    for t in targets:
        l, r, _, letter = event_for(t)
        specs += [laid([l, r, 2]), laid([3, l, r])]
        paint += [(len(specs) - 2, 0, letter), (len(specs) - 1, 1, letter)]
    return make(name, rng, specs + list(extra), k=k, paint=paint)


# ---------------------------------------------------------------------------------------------------------------- 1. a segment named 0
def zero_cases():
    """{variant: case}: all A but for the painted letters, so the ids alone decide.  Names under the variants."""
    a = lambda name, walks, paint=(): _all_a(name, walks, paint)
    return {
        "zero_start": of_ids("zero_start", [np.arange(0, 6)]),                    # 0 8 16 24 32
        "zero_middle": a("zero_middle", [[5, 6, 0, 7, 8]]),                             # 40 -3 0 56
        "zero_twice": a("zero_twice", [[0, 9, 0, 9, 10]]),                              # 0 -3 0 72
        "zero_last": a("zero_last", [[4, 5, 0, 6]]),                                    # 32 -3 0
        "zero_two_sequences": a("zero_two_sequences", [[0, 3, 4], [7, 0, 8, 9], [0, 2]]),
        "minus_zero": a("minus_zero", [[5, 0, 3, 4], [6, 0]], [(0, 0, "T"), (0, 1, "C"), (1, 0, "T")]),   # "-0" 1 24 | "-0"
    }


def _all_a(name, walks, paint):
    specs = [laid(ids) for ids in walks]
    c = make(name, np.random.default_rng(0), specs, paint=paint)
    for s, (pos, ids, length) in enumerate(specs):
        keep = c.seqs[s].copy()
        c.seqs[s][:] = ord("A")
        for ps, e, _ in paint:
            if ps == s:
                l, r = abs(ids[e]), abs(ids[e + 1])
                at = pos[e] + c.k if (l < r or (l == r and l > 0)) else pos[e + 1] - 1
                c.seqs[s][at] = keep[at]
    return c


# ---------------------------------------------------------------------------------------------------------------- 2. every width of a name
SMALL_NAMES = [s * v for d in range(1, 9) for v in (10 ** d - 1, 10 ** d) for s in (1, -1)]      # 9, 10, 99, ... 10^8, both strands
BIG_NAMES = [s * v for v in (10 ** 9 - 1, 10 ** 9) for s in (1, -1)]


def fresh_walk(n):
    """A walk whose n events all read 'N': the names 2^34 .. 2^34 + n - 1."""
    return laid(np.arange(20, 21 + n))


def build_name_widths():
    """|name| = 10^d - 1 and 10^d for d = 1 .. 8 on both strands, 2^34 + i for i = 0 .. 104, and -1 from a forward IUPAC letter."""
    rng = np.random.default_rng(20261020)
    c = by_names("name_widths", rng, SMALL_NAMES, extra=[fresh_walk(105), laid([11, 12, 13])])
    s = len(c.seqs) - 2
    for e in range(105):
        c.seqs[s][G.GAP * e + G.K] = ord("N")
    c.seqs[s + 1][G.K] = ord("R")
    return c


def build_big_names():
    """10^9 - 1 and 10^9 on both strands (the 4 GB first-sight table), and a path that mixes them with names of 1 to 11 digits."""
    rng = np.random.default_rng(20261021)
    ids = [1, 12, 13, 125, 1250, 12500, 125000, 1250000, 12500000, 125000000, 125000001, 125000002]      # 8 id + code: 1 .. 10 digits
    c = by_names("big_names", rng, BIG_NAMES, extra=[laid(ids), laid(ids[:10][::-1])])   # reversed, id 125 000 000 would be named 10^9 + 4
    up = len(c.seqs) - 2
    for e, letter in ((0, "A"), (9, "A"), (10, "N")):                                       # 8, 10^9, a name of 11 digits
        c.seqs[up][G.GAP * e + G.K] = ord(letter)
    c.seqs[up + 1][G.GAP - 1] = ord("N")
    return c


# ---------------------------------------------------------------------------------------------------------------- 3. every width of a position
POSITION_K = 31
POSITION_LENGTH = 10 ** 7 + 200


def build_positions():
    """k = 31.  Sequence 0, 10^7 + 200 letters, ascending ids: junctions at 0, 9, 10, 99, 100, ... 9 999 999, 10 000 000 and at the
    last k-mer.  Sequence 1, as long, descending ids: junctions at 0, 10^7 + 100 and the last k-mer -- a reversed body of 10^7 + 131
    letters and a reversed event behind it.  Sequences 2 ..: one event over all of 10^d - 1 and 10^d letters, d = 2 .. 6."""
    rng = np.random.default_rng(20261022)
    k, n = POSITION_K, POSITION_LENGTH
    ladder = [0] + [v for d in range(1, 8) for v in (10 ** d - 1, 10 ** d)] + [n - k]
    specs = [(ladder, np.arange(1, len(ladder) + 1), n), ([0, 10 ** 7 + 100, n - k], [900, 800, 700], n)]
    for d in range(2, 7):
        for length in (10 ** d - 1, 10 ** d):
            specs.append(([0, length - k], [1000 + 2 * len(specs), 1001 + 2 * len(specs)], length))
    return make("positions", rng, specs, k=k)


# ---------------------------------------------------------------------------------------------------------------- 4. the fasta wrap
WRAP_SIZES = (79, 80, 81, 159, 160, 161, 240)


def build_wrap():
    """k = 3: first-sight bodies of exactly 79 .. 240 letters, sequence 1 forward (ascending ids), sequence 2 reversed; in front of them
    one body of 9000 letters, so that a tile edge can be laid on every byte behind it in all three formats."""
    rng = np.random.default_rng(20261023)
    pos = np.concatenate([[0], np.cumsum(np.array(WRAP_SIZES) - G.K)])
    n = len(pos)
    return make("wrap", rng, [([0, 9000 - G.K], [500, 501], 9000), (pos, np.arange(1, n + 1), int(pos[-1]) + G.K), (pos, np.arange(100 + n, 100, -1), int(pos[-1]) + G.K)])


# ---------------------------------------------------------------------------------------------------------------- 5. sequences
LONG_NAME = bytes(33 + i % 94 for i in range(300))         # printable, no white space, no '>' at its front


def build_sequences():
    """Sequences without events (one record) at the first place, in the middle, twice in a row and at the last place; a sequence of one
    event; printed names of 0, 1 and 300 bytes; 330 events in front of the long name, so that a tile edge can be laid on it."""
    rng = np.random.default_rng(20261024)
    walk = lambda n, base: laid(base + rng.integers(1, 40, n) * rng.choice(np.array([-1, 1]), n))
    specs = [laid([7]), walk(330, 0), laid([8]), laid([9]), walk(5, 50), walk(2, 100), walk(4, 150), laid([3])]
    names = [b"none0", b"front", b"none2", b"none3", LONG_NAME, b"", b"x", b"none7"]
    return make("sequences", rng, specs, names=names, serial=False)   # a FASTA header cannot be empty


# ---------------------------------------------------------------------------------------------------------------- 6. letters
LETTER_STEP, LETTER_SIZE = 37, 40


def build_letters(name, n_events, every, put=()):
    """k = 3, bodies of 40 letters, record i at 37 i; sequence 0 forward, sequence 1 reversed.  In both, every `every`-th body has an
    ambiguity letter at its first letter and the body before it one at its last letter (which is letter 2 of the next), and an N run
    in between; no deciding letter is touched (37 i + 3 and 37 i + 36).  put: further letters."""
    rng = np.random.default_rng(20261025 + n_events)
    pos = LETTER_STEP * np.arange(n_events + 1)
    length = int(pos[-1]) + G.K
    put = list(put)
    for s in (0, 1):
        for i in range(2, n_events, every):
            put += [(s, LETTER_STEP * i, IUPAC[(i + s) % len(IUPAC)]), (s, LETTER_STEP * i + 2, IUPAC[(i + s + 3) % len(IUPAC)])]
            put += [(s, LETTER_STEP * i + at, "N") for at in range(10, 15)]
    return make(name, rng, [(pos, np.arange(1, n_events + 2), length), (pos, np.arange(5000 + n_events, 4999, -1), length)], put=put)


def build_letters_one():
    return make("letters_one", np.random.default_rng(20261026), [laid([1, 2, 3, 4]), laid([9, 8, 7, 6])], put=[(1, 4, "Y")])


def build_letters_many():
    """And one deciding letter: event 1 of sequence 0 reads 'R' forward and is named -1."""
    return build_letters("letters_many", 520, 2, put=[(0, LETTER_STEP + G.K, "R")])


# ---------------------------------------------------------------------------------------------------------------- 7. path lines
def mixed_ids(rng, n):
    """n ids whose names have 1 to 9 digits, random strands: magnitudes 10^u for u uniform in [0, 7.09)."""
    mag = np.maximum(1, (10 ** rng.uniform(0, 7.09, n)).astype(np.int64))
    assert int(mag.max()) * 8 + 7 <= 10 ** 8
    return mag * rng.choice(np.array([-1, 1]), n)


def build_paths():
    """Sequences of 1, 2 and 3000 events over ids of every magnitude; one event in forty reads 'N' (11 digits)."""
    rng = np.random.default_rng(20261027)
    specs = [laid(mixed_ids(rng, 2)), laid(mixed_ids(rng, 3)), laid(mixed_ids(rng, 3001)), laid(mixed_ids(rng, 2))]
    specs[2][1][[100, 101, 1700, 1701]] = [12500000, 12500001, 12500000, 12500001]          # 10^8, the one name of 9 digits (reversed it would be 10^8 + 4)
    paint = [(2, e, "N") for e in range(0, 3000, 40)] + [(2, 100, "A"), (2, 1700, "A")]
    return make("paths", rng, specs, paint=paint)


# ---------------------------------------------------------------------------------------------------------------- 8. + 9. past the grid turn
def build_turn_events():
    """One sequence of TURN + 300 events: a random walk over 12 ids, and from event TURN - 1 on eight names not seen before; a second short
    sequence behind it.  All A: the ids alone decide."""
    rng = np.random.default_rng(20261028)
    ids = rng.integers(1, 13, TURN + 301) * rng.choice(np.array([-1, 1]), TURN + 301)
    ids[TURN - 1:TURN + 8] = np.arange(1001, 1010)      # ascending: events TURN - 1 .. TURN + 6 are named after them
    return of_ids("turn_events", [ids, np.array([3, 4, 5])])


def build_turn_sequences():
    """TURN + 70 sequences of one event each over 50 ids, and one without events (one record) at place TURN - 1."""
    rng = np.random.default_rng(20261029)
    n = TURN + 70
    ids = np.stack([rng.integers(1, 26, n), rng.integers(26, 51, n)], axis=1) * rng.choice(np.array([-1, 1]), (n, 2))
    ids[TURN + 3] = [2001, 2002]                       # a first sight behind the turn
    return of_ids("turn_sequences", [ids[:TURN - 1], np.array([[1]]), ids[TURN - 1:]])


BUILDERS = {"name_widths": build_name_widths, "big_names": build_big_names, "positions": build_positions, "wrap": build_wrap, "sequences": build_sequences,
            "letters_one": build_letters_one, "letters_many": build_letters_many, "paths": build_paths, "turn_events": build_turn_events,
            "turn_sequences": build_turn_sequences}
WHOLE = ("name_widths", "big_names", "wrap", "sequences", "letters_one", "letters_many", "paths")    # small enough to render whole in Python
_BUILT = {}


def case(name, keep=True):
    """Built once, shared, never changed (keep = False: for the cases of tens of megabytes)."""
    if name in _BUILT:
        return _BUILT[name]
    c = zero_cases()[name] if name in ZERO_VARIANTS else BUILDERS[name]()
    if keep:
        _BUILT[name] = c
    return c


ZERO_VARIANTS = ("zero_start", "zero_middle", "zero_twice", "zero_last", "zero_two_sequences", "minus_zero")


def cuts(total, seed=20261020, n=64):
    """A seeded cut list of [0, total]."""
    rng = np.random.default_rng(seed)
    return sorted({0, total} | {int(x) for x in rng.integers(0, total + 1, n)})
