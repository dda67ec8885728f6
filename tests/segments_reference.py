"""The EVENT TABLE of a junction stream by the walk's definition, vectorised: what csrc/tpc_segments.hip must build.

The definition is the reference's graphdump (src/graphdump/graphdump.cpp: the class Segment, :47-113, and the loop over the junction
records, :398-480; restated in twopaco_amd/host/junctiondump.cpp as SegmentNamer::Name and WalkSegments) and include/twopaco_hip.h (the
tpc_segments_* group), stated over whole arrays of 64-bit integers so that a stream of millions of events takes a second or two:

  slot      12 bytes {uint32 position, int64 id}; a SEPARATOR when its position field OR its id field holds the separator value; every
            other slot is a record of the sequence whose id is the number of separators before it
  event     two consecutive slots that are both records; begin / end = their position fields
  checks    the walk's, in file order: the first record must be of sequence 0, a record behind separators must be of the sequence after
            the previous record's ("The input is corrupted", at that record's slot); an event needs begin < end and end + k inside its
            sequence (sequences beyond the ones given are empty) -- corrupted, at the right record's slot -- and then both |id| < 2^31
            ("A vertex id is too large, cannot generate GFA")
  name      l, r = |left id|, |right id|; forward = l < r or (l == r and l > 0); the segment starts at  start = left id  when forward,
            -right id  otherwise; the deciding letter is the one behind the left k-mer (position begin + k) when forward, the complement
            of the one before the right k-mer (position end - 1) otherwise, and the complement of anything but ACGT is N.
            N: a fresh name 2^34, 2^34 + 1, ... in file order.  Another letter that is not ACGT (forward only): -1.  Otherwise
            v = code | (start < 0 ? 4 | |start| << 3 : start << 3), and the name is -v when start differs from the left id, v when not.
            (start equals the left id when forward -- and when both ids are 0, the one reverse case that keeps its sign.)
  first     no earlier event has this |name|
  An event that fails its own checks has the name 0 and takes part in first[] as such (twopaco_hip.h); its begin / end are unspecified.

Also the builder of such streams from per-sequence records, with every separator written one of three ways."""
import collections

import numpy as np

SEP_POS = 0xFFFFFFFF
SEP_ID = (1 << 63) - 1
FRESH = 1 << 34
ID_LIMIT = 1 << 31
CORRUPTED = "The input is corrupted"
TOO_LARGE = "A vertex id is too large, cannot generate GFA"
SLOT = np.dtype([("pos", "<u4"), ("id", "<i8")])   # 12 bytes, packed

Table = collections.namedtuple("Table", "name first begin end seq_event_begin n_named error")


# ---------------------------------------------------------------------------------------------------------------- the stream builder
def build_stream(sequences, separators="both", last_separator=False, filler=(7, 5)):
    """The bytes of a stream.  sequences: one entry per sequence, each a list of (pos, id) or a pair of arrays (pos[], id[]); an empty
    entry is a sequence without records.  One separator follows every sequence but the last, and the last too when last_separator.
    separators: "both" | "pos" | "id" for all, or one of them per separator written: "pos" sets the position field only and carries the
    ordinary id filler[1], "id" sets the id field only and carries the ordinary position filler[0]."""
    n_sep = len(sequences) - (0 if last_separator else 1) if sequences else 0
    kinds = [separators] * n_sep if isinstance(separators, str) else list(separators)
    assert len(kinds) == n_sep and set(kinds) <= {"both", "pos", "id"}
    parts = []
    for s, recs in enumerate(sequences):
        if isinstance(recs, tuple) and len(recs) == 2 and isinstance(recs[0], np.ndarray):
            pos, ident = recs
        else:
            pos = np.array([p for p, _ in recs], dtype=np.int64)
            ident = np.array([i for _, i in recs], dtype=np.int64)
        assert pos.size == ident.size
        assert pos.size == 0 or (0 <= int(pos.min()) and int(pos.max()) < SEP_POS and SEP_ID not in ident), "a record must not read as a separator"
        part = np.zeros(pos.size + (1 if s < n_sep else 0), dtype=SLOT)
        part["pos"][:pos.size] = pos
        part["id"][:pos.size] = ident
        if s < n_sep:
            part["pos"][-1] = filler[0] if kinds[s] == "id" else SEP_POS
            part["id"][-1] = filler[1] if kinds[s] == "pos" else SEP_ID
        parts.append(part)
    return np.concatenate(parts).tobytes() if parts else b""


def letters_of(seq):
    """A sequence as the uint8 array of its upper-case letters (str, bytes or such an array)."""
    if isinstance(seq, str):
        seq = seq.encode()
    if isinstance(seq, (bytes, bytearray)):
        return np.frombuffer(bytes(seq), dtype=np.uint8)
    return np.asarray(seq, dtype=np.uint8)


def codes_of(seq):
    """0..3 for ACGT and 4 for everything else: the records capi.PackedText.from_codes takes (a text of ACGTN only)."""
    lut = np.full(256, 4, dtype=np.uint8)
    lut[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.arange(4, dtype=np.uint8)
    return lut[letters_of(seq)]


def ambiguous_positions(seqs, rec_start):
    """Ascending global text positions of the letters that are none of ACGTN, sequence s beginning at rec_start[s]."""
    out = []
    for s, start in zip(seqs, rec_start):
        a = letters_of(s)
        out.append(int(start) + np.nonzero(~np.isin(a, np.frombuffer(b"ACGTN", dtype=np.uint8)))[0].astype(np.int64))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------- the definition
class Walk:
    """Everything the definition gives for a stream; event_table() hands out the table, the tests read the rest to prove that a case
    reaches the branch it names.  Per event, in file order (all int64 unless said):
      right_slot, seq, begin, end, left_id, right_id, ok (bool: passes its own checks), forward (bool), start, where (position of the
      deciding letter in its sequence), letter (uint8, 0 where not ok), fresh (bool), name, first (bool)"""


def walk(data, seqs, k):
    n = len(data) // 12                       # trailing bytes that fill no slot end the stream
    slots = np.frombuffer(bytes(data[:n * 12]), dtype=SLOT)
    pos, ident = slots["pos"].astype(np.int64), slots["id"].astype(np.int64)
    sep = (pos == SEP_POS) | (ident == SEP_ID)
    seq_of = np.cumsum(sep, dtype=np.int64) - sep     # separators before each slot
    n_rec = len(seqs)
    lens = np.array([len(s) for s in seqs] + [0], dtype=np.int64)            # the extra entry: every sequence beyond the given ones
    starts = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)    # in the concatenation of the letters, not the device's text
    letters = np.concatenate([letters_of(s) for s in seqs] + [np.zeros(1, dtype=np.uint8)])

    w = Walk()
    w.slots, w.n_rec, w.k = n, n_rec, k
    w.n_separators = int(sep.sum())
    rec = np.nonzero(~sep)[0]                  # the records' slots
    rec_seq = seq_of[rec]
    errors = []                                # (slot, kind) candidates; the first in file order is the walk's
    if rec.size and rec_seq[0] != 0:
        errors.append((int(rec[0]), CORRUPTED))
    step = np.nonzero((rec_seq[1:] != rec_seq[:-1]) & (rec_seq[1:] != rec_seq[:-1] + 1))[0]
    if step.size:
        errors.append((int(rec[step[0] + 1]), CORRUPTED))

    right = np.nonzero(~sep[1:] & ~sep[:-1])[0] + 1 if n > 1 else np.zeros(0, dtype=np.int64)
    left = right - 1
    w.right_slot, w.seq = right, seq_of[right]
    w.begin, w.end, w.left_id, w.right_id = pos[left], pos[right], ident[left], ident[right]
    sq = np.minimum(w.seq, n_rec)
    corrupted = (w.end <= w.begin) | (w.end + k > lens[sq])
    small = lambda x: (x > -ID_LIMIT) & (x < ID_LIMIT)   # |x| < 2^31 without taking |INT64_MIN|
    too_large = ~corrupted & ~(small(w.left_id) & small(w.right_id))
    for bad, kind in ((corrupted, CORRUPTED), (too_large, TOO_LARGE)):
        if bad.any():
            errors.append((int(right[np.argmax(bad)]), kind))
    w.error = min(errors) if errors else None
    w.ok = ~corrupted & ~too_large

    lid, rid = np.where(w.ok, w.left_id, 1), np.where(w.ok, w.right_id, 2)   # harmless stand-ins where the rule does not apply
    l, r = np.abs(lid), np.abs(rid)
    w.forward = (l < r) | ((l == r) & (l > 0))
    w.start = np.where(w.forward, lid, -rid)
    w.where = np.where(w.forward, w.begin + k, w.end - 1)
    w.letter = np.where(w.ok, letters[np.where(w.ok, starts[sq] + w.where, 0)], 0).astype(np.uint8)
    code = np.full(256, -1, dtype=np.int64)
    code[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.arange(4)
    c = code[w.letter]
    c = np.where(w.forward | (c < 0), c, 3 - c)      # the complement's code
    # N when forward; when reversed the complement of anything but ACGT
    w.fresh = w.ok & np.where(w.forward, w.letter == ord("N"), c < 0)
    w.n_named = int(w.fresh.sum())
    mag = np.abs(w.start)
    v = np.where(c < 0, 0, c) | np.where(w.start < 0, 4 | (mag << 3), w.start << 3)
    name = np.where(w.start != lid, -v, v)
    name = np.where(w.forward & (c < 0), -1, name)
    name = np.where(w.fresh, FRESH + np.cumsum(w.fresh, dtype=np.int64) - 1, name)
    w.name = np.where(w.ok, name, 0).astype(np.int64)
    w.first = np.zeros(right.size, dtype=bool)
    if right.size:
        w.first[np.unique(np.abs(w.name), return_index=True)[1]] = True
    w.seq_event_begin = np.searchsorted(w.seq, np.arange(n_rec + 1), side="left").astype(np.uint32)   # events with a sequence id < s
    plain = np.abs(w.name[~w.fresh])
    w.table_bytes = 4 * (int(plain.max() if plain.size else 0) + 1) if right.size else 0   # the direct-addressed first-sight table
    return w


def event_table(data, seqs, k):
    """Table(name int64[], first bool[], begin uint32[], end uint32[], seq_event_begin uint32[len(seqs) + 1], n_named, error): the
    arrays of graph_table.event_table, the number of 'N'-named events and the walk's first error (slot, kind) or None."""
    w = walk(data, seqs, k)
    return Table(w.name, w.first, w.begin.astype(np.uint32), w.end.astype(np.uint32), w.seq_event_begin, w.n_named, w.error)
