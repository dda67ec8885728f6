"""The junction stream (the bytes of de_bruijn.bin) by its definition, one sequence and one marked position after the other: what
csrc/tpc_stream.hip computes with scans and slot arithmetic, stated as the reference's writer does it.  No GPU, no slot arithmetic.

The definition (reference src/graphconstructor/vertexenumerator.h:927-958, the edge worker, and src/common/junctionapi.h:118-132,
JunctionPositionWriter::WriteJunction):
  * sequences are walked in order; a sequence shorter than k emits nothing;
  * in a sequence of at least k bases the k-mer starts are walked in order.  A marked one whose id is real emits the record
    (u32 position inside the sequence, i64 id).  The first and the last k-mer emit a stub when they carry no real id -- unmarked, or
    marked with INVALID: a mark whose id is INT64_MAX is skipped -- with the ids J + 42, J + 43, ... in emission order.  A sequence of
    exactly k bases has one such k-mer;
  * the writer keeps a current sequence id, 0 at the start.  Before it writes a record of sequence c it writes one separator
    (0xFFFFFFFF, INT64_MAX) per step of that id up to c.  Nothing follows the last record.

Input contract: `marks` are global text positions (the packed text is N seq0 N seq1 N ...: sequence r starts at rec_start[r], with
rec_start[0] = 1 and rec_start[r + 1] = rec_start[r] + rec_len[r] + 1), strictly ascending, and each lies on a k-mer start of a sequence
of at least k bases: rec_start[r] <= g <= rec_start[r] + rec_len[r] - k.  The pipeline never produces anything else and the kernels do
not defend against it; write() refuses such input.

Every 12-byte slot is annotated with its kind, its sequence, its position field and the text position that owns it: a record or a stub
is owned by its k-mer's position, the separator that steps the writer from j to j + 1 (annotated with sequence j) by the separator
character in front of sequence j + 1, rec_start[j + 1] - 1.  shard() derives everything the ranks of a sharded run exchange by counting
annotated slots per chunk of text positions."""
import numpy as np

INVALID = (1 << 63) - 1        # INVALID_VERTEX
SEPARATOR_POS = 0xFFFFFFFF
FIRST_STUB = 42                # the first stub id is J + 42
UINT64_MAX = (1 << 64) - 1

RECORD, STUB_FIRST, STUB_LAST, SEPARATOR = 0, 1, 2, 3
KIND_NAMES = ("record", "stub-first", "stub-last", "separator")
SLOT = np.dtype([("pos", "<u4"), ("id", "<i8")])
assert SLOT.itemsize == 12


def rec_starts(rec_len):
    """Global text position of the first base of every sequence: the text is N seq0 N seq1 N ..."""
    out, at = [], 1
    for n in rec_len:
        out.append(at)
        at += int(n) + 1
    return out


class Stream:
    """bytes: the file; pos / id: the two fields of every slot; kind / seq / owner: the annotation of every slot."""

    def __init__(self, k, J, rec_start, rec_len, pos, ids, kind, seq, owner):
        self.k, self.J = k, J
        self.rec_start, self.rec_len = list(rec_start), list(rec_len)
        slots = np.zeros(len(pos), dtype=SLOT)
        slots["pos"], slots["id"] = pos, ids
        self.pos = np.asarray(pos, dtype=np.uint32)
        self.id = np.asarray(ids, dtype=np.int64)
        self.kind = np.asarray(kind, dtype=np.uint8)
        self.seq = np.asarray(seq, dtype=np.int64)
        self.owner = np.asarray(owner, dtype=np.uint64)
        self.bytes = slots.tobytes()
        self.n_slots = len(pos)
        self.n_records = int(np.count_nonzero(self.kind != SEPARATOR))   # "True marks count": junction occurrences + stubs

    def records(self):
        """[(pos, id)] of every slot, separators included: what a hand-written expectation lists."""
        return list(zip(self.pos.tolist(), self.id.tolist()))


def write(k, J, rec_len, marks, ids, rec_start=None):
    """The stream of the sequences of rec_len under the marks (ascending global positions) and their ids; see the module's docstring."""
    rec_len = [int(x) for x in rec_len]
    rec_start = rec_starts(rec_len) if rec_start is None else [int(x) for x in rec_start]
    marks = np.asarray(marks, dtype=np.uint64).tolist()
    ids = np.asarray(ids, dtype=np.int64).tolist()
    if len(marks) != len(ids):
        raise ValueError("one id per mark")
    out_pos, out_id, kind, seq, owner = [], [], [], [], []
    state = {"now": 0, "stub": J + FIRST_STUB}

    def put(c, position, jid, what):           # JunctionPositionWriter::WriteJunction
        while state["now"] < c:
            out_pos.append(SEPARATOR_POS), out_id.append(INVALID), kind.append(SEPARATOR), seq.append(state["now"])
            owner.append(rec_start[state["now"] + 1] - 1)
            state["now"] += 1
        out_pos.append(position), out_id.append(jid), kind.append(what), seq.append(c), owner.append(rec_start[c] + position)

    def stub(c, position, what):
        put(c, position, state["stub"], what)
        state["stub"] += 1

    m, n_marks, before = 0, len(marks), -1
    for c, (first, length) in enumerate(zip(rec_start, rec_len)):
        if length < k:
            continue
        last = first + length - k
        if m < n_marks and marks[m] < first:
            raise ValueError("mark %d lies on no k-mer start of a sequence of at least k bases" % marks[m])
        first_done = last_done = False
        while m < n_marks and marks[m] <= last:  # the marked k-mer starts of sequence c, in order
            g, jid = marks[m], ids[m]
            if g <= before:
                raise ValueError("marks are not strictly ascending at %d" % g)
            before = g
            m += 1
            if jid == INVALID:
                continue
            if g != first and not first_done:
                stub(c, 0, STUB_FIRST)
            first_done = True
            put(c, g - first, jid, RECORD)
            last_done = g == last
        if not first_done:
            stub(c, 0, STUB_FIRST)
            last_done = last == first
        if not last_done:
            stub(c, length - k, STUB_LAST)
    if m < n_marks:
        raise ValueError("mark %d lies on no k-mer start of a sequence of at least k bases" % marks[m])
    return Stream(k, J, rec_start, rec_len, out_pos, out_id, kind, seq, owner)


def chunks_of(cuts):
    """[lo, hi) of every rank for W - 1 ascending cuts: rank 0 starts at 0, the last rank's end is UINT64_MAX."""
    cuts = [int(c) for c in cuts]
    if sorted(cuts) != cuts:
        raise ValueError("cuts ascend")
    return list(zip([0] + cuts, cuts + [UINT64_MAX]))


def shard(s, cuts):
    """What the ranks of a run cut at `cuts` exchange, counted from the annotated slots of Stream s alone.  Returns a dict:
       chunks            [lo, hi) of every rank
       cnt[r], flags[r]  per sequence: the real-id records owned by rank r's chunk; bit 0 / 1: the record of the first / last k-mer is one of them
       gflags            per sequence: the OR of the ranks' flags, | 4 when the sequence has any slot of its own (it has at least k bases)
       e_scan, s_scan    per sequence and one more: the records + stubs / the stubs of the sequences before it
       r_last            the sequence of the last slot (0 for an empty stream)
       before[r]         per sequence: its real-id records owned by positions in front of rank r's chunk
       slot0[r], n_slots[r]   the slots owned by positions in front of rank r's chunk / inside it"""
    n = len(s.rec_len)
    own = s.kind != SEPARATOR
    rec = s.kind == RECORD
    last_pos = np.array([max(length - s.k, 0) for length in s.rec_len], dtype=np.int64)
    is_first = rec & (s.pos == 0)
    is_last = rec & (s.pos.astype(np.int64) == last_pos[s.seq])

    def per_seq(mask):
        return np.bincount(s.seq[mask], minlength=n).astype(np.uint64)

    out = {"chunks": chunks_of(cuts), "cnt": [], "flags": [], "before": [], "slot0": [], "n_slots": []}
    for lo, hi in out["chunks"]:
        inside = (s.owner >= np.uint64(lo)) & (s.owner < np.uint64(hi))
        front = s.owner < np.uint64(lo)
        out["cnt"].append(per_seq(rec & inside))
        out["flags"].append(((per_seq(is_first & inside) > 0).astype(np.uint32) | ((per_seq(is_last & inside) > 0).astype(np.uint32) << 1)))
        out["before"].append(per_seq(rec & front))
        out["slot0"].append(int(np.count_nonzero(front)))
        out["n_slots"].append(int(np.count_nonzero(inside)))
    gflags = np.zeros(n, dtype=np.uint32)
    for f in out["flags"]:
        gflags |= f
    gflags |= (per_seq(own) > 0).astype(np.uint32) << 2
    out["gflags"] = gflags
    out["e_scan"] = np.concatenate([[0], np.cumsum(per_seq(own))]).astype(np.uint64)
    out["s_scan"] = np.concatenate([[0], np.cumsum(per_seq((s.kind == STUB_FIRST) | (s.kind == STUB_LAST)))]).astype(np.uint64)
    out["r_last"] = int(s.seq[-1]) if s.n_slots else 0
    return out


def parse(data, n_real):
    """The real-id records of a stream's bytes: [(sequence, position, id)] of the slots with |id| <= n_real, which leaves out stubs and
    separators (a slot is a separator when either field holds the separator's value, junctionapi.h:94)."""
    slots = np.frombuffer(data, dtype=SLOT)
    sep = (slots["pos"] == SEPARATOR_POS) | (slots["id"] == INVALID)
    seq = np.cumsum(sep)
    real = ~sep & (np.abs(slots["id"]) <= n_real)
    return list(zip(seq[real].tolist(), slots["pos"][real].tolist(), slots["id"][real].tolist()))
