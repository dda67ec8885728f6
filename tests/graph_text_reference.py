"""The TEXT of the compacted graph (gfa1 / gfa2 / fasta, without the header lines) by its definition, from an event table: what
csrc/tpc_segtext.hip must render.  Plain Python: integers are Python's, numbers are printed by str(), nothing is taken from the host
formatter.  The rules are those of the three sinks of twopaco_amd/host/graphformat.h (the reference's src/graphdump/graphdump.cpp):

  event      e of sequence s has the signed name nm, m = |nm|, its strand is '+' when nm >= 0 (so the strand of 0 is '+'), its junction
             positions begin < end, size = end + k - begin letters: the sequence's letters [begin, end + k) when nm > 0, and their
             reverse complement otherwise (so the body of 0 is reversed); the complement of anything but A C G T is N
  order      an event owns, in this order: its segment line when first[e]; its occurrence line; its link line when it is not the first
             event of its sequence AND the name of the event before it is not 0 (0 is the walk's "no segment yet"); and the path line of
             its sequence when it is the sequence's last event.  A sequence without events prints nothing.
  gfa1       S <m> <body> | C <m> <strand> <sequence name> + <end> | L <m'> <strand'> <m> <strand> <k>M | P <sequence name> <m><strand>,... *
  gfa2       S <m> <size> <body> | F <m> <sequence name><strand> 0 <size>$ <at(begin)> <at(end + k)> <k>M, at(p) against the length of the
             sequence | E <m'><strand'> <m><strand> <at(a0)> <at(a1)> <at(b0)> <at(b1)> <k>M, the overlapping k-mer on each segment:
             a' read forward (nm' > 0) ends with it, [size' - k, size'), otherwise it begins with it, [0, k); b read forward (nm > 0)
             begins with it, otherwise ends with it; at(p) against the segment's size | O <sequence name>p <m><strand> ...
             at(p) is p, and p followed by '$' where p equals the length it is held against
  fasta      first sights only: ><m>, then the body in lines of 80 letters (the last one shorter; none is empty)
Fields of a line are separated by tabs, the pieces of a P line by ',' and of an O line by ' '; every line ends with a newline.

Three things are offered: text() -- all of it; event_bytes(e) -- what event e owns, its sequence's path line included when it is the
last, so that a window of a huge text can be stated without building the rest (offset(e) says where it begins, tail(n) gives the last
bytes); and sizes() -- every event's byte count in numpy, digit counts by comparison against the powers of ten as uint64."""
import copy

import numpy as np

FORMATS = ("gfa1", "gfa2", "fasta")
_COMPLEMENT = np.full(256, ord("N"), dtype=np.uint8)
_COMPLEMENT[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.frombuffer(b"TGCA", dtype=np.uint8)
_P10 = np.array([10 ** d for d in range(1, 20)], dtype=np.uint64)   # 10 .. 10^19 < 2^64


def letters_of(seq):
    if isinstance(seq, str):
        seq = seq.encode()
    if isinstance(seq, (bytes, bytearray)):
        return np.frombuffer(bytes(seq), dtype=np.uint8)
    return np.asarray(seq, dtype=np.uint8)


def reverse_complement(letters):
    return _COMPLEMENT[letters[::-1]]


def digits(v):
    """Decimal digits of every entry of a non-negative integer array: 1 + the powers of ten, from 10 on, that it reaches."""
    v = np.asarray(v).astype(np.uint64)
    n = np.ones(v.shape, dtype=np.int64)
    for p in _P10:
        n += v >= p
    return n


class Text:
    """name int64[], first bool[], begin, end (positions), seq_event_begin [sequences + 1], the sequences' upper-case letters (str,
    bytes or uint8 arrays), the sequence names as they are printed (str or bytes), k."""

    def __init__(self, fmt, k, name, first, begin, end, seq_event_begin, seqs, seq_names):
        assert fmt in FORMATS
        self.fmt, self.k = fmt, int(k)
        self.name = np.asarray(name, dtype=np.int64)
        self.first = np.asarray(first, dtype=bool)
        self.begin, self.end = np.asarray(begin).astype(np.int64), np.asarray(end).astype(np.int64)
        self.seq_begin = np.asarray(seq_event_begin).astype(np.int64)
        self.seqs = [s if isinstance(s, np.ndarray) else letters_of(s) for s in seqs]      # there may be millions: arrays are taken as they are
        self.names = [n if type(n) is bytes else n.encode() if isinstance(n, str) else bytes(n) for n in seq_names]
        self.events = int(self.name.size)
        assert len(self.seqs) == len(self.names) == self.seq_begin.size - 1 and int(self.seq_begin[-1]) == self.events
        # the sequence of every event: the one whose range holds it
        self.seq_of = np.repeat(np.arange(len(self.seqs), dtype=np.int64), np.diff(self.seq_begin))
        self.name_len = np.fromiter(map(len, self.names), dtype=np.int64, count=len(self.names))
        self.seq_len = np.fromiter(map(len, self.seqs), dtype=np.int64, count=len(self.seqs))
        self._sizes = None

    def in_format(self, fmt):
        """The same table in another format, sharing the arrays."""
        assert fmt in FORMATS
        other = copy.copy(self)
        other.fmt, other._sizes = fmt, None
        return other

    # ------------------------------------------------------------------------------------------------------------ one event
    def body(self, e):
        s = int(self.seq_of[e])
        letters = letters_of(self.seqs[s])[int(self.begin[e]):int(self.end[e]) + self.k]
        return (letters if int(self.name[e]) > 0 else reverse_complement(letters)).tobytes()

    def links(self, e):
        """Whether event e prints a link line: not the first of its sequence, and not behind a segment named 0."""
        return e > int(self.seq_begin[self.seq_of[e]]) and int(self.name[e - 1]) != 0

    def path_line(self, s, last_pieces=None):
        """The P / O line of sequence s (empty for fasta and for a sequence without events); last_pieces: only that many of its last
        pieces and what follows them."""
        e0, e1 = int(self.seq_begin[s]), int(self.seq_begin[s + 1])
        if self.fmt == "fasta" or e1 == e0:
            return b""
        whole = last_pieces is None or last_pieces >= e1 - e0
        nm = self.name[e0 if whole else e1 - last_pieces:e1].tolist()
        pieces = [str(abs(x)) + ("+" if x >= 0 else "-") for x in nm]
        if self.fmt == "gfa1":
            return (b"P\t" + self.names[s] + b"\t" if whole else b"") + ",".join(pieces).encode() + b"\t*\n"
        return (b"O\t" + self.names[s] + b"p\t" if whole else b"") + " ".join(pieces).encode() + b"\n"

    def event_lines(self, e):
        """The bytes of event e but the path line."""
        k, s, nm = self.k, int(self.seq_of[e]), int(self.name[e])
        m, strand = abs(nm), "+" if nm >= 0 else "-"
        begin, end = int(self.begin[e]), int(self.end[e])
        size = end + k - begin
        if self.fmt == "fasta":
            if not self.first[e]:
                return b""
            body = self.body(e)
            return b">%d\n" % m + b"".join(body[i:i + 80] + b"\n" for i in range(0, size, 80))
        out = []
        sname = self.names[s]
        if self.fmt == "gfa1":
            if self.first[e]:
                out += [b"S\t%d\t" % m, self.body(e), b"\n"]
            out.append(b"C\t%d\t%s\t" % (m, strand.encode()) + sname + b"\t+\t%d\n" % end)
            if self.links(e):
                a = int(self.name[e - 1])
                out.append(("L\t%d\t%s\t%d\t%s\t%dM\n" % (abs(a), "+" if a >= 0 else "-", m, strand, k)).encode())
            return b"".join(out)
        at = lambda p, length: str(p) + "$" if p == length else str(p)
        total = int(self.seq_len[s])
        if self.first[e]:
            out += [b"S\t%d\t%d\t" % (m, size), self.body(e), b"\n"]
        out.append(b"F\t%d\t" % m + sname + ("%s\t0\t%d$\t%s\t%s\t%dM\n" % (strand, size, at(begin, total), at(end + k, total), k)).encode())
        if self.links(e):
            a = int(self.name[e - 1])
            a_size = int(self.end[e - 1]) + k - int(self.begin[e - 1])
            a0, a1 = (a_size - k, a_size) if a > 0 else (0, k)
            b0, b1 = (0, k) if nm > 0 else (size - k, size)
            out.append(("E\t%d%s\t%d%s\t%s\t%s\t%s\t%s\t%dM\n" % (abs(a), "+" if a >= 0 else "-", m, strand, at(a0, a_size), at(a1, a_size), at(b0, size), at(b1, size), k)).encode())
        return b"".join(out)

    def event_bytes(self, e):
        """Everything event e owns: its lines and, when it is its sequence's last event, the path line."""
        s = int(self.seq_of[e])
        lines = self.event_lines(e)
        return lines + self.path_line(s) if e + 1 == int(self.seq_begin[s + 1]) else lines

    # ------------------------------------------------------------------------------------------------------------ the whole
    def text(self):
        return b"".join(self.event_bytes(e) for e in range(self.events))

    def tail(self, n):
        """The last n bytes of the text without building it: events from the last one back; of a long path line only the pieces needed
        (a piece has 3 bytes or more)."""
        n = min(n, self.total())
        parts, have, e = [], 0, self.events
        while have < n and e > 0:
            e -= 1
            s = int(self.seq_of[e])
            if e + 1 == int(self.seq_begin[s + 1]):
                line = self.path_line(s, last_pieces=(n - have) // 3 + 1)
                parts.append(line)
                have += len(line)
                if have >= n:
                    break
            lines = self.event_lines(e)
            parts.append(lines)
            have += len(lines)
        return b"".join(reversed(parts))[-n:] if n else b""

    # ------------------------------------------------------------------------------------------------------------ sizes, vectorised
    def sizes(self):
        """(bytes of every event, path line included on a sequence's last event; their sum), int64 / int."""
        if self._sizes is not None:
            return self._sizes
        k, nm = self.k, self.name
        n = self.events
        if n == 0:
            self._sizes = (np.zeros(0, dtype=np.int64), 0)
            return self._sizes
        m = np.abs(nm)
        dm = digits(m)
        size = self.end + k - self.begin
        first = self.first.astype(np.int64)
        if self.fmt == "fasta":
            out = first * (2 + dm + size + (size + 79) // 80)
            self._sizes = (out, int(out.sum()))
            return self._sizes
        s = self.seq_of
        snl, total = self.name_len, self.seq_len[s]
        dk = int(digits(np.array([k]))[0])
        link = np.zeros(n, dtype=bool)
        link[1:] = (s[1:] == s[:-1]) & (nm[:-1] != 0)
        prev = np.concatenate([[0], np.arange(n - 1)])
        a, a_size = nm[prev], size[prev]
        if self.fmt == "gfa1":
            out = first * (dm + size + 4)                                  # S \t m \t body \n
            out += dm + snl[s] + digits(self.end) + 9                      # C \t m \t strand \t name \t + \t end \n
            out += link * (digits(np.abs(a)) + dm + dk + 10)               # L \t m' \t strand' \t m \t strand \t k M \n
            head_tail = 5                                                  # P \t name \t ... \t * \n
        else:
            at = lambda p, length: digits(p) + (p == length)
            out = first * (dm + digits(size) + size + 5)                   # S \t m \t size \t body \n
            out += dm + snl[s] + digits(size) + at(self.begin, total) + at(self.end + k, total) + dk + 13
            a0, a1 = np.where(a > 0, a_size - k, 0), np.where(a > 0, a_size, k)
            b0, b1 = np.where(nm > 0, 0, size - k), np.where(nm > 0, k, size)
            out += link * (digits(np.abs(a)) + dm + at(a0, a_size) + at(a1, a_size) + at(b0, size) + at(b1, size) + dk + 12)
            head_tail = 4                                                  # O \t name p \t ... \n
        # the path line: every piece is its digits, its strand and one separator or terminator byte
        cum = np.concatenate([[0], np.cumsum(dm + 2)])
        e0, e1 = self.seq_begin[:-1], self.seq_begin[1:]
        held = e1 > e0
        out[e1[held] - 1] += snl[held] + (cum[e1[held]] - cum[e0[held]]) + head_tail
        self._sizes = (out, int(out.sum()))
        return self._sizes

    def total(self):
        return self.sizes()[1]

    def offset(self, e):
        """Where event e begins in the text (e = events: the total)."""
        return int(self.sizes()[0][:e].sum())


def of_case(fmt, c, names=None):
    """The Text of a graph_walks.Case (or anything with w, seqs, k and, optionally, names)."""
    w = c.w
    names = names if names is not None else getattr(c, "names", None) or ["w%d" % i for i in range(len(c.seqs))]
    return Text(fmt, c.k, w.name, w.first, w.begin, w.end, w.seq_event_begin, c.seqs, names)
