"""The oracle of the EDGE INDEX and of LOCATE (include/twopaco_hip.h, the tpc_segments_edges_* / tpc_segments_locate_* groups), not
through the project's locate code: the definition over graph_table.event_table and the letters of the sequences, with plain dicts of
canonical strings.

  n = k + 1; T = N rec0 N rec1 N ... with every letter other than ACGT an N; a window is valid when it holds no N.
  ROWS    the events whose first bit is set, in event order; the span of row r is T[g0, g0 + end - begin), g0 = rec_start[seq] + begin.
  INDEX   canon(window) -> (g, row) for every span position with a valid window, the SMALLEST g kept, the others duplicates, span
          positions with an invalid window skipped.
  QUERY   a text packed like T; every position p with p + n <= |Q| is invalid, absent or a hit (g, row, rev), rev = 0 when the
          window equals T's letter for letter.
  RUNS    a hit continues the one before it when both lie in one row on one strand at offsets that step by + 1 (forward) or - 1.
  SUMS    per record windows, found, forward, runs and, with colours, shared[record][colour].
The arrays are encoded as the device encodes them (hit all ones = invalid, all ones - 1 = absent, else rev << 63 | g)."""
import numpy as np

import graph_table

INVALID = (1 << 64) - 1
ABSENT = (1 << 64) - 2
ROW_INVALID = 0xFFFFFFFF
ROW_ABSENT = 0xFFFFFFFE
_COMP = str.maketrans("ACGT", "TGCA")

# entries, duplicates, skipped of the golden vectors' index: the definition above evaluated once by Index below, pinned here so that a
# change of the oracle itself shows
RECORDED = {"edge_k5": (75, 6, 62), "edge_k3": (51, 2, 23), "rand6_k9_fp": (7168, 1, 170), "rand6_k3": (136, 2, 68), "tr_k25_L28": (36838, 1, 312),
            "tr_k11_L28_r2": (31775, 15, 144), "tr_k31_L30_q3": (38855, 33, 384), "c2_k29": (4705, 0, 90), "rand6_k9_a3": (6340, 6396, 140),
            "wd_k93_a3": (6562, 3427, 0)}


def revcomp(s):
    return s.translate(_COMP)[::-1]


def canon(s):
    r = revcomp(s)
    return s if s <= r else r


def pack(records):
    """(text, rec_start) of N rec0 N rec1 N ...: letters other than ACGT are N."""
    parts, start, at = ["N"], [], 1
    for r in records:
        r = "".join(ch if ch in "ACGT" else "N" for ch in r.upper())
        start.append(at)
        parts += [r, "N"]
        at += len(r) + 1
    return "".join(parts), start


class Index:
    """The edge index of an event table (name, first, begin, end, seq_event_begin as graph_table.event_table gives them) over `seqs`."""

    def __init__(self, table, seqs, k, color_of_seq=None, n_colors=0):
        name, first, begin, end, seq_event_begin = table
        self.k, self.n = k, k + 1
        self.text, self.rec_start = pack(seqs)
        seq_event_begin = [int(x) for x in seq_event_begin]
        seq_of = np.searchsorted(np.asarray(seq_event_begin), np.arange(len(name)), side="right") - 1   # the last entry <= e
        self.g0, self.span, self.name0 = [], [], []
        self.entries, self.duplicates, self.skipped = {}, 0, 0
        row_of_name = {}
        for e in range(len(name)):
            if not first[e]:
                continue
            row = len(self.g0)
            row_of_name[abs(int(name[e]))] = row
            self.name0.append(int(name[e]))
            g0, length = self.rec_start[int(seq_of[e])] + int(begin[e]), int(end[e]) - int(begin[e])
            self.g0.append(g0)
            self.span.append(length)
            for g in range(g0, g0 + length):
                w = self.text[g:g + self.n]
                if len(w) < self.n or "N" in w:
                    self.skipped += 1
                    continue
                key = canon(w)
                if key in self.entries:
                    self.duplicates += 1
                    if g < self.entries[key][0]:
                        self.entries[key] = (g, row)
                else:
                    self.entries[key] = (g, row)
        self.n_rows = len(self.g0)
        self.n_colors = n_colors
        self.presence = [set() for _ in range(self.n_rows)]
        if n_colors:
            for e in range(len(name)):
                self.presence[row_of_name[abs(int(name[e]))]].add(int(color_of_seq[int(seq_of[e])]))

    def counts(self):
        return len(self.entries), self.duplicates, self.skipped

    def locate(self, records):
        return Located(self, records)


class Located:
    """Every position of the query records through the index."""

    def __init__(self, index, records):
        n, k = index.n, index.k
        self.records = list(records)
        q, rec_start = pack(self.records)
        self.text, self.rec_start = q, rec_start
        positions = len(q) - n + 1 if len(q) >= n else 0
        rec_of = np.zeros(len(q), dtype=np.int64) - 1
        for r, (s, rec) in enumerate(zip(rec_start, self.records)):
            rec_of[s:s + len(rec)] = r
        hit = np.full(positions, INVALID, dtype=np.uint64)
        row = np.full(positions, ROW_INVALID, dtype=np.uint32)
        C = index.n_colors
        sums = np.zeros((4, len(self.records)), dtype=np.uint64)
        shared = np.zeros((len(self.records), C), dtype=np.uint64)
        found = []          # per position: None, or (g, row, rev)
        for p in range(positions):
            w = q[p:p + n]
            if "N" in w:
                found.append(None)
                continue
            rec = int(rec_of[p])
            sums[0, rec] += 1
            e = index.entries.get(canon(w))
            if e is None:
                hit[p], row[p] = ABSENT, ROW_ABSENT
                found.append(None)
                continue
            g, r = e
            rev = 0 if index.text[g:g + n] == w else 1
            assert index.text[g:g + n] == (revcomp(w) if rev else w)
            hit[p], row[p] = (rev << 63) | g, r
            found.append((g, r, rev))
            sums[1, rec] += 1
            sums[2, rec] += 1 - rev
            for c in index.presence[r]:
                shared[rec, c] += 1
        runs = []           # [q_first, length, row, rev, off_first]
        for p, f in enumerate(found):
            if f is None:
                continue
            g, r, rev = f
            off = g - index.g0[r]
            before = found[p - 1] if p else None
            if before is not None and before[1] == r and before[2] == rev and off == before[0] - index.g0[r] + (-1 if rev else 1):
                runs[-1][1] += 1
            else:
                runs.append([p, 1, r, rev, off])
                sums[3, int(rec_of[p])] += 1
        self.positions, self.hit, self.row, self.sums, self.shared = positions, hit, row, sums, shared
        self.runs = tuple(np.array([x[i] for x in runs], dtype=np.uint32) for i in range(5))
        self.info = {"positions": positions, "windows": int(sums[0].sum()), "found": int(sums[1].sum()), "runs": len(runs), "colors": C}
        # a run spells back: the query letters are the span's letters in text orientation
        for p, length, r, rev, off in runs:
            letters = q[p:p + length + k]
            if rev:
                lo = index.g0[r] + off - length + 1
                assert letters == revcomp(index.text[lo:lo + length + k])
            else:
                assert letters == index.text[index.g0[r] + off:index.g0[r] + off + length + k]


def read_named(path):
    """(name, letters) of every record: the name is the header's first word."""
    recs = []
    for line in open(path):
        if line.startswith(">"):
            recs.append([(line[1:].split() or [""])[0], []])
        else:
            recs[-1][1].append("".join(line.split()).upper())
    return [(n, "".join(b)) for n, b in recs]


def tsv(index, located, names, by, labels):
    """The bytes of the locate table: graphformat.h: WriteLocate."""
    out = ["#twopaco-locate\t1\tby=%s\tk=%d\tcolors=%d\tsegments=%d\tentries=%d\tduplicates=%d\tqueries=%d\n"
           % (by, index.k, index.n_colors, index.n_rows, len(index.entries), index.duplicates, len(names))]
    out += ["#color\t%d\t%s\n" % (c, label) for c, label in enumerate(labels)]
    for q, name in enumerate(names):
        cells = [name, len(located.records[q])] + [int(located.sums[i, q]) for i in range(4)] + [int(x) for x in located.shared[q]]
        out.append("\t".join(str(x) for x in cells) + "\n")
    out.append("#total\t%d\t%d\t%d\t%d\n" % tuple(int(located.sums[i].sum()) for i in range(4)))
    return "".join(out).encode()


def walks(index, located):
    """The bytes of the walks file: graphformat.h: WriteLocateWalks.  Coordinates on the S line's body, which is the reverse
    complement of the span when the row's first event has a negative name."""
    k = index.k
    rec_of = np.searchsorted(np.asarray(located.rec_start), np.arange(len(located.text)), side="right") - 1
    out = ["#twopaco-locate-walks\t1\tk=%d\n" % k]
    for p, length, row, rev, off in zip(*(a.tolist() for a in located.runs)):
        q = int(rec_of[p])
        lo = off - length + 1 if rev else off
        hi, minus, body = lo + length + k, bool(rev), index.span[row] + k
        if index.name0[row] < 0:
            lo, hi, minus = body - hi, body - lo, not minus
        begin = p - located.rec_start[q]
        out.append("%d\t%d\t%d\t%d\t%s\t%d\t%d\n" % (q, begin, begin + length + k, abs(index.name0[row]), "-" if minus else "+", lo, hi))
    return "".join(out).encode()


def check_by_gfa1(gfa1, k, records, tsv_bytes, walks_bytes):
    """The second statement, over the serial gfa1 text alone: the key set is every canonical (k+1)-mer of every S body.  Every run
    spells back on the body it names; every window no run covers is absent from the key set or holds a letter other than ACGT;
    the table's found counts are the covered windows.  Exact without knowing which of several positions the index keeps."""
    n = k + 1
    bodies, keys = {}, set()
    for line in gfa1.decode().split("\n"):
        f = line.split("\t")
        if f[0] == "S" and len(f) > 2 and f[2] != "*":
            bodies[f[1]] = f[2]
            b = "".join(ch if ch in "ACGT" else "N" for ch in f[2].upper())
            for i in range(len(b) - n + 1):
                if "N" not in b[i:i + n]:
                    keys.add(canon(b[i:i + n]))
    clean = ["".join(ch if ch in "ACGT" else "N" for ch in r.upper()) for r in records]
    covered = [np.zeros(max(len(r) - n + 1, 0), dtype=bool) for r in clean]
    lines = walks_bytes.decode().split("\n")
    assert lines[0] == "#twopaco-locate-walks\t1\tk=%d" % k and lines[-1] == ""
    for line in lines[1:-1]:
        q, qb, qe, seg, strand, sb, se = line.split("\t")
        q, qb, qe, sb, se = int(q), int(qb), int(qe), int(sb), int(se)
        body = "".join(ch if ch in "ACGT" else "N" for ch in bodies[seg].upper())
        assert 0 <= sb < se <= len(body) and se - sb == qe - qb > k and 0 <= qb and qe <= len(clean[q])
        spelled = body[sb:se] if strand == "+" else revcomp(body[sb:se])
        assert strand in "+-" and clean[q][qb:qe] == spelled and "N" not in spelled
        assert not covered[q][qb:qe - k].any()
        covered[q][qb:qe - k] = True
    rows = [l.split("\t") for l in tsv_bytes.decode().split("\n") if l and not l.startswith("#")]
    assert len(rows) == len(records)
    for q, r in enumerate(clean):
        for p in np.nonzero(~covered[q])[0].tolist():
            w = r[p:p + n]
            assert "N" in w or canon(w) not in keys, (q, p)
        valid = sum(1 for p in range(len(r) - n + 1) if "N" not in r[p:p + n])
        assert int(rows[q][2]) == valid and int(rows[q][3]) == int(covered[q].sum()) and int(rows[q][1]) == len(records[q])


def golden_index(case, golden_dir, by=None):
    """The index of a case of tests/golden/cases.json; by = "sequence": one colour per sequence, None: no colours."""
    import os
    seqs = graph_table.read_fasta(os.path.join(golden_dir, case["fasta"]))
    data = open(os.path.join(golden_dir, case["bin"]), "rb").read()
    table = graph_table.event_table(data, seqs, case["k"])
    if by == "sequence":
        return Index(table, seqs, case["k"], list(range(len(seqs))), len(seqs)), seqs
    return Index(table, seqs, case["k"]), seqs
