"""The presence tracks by their definition (include/twopaco_hip.h, the tpc_segments_tracks_* group) -- the oracle of
test_tracks_cpu.py and test_gpu_tracks.py.  Nothing here goes through the project's own track code.  Three statements:

  Tracks           PART 1, from the text the serial `graphdump -f gfa1` prints (pinned to the reference's bytes by
                   tests/golden/graphdump.json) and the lengths of the FASTA records.  The events, their ends and their begins are
                   read exactly as anchors_reference.Anchors reads them (a later event of a sequence begins where the one before it
                   ended); presence per name comes from colors_reference.  The intervals, the sums, the TSV and the bedGraph, with
                   plain loops.
  fasta_intervals  PART 2, from the FASTA alone, without any graph: a dict from each canonical (k+1)-mer to the set of colours that
                   hold it, and per sequence the maximal runs of positions 0 .. len - k - 1 with equal sets.  For inputs with no
                   abundance cut; a sequence with a letter other than A C G T has no statement of its own (its (k+1)-mers without
                   such a letter still count for the others).
  direct           the definition over event arrays (name, begin, end, seq_event_begin) in numpy, at any size: what the device
                   arrays of the generated walks are compared with; pinned to Tracks on the small cases."""
import numpy as np

import anchors_reference as A
import colors_reference as C
from anchors_reference import fasta_of, k_of, lengths_of  # noqa: F401
from classes_reference import (BOUNDARY_COLORS, BOUNDARY_K, BOUNDARY_L, BOUNDARY_Q, BOUNDARY_SEED, GFA1_VECTORS, GOOD_VECTORS, GRAPHDUMP, TWOPACO, boundary_fasta,  # noqa: F401
                               case_vector, colors_args, different_case, golden_gfa1, hot_case, presence_words, run_graphdump, twins_case, vector_id, vector_of, _case)
from links_reference import plain, read_fasta, reverse_complement  # noqa: F401

ALL = 0xFFFFFFFF
tracks_args = colors_args   # the arguments of a gfa1 vector without its `-f gfa1`


# ------------------------------------------------------------------------------------------------------------------ part 1
class Tracks:
    """only: one colour, None = all.  lengths: the number of letters of every input sequence, in input order."""

    def __init__(self, gfa1_text, k, lengths, by="file", only=None, color_of_seq=None, labels=None):
        a = A.Anchors(gfa1_text, k, lengths, by, 0, color_of_seq=color_of_seq, labels=labels)   # the events as the anchor oracle reads them
        self.k, self.by, self.only = k, by, only
        self.seq_name, self.seq_length, self.color_of_seq, self.labels, self.n_colors = a.seq_name, a.seq_length, a.color_of_seq, a.labels, a.n_colors
        self.name, self.seq, self.begin, self.end = a.name, a.seq, a.begin, a.end
        assert only is None or 0 <= only < self.n_colors
        g = C.Gfa1(gfa1_text)
        self.colors = t = C.table(g, self.color_of_seq, self.n_colors)
        row_of = {n: r for r, n in enumerate(g.row_name)}
        self.rows = len(g.row_name)
        self.row = [row_of[n] for n in self.name]
        presence = [tuple(t["presence"][r].tolist()) for r in range(self.rows)]
        n = len(self.name)
        selected = [only is None or self.color_of_seq[self.seq[e]] == only for e in range(n)]
        self.selected = sum(selected)

        def continues(e):
            return e > 0 and self.seq[e] == self.seq[e - 1] and presence[self.row[e]] == presence[self.row[e - 1]]

        self.intervals = []       # (first, last)
        e = 0
        while e < n:
            if not selected[e]:
                e += 1
                continue
            last = e
            while last + 1 < n and selected[last + 1] and continues(last + 1):
                last += 1
            self.intervals.append((e, last))
            e = last + 1
        c = self.n_colors
        self.per_color = [[0, 0, 0, 0] for _ in range(c)]     # intervals, edges, core_edges, private_edges
        self.depth = [[0, 0] for _ in range(c + 1)]           # intervals, edges
        for first, last in self.intervals:
            edges, depth = self.end[last] - self.begin[first], int(t["n_colors"][self.row[first]])
            s = self.per_color[self.color_of_seq[self.seq[first]]]
            s[0] += 1
            s[1] += edges
            s[2] += edges if depth == c else 0
            s[3] += edges if depth == 1 else 0
            self.depth[depth][0] += 1
            self.depth[depth][1] += edges

    def count(self):
        return len(self.intervals)

    def arrays(self):
        """What the C-ABI fetches: [first_event, last_event, row] uint32, the four per-colour sums and the two per-depth sums uint64."""
        rows = [np.array([i[0] for i in self.intervals], dtype=np.uint32), np.array([i[1] for i in self.intervals], dtype=np.uint32),
                np.array([self.row[i[0]] for i in self.intervals], dtype=np.uint32)]
        return rows, [np.array([s[i] for s in self.per_color], dtype=np.uint64) for i in range(4)], [np.array([d[i] for d in self.depth], dtype=np.uint64) for i in range(2)]

    def lines(self):
        """Per interval (sequence, begin, end, events, n_colors, presence as a tuple of bools)."""
        t = self.colors
        return [(self.seq[f], self.begin[f], self.end[l], l - f + 1, int(t["n_colors"][self.row[f]]), tuple(t["presence"][self.row[f]].tolist())) for f, l in self.intervals]

    def tsv(self):
        out = ["#twopaco-tracks\t1\tby=%s\tk=%d\tcolors=%d\tsegments=%d\tof=%s\tintervals=%d" % (self.by, self.k, self.n_colors, self.rows,
                                                                                            "all" if self.only is None else str(self.only), self.count())]
        out += ["#color\t%d\t%s" % (c, label) for c, label in enumerate(self.labels)]
        out += ["#sequence\t%d\t%d\t%d\t%s" % (s, self.color_of_seq[s], self.seq_length[s], self.seq_name[s]) for s in range(len(self.seq_name))]
        out += ["#genome\t%d\t%d\t%d\t%d\t%d" % tuple([c] + self.per_color[c]) for c in range(self.n_colors) if self.only is None or c == self.only]
        out += ["#depth\t%d\t%d\t%d" % (n, d[0], d[1]) for n, d in enumerate(self.depth) if d[0]]
        out += ["%d\t%d\t%d\t%d\t%d\t%s" % (s, b, e, ev, n, C.hex_of(list(p))) for s, b, e, ev, n, p in self.lines()]
        return ("\n".join(out) + "\n").encode()

    def bedgraph(self):
        out = ['track type=bedGraph name="n_colors" description="twopaco tracks k=%d by=%s"' % (self.k, self.by)]
        out += ["%s\t%d\t%d\t%d" % (self.seq_name[s], b, e, n) for s, b, e, _, n, _ in self.lines()]
        return ("\n".join(out) + "\n").encode()


_TRACKS = {}


def golden_tracks(v, by="file", only=None):
    key = (vector_id(v), by, only)
    if key not in _TRACKS:
        _TRACKS[key] = Tracks(golden_gfa1(v), k_of(v), lengths_of(fasta_of(v)), by, only)
    return _TRACKS[key]


def case_tracks(case, only=None, by="file", color_of_seq=None, n_colors=None):
    """Part 1 over the serial gfa1 of a generated case (graph_walks.Case), under the case's colour map or the caller's."""
    color_of_seq = case.color_of_seq if color_of_seq is None else color_of_seq
    n_colors = case.n_colors if n_colors is None else n_colors
    return Tracks(case.gfa1(), case.k, [int(s.size) for s in case.seqs], by, only, color_of_seq=list(color_of_seq), labels=["colour %d" % c for c in range(n_colors)])


# ---------------------------------------------------------------------------------------------- the text alone
def check_text(tsv, bedgraph=None):
    """On the table's text alone (and the bedGraph's): the intervals ascend and tile every sequence that has any, with no gap and no
    overlap, inside [0, length - k); neighbouring intervals of one sequence differ in presence; n_colors is the popcount; the
    "#genome" and "#depth" lines are the rows summed; the per-depth edges sum to the per-colour edges; the bedGraph holds the same
    intervals under the sequences' names.  Returns (intervals, {colour: edges})."""
    text = tsv.decode().split("\n")
    assert text[-1] == ""
    head = dict(f.split("=") for f in text[0].split("\t")[2:])
    k, colors = int(head["k"]), int(head["colors"])
    seqs = {int(f[1]): (int(f[2]), int(f[3]), f[4]) for f in (line.split("\t") for line in text if line.startswith("#sequence\t"))}
    genome = {int(f[1]): [int(x) for x in f[2:]] for f in (line.split("\t") for line in text if line.startswith("#genome\t"))}
    depth = {int(f[1]): [int(x) for x in f[2:]] for f in (line.split("\t") for line in text if line.startswith("#depth\t"))}
    rows = [line.split("\t") for line in text if line and not line.startswith("#")]
    assert int(head["intervals"]) == len(rows)
    assert sorted(genome) == (list(range(colors)) if head["of"] == "all" else [int(head["of"])])
    sums, by_depth = {c: [0, 0, 0, 0] for c in genome}, {}
    before = None
    for r in rows:
        assert len(r) == 6, r
        s, b, e, events, n = (int(x) for x in r[:5])
        colour, length, _ = seqs[s]
        assert 0 <= b < e <= length - k and events >= 1 and colour in genome, r
        assert n == sum(bin(int(d, 16)).count("1") for d in r[5]) and 1 <= n <= colors and len(r[5]) == (colors + 3) // 4
        assert int(r[5][colour // 4], 16) >> (colour % 4) & 1, r        # a sequence holds its own stretches
        if before is not None and before[0] == s:
            assert b == before[2] and r[5] != before[3], r              # no gap, no overlap, and a reason to split
        else:
            assert before is None or s > before[0], r
        before = (s, b, e, r[5])
        got = sums[colour]
        got[0], got[1], got[2], got[3] = got[0] + 1, got[1] + e - b, got[2] + (e - b if n == colors else 0), got[3] + (e - b if n == 1 else 0)
        d = by_depth.setdefault(n, [0, 0])
        d[0], d[1] = d[0] + 1, d[1] + e - b
    assert sums == genome and by_depth == depth
    assert sum(d[1] for d in depth.values()) == sum(g[1] for g in genome.values())
    if colors == 1:
        assert all(g[2] == g[3] == g[1] for g in genome.values())
    if bedgraph is not None:
        lines = bedgraph.decode().split("\n")
        assert lines[-1] == "" and lines[0] == 'track type=bedGraph name="n_colors" description="twopaco tracks k=%d by=%s"' % (k, head["by"])
        assert [line.split("\t") for line in lines[1:-1]] == [[seqs[int(r[0])][2], r[1], r[2], r[4]] for r in rows]
    return len(rows), {c: g[1] for c, g in genome.items()}


def rows_of(tsv):
    """(the "#genome" lines, the interval lines) of a table's text."""
    text = tsv.decode().split("\n")
    return [line for line in text if line.startswith("#genome\t")], [line for line in text if line and not line.startswith("#")]


# ------------------------------------------------------------------------------------------------------------------ part 2
def fasta_intervals(records, color_of_seq, k):
    """records: the letters of every input sequence.  Per sequence the list of (begin, end, frozenset of colours) of the maximal runs
    of positions with equal sets, or None for a sequence that holds a letter other than A C G T."""
    seqs = [plain(s) for s in records]
    held = {}
    for s, letters in enumerate(seqs):
        for p in range(len(letters) - k):
            mer = letters[p:p + k + 1]
            if "N" not in mer:
                held.setdefault(A.canonical(mer)[0], set()).add(color_of_seq[s])
    out = []
    for letters in seqs:
        if "N" in letters:
            out.append(None)
            continue
        runs = []
        for p in range(len(letters) - k):
            colours = frozenset(held[A.canonical(letters[p:p + k + 1])[0]])
            if runs and runs[-1][2] == colours:
                runs[-1][1] = p + 1
            else:
                runs.append([p, p + 1, colours])
        out.append([tuple(r) for r in runs])
    return out


def intervals_by_sequence(w):
    """The intervals of a Tracks per sequence, in the form of fasta_intervals."""
    out = [[] for _ in w.seq_name]
    for s, b, e, _, _, p in w.lines():
        out[s].append((b, e, frozenset(c for c, held in enumerate(p) if held)))
    return out


def check_fasta_statement(w, records):
    """Part 1 == part 2 on every sequence part 2 speaks about; returns how many those are."""
    assert w.only is None
    mine, theirs = intervals_by_sequence(w), fasta_intervals(records, w.color_of_seq, w.k)
    spoken = 0
    for s, runs in enumerate(theirs):
        if runs is not None:
            assert mine[s] == runs, (s, mine[s][:3], runs[:3])
            spoken += 1
    return spoken


# ------------------------------------------------------------------------------------------------------------------ numpy, at any size
def direct(name, begin, end, seq_event_begin, color_of_seq, n_colors, only=None):
    """The definition over the event table: ([first_event, last_event, row] uint32, [intervals, edges, core_edges, private_edges] uint64
    [colours], [depth_intervals, depth_edges] uint64 [colours + 1], selected events).  Rows are |name| in the order of their first
    events; 'N'-named events (>= 2^34) are rows of their own."""
    name = np.asarray(name, dtype=np.int64)
    begin, end = np.asarray(begin, dtype=np.int64), np.asarray(end, dtype=np.int64)
    sb = np.asarray(seq_event_begin, dtype=np.int64)
    n = name.size
    e = np.arange(n, dtype=np.int64)
    seq = np.searchsorted(sb, e, side="right") - 1
    color = np.asarray(color_of_seq, dtype=np.int64)[seq] if n else np.zeros(0, dtype=np.int64)
    mag = np.abs(name)
    mag = np.where(mag >= (1 << 34), (1 << 40) + e, mag)          # every 'N'-named event its own row
    uniq, first_at, inverse = np.unique(mag, return_index=True, return_inverse=True)
    order = np.argsort(first_at, kind="stable")
    rank = np.empty(uniq.size, dtype=np.int64)
    rank[order] = np.arange(uniq.size)
    row = rank[inverse]
    presence = np.zeros((uniq.size, n_colors), dtype=bool)
    presence[row, color] = True
    depth_of_row = presence.sum(axis=1)
    selected = np.ones(n, dtype=bool) if only is None else color == only
    cont = np.zeros(n, dtype=bool)
    if n > 1:
        cont[1:] = (seq[1:] == seq[:-1]) & ((row[1:] == row[:-1]) | (presence[row[1:]] == presence[row[:-1]]).all(axis=1))
    head = selected & ~cont
    tail = selected & ~np.append((selected & cont)[1:], False)
    first, last = e[head], e[tail]
    assert first.size == last.size and (first <= last).all()
    edges, c, d = end[last] - begin[first], color[first], depth_of_row[row[first]]
    zero = np.zeros_like(edges)
    per_color = [np.bincount(c, minlength=n_colors).astype(np.uint64)] + [np.bincount(c, weights=x.astype(np.float64), minlength=n_colors).astype(np.uint64)
                                                                         for x in (edges, np.where(d == n_colors, edges, zero), np.where(d == 1, edges, zero))]
    per_depth = [np.bincount(d, minlength=n_colors + 1).astype(np.uint64), np.bincount(d, weights=edges.astype(np.float64), minlength=n_colors + 1).astype(np.uint64)]
    return [first.astype(np.uint32), last.astype(np.uint32), row[first].astype(np.uint32)], per_color, per_depth, int(selected.sum())


def direct_of(case, only=None, color_of_seq=None, n_colors=None):
    w = case.w
    return direct(w.name, w.begin, w.end, w.seq_event_begin, case.color_of_seq if color_of_seq is None else color_of_seq, case.n_colors if n_colors is None else n_colors, only)


def same(a, b):
    """Two results of direct / Tracks.arrays() (the first three entries) hold the same arrays."""
    return all(x.size == y.size and (x == y).all() for p, q in zip(a[:3], b[:3]) for x, y in zip(p, q))


# ------------------------------------------------------------------------------------------------------------------ the generated inputs
HOT_EVENTS, HOT_INTERVALS = 5014, 18
PAIR_SEGMENTS = 40


def pair_case(colours):
    """Two walks over the same 40 segments: under one colour (colours = 1) or a colour each (2)."""
    walks = [np.arange(1, PAIR_SEGMENTS + 2), np.arange(1, PAIR_SEGMENTS + 2)]
    return _case("pair_%d" % colours, walks, 40 + colours, [0, 0] if colours == 1 else [0, 1], colours)


def gap_case():
    """Three sequences, a colour each: two walks over the same four segments and between them a sequence of one junction record, which
    has no event -- a sequence without events between two that have some.  (A sequence without any record between two that have
    some is not a stream the walk accepts: a record behind two separators is "The input is corrupted".)"""
    return _case("gap", [np.arange(1, 6), np.array([9]), np.arange(1, 6)], 3)


def check_hot(rows):
    """rows: [first_event, last_event, row] of the hot case under any of its maps: the long walk splits into 11 at the seven special
    rows, the seven short walks give one interval each."""
    from classes_reference import HOT_CORE, HOT_SPECIAL
    first, last, row = (np.asarray(a, dtype=np.int64) for a in rows)
    n_rows = HOT_CORE + len(HOT_SPECIAL)
    assert first.size == HOT_INTERVALS and int((last - first + 1).sum()) == HOT_EVENTS
    long_walk = first < n_rows
    assert int(long_walk.sum()) == 11 and (last[~long_walk] == first[~long_walk]).all() and sorted(row[~long_walk].tolist()) == list(HOT_SPECIAL)
    cuts = sorted(set([0, n_rows] + [r for s in HOT_SPECIAL for r in (s, s + 1)]))
    assert first[long_walk].tolist() == cuts[:-1] and (last[long_walk] + 1).tolist() == cuts[1:]
