"""The colour classes of the compacted graph by their definition, from the text of a gfa1 graph -- the oracle of test_classes_cpu.py
and test_gpu_classes.py.  Nothing here goes through the project's own class code: the input is what the serial `graphdump -f gfa1`
prints (pinned to the reference's bytes by tests/golden/graphdump.json).  Rows, lengths, occurrences and presence come through
colors_reference (Gfa1, table); the rows are grouped in a Python dict keyed by the presence tuple, in row order, so that the ids ascend
by the first row of every class; the TSV and the members file of `--classes` are rendered from that.  Below: the generated inputs
(graph_walks.lay and Case) whose ids and colour maps decide the classes -- hot, all different, twins."""
import numpy as np

import colors_reference as C
import graph_walks as G
from colors_reference import (BOUNDARY_COLORS, BOUNDARY_K, BOUNDARY_L, BOUNDARY_Q, BOUNDARY_SEED, GFA1_VECTORS, GOOD_VECTORS, GRAPHDUMP, TWOPACO, boundary_fasta,  # noqa: F401
                              case_vector, colors_args, golden_gfa1, presence_words, run_graphdump, vector_id, vector_of)

classes_args = colors_args   # the arguments of a gfa1 vector without its `-f gfa1`


class Classes:
    """class_of[r] per row; per class first, segments, length, edges, occurrences, presence (bool [P, C]), n_colors; per number of
    colours n the classes, segments and edges (sets_*, [C + 1])."""

    def __init__(self, gfa1_text, by="file", k=None, files=None, color_of_seq=None, n_colors=None):
        """color_of_seq (and n_colors, default its largest entry + 1): a colour map of the caller's own instead of `by`."""
        assert k is not None
        self.g = g = C.Gfa1(gfa1_text)
        if color_of_seq is None:
            color_of_seq, self.labels = C.color_map(g, by, files)
        else:
            self.labels = ["colour %d" % c for c in range(max(color_of_seq) + 1 if n_colors is None else n_colors)]
        self.by, self.k, self.color_of_seq = by, k, list(color_of_seq)
        self.colors = t = C.table(g, color_of_seq, len(self.labels))
        self.rows = rows = len(g.row_name)
        id_of = {}
        self.class_of = np.zeros(rows, dtype=np.int64)
        first = []
        for r in range(rows):
            key = tuple(t["presence"][r].tolist())
            if key not in id_of:          # rows come in ascending order: a key's first row opens its class
                id_of[key] = len(first)
                first.append(r)
            self.class_of[r] = id_of[key]
        n = len(first)
        self.first = np.array(first, dtype=np.int64)
        self.segments = np.bincount(self.class_of, minlength=n).astype(np.int64) if rows else np.zeros(0, dtype=np.int64)
        self.length = np.zeros(n, dtype=np.int64)
        self.occurrences = np.zeros(n, dtype=np.int64)
        np.add.at(self.length, self.class_of, t["length"])
        np.add.at(self.occurrences, self.class_of, t["occurrences"])
        self.edges = self.length - k * self.segments
        self.presence = t["presence"][self.first] if n else np.zeros((0, t["colors"]), dtype=bool)
        self.n_colors = self.presence.sum(axis=1).astype(np.int64)
        bins = t["colors"] + 1
        self.sets_classes = np.bincount(self.n_colors, minlength=bins).astype(np.int64)
        self.sets_segments = np.bincount(self.n_colors, weights=self.segments, minlength=bins).astype(np.int64)
        self.sets_edges = np.bincount(self.n_colors, weights=self.edges, minlength=bins).astype(np.int64)

    def count(self):
        return len(self.first)

    def largest(self):
        return int(self.segments.max()) if len(self.segments) else 0

    def tsv(self):
        return render(self)[0]

    def members(self):
        return render(self)[1]

    def matrices(self):
        """(segments, edges) [C, C] of the distance matrices, as sums over the classes that hold both colours."""
        p = self.presence.astype(np.int64)
        return p.T @ (p * self.segments[:, None]), p.T @ (p * self.edges[:, None])


def render(w):
    """(the table, the members file) of a Classes, as `--classes` writes them."""
    c = w.colors
    out = ["#twopaco-classes\t1\tby=%s\tk=%d\tcolors=%d\tsegments=%d\tclasses=%d" % (w.by, w.k, c["colors"], w.rows, w.count())]
    out += ["#color\t%d\t%s" % (i, label) for i, label in enumerate(w.labels)]
    out += ["#sets\t%d\t%d\t%d\t%d" % (n, w.sets_classes[n], w.sets_segments[n], w.sets_edges[n]) for n in range(c["colors"] + 1) if w.sets_classes[n]]
    for p in range(w.count()):
        out.append("%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s" % (p, c["name"][w.first[p]], w.segments[p], w.length[p], w.edges[p], w.occurrences[p], w.n_colors[p],
                                                         C.hex_of(w.presence[p].tolist())))
    members = ["#twopaco-class-members\t1\tk=%d\tsegments=%d\tclasses=%d" % (w.k, w.rows, w.count())]
    members += ["%d\t%d" % (n, p) for n, p in zip(c["name"].tolist(), w.class_of.tolist())]
    return ("\n".join(out) + "\n").encode(), ("\n".join(members) + "\n").encode()


_CLASSES = {}


def k_of(v):
    return int(v["args"][v["args"].index("-k") + 1])


def golden_classes(v, by="file"):
    key = (vector_id(v), by)
    if key not in _CLASSES:
        _CLASSES[key] = Classes(golden_gfa1(v), by, k=k_of(v))
    return _CLASSES[key]


# ---------------------------------------------------------------------------------------------- the text alone
def check_text(tsv, members, colors_tsv):
    """On the two files' text and the colour table's text alone, with no code shared with Classes: the members file is a partition of
    the colour table's rows, in row order, whose ids first appear in ascending order; rows of one id have one presence and rows of two
    ids differ; segments, length and occurrences per class recounted from the colour rows equal the table; the segments sum to S and
    the per-n sums to the colour table's "#hist"; the "#sets" lines are the table's rows summed by n.  Returns the number of classes."""
    color_rows = [line.split("\t") for line in colors_tsv.decode().split("\n") if line and not line.startswith("#")]
    hist = {int(f[1]): int(f[2]) for f in (line.split("\t") for line in colors_tsv.decode().split("\n") if line.startswith("#hist"))}
    lines = members.decode().split("\n")
    assert lines[-1] == "" and lines[0].startswith("#twopaco-class-members\t1\t") and len(lines) - 2 == len(color_rows)
    seen, key_of, sums = [], {}, {}
    for line, row in zip(lines[1:-1], color_rows):
        name, p = line.split("\t")
        p = int(p)
        assert name == row[0]
        if p not in key_of:
            assert p == len(seen) and row[5] not in key_of.values()     # ids ascend by first row; a new id has a new presence
            seen.append(p)
            key_of[p] = row[5]
            sums[p] = [0, 0, 0]
        assert key_of[p] == row[5]
        sums[p][0] += 1
        sums[p][1] += int(row[1])
        sums[p][2] += int(row[2])
    text = tsv.decode().split("\n")
    head = dict(f.split("=") for f in text[0].split("\t")[2:])
    rows = [line.split("\t") for line in text if line and not line.startswith("#")]
    assert [int(r[0]) for r in rows] == seen and int(head["classes"]) == len(rows) and int(head["segments"]) == len(color_rows)
    by_n = {}
    for r in rows:
        p, n = int(r[0]), int(r[6])
        assert [int(r[2]), int(r[3]), int(r[5])] == sums[p] and int(r[4]) == int(r[3]) - int(head["k"]) * int(r[2]) and r[7] == key_of[p]
        assert n == sum(bin(int(d, 16)).count("1") for d in r[7]) and int(r[2]) > 0
        got = by_n.setdefault(n, [0, 0, 0])
        got[0], got[1], got[2] = got[0] + 1, got[1] + int(r[2]), got[2] + int(r[4])
    assert sum(int(r[2]) for r in rows) == len(color_rows)
    assert {n: v[1] for n, v in by_n.items()} == hist
    sets = [[int(x) for x in line.split("\t")[1:]] for line in text if line.startswith("#sets")]
    assert sets == [[n] + by_n[n] for n in sorted(by_n)]
    return len(rows)


# ---------------------------------------------------------------------------------------------- the generated inputs
HOT_CORE, HOT_SPECIAL = 5000, (0, 63, 64, 2559, 2560, 4991, 5006)    # the first row, the last row, and both sides of wave borders
HOT_WIDE_COLOURS, HOT_WIDE_MAP = 70, [0, 1, 31, 32, 33, 63, 64, 69]  # three words, colours at every word's ends
DIFFERENT_ROWS = 256
TWINS_COLOURS, TWINS_ROWS, TWINS_ROW = 65, 20, 5


def _case(name, walks, seed, color_of_seq=None, n_colors=None):
    """One letter everywhere: the ids alone decide the segments.  No id of 0."""
    rng = np.random.default_rng(seed)
    paint = [(wk, e, "A") for wk, ids in enumerate(walks) for e in range(len(ids) - 1)]
    seqs, sequences = G.lay(rng, walks, paint)
    color_of_seq = list(range(len(walks))) if color_of_seq is None else color_of_seq
    c = G.Case(name, seqs, sequences, n_colors=len(walks), color_of_seq=color_of_seq)
    c.n_colors = max(color_of_seq) + 1 if n_colors is None else n_colors
    return c


def hot_case(wide=False):
    """One walk over 5007 segments, and one more walk over each of the seven special ones: 5000 rows in the class of the first walk's
    colour alone and 7 rows in 7 classes of their own.  By sequence that is 8 colours and one word; wide: the same walks under a map
    of 70 colours, three words."""
    rows = HOT_CORE + len(HOT_SPECIAL)
    walks = [np.arange(1, rows + 2)] + [np.array([r + 1, r + 2]) for r in HOT_SPECIAL]
    return _case("hot_wide" if wide else "hot", walks, 5007, HOT_WIDE_MAP if wide else None, HOT_WIDE_COLOURS if wide else None)


def check_hot(w):
    assert w.rows == HOT_CORE + len(HOT_SPECIAL) and w.count() == 8 and w.largest() == HOT_CORE
    alone = np.flatnonzero(w.segments == 1)
    assert w.first[alone].tolist() == list(HOT_SPECIAL) and w.first[int(w.segments.argmax())] == 1 and w.class_of[0] == 0 and w.class_of[w.rows - 1] == 7


def different_case(stride=1):
    """256 segments in one walk, and for every set bit b of a segment's number + 1 one more walk over it: every row a class of its
    own.  By sequence every walk is a colour (more than a thousand); the map of the C-ABI tests gives bit b the colour 1 + stride b --
    stride 1: 10 colours, one word; stride 8: 66 colours, three words."""
    walks, colour = [np.arange(1, DIFFERENT_ROWS + 2)], [0]
    for r in range(DIFFERENT_ROWS):
        for b in range(9):
            if (r + 1) >> b & 1:
                walks.append(np.array([r + 1, r + 2]))
                colour.append(1 + stride * b)
    c = _case("different_%d" % stride, walks, 256)
    c.bit_map, c.bit_colours = colour, 2 + stride * 8
    return c


def twins_case():
    """65 walks, a colour each: the first over 20 segments, 63 over a segment of their own, the last over segment 5 of the first --
    the classes of rows 4 and 5 differ only in the last colour of the last of three words."""
    walks = [np.arange(1, TWINS_ROWS + 2)] + [np.array([100 + 2 * i, 101 + 2 * i]) for i in range(TWINS_COLOURS - 2)] + [np.array([TWINS_ROW + 1, TWINS_ROW + 2])]
    return _case("twins", walks, 65)


def check_twins(w):
    a, b = int(w.class_of[TWINS_ROW - 1]), int(w.class_of[TWINS_ROW])
    assert w.colors["colors"] == TWINS_COLOURS and a != b and w.segments[a] == TWINS_ROWS - 1 and w.segments[b] == 1
    differ = np.flatnonzero(w.presence[a] != w.presence[b])
    assert differ.tolist() == [TWINS_COLOURS - 1] and w.count() == TWINS_COLOURS
