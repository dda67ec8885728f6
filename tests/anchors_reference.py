"""The anchor blocks by their definition (include/twopaco_hip.h, the tpc_segments_anchors_* group) -- the oracle of
test_anchors_cpu.py and test_gpu_anchors.py.  Nothing here goes through the project's own anchor code.  Three statements:

  Anchors          PART 1, from the text the serial `graphdump -f gfa1` prints (pinned to the reference's bytes by
                   tests/golden/graphdump.json) and the lengths of the FASTA records:
                       S <sequence> * UR:Z:<file>                 one per input sequence, in order
                       S <segment> <body>                         a row; its edges are len(body) - k
                       C <segment> <strand> <sequence> + <pos>    one event, in event order; <pos> is the event's END, so
                                                                  begin = end - (len(body) - k) for a sequence's first
                                                                  event and the end of the event before it for the others
                   count[row][colour], the mates, the blocks, the per-colour sums, the TSV and the PAF, with plain dicts and loops.
  fasta_runs       PART 2, from the FASTA alone: a dictionary of canonical (k+1)-mers per colour, the positions whose (k+1)-mer
                   occurs once in the reference colour and once in the query's colour, and the maximal runs of such positions on a
                   constant diagonal (forward) or anti-diagonal (reverse), within one sequence on each side.
  direct           the definition over event arrays (name, begin, end, seq_event_begin) in numpy, at any size: what the device
                   arrays of the generated walks are compared with; pinned to Anchors on the small cases."""
import os

import numpy as np

from bubbles_reference import oracle_stream  # noqa: F401  (the tests make their streams as test_bubbles_cpu.py does)
from colors_reference import (GFA1_VECTORS, GOOD_VECTORS, GRAPHDUMP, TWOPACO, case_vector, colors_args, golden_gfa1, run_graphdump, vector_id, vector_of)  # noqa: F401
from helpers import GOLDEN
from links_reference import few_events_fasta, plain, read_fasta, reverse_complement  # noqa: F401

NONE = 0xFFFFFFFF


def k_of(v):
    return int(v["args"][v["args"].index("-k") + 1])


def fasta_of(v):
    """The FASTA files of a golden vector, as given (relative to tests/golden)."""
    a = v["args"]
    return [a[i + 1] for i in range(len(a)) if a[i] == "-s"]


def anchors_args(v):
    return colors_args(v)


# ------------------------------------------------------------------------------------------------------------------ part 1
class Anchors:
    """lengths: the number of letters of every input sequence, in input order (the gfa1 text does not hold them)."""

    def __init__(self, gfa1_text, k, lengths, by="file", ref=0, color_of_seq=None, labels=None):
        self.k, self.by, self.ref = k, by, ref
        self.seq_name, self.seq_file = [], []
        edges_of = {}
        self.rows = []
        events = []
        for line in gfa1_text.decode().split("\n"):
            f = line.split("\t")
            if f[0] == "S" and len(f) == 4 and f[2] == "*" and f[3].startswith("UR:Z:"):
                self.seq_name.append(f[1])
                self.seq_file.append(f[3][5:])
            elif f[0] == "S":
                assert len(f) == 3 and int(f[1]) not in edges_of, line
                edges_of[int(f[1])] = len(f[2]) - k
                self.rows.append(int(f[1]))
            elif f[0] == "C":
                assert len(f) == 6 and f[2] in "+-" and f[4] == "+", line
                events.append((int(f[1]), f[2] == "+", f[3], int(f[5])))
        assert len(set(self.seq_name)) == len(self.seq_name), "the oracle tells sequences apart by their names"
        assert len(lengths) == len(self.seq_name)
        self.seq_length = list(lengths)
        index = {n: i for i, n in enumerate(self.seq_name)}
        if color_of_seq is None:
            if by == "sequence":
                color_of_seq = list(range(len(self.seq_name)))
                labels = ["%d\t%s" % (s + 1, f) for s, f in enumerate(self.seq_file)]
            else:
                files = list(dict.fromkeys(self.seq_file))
                color_of_seq, labels = [files.index(f) for f in self.seq_file], files
        self.color_of_seq, self.labels = list(color_of_seq), list(labels)
        self.n_colors = len(self.labels)
        assert 0 <= ref < self.n_colors

        self.name = [n for n, _, _, _ in events]             # the row of an event is its name: an S line per name
        self.forward = [fw for _, fw, _, _ in events]
        self.seq = [index[s] for _, _, s, _ in events]
        self.end = [e for _, _, _, e in events]
        self.begin = [e - edges_of[n] for n, _, _, e in events]
        assert all(a <= b for a, b in zip(self.seq, self.seq[1:])), "events come in sequence order"
        # Consecutive events of one sequence share their junction, so behind a sequence's first event begin is the end before it.
        # The two agree on every golden vector but rand6_k9_a3, whose abundance cut lets one name cover bodies of different
        # lengths (101 of its 973 events): there the S line's body is not the event's, and the junction is.
        for e in range(1, len(events)):
            if self.seq[e] == self.seq[e - 1]:
                self.begin[e] = self.end[e - 1]
        n = len(events)
        color = [self.color_of_seq[s] for s in self.seq]
        # count[row][colour], with the events themselves
        self.count = {}
        for e in range(n):
            self.count.setdefault((self.name[e], color[e]), []).append(e)
        self.mate = [NONE] * n
        for e in range(n):
            if color[e] == ref or len(self.count[(self.name[e], color[e])]) != 1:
                continue
            in_ref = self.count.get((self.name[e], ref), [])
            if len(in_ref) == 1:
                self.mate[e] = in_ref[0]
        self.ref_edges = sum(self.end[e] - self.begin[e] for e in range(n) if color[e] == ref)

        def reverse(e):
            return self.forward[e] != self.forward[self.mate[e]]

        def continues(e):
            if e == 0 or self.mate[e] == NONE or self.mate[e - 1] == NONE or self.seq[e] != self.seq[e - 1] or reverse(e) != reverse(e - 1):
                return False
            m, before = self.mate[e], self.mate[e - 1]
            if (m != before - 1) if reverse(e) else (m != before + 1):
                return False
            return self.seq[m] == self.seq[before]

        self.blocks = []          # (query_first, query_last, ref_first, ref_last, reverse)
        e = 0
        while e < n:
            if self.mate[e] == NONE:
                e += 1
                continue
            assert not continues(e)
            last = e
            while last + 1 < n and continues(last + 1):
                last += 1
            rv = reverse(e)
            self.blocks.append((e, last, self.mate[last] if rv else self.mate[e], self.mate[e] if rv else self.mate[last], rv))
            e = last + 1
        self.shared = [[0, 0, 0, 0] for _ in range(self.n_colors)]
        self.same_length = True   # both intervals of every block have the same length
        for qf, ql, rf, rl, rv in self.blocks:
            edges = self.end[ql] - self.begin[qf]
            assert rl - rf == ql - qf
            # (false only where one name covers different bodies: rand6_k9_a3)
            self.same_length = self.same_length and self.end[rl] - self.begin[rf] == edges
            s = self.shared[color[qf]]
            s[0] += 1
            s[1] += ql - qf + 1
            s[2] += edges
            s[3] += edges if rv else 0
        self.color = color

    def arrays(self):
        """What the C-ABI fetches: mate uint32 [events], the four row arrays, the four sums uint64 [colours]."""
        rows = [np.array([b[i] for b in self.blocks], dtype=np.uint32) for i in range(4)]
        sums = [np.array([s[i] for s in self.shared], dtype=np.uint64) for i in range(4)]
        return np.array(self.mate, dtype=np.uint32), rows, sums

    def lines(self):
        """Per block (colour, ref_seq, ref_begin, ref_end, strand, query_seq, query_begin, query_end, anchors)."""
        out = []
        for qf, ql, rf, rl, rv in self.blocks:
            out.append((self.color[qf], self.seq[rf], self.begin[rf], self.end[rl] + self.k, "-" if rv else "+", self.seq[qf], self.begin[qf], self.end[ql] + self.k,
                        ql - qf + 1))
        return out

    def tsv(self):
        out = ["#twopaco-anchors\t1\tby=%s\tk=%d\tcolors=%d\tsegments=%d\tref=%d\tref_edges=%d\tblocks=%d" % (self.by, self.k, self.n_colors, len(self.rows), self.ref,
                                                                                                           self.ref_edges, len(self.blocks))]
        out += ["#color\t%d\t%s" % (c, label) for c, label in enumerate(self.labels)]
        out += ["#sequence\t%d\t%d\t%d\t%s" % (s, self.color_of_seq[s], self.seq_length[s], self.seq_name[s]) for s in range(len(self.seq_name))]
        out += ["#shared\t%d\t%d\t%d\t%d\t%d" % tuple([c] + self.shared[c]) for c in range(self.n_colors) if c != self.ref]
        out += ["%d\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d" % line for line in self.lines()]
        return ("\n".join(out) + "\n").encode()

    def paf(self):
        out = []
        for _, rs, rb, re, strand, qs, qb, qe, anchors in self.lines():
            out.append("%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t255\ttp:A:P\tcg:Z:%d=\tan:i:%d" % (self.seq_name[qs], self.seq_length[qs], qb, qe, strand, self.seq_name[rs],
                                                                                                 self.seq_length[rs], rb, re, qe - qb, qe - qb, qe - qb, anchors))
        return "".join(line + "\n" for line in out).encode()

    def counts_of(self, in_ref, in_query):
        """The (row, query colour) pairs with count[row][ref] == in_ref and count[row][colour] == in_query."""
        return [(r, c) for (r, c), ev in self.count.items() if c != self.ref and len(ev) == in_query and len(self.count.get((r, self.ref), [])) == in_ref]


def lengths_of(fastas, cwd=GOLDEN):
    return [len(s) for f in fastas for _, s in read_fasta(os.path.join(cwd, f))]


_ANCHORS = {}


def golden_anchors(v, by, ref):
    """ref: 0 or "last"."""
    key = (vector_id(v), by, ref)
    if key not in _ANCHORS:
        text, lengths = golden_gfa1(v), lengths_of(fasta_of(v))
        if ref == "last":
            ref = golden_anchors(v, by, 0).n_colors - 1
        _ANCHORS[key] = Anchors(text, k_of(v), lengths, by, ref)
    return _ANCHORS[key]


def check_text(tsv_text, fastas, cwd=GOLDEN):
    """On the table's text and the FASTA alone: every block's two intervals spell the same letters, or reverse complements when
    '-'.  Letters other than A C G T cannot lie in a block.  Returns the number of blocks checked."""
    seqs = [plain(s) for f in fastas for _, s in read_fasta(os.path.join(cwd, f))]
    rows = 0
    for line in tsv_text.decode().split("\n"):
        if not line or line.startswith("#"):
            continue
        f = line.split("\t")
        assert len(f) == 9 and f[4] in "+-", line
        ref, query = seqs[int(f[1])][int(f[2]):int(f[3])], seqs[int(f[5])][int(f[6]):int(f[7])]
        assert len(ref) == int(f[3]) - int(f[2]) == len(query) and "N" not in ref, line
        assert ref == (query if f[4] == "+" else reverse_complement(query)), line
        rows += 1
    return rows


# ------------------------------------------------------------------------------------------------------------------ part 2
def canonical(s):
    r = reverse_complement(s)
    return (s, True) if s <= r else (r, False)


def fasta_runs(records, color_of_seq, k, ref):
    """records: the letters of every input sequence.  The set of (colour, ref_seq, ref_begin, ref_end, strand, query_seq, query_begin,
    query_end); and whether any (k+1)-mer is its own reverse complement."""
    seqs = [plain(s) for s in records]
    where = {}            # colour -> canonical (k+1)-mer -> [(sequence, position, spelled as the canonical form)]
    palindrome = False
    for s, letters in enumerate(seqs):
        held = where.setdefault(color_of_seq[s], {})
        for p in range(len(letters) - k):
            mer = letters[p:p + k + 1]
            if "N" in mer:
                continue
            c, same = canonical(mer)
            palindrome = palindrome or mer == reverse_complement(mer)
            held.setdefault(c, []).append((s, p, same))
    in_ref = where.get(ref, {})
    runs = set()
    for s, letters in enumerate(seqs):
        col = color_of_seq[s]
        if col == ref:
            continue
        open_run = None   # [ref_seq, strand, first ref position, last ref position, first query position, last query position]
        def close():
            if open_run is not None:
                rs, rv, r0, r1, q0, q1 = open_run
                runs.add((col, rs, min(r0, r1), max(r0, r1) + k + 1, "-" if rv else "+", s, q0, q1 + k + 1))
        for p in range(len(letters) - k):
            mer = letters[p:p + k + 1]
            hit = None
            if "N" not in mer:
                c, same = canonical(mer)
                mine, theirs = where[col][c], in_ref.get(c, [])
                if len(mine) == 1 and len(theirs) == 1:
                    hit = (theirs[0][0], theirs[0][2] != same, theirs[0][1])
            if hit is not None and open_run is not None and open_run[0] == hit[0] and open_run[1] == hit[1] and open_run[5] == p - 1 and \
                    hit[2] == open_run[3] + (-1 if hit[1] else 1):
                open_run[3], open_run[5] = hit[2], p
                continue
            close()
            open_run = None if hit is None else [hit[0], hit[1], hit[2], hit[2], p, p]
        close()
    return runs, palindrome


# ------------------------------------------------------------------------------------------------------------------ numpy, at any size
def direct(name, begin, end, seq_event_begin, color_of_seq, n_colors, ref):
    """The definition over the event table: (mate uint32 [events], [query_first, query_last, ref_first, ref_last] uint32, [blocks,
    anchors, edges, reverse_edges] uint64 [colours], ref_edges).  Rows are |name|; 'N'-named events (>= 2^34) are rows of their own."""
    name = np.asarray(name, dtype=np.int64)
    begin, end = np.asarray(begin, dtype=np.int64), np.asarray(end, dtype=np.int64)
    sb = np.asarray(seq_event_begin, dtype=np.int64)
    n = name.size
    e = np.arange(n, dtype=np.int64)
    seq = np.searchsorted(sb, e, side="right") - 1
    color = np.asarray(color_of_seq, dtype=np.int64)[seq] if n else np.zeros(0, dtype=np.int64)
    mag = np.abs(name)
    fresh = mag >= (1 << 34)
    mag = np.where(fresh, (1 << 40) + e, mag)          # every 'N'-named event its own row
    key = mag * n_colors + color
    uniq, inverse, counts = np.unique(key, return_inverse=True, return_counts=True)
    alone = counts[inverse] == 1
    ref_key = mag * n_colors + ref
    at = np.searchsorted(uniq, ref_key)
    at_ok = (at < uniq.size)
    found = np.zeros(n, dtype=bool)
    found[at_ok] = uniq[at[at_ok]] == ref_key[at_ok]
    ref_alone = np.zeros(n, dtype=bool)
    ref_alone[found] = counts[at[found]] == 1
    # the one event of every key that is alone
    event_of = np.full(uniq.size, -1, dtype=np.int64)
    event_of[inverse[alone]] = e[alone]
    mate = np.full(n, NONE, dtype=np.int64)
    anchor = alone & ref_alone & (color != ref)
    mate[anchor] = event_of[at[anchor]]
    rev = np.zeros(n, dtype=bool)
    rev[anchor] = (name[anchor] < 0) != (name[mate[anchor]] < 0)
    cont = np.zeros(n, dtype=bool)
    if n > 1:
        a, b = e[1:], e[:-1]
        ok = anchor[a] & anchor[b] & (seq[a] == seq[b]) & (rev[a] == rev[b])
        ma, mb = np.where(anchor[a], mate[a], 0), np.where(anchor[b], mate[b], 0)
        ok &= np.where(rev[a], ma + 1 == mb, ma == mb + 1) & (seq[ma] == seq[mb])
        cont[1:] = ok
    head = anchor & ~cont
    tail = anchor & ~np.append(cont[1:], False)
    qf, ql = e[head], e[tail]
    rv = rev[qf]
    rf, rl = np.where(rv, mate[ql], mate[qf]), np.where(rv, mate[qf], mate[ql])
    edges = end[ql] - begin[qf]
    c = color[qf]
    sums = [np.bincount(c, minlength=n_colors).astype(np.uint64), np.bincount(c, weights=(ql - qf + 1).astype(np.float64), minlength=n_colors).astype(np.uint64),
            np.bincount(c, weights=edges.astype(np.float64), minlength=n_colors).astype(np.uint64),
            np.bincount(c, weights=np.where(rv, edges, 0).astype(np.float64), minlength=n_colors).astype(np.uint64)]
    ref_edges = int((end - begin)[color == ref].sum())
    return mate.astype(np.uint32), [x.astype(np.uint32) for x in (qf, ql, rf, rl)], sums, ref_edges


# ------------------------------------------------------------------------------------------------------------------ the generated family
FAMILY_K, FAMILY_L, FAMILY_Q, FAMILY_SEED = 21, 24, 5, 11
FAMILY_COLOURS = ("base", "substitutions", "inversion", "moved", "duplicated", "reversed", "cut", "gap", "unrelated")


def family_records():
    """[(file label, [(record name, letters)])], one file per colour, over a random 20 kbp base with a 600 bp tandem duplication at
    5000: the base (the reference); a copy with 30 substitutions; one with the 2 kbp at 8000 inverted; one with the 3 kbp at 12000
    moved to 3000; one with the 500 bp at 15000 duplicated in place; one reverse-complemented whole; one cut into three records; one
    with a run of 30 N at 10000; an unrelated random genome."""
    rng = np.random.default_rng(20261020)

    def letters(n):
        return "".join("ACGT"[c] for c in rng.integers(0, 4, n))

    base = letters(20000)
    base = base[:5600] + base[5000:5600] + base[5600:]
    subs = list(base)
    for p in sorted(int(x) for x in rng.choice(np.arange(100, len(base) - 100), 30, replace=False)):
        subs[p] = "ACGT"[("ACGT".index(subs[p]) + 1 + int(rng.integers(0, 3))) % 4]
    inversion = base[:8000] + reverse_complement(base[8000:10000]) + base[10000:]
    moved = base[:3000] + base[12000:15000] + base[3000:12000] + base[15000:]
    duplicated = base[:15500] + base[15000:15500] + base[15500:]
    gap = base[:10000] + "N" * 30 + base[10030:]
    return [("base", [("base", base)]), ("substitutions", [("subs", "".join(subs))]), ("inversion", [("inv", inversion)]), ("moved", [("moved", moved)]),
            ("duplicated", [("dup", duplicated)]), ("reversed", [("rc", reverse_complement(base))]),
            ("cut", [("cut_a", base[:7000]), ("cut_b", base[7000:13500]), ("cut_c", base[13500:])]), ("gap", [("gap", gap)]), ("unrelated", [("other", letters(20000))])]


def family_files(directory):
    """The FASTA files, one per colour, written into directory; their paths in colour order."""
    paths = []
    for label, recs in family_records():
        path = os.path.join(str(directory), label + ".fa")
        with open(path, "w") as f:
            for name, s in recs:
                f.write(">%s\n" % name)
                for i in range(0, len(s), 70):
                    f.write(s[i:i + 70] + "\n")
        paths.append(path)
    return paths


def streams_of(fastas, out, k, L, q, seed):
    """The junction stream of several FASTA files, in order, from the CPU restatement of the pipeline (oracle/): oracle_stream of
    bubbles_reference.py for more than one file."""
    from oracle import oracle as O
    o = O.Oracle(k, L, q, O.seed_table(seed, q, L))
    for f in fastas:
        o.add_fasta(f)
    o.enumerate()
    o.write_bin(out)
    o.close()
    return out
