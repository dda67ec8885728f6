"""The connected components of the compacted graph by their definition, from the text of a gfa1 graph -- the oracle of
test_components_cpu.py and test_gpu_components.py.  Nothing here goes through the project's own component code: the input is what
the serial `graphdump -f gfa1` prints (pinned to the reference's bytes by tests/golden/graphdump.json).  Rows, lengths, occurrences
and presence come through colors_reference; the joined pairs are read off the L lines; the classes are found by a breadth-first
search over Python sets; the TSV and the members file of `--components` are rendered from that."""
import numpy as np

import colors_reference as C
from bubbles_reference import BUBBLE_GENOMES, BUBBLE_HUB, BUBBLE_K, BUBBLE_L, BUBBLE_Q, BUBBLE_SEED, bubble_fasta, oracle_stream  # noqa: F401
from colors_reference import (FRESH, GFA1_VECTORS, GOOD_VECTORS, GRAPHDUMP, TWOPACO, case_vector, colors_args, golden_gfa1, run_graphdump,  # noqa: F401
                              vector_id, vector_of)
from links_reference import class_of, few_events_fasta, reverse_complement, signed  # noqa: F401

components_args = colors_args   # the arguments of a gfa1 vector without its `-f gfa1`


def classes_of(n, pairs):
    """label[r]: the smallest row of the class of r under the transitive closure of the pairs, by breadth-first search."""
    near = [set() for _ in range(n)]
    for a, b in pairs:
        near[a].add(b)
        near[b].add(a)
    label = [-1] * n
    for r in range(n):
        if label[r] >= 0:
            continue
        label[r] = r          # rows are visited in ascending order: the first row met of a class is its smallest
        front = [r]
        while front:
            nxt = []
            for x in front:
                for y in near[x]:
                    if label[y] < 0:
                        label[y] = r
                        nxt.append(y)
            front = nxt
    return label


class Components:
    """component[r] per row; per component root, segments, links, length, edges, occurrences, presence (bool [P, C]), n_colors;
    pairs: the joined rows of every distinct link class, in the order of the classes' first L lines; k from the L lines' overlaps
    (or given, for a graph without any link)."""

    def __init__(self, gfa1_text, by="file", k=None, files=None, color_of_seq=None):
        """color_of_seq: a colour map of the caller's own instead of `by` (as many colours as its largest entry + 1)."""
        self.g = g = C.Gfa1(gfa1_text)
        if color_of_seq is None:
            color_of_seq, self.labels = C.color_map(g, by, files)
        else:
            self.labels = ["colour %d" % c for c in range(max(color_of_seq) + 1)]
        self.by = by
        self.colors = c = C.table(g, color_of_seq, len(self.labels))
        self.rows = len(g.row_name)
        self.row_of = row_of = {n: r for r, n in enumerate(g.row_name)}
        seen = set()
        self.pairs = []
        self.k = k
        for line in gfa1_text.decode().split("\n"):
            f = line.split("\t")
            if f[0] != "L":
                continue
            assert f[5].endswith("M")
            assert self.k in (None, int(f[5][:-1]))
            self.k = int(f[5][:-1])
            a, b = signed(f[1], f[2]), signed(f[3], f[4])
            cl = class_of(a, b)
            if cl not in seen:
                seen.add(cl)
                self.pairs.append((row_of[abs(a)], row_of[abs(b)]))   # strands do not matter
        assert self.k is not None, "no L line: give k"
        self.n_links = len(self.pairs)
        label = classes_of(self.rows, self.pairs)
        self.root = np.array(sorted(set(label)), dtype=np.int64)
        id_of = {int(r): p for p, r in enumerate(self.root.tolist())}
        self.component = np.array([id_of[x] for x in label], dtype=np.int64)
        n = len(self.root)
        self.segments = np.bincount(self.component, minlength=n).astype(np.int64) if self.rows else np.zeros(0, dtype=np.int64)
        self.links = np.zeros(n, dtype=np.int64)
        for a, b in self.pairs:
            assert self.component[a] == self.component[b]
            self.links[self.component[a]] += 1
        self.length = np.zeros(n, dtype=np.int64)
        self.occurrences = np.zeros(n, dtype=np.int64)
        self.presence = np.zeros((n, c["colors"]), dtype=bool)
        np.add.at(self.length, self.component, c["length"])
        np.add.at(self.occurrences, self.component, c["occurrences"])
        for r in range(self.rows):
            self.presence[self.component[r]] |= c["presence"][r]
        self.edges = self.length - self.k * self.segments
        self.n_colors = self.presence.sum(axis=1).astype(np.int64)

    def count(self):
        return len(self.root)

    def largest(self):
        return int(self.segments.max()) if len(self.segments) else 0

    def tsv(self):
        c = self.colors
        out = ["#twopaco-components\t1\tby=%s\tk=%d\tcolors=%d\tsegments=%d\tlinks=%d\tcomponents=%d" % (self.by, self.k, c["colors"], self.rows, self.n_links, self.count())]
        out += ["#color\t%d\t%s" % (i, label) for i, label in enumerate(self.labels)]
        sizes = {}
        for s in self.segments.tolist():
            b = s.bit_length() - 1
            n, total = sizes.get(b, (0, 0))
            sizes[b] = (n + 1, total + s)
        out += ["#size\t%d\t%d\t%d" % (b, sizes[b][0], sizes[b][1]) for b in sorted(sizes)]
        for p in range(self.count()):
            out.append("%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s" % (p, c["name"][self.root[p]], self.segments[p], self.links[p], self.length[p], self.edges[p], self.occurrences[p],
                                                                 self.n_colors[p], C.hex_of(self.presence[p].tolist())))
        return ("\n".join(out) + "\n").encode()

    def members(self):
        out = ["#twopaco-component-members\t1\tk=%d\tsegments=%d\tcomponents=%d" % (self.k, self.rows, self.count())]
        out += ["%d\t%d" % (n, p) for n, p in zip(self.colors["name"].tolist(), self.component.tolist())]
        return ("\n".join(out) + "\n").encode()


_COMPONENTS = {}


def k_of(v):
    return int(v["args"][v["args"].index("-k") + 1])


def golden_components(v, by="file"):
    key = (vector_id(v), by)
    if key not in _COMPONENTS:
        _COMPONENTS[key] = Components(golden_gfa1(v), by, k=k_of(v))
    return _COMPONENTS[key]


# ---------------------------------------------------------------------------------------------- the text alone
def check_partition(tsv, members, gfa1):
    """On the two files' text and the gfa1 text alone, with no code shared with Components: every L line's two names carry one id in
    the members file; ids appear in ascending order of first S line; segments / links / length per component recounted from the text
    equal the table; the segments sum to S.  Returns the number of components."""
    member_lines = members.decode().split("\n")
    assert member_lines[-1] == "" and member_lines[0].startswith("#twopaco-component-members\t1\t")
    id_of, order = {}, []
    for line in member_lines[1:-1]:
        name, p = line.split("\t")
        assert int(name) not in id_of
        id_of[int(name)] = int(p)
        order.append(int(name))
    segments, length, links, first_seen, seen_links = {}, {}, {}, [], set()
    s_names = []
    for line in gfa1.decode().split("\n"):
        f = line.split("\t")
        if f[0] == "S" and len(f) == 3:
            p = id_of[int(f[1])]
            s_names.append(int(f[1]))
            if p not in segments:
                first_seen.append(p)
            segments[p] = segments.get(p, 0) + 1
            length[p] = length.get(p, 0) + len(f[2])
        elif f[0] == "L":
            assert id_of[int(f[1])] == id_of[int(f[3])], line
            a, b = (int(f[1]) if f[2] == "+" else -int(f[1])), (int(f[3]) if f[4] == "+" else -int(f[3]))
            key = min((a, b), (-b, -a))
            if key not in seen_links:
                seen_links.add(key)
                links[id_of[int(f[1])]] = links.get(id_of[int(f[1])], 0) + 1
    assert s_names == order                                    # the members are the rows, in row order
    assert first_seen == list(range(len(first_seen)))          # ids ascend by first S line
    rows = [line.split("\t") for line in tsv.decode().split("\n") if line and not line.startswith("#")]
    head = dict(f.split("=") for f in tsv.decode().split("\n")[0].split("\t")[2:])
    assert [int(r[0]) for r in rows] == list(range(len(first_seen))) and int(head["components"]) == len(rows)
    for r in rows:
        p = int(r[0])
        assert (int(r[2]), int(r[3]), int(r[4])) == (segments[p], links.get(p, 0), length[p]), r
        assert int(r[5]) == length[p] - int(head["k"]) * segments[p]
    assert sum(int(r[2]) for r in rows) == len(s_names) == int(head["segments"])
    assert sum(int(r[3]) for r in rows) == len(seen_links) == int(head["links"])
    return len(rows)


# ---------------------------------------------------------------------------------------------- the generated input
ISLANDS_K, ISLANDS_L, ISLANDS_Q, ISLANDS_SEED = 21, 24, 5, 11
ISLANDS_CHAIN, ISLANDS_REVERSED, ISLANDS_MID = 210000, 60000, 16000
ISLANDS_SMALL, ISLANDS_SINGLE = 72, 40


def islands_records():
    """Every way the union-find can go wrong, in one file (k = 21, so that no two families share a 22-mer by chance):
        s0, s1    a small family FIRST: the largest component's root is not row 0
        a0 .. a3  the CHAIN family: one random base of 210000 letters, a substitution every 35 .. 45 letters, record r takes site i's
                  other allele by the bit (r >> (i % 2)) & 1 -- one component of thousands of bubbles in a row, whose link rows dozens
                  of workgroups hook into one tree at once
        b0 .. b3  the same kind of family over 60000 letters, every record a suffix of it, reverse-complemented, the longest first
        c0 .. c3 and d0 .. d3  two mid-sized families of the same kind over 16000 letters each (c1 carries seven N)
        n0 .. n2  three records that run from random letters into a 21-mer of d's base, an N and random letters: 'N'-named segments
        t*        72 small families of two records, 1 .. 10 substitutions: components of a few segments
        u*        40 records of 60 random letters: exactly one event, no link, a component of one segment
        x*        7 records of exactly k letters, scattered: one junction, too short for any event
        bridge    LAST of all: a stretch of c's base, then a stretch of d's -- the one record that joins the two mid-sized families"""
    rng = np.random.default_rng(20261022)

    def letters(n):
        return "".join("ACGT"[c] for c in rng.integers(0, 4, n))

    def other(ch, step=1):
        return "ACGT"[("ACGT".index(ch) + step) % 4]

    def family(base, n_records, sites):
        out = []
        for r in range(n_records):
            s = list(base)
            for i, at in enumerate(sites):
                if (r >> (i % 2)) & 1:
                    s[at] = other(base[at])
            out.append("".join(s))
        return out

    def chain_sites(n):
        at, sites = 40, []
        while at < n - 40:
            sites.append(at)
            at += int(rng.integers(35, 46))
        return sites

    recs = []
    base = letters(300)
    recs += [("s%d" % r, s) for r, s in enumerate(family(base, 2, [100, 200]))]
    base = letters(ISLANDS_CHAIN)
    recs += [("a%d" % r, s) for r, s in enumerate(family(base, 4, chain_sites(len(base))))]
    recs.append(("x0", letters(ISLANDS_K)))
    base = letters(ISLANDS_REVERSED)
    for r, s in enumerate(family(base, 4, chain_sites(len(base)))):
        recs.append(("b%d" % r, reverse_complement(s[r * (ISLANDS_REVERSED // 8):])))
    mids = []
    for name in "cd":
        base = letters(ISLANDS_MID)
        mids.append(base)
        four = family(base, 4, chain_sites(len(base)))
        if name == "c":
            four[1] = four[1][:8000] + "N" * 7 + four[1][8007:]
        recs += [("%s%d" % (name, r), s) for r, s in enumerate(four)]
    # a 21-mer of d's base followed by N: a junction whose next letter is N, the segment after it gets a fresh name
    recs += [("n%d" % r, letters(30) + mids[1][2000 + 500 * r:2000 + 500 * r + ISLANDS_K] + "N" + letters(30)) for r in range(3)]
    for t in range(ISLANDS_SMALL):
        base = letters(int(rng.integers(120, 600)))
        n_sites = 1 + t % 10
        sites = sorted(set(int(x) for x in rng.integers(30, len(base) - 30, n_sites)))
        recs += [("t%d_%d" % (t, r), s) for r, s in enumerate(family(base, 2, sites))]
        if t % 12 == 0:
            recs.append(("x%d" % (1 + t // 12), letters(ISLANDS_K)))
    recs += [("u%d" % u, letters(60)) for u in range(ISLANDS_SINGLE)]
    recs.append(("bridge", mids[0][5000:5100] + mids[1][9000:9100]))
    return recs


def islands_fasta(path):
    with open(path, "w") as f:
        for name, s in islands_records():
            f.write(">%s\n" % name)
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + "\n")
    return path


def generated_inputs(directory):
    """{name: (fasta, stream, serial gfa1 text, k)} of the generated inputs: `islands` above, `b78` (bubbles_reference: 8 genomes and
    a hub of 70 'N'-named neighbours) and `short` (links_reference: records without any link).  The streams come from the CPU
    restatement of the pipeline (oracle/)."""
    import os
    made = {}
    for name, k, L, q, seed, write in (("islands", ISLANDS_K, ISLANDS_L, ISLANDS_Q, ISLANDS_SEED, islands_fasta),
                                       ("b78", BUBBLE_K, BUBBLE_L, BUBBLE_Q, BUBBLE_SEED, lambda path: bubble_fasta(path, BUBBLE_GENOMES + BUBBLE_HUB)),
                                       ("short", 11, 20, 5, 11, lambda path: few_events_fasta(path, True))):
        fa = write(os.path.join(directory, name + ".fa"))
        stream = oracle_stream(fa, os.path.join(directory, name + ".bin"), k, L, q, seed)
        gfa1 = run_graphdump([stream, "-k", str(k), "-s", fa, "-f", "gfa1"], cwd=directory)
        assert gfa1.returncode == 0 and gfa1.stderr == b"", gfa1.stderr
        made[name] = (fa, stream, gfa1.stdout, k)
    return made


def first_row_of(w, sequence):
    """The row of the first segment of the input sequence named `sequence` (w: a Components)."""
    s = w.g.seq_name.index(sequence)
    return w.row_of[int(w.g.occ_name[np.flatnonzero(w.g.occ_seq == s)[0]])]


def check_islands(w):
    """What islands_records promises, counted on the oracle's own result (w: Components of its gfa1, by sequence)."""
    chain = int(w.component[first_row_of(w, "a0")])
    assert w.links[chain] >= 20000 and w.segments[chain] >= 10000
    assert chain == int(w.segments.argmax()) and w.root[chain] != 0 and chain != 0      # a small family comes first in the file
    back = int(w.component[first_row_of(w, "b0")])
    assert back != chain and w.segments[back] >= 2000 and w.links[back] >= 3000
    assert all(int(w.component[first_row_of(w, "b%d" % r)]) == back for r in range(4))
    # the two mid-sized families hang together through the bridge alone: the shortest prefix of the link rows that joins them ends
    # among the last few rows of the table
    c, d = first_row_of(w, "c0"), first_row_of(w, "d0")
    assert w.component[c] == w.component[d] and w.segments[w.component[c]] >= 2000
    lo, hi = 0, len(w.pairs)
    while lo < hi:
        mid = (lo + hi) // 2
        label = classes_of(w.rows, w.pairs[:mid])
        if label[c] == label[d]:
            hi = mid
        else:
            lo = mid + 1
    assert len(w.pairs) - lo <= 8, (lo, len(w.pairs))
    before = classes_of(w.rows, w.pairs[:lo - 1])
    assert min(sum(1 for x in before if x == before[c]), sum(1 for x in before if x == before[d])) >= 1000   # two large trees, one link
    assert int(((w.segments >= 2) & (w.segments <= 50)).sum()) >= 64
    alone = np.flatnonzero(w.segments == 1)
    assert len(alone) >= 32 and (w.links[alone] == 0).all() and (w.occurrences[alone] == 1).all()
    assert sum(1 for n in w.g.row_name if n >= FRESH) >= 3                               # 'N'-named segments
    assert sum(1 for s in range(len(w.g.seq_name)) if not (w.g.occ_seq == s).any()) >= 7  # records too short for any event
    # every sequence with an event lies in exactly one component
    held = w.presence.sum(axis=0)
    assert set(held.tolist()) <= {0, 1} and int(held.sum()) == len(w.g.seq_name) - 7
