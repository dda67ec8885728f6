"""The simple bubbles of the compacted graph by their definition, from the text of a gfa1 graph -- the oracle of
test_bubbles_cpu.py and test_gpu_bubbles.py.  Nothing here goes through the project's own bubble code: the input is what the
serial `graphdump -f gfa1` prints (pinned to the reference's bytes by tests/golden/graphdump.json).  Rows, lengths, occurrences
and presence come through colors_reference; the arcs are read off the L lines into Python sets; the definition of
include/twopaco_hip.h's tpc_segments_bubbles_* group is stated literally; the TSV of `--bubbles` is rendered from that."""
import numpy as np

import colors_reference as C
from colors_reference import (FRESH, GFA1_VECTORS, GOOD_VECTORS, GRAPHDUMP, TRACTS_VECTORS, TWOPACO, case_vector, colors_args, golden_gfa1, run_graphdump,  # noqa: F401
                              vector_id, vector_of)
from links_reference import class_of, few_events_fasta, plain, read_fasta, reverse_complement, signed  # noqa: F401

bubbles_args = colors_args   # the arguments of a gfa1 vector without its `-f gfa1`
BINS = 6                     # degree 0, 1, 2, 3, 4, 5 or more


def rev(code):
    return code ^ 1


class Bubbles:
    """out[u]: the set of heads of the arcs that leave side u (u = row * 2 + 1 for '-'); deg / lo / hi as the device keeps them;
    source / arm_a / arm_b / sink: the bubble rows in ascending source code; hist[6]; arcs; links (distinct classes)."""

    def __init__(self, gfa1_text, by="file", files=None):
        self.g = g = C.Gfa1(gfa1_text)
        color_of_seq, self.labels = C.color_map(g, by, files)
        self.by = by
        self.colors = C.table(g, color_of_seq, len(self.labels))
        self.segments = len(g.row_name)
        row_of = {n: r for r, n in enumerate(g.row_name)}

        def side(x):
            return row_of[abs(x)] * 2 + (1 if x < 0 else 0)

        self.sides = 2 * self.segments
        self.out = [set() for _ in range(self.sides)]
        classes = set()
        for line in gfa1_text.decode().split("\n"):
            f = line.split("\t")
            if f[0] != "L":
                continue
            a, b = signed(f[1], f[2]), signed(f[3], f[4])
            classes.add(class_of(a, b))
            # the arc from -> to and the arc rev(to) -> rev(from); a set holds an arc once however often it is printed, and a
            # link that is its own reverse gives one arc
            self.out[side(a)].add(side(b))
            self.out[rev(side(b))].add(rev(side(a)))
        self.links = len(classes)
        self.arcs = sum(len(o) for o in self.out)
        self.deg = np.array([len(o) for o in self.out], dtype=np.int64)
        self.lo = np.array([min(o) if o else 0xFFFFFFFF for o in self.out], dtype=np.int64)
        self.hi = np.array([max(o) if o else 0 for o in self.out], dtype=np.int64)
        self.hist = np.bincount(np.minimum(self.deg, BINS - 1), minlength=BINS).astype(np.int64) if self.sides else np.zeros(BINS, dtype=np.int64)
        rows = []
        for s in range(self.sides):
            found = self.bubble_at(s)
            if found is None:
                continue
            a, b, t = found
            # found twice, at s and at rev(t): reported once, where the source code is the smaller
            if s < rev(t):
                rows.append((s, a, b, t))
        self.source, self.arm_a, self.arm_b, self.sink = (np.array([r[i] for r in rows], dtype=np.int64) for i in range(4))

    def bubble_at(self, s):
        out = self.out
        if len(out[s]) != 2:
            return None
        a, b = sorted(out[s])                                    # the arm with the smaller code first
        if len(out[rev(a)]) != 1 or len(out[rev(b)]) != 1:       # s is the only way in to each arm
            return None
        if len(out[a]) != 1 or len(out[b]) != 1 or out[a] != out[b]:
            return None
        (t,) = out[a]
        if len(out[rev(t)]) != 2:
            return None
        if len({s >> 1, a >> 1, b >> 1, t >> 1}) != 4:          # four different rows
            return None
        return a, b, t

    def bubbles(self):
        return len(self.source)

    def tsv(self, k):
        c = self.colors
        out = ["#twopaco-bubbles\t1\tby=%s\tk=%d\tcolors=%d\tsegments=%d\tlinks=%d\tbubbles=%d" % (self.by, k, c["colors"], self.segments, self.links, self.bubbles())]
        out += ["#color\t%d\t%s" % (i, label) for i, label in enumerate(self.labels)]
        out += ["#sides\t%s\t%d" % ("5+" if d == BINS - 1 else str(d), self.hist[d]) for d in range(BINS) if self.hist[d]]

        def spelled(code):
            return "%d\t%s" % (c["name"][code >> 1], "-" if code & 1 else "+")

        for s, a, b, t in zip(self.source.tolist(), self.arm_a.tolist(), self.arm_b.tolist(), self.sink.tolist()):
            ra, rb = a >> 1, b >> 1
            both = int((c["presence"][ra] & c["presence"][rb]).sum())
            out.append("\t".join([spelled(s), spelled(a), spelled(b), spelled(t)] +
                                 ["%d" % v for v in (c["length"][ra], c["length"][rb], c["occurrences"][ra], c["occurrences"][rb], c["n_colors"][ra], c["n_colors"][rb])] +
                                 [C.hex_of(c["presence"][ra].tolist()), C.hex_of(c["presence"][rb].tolist()), "%d" % both]))
        return ("\n".join(out) + "\n").encode()


_BUBBLES = {}


def golden_bubbles(v, by="file"):
    key = (vector_id(v), by)
    if key not in _BUBBLES:
        _BUBBLES[key] = Bubbles(golden_gfa1(v), by)
    return _BUBBLES[key]


# ---------------------------------------------------------------------------------------------- the text alone, spelled back
def check_arms_overlap(tsv_text, gfa1_text, k):
    """On the table's text and the S lines alone: for every row the two arm bodies, oriented, begin with the last k letters of
    the oriented source and end with the first k letters of the oriented sink.  Returns the number of rows checked."""
    body = {}
    for line in gfa1_text.decode().split("\n"):
        f = line.split("\t")
        if f[0] == "S" and len(f) == 3:
            body[int(f[1])] = plain(f[2])

    def oriented(name, strand):
        assert strand in "+-"
        return body[int(name)] if strand == "+" else reverse_complement(body[int(name)])

    rows = 0
    for line in tsv_text.decode().split("\n"):
        if not line or line.startswith("#"):
            continue
        f = line.split("\t")
        assert len(f) == 17, line
        source, arm_a, arm_b, sink = (oriented(f[2 * i], f[2 * i + 1]) for i in range(4))
        for arm, length in ((arm_a, int(f[8])), (arm_b, int(f[9]))):
            assert len(arm) == length, line
            assert arm[:k] == source[-k:] and arm[-k:] == sink[:k], line
        rows += 1
    return rows


# ---------------------------------------------------------------------------------------------- the generated input
BUBBLE_K, BUBBLE_L, BUBBLE_Q, BUBBLE_SEED = 11, 20, 5, 11
BUBBLE_GENOMES, BUBBLE_HUB = 8, 70


def bubble_records():
    """8 records over one random base of 6000 letters with a site every 150 letters from 150 to 5700; site i of record r takes
    its allele bit (r >> (i % 3)) & 1 and is of kind i % 6:
        0  a substitution, two alleles            1  a 3-letter deletion              2  the insertion GATTA
        3  one of three letters by r % 3: three alleles, not a simple bubble
        4  two substitutions five apart: one bubble with longer arms                 5  a substitution in record 7 only
    Record 5 is reverse-complemented, record 6 carries seven N at 3000.  Then 70 short records, 20 random letters +
    base[1000:1011] + N + 25 random letters: one side with many 'N'-named neighbours (the hub)."""
    rng = np.random.default_rng(20261019)
    base = "".join("ACGT"[c] for c in rng.integers(0, 4, 6000))

    def other(ch, step=1):
        return "ACGT"[("ACGT".index(ch) + step) % 4]

    recs = []
    for r in range(BUBBLE_GENOMES):
        s = list(base)
        # from the right, so that the sites further left keep their places
        for i in reversed(range(38)):
            at = 150 * (i + 1)
            bit = (r >> (i % 3)) & 1
            kind = i % 6
            if kind == 0 and bit:
                s[at] = other(base[at])
            elif kind == 1 and bit:
                del s[at:at + 3]
            elif kind == 2 and bit:
                s[at:at] = list("GATTA")
            elif kind == 3:
                s[at] = other(base[at], r % 3)
            elif kind == 4 and bit:
                s[at] = other(base[at])
                s[at + 5] = other(base[at + 5], 2)
            elif kind == 5 and r == 7:
                s[at] = other(base[at], 3)
        s = "".join(s)
        if r == 6:
            s = s[:3000] + "N" * 7 + s[3007:]
        if r == 5:
            s = reverse_complement(s)
        recs.append(("g%d" % r, s))
    for h in range(BUBBLE_HUB):
        head = "".join("ACGT"[c] for c in rng.integers(0, 4, 20))
        tail = "".join("ACGT"[c] for c in rng.integers(0, 4, 25))
        recs.append(("h%d" % h, head + base[1000:1011] + "N" + tail))
    return recs


def bubble_fasta(path, n_records):
    with open(path, "w") as f:
        for name, s in bubble_records()[:n_records]:
            f.write(">%s\n" % name)
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + "\n")
    return path


def oracle_stream(fasta, out, k, L, q, seed):
    """The junction stream of a FASTA file from the CPU restatement of the pipeline (oracle/)."""
    from oracle import oracle as O
    o = O.Oracle(k, L, q, O.seed_table(seed, q, L))
    o.add_fasta(fasta)
    o.enumerate()
    o.write_bin(out)
    o.close()
    return out
