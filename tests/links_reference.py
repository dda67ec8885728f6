"""The link table and the compact gfa1 by their definition, from the text of a gfa1 graph -- the oracle of test_links_cpu.py and
test_gpu_links.py.  Nothing here goes through the project's own link code: the input is what the serial `graphdump -f gfa1`
prints (pinned to the reference's bytes by tests/golden/graphdump.json).  The serial walk prints, per event e in event order,
    [S <segment> <body>]                     when e is the first sight of its segment
    C <segment> <strand> <sequence> + <pos>  always: the e-th C line is event e
    [L <a> <sa> <b> <sb> <k>M]               when e is not the first event of its sequence: one link occurrence, closed by e
and P <sequence> <path> * after the last event of a sequence.  From that text: the rows of include/twopaco_hip.h's
tpc_segments_links_* group, the link_first bits, the TSV of `--links`, and the compact text by filtering lines."""
import numpy as np

from colors_reference import (FRESH, GFA1_VECTORS, GOOD_VECTORS, GRAPHDUMP, TRACTS_VECTORS, TWOPACO, case_vector, colors_args, golden_gfa1, run_graphdump,  # noqa: F401
                              vector_id, vector_of)

links_args = colors_args   # the arguments of a gfa1 vector without its `-f gfa1`


def signed(name, strand):
    assert strand in "+-"
    return int(name) if strand == "+" else -int(name)


def class_of(a, b):
    """The class of the occurrence (a, b): it is the same link as (-b, -a)."""
    return min((a, b), (-b, -a))


class Links:
    """rows in the order of the classes' first occurrences; per row the spelling of that occurrence (from, to), first_event, count,
    same; first_bits: one bool per event; events, occurrences, segments; longest_run: of equal classes in consecutive occurrences
    of one sequence."""

    def __init__(self, gfa1_text):
        lines = gfa1_text.decode().split("\n")
        assert lines[-1] == ""
        self.lines = lines[:-1]
        self.keep = []          # per line: it stays in the compact text
        row_of = {}
        self.frm, self.to, self.first_event, self.count, self.same = [], [], [], [], []
        first_events = []
        e = -1
        self.segments = 0
        self.k = None
        self.both = set()       # rows seen in both spellings
        self.longest_run, run, last = 0, 0, None
        self.touches_named = 0
        for line in self.lines:
            f = line.split("\t")
            if f[0] == "H":
                self.keep.append(True)
            elif f[0] == "S" and len(f) == 4 and f[2] == "*" and f[3].startswith("UR:Z:"):
                self.keep.append(False)
            elif f[0] == "S":
                assert len(f) == 3, line
                self.segments += 1
                self.keep.append(True)
            elif f[0] == "C":
                e += 1
                self.keep.append(False)
            elif f[0] == "L":
                assert len(f) == 6 and f[5].endswith("M"), line
                self.k = int(f[5][:-1])
                a, b = signed(f[1], f[2]), signed(f[3], f[4])
                c = class_of(a, b)
                if c not in row_of:
                    row_of[c] = len(self.frm)
                    self.frm.append(a)
                    self.to.append(b)
                    self.first_event.append(e)
                    self.count.append(0)
                    self.same.append(0)
                    first_events.append(e)
                    self.keep.append(True)
                    if abs(a) >= FRESH or abs(b) >= FRESH:
                        self.touches_named += 1
                else:
                    self.keep.append(False)
                r = row_of[c]
                self.count[r] += 1
                if (a, b) == (self.frm[r], self.to[r]):
                    self.same[r] += 1
                else:
                    self.both.add(r)
                run = run + 1 if c == last else 1
                last = c
                self.longest_run = max(self.longest_run, run)
            elif f[0] == "P":
                self.keep.append(True)
                last = None
            else:
                raise AssertionError(line)
        self.events = e + 1
        self.occurrences = sum(self.count)
        self.first_bits = np.zeros(self.events, dtype=bool)
        self.first_bits[np.array(first_events, dtype=np.int64)] = True
        self.first_event = np.array(self.first_event, dtype=np.int64)
        self.count = np.array(self.count, dtype=np.int64)
        self.same = np.array(self.same, dtype=np.int64)

    def rows(self):
        return len(self.frm)

    def tsv(self, k):
        out = ["#twopaco-links\t1\tk=%d\tsegments=%d\tlinks=%d\toccurrences=%d" % (k, self.segments, self.rows(), self.occurrences)]
        for r in range(self.rows()):
            a, b = self.frm[r], self.to[r]
            out.append("%d\t%s\t%d\t%s\t%d\t%d" % (abs(a), "+" if a >= 0 else "-", abs(b), "+" if b >= 0 else "-", self.count[r], self.same[r]))
        return ("\n".join(out) + "\n").encode()

    def compact(self):
        return "".join(line + "\n" for line, keep in zip(self.lines, self.keep) if keep).encode()


_LINKS = {}


def golden_links(v):
    key = vector_id(v)
    if key not in _LINKS:
        _LINKS[key] = Links(golden_gfa1(v))
    return _LINKS[key]


# ---------------------------------------------------------------------------------------------- the compact text alone, spelled back
def read_fasta(path):
    """[(header, letters upper-cased)]"""
    recs = []
    for line in open(path):
        if line.startswith(">"):
            recs.append([line[1:].rstrip("\n"), []])
        elif recs:
            recs[-1][1].append("".join(line.split()).upper())
    return [(h, "".join(b)) for h, b in recs]


_COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


def plain(s):
    """Letters other than A C G T read as N: the graph's reverse-complemented bodies hold them as N."""
    return "".join(c if c in "ACGT" else "N" for c in s)


def reverse_complement(s):
    return "".join(_COMPLEMENT.get(c, "N") for c in reversed(s))


def spell_back(compact_text, k, sequences):
    """The compact gfa1 stands on its own: every P path spells a substring of one input sequence, consecutive segments overlap by
    k, and every step is a printed L line in one of its two spellings.  Returns (paths, steps) checked."""
    body, printed = {}, set()
    paths = []
    for line in compact_text.decode().split("\n"):
        f = line.split("\t")
        if f[0] == "S":
            assert len(f) == 3 and int(f[1]) not in body, line
            body[int(f[1])] = plain(f[2])
        elif f[0] == "L":
            assert f[5] == "%dM" % k, line
            spelled = (signed(f[1], f[2]), signed(f[3], f[4]))
            reverse = (-spelled[1], -spelled[0])
            assert spelled not in printed and (reverse == spelled or reverse not in printed), "a link printed twice: " + line
            printed.add(spelled)
        elif f[0] == "P":
            paths.append((f[1], [signed(s[:-1], s[-1]) for s in f[2].split(",")]))
        else:
            assert f[0] in ("H", ""), line
    haystack = [plain(s) for _, s in sequences]
    steps = 0
    for name, path in paths:
        oriented = [body[abs(s)] if s > 0 else reverse_complement(body[abs(s)]) for s in path]
        spelled = oriented[0]
        for i in range(1, len(path)):
            assert oriented[i - 1][-k:] == oriented[i][:k], (name, i)
            assert (path[i - 1], path[i]) in printed or (-path[i], -path[i - 1]) in printed, (name, path[i - 1], path[i])
            spelled += oriented[i][k:]
            steps += 1
        assert any(spelled in s for s in haystack), name
    return len(paths), steps


# ---------------------------------------------------------------------------------------------- records with 0, 1 and 2 events
FEW_K, FEW_L, FEW_Q, FEW_SEED = 11, 20, 5, 11


def few_events_fasta(path, only_short=False):
    """Records whose walks have 0, 1 and 2 events (a record's events are its junction occurrences less one; the ends of a record
    are junctions, and so is a k-mer that is followed by different letters in two places): a record of exactly k letters has one
    junction and no event, one of plain random letters has one event, and two records that begin alike and go on differently
    have two each.  only_short: the records without any link alone."""
    rng = np.random.default_rng(20261018)
    def letters(n):
        return "".join("ACGT"[c] for c in rng.integers(0, 4, n))
    recs = [("none", letters(FEW_K)), ("one", letters(40)), ("also_one", letters(33))]
    if not only_short:
        head = letters(30)
        recs += [("two", head + "A" + letters(30)), ("none_again", letters(FEW_K)), ("two_again", head + "C" + letters(44))]
    with open(path, "w") as f:
        for name, s in recs:
            f.write(">%s\n%s\n" % (name, s))
    return path
