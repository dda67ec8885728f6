"""The bounded superbubbles of the compacted graph by their SET DEFINITION, from the text of a gfa1 graph -- the oracle of
test_superbubbles_cpu.py and test_gpu_superbubbles.py.  Nothing here goes through the project's own superbubble code, and nothing
here is the traversal the project uses: rows, lengths and presence come through colors_reference, the arcs are read off the L lines
as bubbles_reference reads them, and the definition of include/twopaco_hip.h's tpc_segments_superbubbles_* group is stated
literally -- U(s, t) by reachability with t closed, matching by the reverse reachability, acyclicity by a depth-first search on the
induced arcs, the row condition, minimality by trying every inside side, the bound; paths, min_edges and max_edges by dynamic
programming over a topological order of its own (Kahn).  The definition rules: where the traversal disagrees, the traversal is wrong.

The one shortcut is in WHICH exits are tried for an entrance s, and it follows from the bound alone: every side strictly nearer to s
(in arcs, by breadth-first search) than t lies in U(s, t) -- a shortest path to it cannot pass t -- so a t with more than 63 sides
nearer than itself has |U| > 64 and fails the bound.  All other t are tried."""
import numpy as np

import bubbles_reference as B
import colors_reference as C
from bubbles_reference import (GFA1_VECTORS, GOOD_VECTORS, GRAPHDUMP, TWOPACO, bubbles_args, case_vector, golden_gfa1, oracle_stream, plain, read_fasta,  # noqa: F401
                               reverse_complement, rev, run_graphdump, vector_id, vector_of)

superbubbles_args = bubbles_args
NONE = 0xFFFFFFFF
MAX_SIDES = 64       # entrance + at most 62 inside + exit
DEFAULT_MAX_INSIDE = 62


class Superbubbles:
    """out[u] / inn[u]: the sets of heads / tails of the arcs at side u.  exit[s] for every side (NONE: no superbubble enters at s);
    the reported rows in ascending entrance code: entrance, exit, inside, arcs, paths, min_edges, max_edges, presence (bool [B, C]),
    n_colors, members (list of sorted lists); unmirrored: the entrances s with exit(rev(exit(s))) != rev(s); verdicts[(s, t)]: the set
    of the conditions (s, t) fails, for every pair tried, '1' .. '4' and the details 'dead_end', 'back_arc', 'self_loop'."""

    def __init__(self, gfa1_text, k, by="file", files=None, max_inside=DEFAULT_MAX_INSIDE, color_of_seq=None):
        assert 2 <= max_inside <= DEFAULT_MAX_INSIDE
        self.k, self.by, self.max_inside = k, by, max_inside
        self.b = b = B.Bubbles(gfa1_text, by, files)
        self.colors, self.labels, self.segments, self.sides, self.links = b.colors, b.labels, b.segments, b.sides, b.links
        self.g = b.g
        if color_of_seq is not None:   # any colouring of the sequences, for the word boundaries of presence
            n_colors = max(color_of_seq) + 1
            self.colors, self.labels = C.table(b.g, color_of_seq, n_colors), ["c%d" % i for i in range(n_colors)]
        self.out = b.out
        self.inn = [{rev(w) for w in self.out[rev(v)]} for v in range(self.sides)]
        for u in range(self.sides):   # an arc is in out[] of its tail and in inn[] of its head
            assert all(u in self.inn[v] for v in self.out[u])
        self.n_arcs = sum(len(o) for o in self.out)
        self.off = np.zeros(self.sides + 1, dtype=np.int64)
        self.off[1:] = np.cumsum([len(o) for o in self.out])
        self.heads = np.array([v for o in self.out for v in sorted(o)], dtype=np.int64)
        self.weight = (self.colors["length"] - k).tolist()
        self.verdicts = {}
        self.exit = np.full(self.sides, NONE, dtype=np.int64)
        self._u = {}
        for s in range(self.sides):
            if len(self.out[s]) >= 2:
                t = self.exit_of(s)
                if t is not None:
                    self.exit[s] = t
        rows = []
        self.unmirrored = 0
        for s in range(self.sides):
            t = int(self.exit[s])
            if t == NONE:
                continue
            mirrored = int(self.exit[rev(t)]) == rev(s)
            self.unmirrored += not mirrored
            if s < rev(t) or not mirrored:
                rows.append(self.row(s, t))
        self.rows = rows
        n = len(rows)
        self.entrance, self.exits, self.inside, self.arcs, self.n_colors = (np.array([r[key] for r in rows], dtype=np.int64) for key in ("entrance", "exit", "inside", "arcs", "n_colors"))
        self.paths, self.min_edges, self.max_edges = (np.array([r[key] for r in rows], dtype=np.uint64) for key in ("paths", "min_edges", "max_edges"))
        self.presence = np.array([r["presence"] for r in rows], dtype=bool).reshape(n, self.colors["colors"])
        self.members = [r["members"] for r in rows]
        self.member_off = np.zeros(n + 1, dtype=np.int64)
        self.member_off[1:] = np.cumsum([len(m) for m in self.members])
        self.member_sides = np.array([u for m in self.members for u in m], dtype=np.int64)

    # ------------------------------------------------------------------------------------------ the definition
    def reach(self, s, t):
        """U(s, t): the sides reachable from s without leaving t; None beyond 64 sides."""
        seen, todo = {s}, [s]
        while todo:
            v = todo.pop()
            if v == t:
                continue      # a path may end at t but not continue through it
            for u in self.out[v]:
                if u not in seen:
                    if len(seen) == MAX_SIDES:
                        return None
                    seen.add(u)
                    todo.append(u)
        return seen

    def reach_back(self, s, t):
        """The sides from which t is reachable without entering s (s itself may start such a path); None beyond 64 sides."""
        seen, todo = {t}, [t]
        while todo:
            v = todo.pop()
            if v == s:
                continue
            for u in self.inn[v]:
                if u not in seen:
                    if len(seen) == MAX_SIDES:
                        return None
                    seen.add(u)
                    todo.append(u)
        return seen

    def cyclic(self, u_set):
        """A cycle among the arcs with both ends in u_set, by depth-first search (white / grey / black)."""
        colour = {}
        for root in u_set:
            if root in colour:
                continue
            colour[root] = 1
            stack = [(root, iter(sorted(self.out[root] & u_set)))]
            while stack:
                v, it = stack[-1]
                for u in it:
                    if colour.get(u) == 1:
                        return True
                    if u not in colour:
                        colour[u] = 1
                        stack.append((u, iter(sorted(self.out[u] & u_set))))
                        break
                else:
                    colour[v] = 2
                    stack.pop()
        return False

    def failed(self, s, t):
        """The conditions 1-4 that (s, t) fails, as a frozenset (empty: all four hold), and U or None."""
        key = (s, t)
        if key in self._u:
            return self.verdicts[key], self._u[key]
        bad = set()
        u_set = self.reach(s, t)
        if len(self.out[s]) < 2 or u_set is None or t not in u_set:
            bad.add("1")
            u_set = None
        else:
            if self.reach_back(s, t) != u_set:
                bad.add("2")
            # the local statement, checked against the first one on every pair ever tried: the set equality implies it, and it implies the
            # set equality where no cycle lies in U (s -> a -> b -> s with s -> t is closed under it and matches nothing)
            local = all(self.out[v] and self.out[v] <= u_set for v in u_set if v != t) and all(self.inn[v] <= u_set for v in u_set if v != s)
            cyclic = self.cyclic(u_set)
            assert local or "2" in bad, (s, t)
            assert cyclic or local == ("2" not in bad), (s, t)
            if any(not self.out[v] for v in u_set if v != t):
                bad.add("dead_end")
            if cyclic:
                bad.add("3")
                if s in self.out[t]:
                    bad.add("back_arc")
                if any(v in self.out[v] for v in u_set):
                    bad.add("self_loop")
            if len({v >> 1 for v in u_set}) != len(u_set):
                bad.add("4")
        self.verdicts[key] = frozenset(bad)
        self._u[key] = u_set
        return self.verdicts[key], u_set

    def holds(self, s, t):
        return not (self.failed(s, t)[0] & {"1", "2", "3", "4"})

    def candidates(self, s):
        """Every t != s with at most 63 sides strictly nearer to s than itself (see the module's text)."""
        layer, seen, got, nearer = [s], {s}, [], 0
        while layer and nearer <= MAX_SIDES - 1:
            got += [v for v in layer if v != s]
            nearer += len(layer)
            nxt = []
            for v in layer:
                for u in sorted(self.out[v]):
                    if u not in seen:
                        seen.add(u)
                        nxt.append(u)
            layer = nxt
        return got

    def exit_of(self, s):
        found = []
        for t in self.candidates(s):
            if not self.holds(s, t):
                continue
            u_set = self._u[(s, t)]
            if any(self.holds(s, t2) for t2 in u_set - {s, t}):       # 5. minimal
                continue
            if len(u_set) - 2 <= self.max_inside:                      # 6. bounded
                found.append(t)
        assert len(found) <= 1, "a side is the entrance of at most one superbubble"
        return found[0] if found else None

    def row(self, s, t):
        u_set = self._u[(s, t)]
        inside = sorted(u_set - {s, t})
        arcs = sum(len(self.out[v] & u_set) for v in u_set)
        # Kahn over the induced arcs
        indeg = {v: len(self.inn[v] & u_set) for v in u_set}
        order, todo = [], [v for v in u_set if indeg[v] == 0]
        assert todo == [s]
        while todo:
            v = todo.pop()
            order.append(v)
            for u in self.out[v] & u_set:
                indeg[u] -= 1
                if indeg[u] == 0:
                    todo.append(u)
        assert len(order) == len(u_set)
        paths, low, high = {s: 1}, {s: 0}, {s: 0}
        for v in order:
            for u in self.out[v] & u_set:
                w = 0 if u == t else self.weight[u >> 1]
                paths[u] = paths.get(u, 0) + paths[v]
                low[u] = min(low.get(u, 1 << 70), low[v] + w)
                high[u] = max(high.get(u, 0), high[v] + w)
        presence = np.zeros(self.colors["colors"], dtype=bool)
        for v in inside:
            presence |= self.colors["presence"][v >> 1]
        return {"entrance": s, "exit": t, "inside": len(inside), "arcs": arcs, "paths": paths[t], "min_edges": low[t], "max_edges": high[t], "presence": presence,
                "n_colors": int(presence.sum()), "members": inside}

    def count(self):
        return len(self.rows)

    # ------------------------------------------------------------------------------------------ the two files
    def spelled(self, code):
        return "%d\t%s" % (self.colors["name"][code >> 1], "-" if code & 1 else "+")

    def tsv(self):
        out = ["#twopaco-superbubbles\t1\tby=%s\tk=%d\tcolors=%d\tsegments=%d\tlinks=%d\tmax_inside=%d\tsuperbubbles=%d" % (
            self.by, self.k, self.colors["colors"], self.segments, self.links, self.max_inside, self.count())]
        out += ["#color\t%d\t%s" % (i, label) for i, label in enumerate(self.labels)]
        sizes = np.bincount(self.inside, minlength=1) if self.count() else []
        out += ["#inside\t%d\t%d" % (n, c) for n, c in enumerate(sizes) if c]
        for r in self.rows:
            out.append("\t".join([self.spelled(r["entrance"]), self.spelled(r["exit"])] + ["%d" % r[key] for key in ("inside", "arcs", "paths", "min_edges", "max_edges", "n_colors")] +
                                 [C.hex_of(r["presence"].tolist())]))
        return ("\n".join(out) + "\n").encode()

    def members_tsv(self):
        out = ["#twopaco-superbubble-members\t1\tk=%d\tsegments=%d\tmax_inside=%d\tsuperbubbles=%d\tmembers=%d" % (self.k, self.segments, self.max_inside, self.count(), len(self.member_sides))]
        out += ["%d\t%s" % (i, self.spelled(u)) for i, m in enumerate(self.members) for u in m]
        return ("\n".join(out) + "\n").encode()


def k_of(v):
    return int(v["args"][v["args"].index("-k") + 1])


_GOLDEN = {}


def golden_superbubbles(v, by="file", max_inside=DEFAULT_MAX_INSIDE):
    key = (vector_id(v), by, max_inside)
    if key not in _GOLDEN:
        _GOLDEN[key] = Superbubbles(golden_gfa1(v), k_of(v), by, max_inside=max_inside)
    return _GOLDEN[key]


# ---------------------------------------------------------------------------------------------- the text alone, spelled back
def check_text(tsv_text, members_text, gfa1_text, k, overlaps=True):
    """On the two files and the S and L lines alone, with code of its own: every first member (one the entrance has an arc to) begins,
    oriented, with the last k letters of the oriented entrance; every member's oriented body lies on some path of overlapping bodies
    from the entrance to the exit that stays within the members; the header's counts and the #inside lines agree with the rows.
    overlaps=False leaves the letters out and keeps the paths: with an abundance cut one name covers different bodies, in the
    reference's own gfa1 as well (rand6_k9_a3, as test_bubbles_cpu.py says).  Returns the number of rows."""
    body, arcs = {}, set()
    for line in gfa1_text.decode().split("\n"):
        f = line.split("\t")
        if f[0] == "S" and len(f) == 3:
            body[int(f[1])] = plain(f[2])
        elif f[0] == "L":
            a, b = (int(f[1]), f[2]), (int(f[3]), f[4])
            arcs.add((a, b))
            arcs.add(((b[0], "+-"[b[1] == "+"]), (a[0], "+-"[a[1] == "+"])))

    def oriented(side):
        return body[side[0]] if side[1] == "+" else reverse_complement(body[side[0]])

    members = {}
    lines = members_text.decode().split("\n")
    assert lines[-1] == "" and lines[0].startswith("#twopaco-superbubble-members\t1\t")
    for line in lines[1:-1]:
        i, name, strand = line.split("\t")
        members.setdefault(int(i), []).append((int(name), strand))
    rows, sizes, header = 0, {}, None
    for line in tsv_text.decode().split("\n"):
        if line.startswith("#twopaco-superbubbles"):
            header = dict(f.split("=") for f in line.split("\t")[2:])
        if line.startswith("#inside"):
            _, n, c = line.split("\t")
            sizes[int(n)] = int(c)
        if not line or line.startswith("#"):
            continue
        f = line.split("\t")
        assert len(f) == 11, line
        s, t = (int(f[0]), f[1]), (int(f[2]), f[3])
        inside = members.get(rows, [])
        assert len(inside) == int(f[4]) <= int(header["max_inside"]) and len(set(n for n, _ in inside)) == len(inside), line
        allowed = set(inside) | {s, t}
        nxt = {u: [v for v in allowed if (u, v) in arcs] for u in allowed}
        assert sum(len(v) for v in nxt.values()) == int(f[5]), line
        for u, vs in nxt.items():
            for v in vs:
                assert not overlaps or oriented(u)[-k:] == oriented(v)[:k], line
        # forward from the entrance and backward from the exit: every member lies on a path
        fwd, todo = {s}, [s]
        while todo:
            for v in nxt[todo.pop()]:
                if v not in fwd:
                    fwd.add(v)
                    todo.append(v)
        back, todo = {t}, [t]
        while todo:
            v = todo.pop()
            for u in allowed:
                if v in nxt[u] and u not in back:
                    back.add(u)
                    todo.append(u)
        assert fwd == allowed == back, line
        first = nxt[s]
        assert len(first) >= 2 and (not overlaps or all(oriented(v)[:k] == oriented(s)[-k:] for v in first)), line
        rows += 1
    assert header is not None and int(header["superbubbles"]) == rows and sum(sizes.values()) == rows
    assert sum(n * c for n, c in sizes.items()) == len(lines) - 2
    return rows


# ---------------------------------------------------------------------------------------------- the generated input
SB_K, SB_L, SB_Q, SB_SEED = 21, 20, 5, 11
SB_GENOMES, SB_HUB = 8, 70
SITES = {"two_subs": 300, "three_alleles": 600, "nested": 900, "del_sub": 1300, "inverted": 1700, "dead_end": 2100, "cluster": 2500, "n_run": 3000, "simple": 3400,
         "insertion": 3700, "four_alleles": 4000}
CLUSTER_SITES, CLUSTER_STEP = 11, 12


def other(ch, step=1):
    return "ACGT"[("ACGT".index(ch) + step) % 4]


def superbubble_records():
    """8 records over one random base of 4400 letters; record r carries allele bits b0 = r & 1, b1 = (r >> 1) & 1 at the sites of
    SITES, far enough apart (300 letters and more, k = 21) not to interact:
        two_subs       substitutions at +0 (b0) and +8 (b1): closer than k, four haplotypes
        three_alleles  one of three letters by r % 3                four_alleles   one of four letters by r % 4
        nested         an insertion of 60 letters (b0) with a substitution at its letter 30 (b1): the inner bubble and the outer one
        del_sub        a 3-letter deletion (b0) beside a substitution at +10 (b1)
        inverted       an insertion Q x rc(Q) (b0), Q of 40 and x of 30 letters: both strands of Q's row between entrance and exit
        dead_end       the extra record `stop`: base[2040:2110] with a substitution at 2100 that no other record has -- it stops in its arm
        cluster        11 substitutions 12 apart, the even ones by b0 and the odd ones by b1: one superbubble, two sides per site and four
                       per pair of neighbours inside
        n_run          seven N in record 6                           simple         a substitution (b0)
        insertion      GATTA (b1)
    Record 5 is reverse-complemented.  Then two records of a ring, P x Q P and P x' Q P[:k]: a simple bubble whose sink has an arc to
    its source.  Then the hub of bubbles_reference: 70 short records that share one k-mer before an N."""
    rng = np.random.default_rng(20261020)

    def letters(n):
        return "".join("ACGT"[c] for c in rng.integers(0, 4, n))

    base = letters(4400)
    ins, q, x, p_ring, q_ring = letters(60), letters(40), letters(30), letters(50), letters(50)
    recs = []
    for r in range(SB_GENOMES):
        b0, b1 = r & 1, (r >> 1) & 1
        s = list(base)
        # from the right, so that the sites further left keep their places
        at = SITES["four_alleles"]
        s[at] = other(base[at], r % 4)
        if b1:
            at = SITES["insertion"]
            s[at:at] = list("GATTA")
        if b0:
            s[SITES["simple"]] = other(base[SITES["simple"]])
        for i in range(CLUSTER_SITES):
            at = SITES["cluster"] + CLUSTER_STEP * i
            if (b1 if i % 2 else b0):
                s[at] = other(base[at], 1 + i % 3)
        if b0:
            at = SITES["inverted"]
            s[at:at] = list(q + x + reverse_complement(q))
        at = SITES["del_sub"]
        if b1:
            s[at + 10] = other(base[at + 10])
        if b0:
            del s[at:at + 3]
        if b0:
            at = SITES["nested"]
            s[at:at] = list(ins[:30] + (other(ins[30]) if b1 else ins[30]) + ins[31:])
        at = SITES["three_alleles"]
        s[at] = other(base[at], r % 3)
        at = SITES["two_subs"]
        if b0:
            s[at] = other(base[at])
        if b1:
            s[at + 8] = other(base[at + 8], 2)
        s = "".join(s)
        if r == 6:
            at = s.index(base[SITES["n_run"]:SITES["n_run"] + 30])
            s = s[:at] + "N" * 7 + s[at + 7:]
        if r == 5:
            s = reverse_complement(s)
        recs.append(("g%d" % r, s))
    at = SITES["dead_end"]
    recs.append(("stop", base[at - 60:at] + other(base[at], 3) + base[at + 1:at + 10]))
    recs.append(("ring0", p_ring + "A" + q_ring + p_ring))
    recs.append(("ring1", p_ring + "C" + q_ring + p_ring[:SB_K]))
    for h in range(SB_HUB):
        recs.append(("h%d" % h, letters(20) + base[1000:1000 + SB_K] + "N" + letters(25)))
    return recs


SB_RECORDS = SB_GENOMES + 3   # without the hub


def superbubble_fasta(path, n_records):
    with open(path, "w") as f:
        for name, s in superbubble_records()[:n_records]:
            f.write(">%s\n" % name)
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + "\n")
    return path


# ---------------------------------------------------------------------------------------------- what the generated input must hold
def check_kinds(full, at8, at2):
    """On the oracle's own results for the generated input at max_inside 62, 8 and 2: every kind occurs, every rejection by its reason.
    Returns the number of entrances without a mirror at the default bound."""
    inside = full.inside.tolist()
    assert 2 in inside and 3 in inside and 4 in inside and max(inside) > 8, sorted(set(inside))
    assert max(inside) <= DEFAULT_MAX_INSIDE
    assert int(full.paths.max()) >= 3 and (full.min_edges != full.max_edges).any()
    # nested: a reported row whose members hold the entrance and the exit of another reported row
    pairs = {(r["entrance"], r["exit"]) for r in full.rows}
    assert any(s in r["members"] and t in r["members"] for r in full.rows for s, t in pairs), "no nested superbubble"
    # the bound: the large rows leave, the small ones stay
    assert at8.count() < full.count() and max(at8.inside.tolist()) <= 8 and at2.count() < at8.count() and set(at2.inside.tolist()) <= {1, 2}
    keep8 = [r for r in full.rows if r["inside"] <= 8]
    assert [(r["entrance"], r["exit"]) for r in keep8] == [(r["entrance"], r["exit"]) for r in at8.rows]
    # the rejections, each by its reason: a pair that holds everything else
    reasons = {}
    for (s, t), bad in full.verdicts.items():
        reasons.setdefault(bad, []).append((s, t))
    assert any(bad == {"4"} for bad in reasons), "no pair rejected by the row condition alone"
    assert any("dead_end" in bad and "3" not in bad and "4" not in bad for bad in reasons), "no dead end inside"
    assert any(bad == {"3", "back_arc"} for bad in reasons), "no pair rejected by an arc from exit to entrance alone"
    # the ring's pair is a simple bubble all the same
    simple = {(int(s), int(t)) for s, t in zip(full.b.source, full.b.sink)}
    ring = [(s, t) for s, t in reasons[frozenset({"3", "back_arc"})] if (s, t) in simple]
    assert ring and all(int(full.exit[s]) == NONE for s, _ in ring)
    assert int(full.b.deg.max()) >= 20, "no hub"
    return full.unmirrored


def simple_rows(sb):
    """(entrance, exit) of the rows with inside == 2 and arcs == 4 whose two members both follow the entrance, and (source, sink) of the
    simple bubbles without an arc from sink to source: the cross-check says they are the same list.  inside == 2 and arcs == 4 alone do
    not say it: s -> a -> b -> t beside the arc s -> t (a deletion next to a chain of two segments; rand6_k9_a3 holds one) has two sides
    inside, four arcs and two paths, is minimal, and is no simple bubble."""
    mine = [(r["entrance"], r["exit"]) for r in sb.rows if r["inside"] == 2 and r["arcs"] == 4 and set(r["members"]) == sb.out[r["entrance"]]]
    theirs = [(int(s), int(t)) for s, t in zip(sb.b.source, sb.b.sink) if int(s) not in sb.out[int(t)]]
    return mine, theirs
