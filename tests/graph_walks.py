"""GENERATED TOPOLOGIES for the six graph-table stages (colours, links, simple bubbles, distances, connected components, superbubbles):
synthetic junction streams that decide the compacted graph, and the references that hold them at any size.  Builders only: numpy, the
references of this directory and the serial `graphdump -f gfa1` they read; no device and none of the project's Python.

A segment's name is (start junction id, deciding letter) and a link is two consecutive events of one sequence, so a list of WALKS over
signed junction ids with drawn or painted letters makes any topology: self-loops, links that are their own reverse, both strands,
hubs, cycles.  The text does not have to be consistent with the ids.  Every walk is laid out the same way (lay): k = 3, record i at
position 3 i, a sequence of 3 n letters for n records; event i reads letter 3 i + 3 when forward and 3 i + 2 when reverse, so every
event has a deciding letter of its own and any letter can be painted without touching another event.

Three references:
  Oracles   the independent oracles of this directory over the serial gfa1 text (small cases: forest, bound, one tile)
  Direct    the link rows, side degrees, colour rows and components straight from segments_reference.walk in numpy, at any size, for
            graphs without a side of degree 2 or more that could open a bubble (chains, hubs); pinned to the oracles on small cases
  tiled     a tile's Oracles repeated T times by arithmetic: a gadget written T times with its ids shifted gives every table of one
            gadget repeated with constant shifts (rows + t R, side codes + 2 t R, events + t E, components + t P, names by the id shift,
            'N' names + t n_named; sums, counts and paths repeat) -- pinned to the oracles of the T-fold stream at T = 3 and 5
Each builder asserts, from the references alone, that the property it is named after occurs a stated number of times."""
import os
import subprocess
import tempfile
import time
import types

import numpy as np

import bubbles_reference as B
import colors_reference as C
import components_reference as CM
import distances_reference as D
import links_reference as L
import segments_reference as R
import superbubbles_reference as S

K = 3
GAP = 3
NONE = 0xFFFFFFFF
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)
TURN = 8192 * 256             # col_grid: events, link slots, link rows, segment rows, sides, arc keys
TURN_HIST = 1024 * 256        # k_bub_hist and k_col_rows<true>
TURN_SEARCH = 8192 * 64       # k_sb_search: candidates
TURN_REPORT = 65535           # k_sb_report: rows


def lay(rng, walks, paint=()):
    """(seqs, sequences) of walks (one array of signed ids each): letters drawn from ACGT, then paint = [(walk, event, letter)] sets
    the deciding letter of that event -- which position decides does not depend on the letters."""
    seqs, sequences = [], []
    for ids in walks:
        ids = np.asarray(ids, dtype=np.int64)
        seqs.append(LETTERS[rng.integers(0, 4, GAP * ids.size)])
        sequences.append((GAP * np.arange(ids.size, dtype=np.int64), ids))
    for wk, e, letter in paint:
        ids = sequences[wk][1]
        l, r = abs(int(ids[e])), abs(int(ids[e + 1]))
        forward = l < r or (l == r and l > 0)
        seqs[wk][GAP * e + (K if forward else GAP - 1)] = ord(letter)
    return seqs, sequences


class Case:
    """k, the text (seqs), the stream's records per sequence, its bytes, the colour of every sequence; walk() on demand."""

    def __init__(self, name, seqs, sequences, n_colors=3, data=None, color_of_seq=None):
        n_colors = min(n_colors, len(seqs))        # every colour is held by a sequence: the oracles count them off the map
        self.name, self.k, self.seqs, self.sequences, self.n_colors = name, K, seqs, sequences, n_colors
        self.color_of_seq = [s % n_colors for s in range(len(seqs))] if color_of_seq is None else color_of_seq
        self.data = R.build_stream(sequences, last_separator=True) if data is None else data
        self._w = self._gfa1 = None
        self._oracles = {}

    @property
    def w(self):
        if self._w is None:
            self._w = R.walk(self.data, self.seqs, self.k)
            assert self._w.error is None and self._w.ok.all()
        return self._w

    def files(self, directory):
        """(fasta, stream) written into directory."""
        fa, stream = os.path.join(directory, self.name + ".fa"), os.path.join(directory, self.name + ".bin")
        with open(fa, "wb") as f:
            for i, s in enumerate(self.seqs):
                f.write(b">w%d\n" % i + np.asarray(s, dtype=np.uint8).tobytes() + b"\n")
        with open(stream, "wb") as f:
            f.write(self.data)
        return fa, stream

    def gfa1(self):
        """The serial program's gfa1 text of the case, made once."""
        if self._gfa1 is None:
            with tempfile.TemporaryDirectory() as d:
                fa, stream = self.files(d)
                r = subprocess.run([C.GRAPHDUMP, os.path.basename(stream), "-k", str(self.k), "-s", os.path.basename(fa), "-f", "gfa1"], cwd=d, capture_output=True, timeout=600)
            assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
            self._gfa1 = r.stdout
        return self._gfa1

    def oracles(self, max_inside=S.DEFAULT_MAX_INSIDE):
        if max_inside not in self._oracles:
            self._oracles[max_inside] = Oracles(self, max_inside)
        return self._oracles[max_inside]


class Oracles:
    """Every stage's oracle over the case's serial gfa1, under the case's colour map."""

    def __init__(self, case, max_inside=S.DEFAULT_MAX_INSIDE):
        text = case.gfa1()
        w = case.w
        self.k, self.n_colors, self.max_inside = case.k, case.n_colors, max_inside
        self.events, self.n_named = int(w.name.size), w.n_named
        self.first_event = np.nonzero(w.first)[0].astype(np.int64)
        base = case._oracles.get(min(case._oracles)) if case._oracles else None   # all but the superbubbles do not depend on the bound
        if base is None:
            self.g = C.Gfa1(text)
            assert len(self.g.seq_name) == len(case.seqs)
            self.colors = C.table(self.g, case.color_of_seq, case.n_colors)
            self.links = L.Links(text)
            self.bubbles = B.Bubbles(text)
            self.components = CM.Components(text, k=case.k, color_of_seq=case.color_of_seq)
            self.distances = D.matrices(self.colors, case.k)
        else:
            self.g, self.colors, self.links, self.bubbles, self.components, self.distances = base.g, base.colors, base.links, base.bubbles, base.components, base.distances
        self.superbubbles = S.Superbubbles(text, case.k, max_inside=max_inside, color_of_seq=case.color_of_seq)
        assert self.colors["colors"] == self.components.colors["colors"] == self.superbubbles.colors["colors"] == case.n_colors
        assert (self.colors["name"][:] == np.abs(w.name[w.first])).all() and self.links.events == self.events


# ---------------------------------------------------------------------------------------------------------------- what a check reads
def arrays_of(o):
    """{stage.field: array} of everything the device checks read of an Oracles or of its tiled stand-in: the two must agree on these."""
    c, l, b, m, s = o.colors, o.links, o.bubbles, o.components, o.superbubbles
    seg, edg = o.distances
    out = {"events": o.events, "colors.first_event": o.first_event}
    out.update({"colors." + key: c[key] for key in ("name", "length", "occurrences", "forward", "n_colors", "presence", "hist_segments", "hist_bases")})
    out.update({"links.rows": l.rows(), "links.occurrences": l.occurrences, "links.events": l.events, "links.frm": np.asarray(l.frm, dtype=np.int64), "links.to": np.asarray(l.to, dtype=np.int64),
                "links.first_event": l.first_event, "links.count": l.count, "links.same": l.same, "links.first_bits": l.first_bits})
    out.update({"bubbles.n": b.bubbles(), "bubbles.sides": b.sides, "bubbles.arcs": b.arcs, "bubbles.deg": b.deg, "bubbles.lo": b.lo, "bubbles.hi": b.hi, "bubbles.hist": b.hist,
                "bubbles.source": b.source, "bubbles.arm_a": b.arm_a, "bubbles.arm_b": b.arm_b, "bubbles.sink": b.sink})
    out.update({"components.n": m.count(), "components.rows": m.rows, "components.largest": m.largest(), "components.n_links": m.n_links, "components.colors": m.colors["colors"]})
    out.update({"components." + key: getattr(m, key) for key in ("component", "root", "segments", "links", "length", "edges", "occurrences", "presence", "n_colors")})
    out.update({"superbubbles.n": s.count(), "superbubbles.sides": s.sides, "superbubbles.unmirrored": s.unmirrored, "superbubbles.n_arcs": s.n_arcs, "superbubbles.max_inside": s.max_inside,
                "superbubbles.colors": s.colors["colors"]})
    out.update({"superbubbles." + key: getattr(s, key) for key in ("off", "heads", "exit", "entrance", "exits", "inside", "arcs", "n_colors", "paths", "min_edges", "max_edges", "presence",
                                                                   "member_off", "member_sides")})
    out.update({"distances.segments": seg, "distances.edges": edg})
    return out


def same_arrays(a, b):
    """The first key on which two arrays_of() differ, or None."""
    if set(a) != set(b):
        return "keys"
    for key in sorted(a):
        x, y = np.asarray(a[key]), np.asarray(b[key])
        if x.shape != y.shape or not (x.astype(np.int64) == y.astype(np.int64)).all():
            return key
    return None


# ---------------------------------------------------------------------------------------------------------------- tiling by arithmetic
def shift_names(name, t_ids, t_named):
    """Names of a copy whose ids are larger by t_ids and in front of which t_named 'N'-named events lie."""
    name = np.asarray(name, dtype=np.int64)
    mag = np.abs(name)
    return np.where(mag >= R.FRESH, name + np.sign(name) * t_named, name + np.sign(name) * 8 * t_ids)


def tiled(o, T, ids_per_tile):
    """The stand-in of the Oracles of o's stream written T times with the ids of copy t larger by t ids_per_tile: every attribute the
    device checks read (arrays_of), by arithmetic."""
    c, l, b, m, s = o.colors, o.links, o.bubbles, o.components, o.superbubbles
    rows, comps, events = len(c["name"]), m.count(), o.events
    t = np.arange(T, dtype=np.int64)

    def rep(a):                       # the same in every copy
        a = np.asarray(a)
        return np.tile(a, (T,) + (1,) * (a.ndim - 1))

    def plus(a, step, keep=None):     # larger by t step in copy t, but for the entries `keep` marks
        a = np.asarray(a, dtype=np.int64)
        add = np.repeat(t * step, a.size)
        return np.tile(a, T) + (add if keep is None else np.where(np.tile(keep, T), 0, add))

    def offsets(off, total):          # a CSR offset array of the concatenation
        off = np.asarray(off, dtype=np.int64)
        return np.concatenate([(off[:-1][None, :] + (t * total)[:, None]).ravel(), [T * total]])

    def names(a):
        a = np.asarray(a, dtype=np.int64)
        return shift_names(np.tile(a, T), np.repeat(t * ids_per_tile, a.size), np.repeat(t * o.n_named, a.size))

    out = types.SimpleNamespace(k=o.k, n_colors=o.n_colors, max_inside=o.max_inside, events=T * events, n_named=T * o.n_named, first_event=plus(o.first_event, events))
    out.colors = {"name": names(c["name"]), "colors": c["colors"], "events": T * c["events"], "hist_segments": T * c["hist_segments"], "hist_bases": T * c["hist_bases"]}
    out.colors.update({key: rep(c[key]) for key in ("length", "occurrences", "forward", "n_colors", "presence")})
    out.links = types.SimpleNamespace(rows=lambda: T * l.rows(), occurrences=T * l.occurrences, events=T * l.events, frm=names(l.frm), to=names(l.to), first_event=plus(l.first_event, events),
                                      count=rep(l.count), same=rep(l.same), first_bits=rep(l.first_bits))
    out.bubbles = types.SimpleNamespace(bubbles=lambda: T * b.bubbles(), sides=T * b.sides, arcs=T * b.arcs, deg=rep(b.deg), lo=plus(b.lo, 2 * rows, b.deg == 0), hi=plus(b.hi, 2 * rows, b.deg == 0),
                                        hist=T * b.hist, source=plus(b.source, 2 * rows), arm_a=plus(b.arm_a, 2 * rows), arm_b=plus(b.arm_b, 2 * rows), sink=plus(b.sink, 2 * rows))
    out.components = types.SimpleNamespace(count=lambda: T * comps, rows=T * rows, largest=lambda: m.largest(), n_links=T * m.n_links, colors={"colors": m.colors["colors"]},
                                           component=plus(m.component, comps), root=plus(m.root, rows), segments=rep(m.segments), links=rep(m.links), length=rep(m.length), edges=rep(m.edges),
                                           occurrences=rep(m.occurrences), presence=rep(m.presence), n_colors=rep(m.n_colors))
    out.superbubbles = types.SimpleNamespace(count=lambda: T * s.count(), sides=T * s.sides, unmirrored=T * s.unmirrored, n_arcs=T * s.n_arcs, max_inside=s.max_inside, colors={"colors": s.colors["colors"]},
                                             off=offsets(s.off, s.n_arcs), heads=plus(s.heads, 2 * rows), exit=plus(s.exit, 2 * rows, s.exit == NONE), entrance=plus(s.entrance, 2 * rows),
                                             exits=plus(s.exits, 2 * rows), inside=rep(s.inside), arcs=rep(s.arcs), n_colors=rep(s.n_colors), paths=rep(s.paths), min_edges=rep(s.min_edges),
                                             max_edges=rep(s.max_edges), presence=rep(s.presence).reshape(T * s.count(), s.colors["colors"]), member_off=offsets(s.member_off, len(s.member_sides)),
                                             member_sides=plus(s.member_sides, 2 * rows))
    out.distances = (T * o.distances[0], T * o.distances[1])
    return out


# ---------------------------------------------------------------------------------------------------------------- at size, in numpy
def classes_by_labels(n, a, b):
    """label[r]: the smallest row of the class of r under the pairs (a[i], b[i]) -- min-label propagation over the pairs' current roots
    with pointer jumping, until nothing changes."""
    label = np.arange(n, dtype=np.int64)
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    while True:
        la, lb = label[a], label[b]
        if (la == lb).all():
            return label
        low = np.minimum(la, lb)
        np.minimum.at(label, la, low)
        np.minimum.at(label, lb, low)
        while True:
            up = label[label]
            if (up == label).all():
                break
            label = up


class Direct:
    """The tables straight from the walk, for cases of any size whose names are all plain (no 'N', no -1, no 0): rows by first sight
    of |name|, link occurrences from consecutive events of one sequence, classes under (a, b) ~ (-b, -a), arcs, components."""

    def __init__(self, case):
        w = case.w
        name = w.name
        mag = np.abs(name)
        assert name.size and not w.fresh.any() and (mag > 1).all() and int(mag.max()) < 1 << 31
        self.k, self.n_colors, self.events = case.k, case.n_colors, int(name.size)
        self.first_event = np.nonzero(w.first)[0].astype(np.int64)
        uniq, at, inverse = np.unique(mag, return_index=True, return_inverse=True)
        rank = np.empty(uniq.size, dtype=np.int64)
        rank[np.argsort(at, kind="stable")] = np.arange(uniq.size)
        row = rank[inverse]                                         # per event
        self.rows = rows = int(uniq.size)
        assert (row[self.first_event] == np.arange(rows)).all()
        # the colour rows
        length = (w.end - w.begin + case.k)[self.first_event]
        colour = np.asarray(case.color_of_seq, dtype=np.int64)[w.seq]
        presence = np.zeros((rows, case.n_colors), dtype=bool)
        presence[row, colour] = True
        ncol = presence.sum(axis=1).astype(np.int64)
        self.colors = {"name": mag[self.first_event], "length": length, "occurrences": np.bincount(row, minlength=rows).astype(np.int64),
                       "forward": np.bincount(row, weights=name > 0, minlength=rows).astype(np.int64), "n_colors": ncol, "presence": presence, "colors": case.n_colors, "events": self.events,
                       "hist_segments": np.bincount(ncol, minlength=case.n_colors + 1).astype(np.int64),
                       "hist_bases": np.bincount(ncol, weights=length, minlength=case.n_colors + 1).astype(np.int64)}
        # the link rows
        e = np.nonzero(w.seq[1:] == w.seq[:-1])[0] + 1              # the events that close a link occurrence
        a, b = name[e - 1], name[e]
        keep = (a < -b) | ((a == -b) & (b <= -a))                   # (a, b) <= (-b, -a)
        ca, cb = np.where(keep, a, -b), np.where(keep, b, -a)
        key = ca * (1 << 32) + cb
        _, at, inverse, count = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
        order = np.argsort(at, kind="stable")
        rank = np.empty(order.size, dtype=np.int64)
        rank[order] = np.arange(order.size)
        link_row = rank[inverse]
        first_occ = at[order]
        frm, to = a[first_occ], b[first_occ]
        first_bits = np.zeros(self.events, dtype=bool)
        first_bits[e[first_occ]] = True
        same = np.bincount(link_row, weights=(a == frm[link_row]) & (b == to[link_row]), minlength=order.size).astype(np.int64)
        self.links = types.SimpleNamespace(rows=lambda: int(order.size), occurrences=int(e.size), events=self.events, frm=frm, to=to, first_event=e[first_occ], count=count[order].astype(np.int64),
                                           same=same, first_bits=first_bits)
        # the arcs of the classes
        self.pair_a, self.pair_b = row[e[first_occ] - 1], row[e[first_occ]]
        side_a, side_b = 2 * self.pair_a + (frm < 0), 2 * self.pair_b + (to < 0)
        arcs = np.unique(np.concatenate([side_a * (1 << 32) + side_b, (side_b ^ 1) * (1 << 32) + (side_a ^ 1)]))   # a link that is its own reverse: one arc
        tail, head = arcs >> 32, arcs & 0xFFFFFFFF
        sides = 2 * rows
        deg = np.bincount(tail, minlength=sides).astype(np.int64)
        lo, hi = np.full(sides, NONE, dtype=np.int64), np.zeros(sides, dtype=np.int64)
        np.minimum.at(lo, tail, head)
        np.maximum.at(hi, tail, head)
        self.tail, self.head = tail, head
        empty = np.zeros(0, dtype=np.int64)
        # no bubble and no superbubble: wherever two or more arcs leave a side, two of their heads are dead ends, and only one head
        # can be the exit -- a side inside without a way on fails the matching; a simple bubble is a superbubble
        wide = deg[tail] >= 2
        dead = np.bincount(tail[wide], weights=deg[head[wide]] == 0, minlength=sides)
        assert (dead[deg >= 2] >= 2).all(), "Direct holds graphs without bubbles only"
        self.bubbles = types.SimpleNamespace(bubbles=lambda: 0, sides=sides, arcs=int(arcs.size), deg=deg, lo=lo, hi=hi, hist=np.bincount(np.minimum(deg, B.BINS - 1), minlength=B.BINS).astype(np.int64),
                                             source=empty, arm_a=empty, arm_b=empty, sink=empty)
        off = np.zeros(sides + 1, dtype=np.int64)
        off[1:] = np.cumsum(deg)
        self.superbubbles = types.SimpleNamespace(count=lambda: 0, sides=sides, unmirrored=0, n_arcs=int(arcs.size), max_inside=S.DEFAULT_MAX_INSIDE, colors={"colors": case.n_colors}, off=off,
                                                  heads=head, exit=np.full(sides, NONE, dtype=np.int64), entrance=empty, exits=empty, inside=empty, arcs=empty, n_colors=empty,
                                                  paths=empty.astype(np.uint64), min_edges=empty.astype(np.uint64), max_edges=empty.astype(np.uint64),
                                                  presence=np.zeros((0, case.n_colors), dtype=bool), member_off=np.zeros(1, dtype=np.int64), member_sides=empty)
        # the components
        self.label = label = classes_by_labels(rows, self.pair_a, self.pair_b)
        root = np.nonzero(label == np.arange(rows))[0]
        component = np.searchsorted(root, label)
        n = root.size
        comp_presence = np.zeros((n, case.n_colors), dtype=bool)
        comp_presence[component[row], colour] = True
        segments = np.bincount(component, minlength=n).astype(np.int64)
        clen = np.bincount(component, weights=length, minlength=n).astype(np.int64)
        self.components = types.SimpleNamespace(count=lambda: int(n), rows=rows, largest=lambda: int(segments.max()), n_links=int(order.size), colors={"colors": case.n_colors}, component=component,
                                                root=root, segments=segments, links=np.bincount(component[self.pair_a], minlength=n).astype(np.int64), length=clen, edges=clen - case.k * segments,
                                                occurrences=np.bincount(component[row], minlength=n).astype(np.int64), presence=comp_presence, n_colors=comp_presence.sum(axis=1).astype(np.int64))
        self.distances = D.matrices(self.colors, case.k)
        self.n_named, self.max_inside = 0, S.DEFAULT_MAX_INSIDE


# ---------------------------------------------------------------------------------------------------------------- forest
FOREST_GADGETS, FOREST_IDS, FOREST_WALKS, FOREST_RECORDS = 220, 12, 4, 10
FOREST_LADDERS = (2, 2, 2, 2, 2, 8, 11)


def gadget_walks(rng, base, n_ids=FOREST_IDS, n_walks=FOREST_WALKS, n_records=FOREST_RECORDS):
    return [(base + rng.integers(1, n_ids + 1, n_records)) * rng.choice(np.array([-1, 1], dtype=np.int64), n_records) for _ in range(n_walks)]


def build_forest(name="forest", gadgets=FOREST_GADGETS, seed=20261101):
    """Random walks in disjoint id blocks: `gadgets` gadgets of 4 walks x 10 records over 12 ids each with random signs, and one
    hand-written gadget in front that holds a link that is its own reverse, a self-loop and a segment alone in its component.  Behind
    them, ladders (two arms between one entrance and one exit): five simple bubbles and superbubbles of 8 and 11 sides inside, which
    random walks of this size give too rarely (99 gadgets: 8 superbubbles of at most 4 sides inside, one simple bubble).
    Measured: with 220 gadgets all oracles together take 2.9 s on the machine this was written on, 1.2 s beside an MI355X; the
    superbubble oracle takes nine tenths of it (300 gadgets: 4 s)."""
    rng = np.random.default_rng(seed)
    hand = [np.array([1, 2, -2, -1, 1, 1, 3]),          # 1 -> 2 then 2 -> -2: the segment of 2 linked to its own reverse
            np.array([5, 6]), np.array([8, 9, 8, 9, 8])]
    base = FOREST_IDS * (gadgets + 2)
    for inside in FOREST_LADDERS:                       # what random walks of this size rarely give: simple bubbles, a wide superbubble
        hand += ladder_walks(base, inside)
        base += inside + 6
    walks = hand[:3] + [wk for g in range(gadgets) for wk in gadget_walks(rng, FOREST_IDS * (g + 1))] + hand[3:]
    n = len(walks) - len(hand) + 3
    paint = [(2, 0, "A"), (2, 1, "C"), (2, 2, "A"), (2, 3, "C")] + [(wk, e, "A") for wk in range(n, len(walks)) for e in range(len(walks[wk]) - 1)]
    seqs, sequences = lay(rng, walks, paint)
    c = Case(name, seqs, sequences)
    if gadgets < 100:
        return c
    t0 = time.time()
    o = c.oracles()
    c.oracle_seconds = time.time() - t0
    s, b, m, l = o.superbubbles, o.bubbles, o.components, o.links
    kinds = {key: sum(1 for v in s.verdicts.values() if key in v) for key in ("2", "3", "dead_end", "self_loop", "back_arc")}
    assert min(kinds.values()) >= 20, kinds
    assert s.count() >= 20 and int(s.inside.max()) >= 8 and b.bubbles() >= 5
    assert sum(1 for u in range(s.sides) if u in s.out[u] or (u ^ 1) in s.out[u]) >= 20             # self-loops, on one strand and across
    assert sum(1 for a, z in zip(l.frm, l.to) if a == -z) >= 1                                       # a+ a-: its own reverse
    assert int((b.deg.reshape(-1, 2) > 0).all(axis=1).sum()) >= 100                                  # both strands of one row linked
    assert int((m.segments == 1).sum()) >= 1 and m.count() >= gadgets // 2 and len(l.both) >= 20
    assert c.w.n_named == 0 and (np.abs(c.w.name) > 1).all()
    return c


# ---------------------------------------------------------------------------------------------------------------- bound
def ladder_walks(base, inside):
    """A superbubble of `inside` sides inside between the segments of base + 1 and base + 2 + inside: two arms side by side,
    inside // 2 and inside - inside // 2 segments long, as two walks over ascending ids."""
    n_a = inside // 2
    first, last = base + 1, base + 2 + inside
    arm_a = [first + 1 + i for i in range(n_a)]
    arm_b = [first + 1 + n_a + i for i in range(inside - n_a)]
    return [np.array([base, first] + arm_a + [last, last + 1]), np.array([base, first] + arm_b + [last, last + 1])]


def fan_walks(base, degree, into):
    """`degree` walks hub -> leaf_i (out-degree) or leaf_i -> hub (in-degree) over ids above base; the hub's id is the smallest."""
    hub = [base + 1, base + 2]
    if into:
        return [np.array([base + 3 + 2 * i, base + 4 + 2 * i, -(base + 2), -(base + 1)]) for i in range(degree)]
    return [np.array(hub + [base + 3 + 2 * i, base + 4 + 2 * i]) for i in range(degree)]


def build_bound(name="bound"):
    """Superbubbles of exactly 61, 62 and 63 sides inside (the default bound is 62), and sides of out-degree 64 and 65 and one of
    in-degree 65 (SB_LIST)."""
    rng = np.random.default_rng(62)
    walks, base = [], 1         # no id of 0: a segment named 0 (from junction 0, letter A) is the serial walk's "no segment yet"
    for inside in (61, 62, 63):
        walks += ladder_walks(base, inside)
        base += 100
    for degree, into in ((64, False), (65, False), (65, True)):
        walks += fan_walks(base, degree, into)
        base += 200
    paint = [(wk, e, "A") for wk, ids in enumerate(walks) for e in range(len(ids) - 1)]   # one letter everywhere: the ids alone decide
    seqs, sequences = lay(rng, walks, paint)
    c = Case(name, seqs, sequences)
    full, at8, at2 = c.oracles(62), c.oracles(8), c.oracles(2)
    assert sorted(full.superbubbles.inside.tolist()) == [61, 62] and c.oracles(61).superbubbles.inside.tolist() == [61]
    assert at8.superbubbles.count() == 0 and at2.superbubbles.count() == 0
    # three ladders of one shape (an entrance and, mirrored, an exit of degree 2 each); the one of 63 is 65 sides, one beyond the search
    deg = full.bubbles.deg
    assert (deg == 2).sum() == 6 and (full.superbubbles.exit != NONE).sum() == 4
    inn = np.array([len(x) for x in full.superbubbles.inn])
    assert (deg == 64).sum() >= 1 and (deg == 65).sum() >= 1 and (inn == 65).sum() >= 1 and full.bubbles.hist[5] >= 3
    return c


# ---------------------------------------------------------------------------------------------------------------- chains and hubs
CHAIN_ROWS, HUB_LEAVES = 300000, 100000


def case_of_ids(name, groups):
    """The case of groups of walks, each group an int64 [walks, records] array of signed ids: the stream written a group at a time
    (what segments_reference.build_stream gives walk by walk, with every separator written both ways and one behind the last), the text
    all A -- one letter everywhere, so the ids alone decide the segments."""
    parts, lens = [], []
    for ids in groups:
        ids = np.atleast_2d(np.asarray(ids, dtype=np.int64))
        n, r = ids.shape
        slots = np.zeros((n, r + 1), dtype=R.SLOT)
        slots["pos"][:, :r], slots["id"][:, :r] = GAP * np.arange(r), ids
        slots["pos"][:, r], slots["id"][:, r] = R.SEP_POS, R.SEP_ID
        parts.append(slots.ravel())
        lens.append(np.full(n, GAP * r, dtype=np.int64))
    lens = np.concatenate(lens)
    ends = np.cumsum(lens)
    flat = np.full(int(ends[-1]), ord("A"), dtype=np.uint8)
    seqs = [flat[a:b] for a, b in zip((ends - lens).tolist(), ends.tolist())]
    return Case(name, seqs, None, data=np.concatenate(parts).tobytes())


def build_chain(name, rows=CHAIN_ROWS, order="up"):
    """One sequence over rows + 1 ids: a chain of `rows` segments in one component.  up: ascending ids, forward events.  down:
    descending ids, reverse events, the strand bit set.  shuffled: the segments are first seen in a random order, one sequence of one
    event each, before the sequence that links them: the union-find hooks against the row order."""
    ids = np.arange(1, rows + 2, dtype=np.int64)
    if order == "down":
        walks = [ids[::-1]]
    elif order == "shuffled":
        first = np.random.default_rng(rows).permutation(rows)
        walks = [np.stack([ids[first], ids[first] + 1], axis=1), ids]
    else:
        walks = [ids]
    c = case_of_ids(name, walks)
    c.groups = walks
    d = c.direct = Direct(c)
    w = c.w
    assert d.rows == rows and d.links.rows() == rows - 1 and d.components.count() == 1 and d.components.largest() == rows
    assert int(d.bubbles.deg.max()) == 1 and d.bubbles.hist.tolist() == [2, 2 * rows - 2, 0, 0, 0, 0]
    if order == "down":
        assert not w.forward.any() and (w.name < 0).all()
    elif order == "shuffled":
        assert w.forward.all() and (np.diff(d.pair_a) < 0).sum() >= rows // 3 and (d.pair_a > d.pair_b).sum() >= rows // 3
    else:
        assert w.forward.all() and (w.name > 0).all() and (d.pair_b == d.pair_a + 1).all()
    return c


def build_late_hub(name, leaves=HUB_LEAVES, hub_first=False):
    """`leaves` segments, each first seen in a sequence of its own; behind them the sequences leaf_i -> hub: the hub is the last row
    and every hook competes for parent[hub].  hub_first: the mirror image, the hub is row 0 and every leaf is hooked under it."""
    i = np.arange(leaves, dtype=np.int64)
    a, b = 10 + 2 * i, 11 + 2 * i
    alone = np.stack([a, b], axis=1)
    joined = np.stack([a, b, np.full(leaves, 1, dtype=np.int64)], axis=1)           # the hub starts at id 1, the smallest: read in reverse
    walks = [np.array([5, 1]), joined] if hub_first else [alone, joined]
    c = case_of_ids(name, walks)
    d = c.direct = Direct(c)
    hub = 0 if hub_first else leaves
    assert d.rows == leaves + 1 and d.links.rows() == leaves and d.components.count() == 1
    assert ((d.pair_a == hub) | (d.pair_b == hub)).all()
    assert int(d.bubbles.deg.max()) == leaves > 64 and d.bubbles.hist.tolist() == [leaves + 1, leaves, 0, 0, 0, 1]
    return c


# ---------------------------------------------------------------------------------------------------------------- tiles
TILE_IDS, TILE_SEED = 32, 7


def tile_walks(rng):
    """One tile over ids 1 .. 31: a superbubble of 3 sides inside, a simple bubble in a component of its own, a gadget of 4 random
    walks in a third, and in it one 'N' at a deciding position."""
    return ladder_walks(1, 3) + ladder_walks(9, 2) + gadget_walks(rng, 19)


def tile_records(seed=TILE_SEED):
    """(letters per walk, ids per walk) of the tile."""
    rng = np.random.default_rng(seed)
    walks = tile_walks(rng)
    ladders = [(wk, e, "A") for wk in range(4) for e in range(len(walks[wk]) - 1)]
    seqs, _ = lay(rng, walks, paint=ladders + [(5, 3, "N")])
    return seqs, walks


def tile_colours(T, n_walks):
    """Three colours, the same in every copy."""
    return [wk % 3 for wk in range(n_walks)] * T


def tiles_case(name, T, seed=TILE_SEED, vectorised=True):
    """The tile written T times, the ids of copy t larger by 32 t.  vectorised: the stream and the text of all copies as whole arrays,
    with no loop over the copies; otherwise through lay's records and build_stream, for the test that pins the two to each other."""
    letters, walks = tile_records(seed)
    colours = tile_colours(T, len(walks))
    if not vectorised:
        seqs = [s.copy() for t in range(T) for s in letters]
        return Case(name, seqs, [(GAP * np.arange(len(ids), dtype=np.int64), ids + np.sign(ids) * TILE_IDS * t) for t in range(T) for ids in walks], color_of_seq=colours)
    one = np.zeros(sum(len(ids) + 1 for ids in walks), dtype=R.SLOT)
    sign, at = np.zeros(one.size, dtype=np.int64), 0
    for ids in walks:
        n = len(ids)
        one["pos"][at:at + n], one["id"][at:at + n], sign[at:at + n] = GAP * np.arange(n), ids, np.sign(ids)
        one["pos"][at + n], one["id"][at + n] = R.SEP_POS, R.SEP_ID
        at += n + 1
    slots = np.tile(one, T)
    slots["id"] += np.tile(sign, T) * np.repeat(TILE_IDS * np.arange(T, dtype=np.int64), one.size)
    flat = np.tile(np.concatenate(letters), T)
    ends = np.cumsum(np.tile([s.size for s in letters], T))
    seqs = [flat[a:b] for a, b in zip((ends - np.tile([s.size for s in letters], T)).tolist(), ends.tolist())]
    return Case(name, seqs, None, data=slots.tobytes(), color_of_seq=colours)


def tile_ok(o):
    """What a tile has to hold: a reported superbubble that is no simple bubble, a simple bubble, two components, a link class that
    occurs twice, an 'N'-named segment, every colour."""
    s, b, m, l = o.superbubbles, o.bubbles, o.components, o.links
    simple = {(int(x), int(y)) for x, y in zip(b.source, b.sink)}
    return (any((int(x), int(y)) not in simple and n >= 2 for x, y, n in zip(s.entrance, s.exits, s.inside)) and b.bubbles() >= 1 and m.count() >= 2 and int(l.count.max()) >= 2
            and o.n_named >= 1 and (o.colors["name"] >= R.FRESH).sum() >= 1 and s.count() >= 2 and o.colors["presence"].any(axis=0).all())


def build_tiles(name, T):
    """(case, the tile's Oracles, the tiled reference)."""
    o = tiles_case("tile", 1).oracles()
    assert tile_ok(o)
    c = tiles_case(name, T)
    c.tile, c.T = o, T
    c.want = tiled(o, T, TILE_IDS)
    return c


def tiles_for(o, what):
    """The smallest T that carries the tile's tables past the grid limits of `what`."""
    s, b, l = o.superbubbles, o.bubbles, o.links
    rows = len(o.colors["name"])
    if what == "report":
        return TURN_REPORT // s.count() + 2
    candidates = int((b.deg >= 2).sum())
    least = min(rows, l.rows(), o.events)
    T = TURN // least + 2
    assert T * candidates > TURN_SEARCH and 2 * T * rows > TURN_HIST and T * s.count() > TURN_REPORT
    return T
