"""Constructed texts of tests/test_gpu_periodic.py and what each must hold by the reference alone (helpers.periodic_reference).
No GPU here: tests/test_periodic_reference_cpu.py runs the same checks on the CPU.

A text is laid out as a flat array of position codes (0..3, 4 = N) behind the leading separator of the global text; the 4s listed as
`splits` become record separators (the records are the pieces between them), every other 4 is an N inside a record.  Both are code 4
in the packed text, so the flat array IS the global text -- the GPU tests assert that on the packed words."""
import numpy as np

import helpers as H

TILE_BACK = 100   # a tile case starts this far before the boundary, plus its offset 0 .. 31
FLANK = 70   # random letters on either side of a case: more than the 63 characters a period looks back
KS = (5, 17, 18, 19, 25, 29, 30, 31, 32, 60, 61, 62, 63, 64, 127, 603)


def primitive_unit(rng, p):
    """p random letters that are not a repetition of a shorter unit."""
    while True:
        u = rng.integers(0, 4, p).astype(np.uint8)
        if not any(p % d == 0 and (np.resize(u[:d], p) == u).all() for d in range(1, p)):
            return u


def other(rng, c):
    """A letter that is not c."""
    return np.uint8((int(c) + int(rng.integers(1, 4))) % 4)


def tract(rng, unit, ln):
    """ln letters of the unit repeated, between two letters chosen to break the period: [b] + tract + [a] (a random neighbour would
    extend the run one time in four)."""
    p = len(unit)
    t = np.resize(unit, ln)
    return np.concatenate([[other(rng, unit[p - 1])], t, [other(rng, unit[ln % p])]]).astype(np.uint8)


class Layout:
    def __init__(self, rng):
        self.rng = rng
        self.parts = [np.array([4], dtype=np.uint8)]  # position 0: the leading separator
        self.n = 1
        self.splits = []
        self.cases = []  # (kind, tag, start, end) in global positions: the body of the case without its flanks

    def filler(self, n):
        if n > 0:
            self.parts.append(self.rng.integers(0, 4, n).astype(np.uint8))
            self.n += n

    def pad_to(self, rel, mod, res):
        """Random letters until position n + rel is res modulo mod."""
        self.filler((res - (self.n + rel)) % mod)

    def put(self, kind, tag, body, splits=(), flank=True):
        if flank:
            self.filler(FLANK)
        s = self.n
        self.parts.append(np.asarray(body, dtype=np.uint8))
        self.n += len(body)
        self.splits += [s + int(x) for x in splits]
        self.cases.append((kind, tag, s, self.n))
        if flank:
            self.filler(FLANK)
        return s

    def finish(self):
        a = np.concatenate(self.parts + [np.array([4], dtype=np.uint8)])
        return a


def records_of(flat, splits):
    """The records whose packed text is `flat`: the pieces between its first and last position and the split positions."""
    cuts = [0] + sorted(splits) + [len(flat) - 1]
    assert all(flat[c] == 4 for c in cuts) and all(b - a > 1 for a, b in zip(cuts, cuts[1:])), "empty record"
    return [flat[a + 1:b] for a, b in zip(cuts, cuts[1:])]


LEN_PERIODS = (1, 2, 3, 7)


def _isolated_counts(snippet, k, s, e):
    qs, _, ins = H.periodic_reference(np.concatenate([[4], snippet, [4]]), k)
    return int(qs[s + 1 - 3:e + 1 + 3].sum()), int(ins[s + 1 - 3:e + 1 + 3].sum())


def constructed_case(k, seed=0, tiles=32):
    """One text for this k with every case of the list in test_gpu_periodic.py's docstring; returns a dict with the flat text, the
    records, the reference masks and the list of cases."""
    rng = np.random.default_rng(9000 + 31 * k + seed)
    lay = Layout(rng)
    ordinary = []  # callables that place one case each

    def add(fn):
        ordinary.append(fn)

    # --- the first 64 positions: a record that begins inside a tract (position 1 is the text's first letter)
    head = np.resize(np.array([2, 0, 1], dtype=np.uint8), k + 100)
    lay.put("head", 3, np.concatenate([head, [other(rng, head[len(head) % 3])]]), flank=False)
    lay.filler(FLANK)

    # --- every period, and units that are too long or periodic themselves
    for p in range(1, 64):
        u = primitive_unit(rng, p)
        add(lambda u=u, p=p: lay.put("period", p, tract(rng, u, k + 3 + p + int(rng.integers(0, 40)))))
    for p in (64, 65, 100):
        def long_unit(p=p):
            for _ in range(400):   # (at k = 5 a random unit of 100 letters repeats some 6-mer within 63 positions more often than not)
                u = primitive_unit(rng, p)
                body = tract(rng, u, 2 * p + k + 40)
                sn = np.concatenate([rng.integers(0, 4, FLANK).astype(np.uint8), body, rng.integers(0, 4, FLANK).astype(np.uint8)])
                q, _, i = H.periodic_reference(np.concatenate([[4], sn, [4]]), k)
                if not q.any() and not i.any():
                    s = lay.n
                    lay.parts.append(sn)
                    lay.n += len(sn)
                    lay.cases.append(("too_long", p, s + FLANK - 3, lay.n - FLANK + 3))
                    return
            raise AssertionError("no unit of %d letters without a chance repeat at k = %d" % (p, k))
        add(long_unit)
    add(lambda: lay.put("self_periodic", 2, tract(rng, np.array([0, 1, 0, 1], dtype=np.uint8), k + 3 + 4 + 37)))
    add(lambda: lay.put("self_periodic", 1, tract(rng, np.array([0, 0, 0], dtype=np.uint8), k + 3 + 3 + 20)))

    # --- the four lengths around the threshold
    for p in LEN_PERIODS + ((31, 63) if k >= 17 else ()):
        for extra in range(4):
            def length_case(p=p, extra=extra):
                for _ in range(400):  # (chance repeats among the neighbours at small k: take a neighbourhood without one)
                    u = primitive_unit(rng, p)
                    body = tract(rng, u, k + extra + p)
                    fl, fr = rng.integers(0, 4, FLANK).astype(np.uint8), rng.integers(0, 4, FLANK).astype(np.uint8)
                    if _isolated_counts(np.concatenate([fl, body, fr]), k, FLANK, FLANK + len(body)) == (max(0, extra - 1), extra):
                        lay.parts.append(fl)
                        lay.n += FLANK
                        lay.put("length", (p, extra), body, flank=False)
                        lay.parts.append(fr)
                        lay.n += FLANK
                        return
                raise AssertionError("no clean neighbourhood for the length case", k, p, extra)
            add(length_case)

    # --- started and ended at every offset of a packed word
    for off in range(32):
        def start_at(off=off):
            p = 1 + (5 * off) % 63
            body = tract(rng, primitive_unit(rng, p), k + 3 + p + 13)
            lay.filler(FLANK)
            lay.pad_to(1, 32, off)     # the tract's first letter (behind the breaking one) at offset `off`
            lay.put("start_offset", (off, p), body, flank=False)
            lay.filler(FLANK)

        def end_at(off=off):
            p = 1 + (11 * off + 3) % 63
            body = tract(rng, primitive_unit(rng, p), k + 3 + p + 21)
            lay.filler(FLANK)
            lay.pad_to(len(body) - 2, 32, off)  # the tract's last letter at offset `off`
            lay.put("end_offset", (off, p), body, flank=False)
            lay.filler(FLANK)
        add(start_at)
        add(end_at)

    # --- an N, and a record separator, inside a tract: at every distance before a window that is periodic otherwise, at its two
    #     outer characters, inside; records that start and end inside a tract; records shorter than k
    for sep in (False, True):
        for p in (1, 2, 3, 7, 31, 62, 63):
            def n_case(p=p, sep=sep):
                before, after = k + p + 8, k + 2 + 64 + p + 8
                body = tract(rng, primitive_unit(rng, p), before + 1 + after)
                body[1 + before] = 4
                lay.put("sep_inside" if sep else "n_inside", p, body, splits=[1 + before] if sep else ())
            add(n_case)

    def short_records():
        ln = 4 * k + 300
        body = tract(rng, np.array([3, 1], dtype=np.uint8), ln)
        cuts = [k + 40, k + 40 + max(2, k - 1), k + 40 + max(2, k - 1) + k + 2, k + 40 + max(2, k - 1) + k + 2 + k + 1]  # records of k - 2 (at least 1), k + 1 and k letters
        body[cuts] = 4
        lay.put("short_records", 2, body, splits=cuts)
    add(short_records)

    # --- a run beyond the counters' 1023, one mismatch behind it: the run restarts from zero
    def saturation():
        ln = 1023 + k + 400
        body = tract(rng, np.array([1], dtype=np.uint8), ln)
        body[1 + 1100] = 2
        lay.put("saturation", 1, body)
        body5 = tract(rng, primitive_unit(rng, 5), ln)
        body5[1 + 1100] = other(rng, body5[1 + 1100])
        lay.put("saturation", 5, body5)
    add(saturation)

    # --- across a tile boundary of 16384 positions, at 32 offsets
    def tile_case(o):
        p = (1, 2, 3, 5, 7, 11, 31, 63)[o % 8]
        body = tract(rng, primitive_unit(rng, p), k + 3 + p + 180)
        return p, body

    rng.shuffle(ordinary)  # (no kind of case sits at one place of the text only)
    next_tile = 0
    pending = list(ordinary)
    while pending or next_tile < tiles:
        if next_tile < tiles:
            boundary = ((lay.n + FLANK + TILE_BACK) // H.PER_TILE + 1) * H.PER_TILE
            room = boundary - TILE_BACK - FLANK - lay.n
        else:
            room = 1 << 40
        # (an ordinary case takes at most 2 flanks + its body + 31 letters of padding; the longest body is the saturation pair)
        need = 2 * (1023 + k + 400 + 2 + 2 * FLANK) if pending and pending[-1] is saturation else 4 * FLANK + 32 + 2 * (k + 3 + 64 + 100) + 2 * 100 + 3 * k
        if pending and need < room:
            pending.pop()()
            continue
        o = next_tile
        p, body = tile_case(o)
        start = boundary - TILE_BACK + o      # the breaking letter; the tract's first letter is the next one
        assert start - lay.n >= FLANK
        lay.filler(start - lay.n)
        lay.put("tile", (o, p), body, flank=False)
        lay.filler(FLANK)
        next_tile += 1

    # --- the last k + 64 positions: a record that ends inside a tract (it runs to the text's last letter)
    lay.filler(FLANK)
    s = lay.n
    tail = np.concatenate([[2], np.resize(np.array([1, 0], dtype=np.uint8), k + 64 + 40)]).astype(np.uint8)
    lay.put("tail", 2, tail, flank=False)
    flat = lay.finish()
    qs, dist, ins = H.periodic_reference(flat, k)
    return dict(k=k, flat=flat, splits=sorted(lay.splits), records=records_of(flat, lay.splits), qs=qs, dist=dist, ins=ins, cases=lay.cases)


def pretest_blocks(k, first):
    """The blocks periodic_may_flag compares for the word of positions first .. first + 31, by its comment: (a, off, four) with
    off = (a - 63) mod 32 the offset of the block's earliest twin in its packed word and four = that read's last character lies
    in a fourth word.  None for k < 18 (the pre-test is off)."""
    B = min(16, (k + 2) // 2)
    if B < 10:
        return []
    s0, s1 = first, first + 31 + k
    if k >= 31 + 2 * B - 1:
        s0, s1 = first + 31, first + k
    out = []
    a = s0
    while a + B - 1 <= s1:
        off = (a - 63) % 32
        out.append((a, off, off + 63 + B > 96))
        a += B
    return out


def check_constructed(case):
    """Everything the constructed text promises, from the reference alone."""
    k, qs, dist, ins, flat = case["k"], case["qs"], case["dist"], case["ins"], case["flat"]
    by = {}
    for kind, tag, s, e in case["cases"]:
        by.setdefault(kind, []).append((tag, s, e))
    assert len(flat) < 600000
    # every period is the copy distance somewhere, and the smallest that fits wins
    for p, s, e in by["period"]:
        assert (dist[s:e] == p).any(), ("period", k, p)
    assert set(range(1, 64)) <= set(dist.tolist())
    assert sorted(t for t, _, _ in by["too_long"]) == [64, 65, 100]
    for p, s, e in by["too_long"]:
        assert not qs[s:e].any() and not ins[s:e].any(), ("too long", k, p)
    for p, s, e in by["self_periodic"]:
        assert qs[s:e].sum() > 20 and set(dist[s:e][qs[s:e]].tolist()) == {p}, ("self periodic", k, p)
    # the four lengths
    assert len(by["length"]) >= 16
    for (p, extra), s, e in by["length"]:
        got = (int(qs[s - 3:e + 3].sum()), int(ins[s - 3:e + 3].sum()))
        assert got == (max(0, extra - 1), extra), ("length", k, p, extra, got)
        if extra >= 2:
            assert set(dist[s:e][qs[s:e]].tolist()) == {p}
    # word offsets of the first and of the last flagged position
    for kind in ("start_offset", "end_offset"):
        assert sorted(t[0] for t, _, _ in by[kind]) == list(range(32))
        for (off, p), s, e in by[kind]:
            assert ((s + 1) % 32 if kind == "start_offset" else (e - 2) % 32) == off
            assert qs[s:e].any() and ins[s:e].any(), (kind, k, off)
    # N and separators inside a tract: the run restarts, the position right behind the restart drops its insert and still probes
    for kind in ("n_inside", "sep_inside"):
        assert len(by[kind]) == 7
        for p, s, e in by[kind]:
            x = s + 1 + k + p + 8
            assert flat[x] == 4 and (x in case["splits"]) == (kind == "sep_inside")
            # (no window holds the N; behind it a window may well repeat one from before the N, at another distance than p)
            assert ins[x - k - 1] and qs[x - k - 1] and not ins[x - k:x + 1].any() and not qs[x - k:x + 2].any(), (kind, k, p)
            assert qs[x + p + 2:x + p + 2 + 66].all() and ins[x + p + 1:x + p + 2 + 66].all(), (kind, k, p)
            assert (dist[x + 2 * p + 2:x + p + 2 + 66] == p).all(), (kind, k, p)
    (_, s, e), = by["short_records"]
    lens = sorted(len(r) for r in case["records"])
    assert lens[0] < k and (k + 1) in lens and k in lens
    # text ends
    (_, s, e), = by["head"]
    assert s == 1 and ins[4:100].all() and not ins[1:4].any() and not qs[:63].any() and qs[63:100].all()  # (the first 63 positions of tile 0)
    (_, s, e), = by["tail"]
    n = len(flat)
    assert e == n - 1 and qs[n - 1 - k - 60:n - 1 - k].all() and ins[n - 1 - k - 60:n - 1 - k].all() and not ins[n - 1 - k:].any()
    # saturation
    for p, s, e in by["saturation"]:
        x = s + 1 + 1100
        assert qs[s + 1 + p + 1:x - k].all() and (dist[s + 1 + p + 1:x - k] == p).all() and x - k - (s + 1 + p + 1) > 1023 - k
        assert not ins[x - k:x + 1].any() and not qs[x + 1] and qs[x + p + 2:e - 2 - k].all() and e - 2 - k - (x + p + 2) > 100
    assert {p for p, _, _ in by["saturation"]} == {1, 5}
    # tile boundaries: the first 63 positions of a tile never copy, their inserts are dropped all the same
    assert sorted(t[0] for t, _, _ in by["tile"]) == list(range(len(by["tile"]))) and len(by["tile"]) >= 32
    for (o, p), s, e in by["tile"]:
        b = (s + TILE_BACK) // H.PER_TILE * H.PER_TILE
        assert b == s + TILE_BACK - o and s < b < e
        assert not qs[b:b + 63].any() and qs[b + 63:b + 66].all() and ins[b:b + 66].all(), ("tile", k, o, p)
        assert qs[s + 1 + p + 1:b].all() and s + 1 + p + 1 < b
    # the pre-test's reads: three words, or four
    four = {f for w in np.unique(np.nonzero(ins)[0] // 32).tolist() for _, _, f in pretest_blocks(k, 32 * w)}
    B = min(16, (k + 2) // 2)
    assert four == (set() if B < 10 else {False} if B == 16 else {False, True}), (k, four)
    return True
