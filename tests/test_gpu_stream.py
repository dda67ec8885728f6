"""GPU (-m gpu): the junction stream kernels (csrc/tpc_stream.hip) and the host's ShardedStream add-up (host/multigpu.cpp) against the
writer's definition, tests/stream_reference.py.  Byte equality throughout.

(a), (b): layouts go straight to the C-ABI -- set_params, junction_keys_set (any J distinct keys), junctions_finalize, emit_import of
sorted positions and ids from torch tensors, then emit_stream, or emit_stream_partial / emit_stream_part with any chunk of text
positions.  No text is uploaded: the stream kernels read the record table, the marks, the ids and the number of keys.  One process, one
context per rank on the one device.

Stale bytes: before every real call the context formats a decoy through the same stream buffer, so that a slot the kernels leave
unwritten cannot pass on what an earlier call wrote there.  The decoy is one sequence with every k-mer marked, as many slots as the
layout's whole stream, ids -(2^40 + i): all its slots are records that no layout's stream contains.  (The layout itself with its ids
negated would leave every separator what and where it is in the real stream: a separator that is never written would pass on it.)

(c): a FASTA file whose record borders, end k-mers and a run of short records sit on the tile cuts of tpc_shard_chunk, through
capi.Enumerator on 2 / 4 / 8 emulated ranks against the one-GPU run and the project's oracle."""
import numpy as np
import pytest

import stream_reference as R

pytestmark = pytest.mark.gpu

INV = R.INVALID
PATTERNS = ("none", "all_invalid", "all_real", "first_only", "last_only", "first_real_last_invalid", "first_invalid_last_real", "random")
N_RECS = (1, 2, 255, 256, 257, 513, 1000)
BIG_MARKS = 2097152 + 300   # beyond 4096 x 256 (k_stream_flags) and 8192 x 256 (k_stream_marks, k_stream_marks_part): both loops turn over


# ---------------------------------------------------------------------------------------------------------------- the layouts
class Layout:
    def __init__(self, name, k, J, rec_len, marks, ids):
        self.name, self.k, self.J = name, k, J
        self.rec_len = [int(x) for x in rec_len]
        self.rec_start = R.rec_starts(self.rec_len)
        self.marks = np.asarray(marks, dtype=np.uint64)
        self.ids = np.asarray(ids, dtype=np.int64)
        assert self.marks.size == self.ids.size and (np.diff(self.marks.astype(np.int64)) > 0).all()
        real = self.ids[self.ids != INV]
        assert real.size == 0 or (1 <= np.abs(real).min() and np.abs(real).max() <= J)
        self.n_rec = len(self.rec_len)
        self.text_end = self.rec_start[-1] + self.rec_len[-1] + 1

    def ends(self):
        """[(sequence, first k-mer, last k-mer)] of the sequences of at least k bases."""
        return [(r, f, f + n - self.k) for r, (f, n) in enumerate(zip(self.rec_start, self.rec_len)) if n >= self.k]

    def id_at(self):
        return dict(zip(self.marks.tolist(), self.ids.tolist()))

    def exact_k(self):
        """(with, without): the sequences of exactly k bases whose one k-mer holds a real id / holds none."""
        at = self.id_at()
        have = [at.get(f, INV) != INV for _, f, last in self.ends() if f == last]
        return sum(have), len(have) - sum(have)

    def short_runs(self):
        """[(first index, one past the last)] of the maximal runs of sequences shorter than k."""
        runs, r = [], 0
        while r < self.n_rec:
            if self.rec_len[r] < self.k:
                e = r
                while e < self.n_rec and self.rec_len[e] < self.k:
                    e += 1
                runs.append((r, e))
                r = e
            else:
                r += 1
        return runs


def real_id(rng, J):
    return int(rng.integers(1, J + 1)) * (1 if rng.random() < 0.5 else -1)


def draw_lengths(rng, k, n_rec):
    """Drawn from {0, 1, k - 1, k, k + 1, 2k, 200}; the first entries are fixed so that even two sequences hold a long one and one of exactly k,
    and so is the first sequence of the second block of 256, which then has work to do even when it is the block's only one."""
    fixed = [200, k, k + 1, 0, 2 * k, 1, k - 1]
    out = fixed[:n_rec] + [int(x) for x in rng.choice([0, 1, k - 1, k, k + 1, 2 * k, 200], max(n_rec - len(fixed), 0))]
    if n_rec > 256:
        out[256] = 2 * k
    return out


def draw_marks(rng, pattern, k, J, rec_len):
    assert J > 0 or pattern in ("none", "all_invalid"), "no real id exists when J = 0"
    marks, ids, exact = [], [], 0
    for first, n in zip(R.rec_starts(rec_len), rec_len):
        if n < k:
            continue
        last = first + n - k
        if pattern == "all_invalid":
            marks += range(first, last + 1)
            ids += [INV] * (last + 1 - first)
        elif pattern == "all_real":
            marks += range(first, last + 1)
            ids += [real_id(rng, J) for _ in range(first, last + 1)]
        elif pattern == "first_only":
            marks.append(first), ids.append(real_id(rng, J))
        elif pattern == "last_only":
            marks.append(last), ids.append(real_id(rng, J))
        elif pattern in ("first_real_last_invalid", "first_invalid_last_real"):
            first_real = pattern == "first_real_last_invalid"
            if first == last:   # the one k-mer is both ends: real on every other such sequence
                exact += 1
                marks.append(first), ids.append(real_id(rng, J) if exact % 2 else INV)
            else:
                marks += [first, last]
                ids += [real_id(rng, J), INV] if first_real else [INV, real_id(rng, J)]
        elif pattern == "random":
            for g in range(first, last + 1):
                if rng.random() < 0.1:
                    marks.append(g), ids.append(INV if rng.random() < 0.3 else real_id(rng, J))
        else:
            assert pattern == "none"
    return marks, ids


def grid_spec(n_rec, pattern):
    i, j = N_RECS.index(n_rec), PATTERNS.index(pattern)
    k = (3, 25)[(i + j) % 2]
    J = (0, 1, 1000)[(i + j // 2) % 3] if pattern in ("none", "all_invalid") else (1, 1000)[(i + j) // 2 % 2]
    return k, J


def build_grid(name, n_rec, pattern):
    k, J = grid_spec(n_rec, pattern)
    rng = np.random.default_rng(1000 * n_rec + PATTERNS.index(pattern))
    rec_len = draw_lengths(rng, k, n_rec)
    lay = Layout(name, k, J, rec_len, *draw_marks(rng, pattern, k, J, rec_len))
    # the named features are really there
    at, ends = lay.id_at(), lay.ends()
    assert lay.n_rec == n_rec and len(ends) >= 1
    if n_rec > 256:
        assert (n_rec + 255) // 256 >= 2 and sum(1 for r, _, _ in ends if r >= 256) > 0      # more than one block of sequences does work
        assert {0, 1, k - 1, k, k + 1, 2 * k, 200} == set(lay.rec_len)
    with_id, without_id = lay.exact_k()
    if n_rec >= 2:
        assert with_id + without_id > 0
    if pattern == "none":
        assert lay.marks.size == 0
    if pattern == "all_invalid":
        assert lay.marks.size == sum(last - f + 1 for _, f, last in ends) and (lay.ids == INV).all()
    if pattern == "all_real":
        assert lay.marks.size == sum(last - f + 1 for _, f, last in ends) and (lay.ids != INV).all() and (n_rec < 2 or with_id > 0)
    if pattern == "first_only":
        assert lay.marks.tolist() == [f for _, f, _ in ends] and (lay.ids != INV).all()
    if pattern == "last_only":
        assert lay.marks.tolist() == [last for _, _, last in ends] and (lay.ids != INV).all()
    if pattern == "first_real_last_invalid":
        assert all(at[f] != INV and at[last] == INV for _, f, last in ends if f != last)
    if pattern == "first_invalid_last_real":   # a first k-mer that is marked, but with an invalid id
        assert all(at[f] == INV and at[last] != INV for _, f, last in ends if f != last)
    if pattern in ("first_real_last_invalid", "first_invalid_last_real") and n_rec > 2:
        assert with_id > 0 and without_id > 0    # a sequence of exactly k bases with and without a real id
    if pattern == "random" and n_rec > 2:
        assert (lay.ids == INV).sum() > 0 and (lay.ids != INV).sum() > 0
    return lay


def build_single(name):
    rng = np.random.default_rng(1)
    lay = Layout(name, 25, 1000, [200], *draw_marks(rng, "random", 25, 1000, [200]))
    assert lay.n_rec == 1 and lay.marks.size > 5
    return lay


def build_all_short(name):
    rng = np.random.default_rng(2)
    lay = Layout(name, 25, 1000, [int(x) for x in rng.choice([0, 1, 24], 300)], [], [])
    assert max(lay.rec_len) < lay.k and lay.n_rec > 256
    return lay


def mixed(rng, k, n):
    return [int(x) for x in rng.choice([k, k + 1, 2 * k, 200, 1, k - 1], n)]


def build_leading_short(name):
    rng = np.random.default_rng(3)
    rec_len = [int(x) for x in rng.choice([0, 1, 24], 300)] + [200] + mixed(rng, 25, 199)
    lay = Layout(name, 25, 1000, rec_len, *draw_marks(rng, "random", 25, 1000, rec_len))
    assert lay.short_runs()[0] == (0, 300)
    return lay


def build_trailing_short(name):
    rng = np.random.default_rng(4)
    rec_len = mixed(rng, 25, 199) + [200] + [int(x) for x in rng.choice([0, 1, 24], 300)]
    lay = Layout(name, 25, 1000, rec_len, *draw_marks(rng, "random", 25, 1000, rec_len))
    assert lay.short_runs()[-1] == (200, 500)
    return lay


def build_straddle(name):
    """Runs of short sequences across the borders of the blocks of 256 sequences, indices 255 / 256 / 257 and 511 / 512 / 513."""
    rng = np.random.default_rng(5)
    rec_len = [int(x) for x in rng.choice([3, 4, 6, 200], 520)]
    for r in list(range(250, 262)) + list(range(505, 518)):
        rec_len[r] = int(rng.choice([0, 1, 2]))
    lay = Layout(name, 3, 1, rec_len, *draw_marks(rng, "first_invalid_last_real", 3, 1, rec_len))
    runs = lay.short_runs()
    assert (250, 262) in runs and (505, 518) in runs
    return lay


def build_k93(name):
    """k = 93: the context holds keys of four words."""
    rng = np.random.default_rng(6)
    rec_len = [200, 93] + [int(x) for x in rng.choice([0, 1, 92, 93, 94, 186, 200], 255)]
    lay = Layout(name, 93, 1000, rec_len, *draw_marks(rng, "random", 93, 1000, rec_len))
    assert lay.n_rec == 257 and sum(lay.exact_k()) > 0 and (93 + 4 + 31) // 32 == 4
    return lay


def build_big(name):
    """2 097 152 + 300 marks, every k-mer start of 700 long sequences, a fifth of them INVALID; a short sequence after every tenth."""
    rng = np.random.default_rng(7)
    k, J, n_long = 25, 1000, 700
    per, extra = divmod(BIG_MARKS, n_long)
    rec_len = []
    for r in range(n_long):
        rec_len.append(per + (1 if r < extra else 0) + k - 1)
        if r % 10 == 9:
            rec_len.append(int(rng.integers(0, k)))
    rec_len = np.array(rec_len, dtype=np.int64)
    start = np.concatenate([[1], 1 + np.cumsum(rec_len + 1)[:-1]])
    long_ = rec_len >= k
    n_kmers = rec_len[long_] - k + 1
    marks = np.repeat(start[long_] - np.concatenate([[0], np.cumsum(n_kmers)[:-1]]), n_kmers) + np.arange(int(n_kmers.sum()))
    ids = rng.integers(1, J + 1, marks.size) * rng.choice([-1, 1], marks.size)
    ids[rng.random(marks.size) < 0.2] = INV
    lay = Layout(name, k, J, rec_len, marks, ids)
    assert lay.marks.size == BIG_MARKS > 8192 * 256 and lay.n_rec == 770
    return lay


SPECS = {"n%d_%s" % (n, p): (build_grid, (n, p)) for n in N_RECS for p in PATTERNS}
SPECS.update(single_sequence=(build_single, ()), all_short=(build_all_short, ()), leading_short_300=(build_leading_short, ()),
             trailing_short_300=(build_trailing_short, ()), short_runs_straddle_blocks=(build_straddle, ()), k93_four_word_keys=(build_k93, ()),
             two_million_marks=(build_big, ()))
SMALL = [n for n in SPECS if n != "two_million_marks"]
_BUILT = {}


def layout(name):
    """(Layout, its reference Stream): built once, shared by every test, never changed."""
    if name not in _BUILT:
        fn, args = SPECS[name]
        lay = fn(name, *args)
        s = R.write(lay.k, lay.J, lay.rec_len, lay.marks, lay.ids)
        if name == "all_short":
            assert s.bytes == b"" and s.n_records == 0
        _BUILT[name] = (lay, s)
    return _BUILT[name]


def test_the_grid_covers_what_it_names():
    """Every k, J and pattern of the grid occurs, with every J also on an unmarked and an all-INVALID layout."""
    specs = {(n, p): grid_spec(n, p) for n in N_RECS for p in PATTERNS}
    assert {k for k, _ in specs.values()} == {3, 25} and {J for _, J in specs.values()} == {0, 1, 1000}
    for p in PATTERNS:
        assert {specs[(n, p)][0] for n in N_RECS} == {3, 25}
        assert {specs[(n, p)][1] for n in N_RECS} == ({0, 1, 1000} if p in ("none", "all_invalid") else {1, 1000})


# ---------------------------------------------------------------------------------------------------------------- the cuts
def cut_lists(lay, s, few=False):
    """[(label, cuts)]: W - 1 ascending cuts for W in 2, 3, 4, 8, each list built around one place where a cut can go wrong; the rest of a
    list is drawn from all those places.  few: the two lists the large layout gets."""
    rng = np.random.default_rng(len(lay.name) + 17 * lay.n_rec)
    rs, rl, k = lay.rec_start, lay.rec_len, lay.k
    ends, at = lay.ends(), lay.id_at()
    groups = []
    for r in sorted({r for r in (1, lay.n_rec // 2, lay.n_rec - 1, 255, 256, 257, 512) if 1 <= r < lay.n_rec}):
        groups += [("separator owner of %d" % r, (rs[r] - 1,)), ("start of %d" % r, (rs[r],)), ("start + 1 of %d" % r, (rs[r] + 1,))]
    for r, first, last in [ends[i] for i in sorted({0, len(ends) // 2, len(ends) - 1})] if ends else []:
        groups += [("last k-mer of %d" % r, (last,)), ("last k-mer + 1 of %d" % r, (last + 1,))]
    real, invalid = lay.marks[lay.ids != INV].tolist(), lay.marks[lay.ids == INV].tolist()
    for g in [real[i] for i in sorted({0, len(real) // 2, len(real) - 1})] if real else []:
        groups += [("real mark", (g,)), ("real mark + 1", (g + 1,))]
    for g in invalid[len(invalid) // 2:len(invalid) // 2 + 1]:
        groups += [("invalid mark", (g,)), ("a rank whose marks are all INVALID", (g, g + 1))]
    anchor = real[len(real) // 3] if real else rs[lay.n_rec // 2]
    groups.append(("two equal cuts", (anchor, anchor)))
    for lo, hi in [x for x in lay.short_runs() if x[1] - x[0] >= 3][:3]:
        groups.append(("inside the short run %d..%d" % (lo, hi), (rs[(lo + hi) // 2],)))
    if ends:
        r, first, last = max(ends, key=lambda e: e[2] - e[1])
        if last - first >= 3:
            a, b = first + (last - first) // 3, first + 2 * (last - first) // 3
            assert first < a < b <= last
            groups.append(("sequence %d spans three ranks" % r, (a, b + 1)))
            if all(at.get(g, INV) != INV for g in range(first, last + 1)):   # every rank holds real-id records of it
                groups.append(("sequence %d spans three ranks, the third sums two" % r, (a, b)))
    pool = sorted({c for _, cuts in groups for c in cuts} | {int(x) for x in rng.integers(0, lay.text_end + 3, 8)})
    out = []
    if few:
        groups = [g for g in groups if g[0].startswith(("real mark + 1", "sequence"))][-2:]
    for i, (label, cuts) in enumerate(groups):
        w = [x for x in (2, 3, 4, 8) if x - 1 >= len(cuts)]
        w = 3 if few else w[i % len(w)]
        fill = [int(x) for x in rng.choice(pool, w - 1 - len(cuts))]
        out.append(("W=%d, %s" % (w, label), sorted(list(cuts) + fill)))
    if not few:
        for w in (2, 3, 4, 8):
            out.append(("W=%d, random" % w, sorted(int(x) for x in rng.integers(0, lay.text_end + 3, w - 1))))
    return out


# ---------------------------------------------------------------------------------------------------------------- the device
class Device:
    """Up to eight contexts on device 0 and the layout's lists in device memory."""

    def __init__(self):
        import torch
        from twopaco_amd import capi
        capi.hip()
        capi.host()
        self.torch, self.capi = torch, capi
        self.ctxs, self.tags = {}, {}
        self.held = None

    def close(self):
        for c in self.ctxs.values():
            c.close()

    def ctx(self, rank, k, J):
        """Rank `rank`'s context, with J distinct keys of k characters behind junctions_finalize."""
        if rank not in self.ctxs:
            self.ctxs[rank] = self.capi.Context(0)
        c = self.ctxs[rank]
        if self.tags.get(rank) != (k, J):
            c.set_params(k, 12, 1, self.capi.seed_table(1, 12, seed=5))
            keys = np.zeros((J, c.key_words()), dtype=np.uint64)
            keys[:, 0] = np.arange(J, dtype=np.uint64)
            c.junction_keys_set(keys)
            assert c.junctions_finalize() == J
            self.tags[rank] = (k, J)
        return c

    def hold(self, lay, n_slots):
        """The layout's marks and ids, and a decoy of n_slots records, as device tensors."""
        if self.held is None or self.held[0] != lay.name:
            t = self.torch
            up = lambda a: t.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()
            n = max(n_slots, 1)
            self.held = (lay.name, up(lay.marks), up(lay.ids), t.arange(1, n + 1, dtype=t.int64, device="cuda"),
                         -((1 << 40) + t.arange(n, dtype=t.int64, device="cuda")), n)
            t.cuda.synchronize()
        return self.held

    def decoy(self, c, lay, n_slots):
        _, _, _, g, ids, n = self.hold(lay, n_slots)
        c.emit_import(g.data_ptr(), ids.data_ptr(), n)
        data, records = c.emit_stream([1], [n + lay.k - 1])
        assert records == n and len(data) == 12 * n

    def load(self, c, lay, n_slots, lo=0, hi=R.UINT64_MAX):
        """The marks of [lo, hi) and their ids into context c."""
        _, g, ids, _, _, _ = self.hold(lay, n_slots)
        a, b = (int(np.searchsorted(lay.marks, np.uint64(x), side="left")) for x in (lo, hi))
        c.emit_import(g.data_ptr() + 8 * a, ids.data_ptr() + 8 * a, b - a)
        return b - a


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.close()


def check_whole(dev, name, decoy=True):
    lay, s = layout(name)
    c = dev.ctx(0, lay.k, lay.J)
    if decoy:
        dev.decoy(c, lay, s.n_slots)
    assert dev.load(c, lay, s.n_slots) == lay.marks.size
    data, records = c.emit_stream(lay.rec_start, lay.rec_len)
    assert records == s.n_records and len(data) == 12 * s.n_slots
    assert data == s.bytes, first_difference(data, s)


def first_difference(data, s, slot0=0):
    got = np.frombuffer(data, dtype=R.SLOT)
    want = np.frombuffer(s.bytes, dtype=R.SLOT)[slot0:slot0 + got.size]
    bad = np.nonzero((got["pos"] != want["pos"]) | (got["id"] != want["id"]))[0]
    if not bad.size:
        return "lengths differ"
    i = int(bad[0])
    return "%d slots differ, the first is slot %d (%s of sequence %d, owner %d): got %r, want %r" % (
        bad.size, slot0 + i, R.KIND_NAMES[s.kind[slot0 + i]], s.seq[slot0 + i], s.owner[slot0 + i], got[i], want[i])


def test_context_takes_wider_keys_after_narrow_ones(dev):
    """set_params with another key width on a context that holds keys: the key buffer is counted in keys, so 1000 four-word keys (k = 93)
    used to be copied into the room of 2024 one-word keys (k = 25) and the copy refused."""
    c = dev.capi.Context(0)
    for k, words in ((25, 1), (93, 4), (61, 3), (25, 1)):
        c.set_params(k, 12, 1, dev.capi.seed_table(1, 12, seed=5))
        assert c.key_words() == words
        keys = np.zeros((1000, words), dtype=np.uint64)
        keys[:, 0] = np.arange(1000, dtype=np.uint64)[::-1]
        keys[:, words - 1] |= np.uint64(1) << np.uint64(40)
        c.junction_keys_set(keys)
        assert c.junctions_finalize() == 1000
        assert (c.junction_keys() == keys[::-1]).all()      # sorted by word 0 first
    c.close()


# ---------------------------------------------------------------------------------------------------------------- (a) whole
@pytest.mark.parametrize("name", SMALL)
def test_whole_stream(dev, name):
    check_whole(dev, name)


def test_whole_stream_two_million_marks(dev):
    check_whole(dev, "two_million_marks")


def test_whole_stream_twice_on_one_context(dev):
    """A larger layout, then smaller ones through the stream buffer it left, with nothing in between."""
    sizes = [layout(n)[1].n_slots for n in ("n1000_all_real", "n257_random", "all_short", "n2_first_only")]
    assert sizes[0] > sizes[1] > sizes[3] > sizes[2] == 0
    for name in ("n1000_all_real", "n257_random", "all_short", "n2_first_only"):
        check_whole(dev, name, decoy=False)


# ---------------------------------------------------------------------------------------------------------------- (b) sharded
def check_sharded(dev, name, few=False):
    lay, s = layout(name)
    lists = cut_lists(lay, s, few)
    assert len(lists) >= (2 if few else 6)
    spans = 0
    for label, cuts in lists:
        d = R.shard(s, cuts)
        parts = []
        for r, (lo, hi) in enumerate(d["chunks"]):
            c = dev.ctx(r, lay.k, lay.J)
            dev.decoy(c, lay, s.n_slots)
            dev.load(c, lay, s.n_slots, lo, hi)
            cnt, flags = c.emit_stream_partial(lay.rec_start, lay.rec_len)
            assert (cnt == d["cnt"][r]).all() and (flags == d["flags"][r]).all(), (label, cuts, r)
            slot0, n = d["slot0"][r], d["n_slots"][r]
            got = c.emit_stream_part(lay.rec_start, lay.rec_len, d["gflags"], d["e_scan"], d["s_scan"], d["before"][r], d["r_last"], lo, hi, slot0, n)
            assert len(got) == 12 * n, (label, cuts, r)
            assert got == s.bytes[12 * slot0:12 * (slot0 + n)], (label, cuts, r, first_difference(got, s, slot0))
            parts.append(got)
        assert b"".join(parts) == s.bytes, (label, cuts)
        if "the third sums two" in label:
            r = int(label.split()[2])
            third = max(i for i, (lo, hi) in enumerate(d["chunks"]) if d["cnt"][i][r] > 0)
            spans += int(sum(1 for i in range(third) if d["cnt"][i][r] > 0) >= 2 and d["before"][third][r] == sum(int(d["cnt"][i][r]) for i in range(third)))
    return spans


@pytest.mark.parametrize("name", SMALL)
def test_sharded_stream(dev, name):
    spans = check_sharded(dev, name)
    if name.endswith("all_real"):
        assert spans > 0    # before[] of a sequence's third rank was the sum of two earlier ranks' counts


def test_sharded_stream_two_million_marks(dev):
    check_sharded(dev, "two_million_marks", few=True)


def test_cut_lists_hold_what_they_name():
    """On a layout with every kind of sequence: each adversarial place is among the lists, for every W."""
    lay, s = layout("n513_random")
    labels = [label for label, _ in cut_lists(lay, s)]
    for what in ("separator owner", "start of", "start + 1", "last k-mer of", "last k-mer + 1", "real mark,", "real mark + 1", "invalid mark",
                 "all INVALID", "two equal cuts", "inside the short run", "spans three ranks", "random"):
        assert any(what in x or x.endswith(what.rstrip(",")) for x in labels), what
    assert {int(x.split(",")[0][2:]) for x in labels} == {2, 3, 4, 8}
    for label, cuts in cut_lists(lay, s):
        d = R.shard(s, cuts)
        if "all INVALID" in label:
            invalid = lay.marks[lay.ids == INV].tolist()
            g = invalid[len(invalid) // 2]
            assert g in cuts and g + 1 in cuts
            r = d["chunks"].index((g, g + 1))
            inside = (lay.marks >= g) & (lay.marks < g + 1)
            assert inside.sum() == 1 and (lay.ids[inside] == INV).all() and d["cnt"][r].sum() == 0
        if "two equal cuts" in label:
            assert any(lo == hi for lo, hi in d["chunks"])
        if "separator owner" in label:
            r = int(label.split()[-1])
            assert lay.rec_start[r] - 1 in cuts


# ---------------------------------------------------------------------------------------------------------------- (c) the host
K_HOST, L_HOST, Q_HOST, SEED_HOST = 25, 28, 5, 11
TILE = 512 * 32   # tpc_shard_chunk cuts at multiples of 512 words of TPC_RUN = 32 positions


def tile_chunk(n_text, rank, world):
    """[lo, hi) of tpc_shard_chunk: the text's tiles dealt out in runs of ceil(tiles / world); the last rank's end is 2^64 - 1."""
    tiles = (n_text // 32 + 512) // 512
    chunk = (tiles + world - 1) // world
    t0 = min(tiles, rank * chunk)
    return t0 * TILE, R.UINT64_MAX if rank + 1 == world else min(tiles, t0 + chunk) * TILE


def tile_cuts(n_text, world):
    """The cuts between the ranks' chunks that lie inside the text."""
    return [lo for lo, _ in (tile_chunk(n_text, r, world) for r in range(1, world)) if lo < n_text]


def host_records():
    """Record lengths so that the tile cuts of 2, 4 and 8 ranks fall on: the last k-mer of a record that spans three chunks at eight ranks
    (65536), a separator character (98304, a cut of every rank count), a first k-mer (131072), a last k-mer + 1 (147456) and the middle
    of a run of records shorter than k (163840).  Returns (lengths, {feature: position})."""
    rng = np.random.default_rng(23)
    k = K_HOST
    rec_len, at, where = [], [1], {}

    def add(n):
        rec_len.append(int(n))
        at[0] += int(n) + 1

    def fill(target):    # ordinary records until the next record starts a little in front of target
        while at[0] < target - 1200:
            add(rng.integers(100, 900))

    fill(21000)
    add(65536 + k - at[0])
    where["last k-mer"] = at[0] - 1 - k
    spanning = len(rec_len) - 1
    fill(98304)
    add(98304 - at[0])
    where["separator"] = at[0] - 1
    fill(131072)
    add(131071 - at[0])
    where["first k-mer"] = at[0]
    fill(147456)
    add(147455 + k - at[0])
    where["last k-mer + 1"] = at[0] - 1 - k + 1
    fill(163840 - 350)
    add(163840 - 350 - 1 - at[0])
    run0 = len(rec_len)
    for i in range(60):
        add((0, 1, k - 1, 7, 24, 3)[i % 6])
    where["short run"] = (run0, len(rec_len))
    fill(172000)
    add(300)
    return rec_len, where, spanning


@pytest.fixture(scope="module")
def host_case(tmp_path_factory):
    """The FASTA file, its features checked against the cuts, the oracle's bytes and the one-GPU run's."""
    from oracle import oracle as O
    from twopaco_amd import capi
    d = tmp_path_factory.mktemp("stream_host")
    rec_len, where, spanning = host_records()
    rs = R.rec_starts(rec_len)
    n_text = rs[-1] + rec_len[-1] + 1
    k = K_HOST
    cuts = {w: tile_cuts(n_text, w) for w in (2, 4, 8)}
    assert cuts[2] == [98304] and cuts[4] == [49152, 98304, 147456] and cuts[8] == [32768, 65536, 98304, 131072, 163840], (n_text, cuts)
    assert 200 <= len(rec_len) <= 500 and sum(1 for n in rec_len if n >= k) > 256
    # every feature sits on a cut
    r = spanning
    assert rs[r] + rec_len[r] - k == where["last k-mer"] == 65536 and rs[r] < 32768         # ranks 0, 1 and 2 of eight hold its k-mers
    assert where["separator"] == 98304 and 98304 + 1 in rs and rec_len[rs.index(98305) - 1] >= k
    assert where["first k-mer"] == 131072 in rs and rec_len[rs.index(131072)] >= k
    assert where["last k-mer + 1"] == 147456 and any(a + n - k + 1 == 147456 and n > k for a, n in zip(rs, rec_len))
    lo, hi = where["short run"]
    assert all(n < k for n in rec_len[lo:hi]) and rs[lo + 20] < 163840 < rs[hi - 20]
    # ACGT with repeated segments (junctions), a few N
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    segments = [letters[rng_i] for rng_i in np.random.default_rng(29).integers(0, 4, (12, 180))]
    rng = np.random.default_rng(31)
    path = str(d / "cuts.fa")
    with open(path, "wb") as f:
        for i, n in enumerate(rec_len):
            seq = letters[rng.integers(0, 4, n)].copy()
            for _ in range(n // 400 + (1 if n >= 60 and i % 3 == 0 else 0)):
                seg = segments[int(rng.integers(0, 12))][:int(rng.integers(30, 181))]
                if seg.size <= n:
                    p = int(rng.integers(0, n - seg.size + 1))
                    seq[p:p + seg.size] = seg
            if n > 300 and i % 7 == 0:
                seq[int(rng.integers(k + 1, n - k - 1))] = ord("N")
            f.write(b">r%d\n" % i)
            for p in range(0, n, 80):
                f.write(seq[p:p + 80].tobytes() + b"\n")
    text = capi.PackedText.from_fasta([path])
    assert text.length == n_text and text.rec_start.tolist() == rs and text.rec_length.tolist() == rec_len
    o = O.Oracle(K_HOST, L_HOST, Q_HOST, O.seed_table(SEED_HOST, Q_HOST, L_HOST))
    o.add_fasta(path)
    o.enumerate(rounds=1)
    o.write_bin(str(d / "oracle.bin"))
    junctions = len(o.keys)
    o.close()
    with open(str(d / "oracle.bin"), "rb") as f:
        want = f.read()
    assert junctions > 100
    one = str(d / "one.bin")
    e = capi.Enumerator([path], K_HOST, L_HOST, q=Q_HOST, tmpdir=str(d), out=one, seed=SEED_HOST)
    assert e.vertices_count() == junctions
    e.close()
    with open(one, "rb") as f:
        one_gpu = f.read()
    return {"path": path, "dir": d, "want": want, "one_gpu": one_gpu, "junctions": junctions, "rec_len": rec_len, "text": text, "cuts": cuts}


def test_host_one_gpu_run_with_more_than_256_records(host_case):
    """The pipeline's own marks and ids over several blocks of sequences: the oracle's bytes, and the writer's definition applied to
    their real-id records gives them back."""
    assert host_case["one_gpu"] == host_case["want"]
    real = R.parse(host_case["want"], host_case["junctions"])
    rs = R.rec_starts(host_case["rec_len"])
    s = R.write(K_HOST, host_case["junctions"], host_case["rec_len"], [rs[q] + p for q, p, _ in real], [i for _, _, i in real])
    assert s.bytes == host_case["want"]
    owners = set(s.owner.tolist())
    assert {65536, 98304, 131072} <= owners      # the end k-mers and the separator on the cuts own slots


@pytest.mark.parametrize("world", [2, 4, 8])
def test_shard_chunk_is_the_tile_split(host_case, world):
    """Context.shard_chunk gives the chunks the cuts above were computed from; at eight ranks the last two lie behind the text."""
    from twopaco_amd import capi
    n_text = host_case["text"].length
    for rank in range(world):
        c = capi.Context(0)
        c.shard_config(rank, world)
        c.set_params(K_HOST, 20, 1, capi.seed_table(1, 20, seed=5))
        c.seq_upload(host_case["text"])
        assert c.shard_chunk() == tile_chunk(n_text, rank, world)
        c.close()
    assert [tile_chunk(n_text, r, world)[0] for r in range(1, world)][:len(host_case["cuts"][world])] == host_case["cuts"][world]


@pytest.mark.parametrize("mode", ["entries", "default"])
@pytest.mark.parametrize("world", [2, 4, 8])
def test_host_sharded_stream_at_tile_cuts(host_case, monkeypatch, world, mode):
    """ShardedStream: every emulated rank formats the byte range of its own chunk; the file is the one-GPU run's and the oracle's."""
    from twopaco_amd import capi
    if mode == "entries":
        monkeypatch.setenv("TWOPACO_MULTIGPU", "entries")
    else:
        monkeypatch.delenv("TWOPACO_MULTIGPU", raising=False)
    monkeypatch.delenv("TWOPACO_GATHER_OUTPUT", raising=False)
    out = str(host_case["dir"] / ("w%d_%s.bin" % (world, mode)))
    e = capi.Enumerator([host_case["path"]], K_HOST, L_HOST, q=Q_HOST, tmpdir=str(host_case["dir"]), out=out, seed=SEED_HOST, gpus=world, emulate_ranks=True)
    assert "GPUs = %d" % world in e.log, e.log     # not the one-GPU fallback of a saturated filter
    assert e.vertices_count() == host_case["junctions"]
    e.close()
    with open(out, "rb") as f:
        got = f.read()
    assert got == host_case["one_gpu"]
    assert got == host_case["want"]
