"""GPU (-m gpu): the kernels of the sharded verification (csrc/tpc_qpartition.hip: k_v_addrs / k_v_addrs2, k_v_probe, k_v_mark,
k_v_finish, k_select, k_surv_gather, k_route_count / _scatter / _count64 / _scatter64, k_permute64, k_survivor_sources, the mask OR)
through their C-ABI calls, each against its definition in tests/shard_verify_reference.py.  One process, up to eight contexts on
device 0, no communication library: what a collective would move is moved with tensor slicing.  Every comparison is exact.

a. routing, selection, marks and the mask calls on synthetic arrays;  b. probe addresses and owners of chosen survivor ids over a
table of geometries (both address kernels, every (first function, count), 1..8 ranks, two and three levels, several batches, a rank
with no tiles);  c. one walk through the whole protocol per world, in both pinned round shapes, against the oracle."""
import numpy as np
import pytest

import shard_verify_reference as R
from helpers import text_codes
from oracle import oracle as O

pytestmark = pytest.mark.gpu

INSERT, QUERY = 0, 1
SEED = 1  # seed of the hash tables.  Under it every L = 14 address case holds edges whose function-0 strand hashes tie although the
# (k+1)-mer is not its own reverse complement (at k = 9 only a handful of letter patterns can: most seeds have none); the test asserts it
SENT64 = -0x0123456789ABCDEF  # pre-fill of output buffers that must stay untouched
N_SMALL = [0, 1, 63, 64, 255, 256, 4095, 4096, 4097, 3 * 4096 + 17]
N_OVER_COUNT_GRID = 2048 * 256 + 1        # k_route_count: 2048 workgroups of 256 items
N_OVER_SCATTER_GRID = 4096 * 4096 + 4097  # k_route_scatter: 4096 workgroups of 4096-item chunks
N_OVER_SELECT_GRID = 8192 * 256 + 257     # k_select / k_v_finish: 8192 workgroups of 256 survivors
N_OVER_ADDR_GRID = 4096 * 256 + 3         # k_v_addrs / k_v_addrs2: 4096 workgroups of 256 ids


@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def to_dev(torch, a):
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).cuda()


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


# ================================================================================================ a. routing
def owners_of(pattern, n, W, rng):
    if pattern == "uniform":
        o = rng.integers(0, W, n)
    elif pattern == "last":
        o = np.full(n, W - 1)
    elif pattern == "absent":  # owner W / 2 gets nothing
        o = rng.integers(0, W - 1, n)
        o[o >= W // 2] += 1
    else:  # alternating
        o = np.where(np.arange(n) % 2 == 0, 0, W - 1)
    return o.astype(np.int32)


def check_route(ctx, torch, owner, W, rng):
    n = owner.size
    o_dev = to_dev(torch, owner) if n else torch.zeros(1, dtype=torch.int32, device="cuda")
    perm = torch.full((n + 5,), -1, dtype=torch.int32, device="cuda")
    counts = ctx.shard_route(o_dev.data_ptr(), n, perm.data_ptr(), W)
    p = u32(perm)
    assert (p[n:] == 0xFFFFFFFF).all()
    p = p[:n].astype(np.int64)
    assert R.route_violations(p, owner, counts, W) == [], (n, W, counts)
    src = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    s_dev = to_dev(torch, src) if n else torch.zeros(1, dtype=torch.int64, device="cuda")
    dst = torch.full((n + 5,), SENT64, dtype=torch.int64, device="cuda")
    ctx.shard_permute64(s_dev.data_ptr(), perm.data_ptr(), n, dst.data_ptr())
    d = dst.cpu().numpy()
    assert (d[n:] == SENT64).all()
    assert (d[:n].view(np.uint64)[p] == src).all(), (n, W)
    if n > (1 << 20):
        return
    for row_words in (1, 3, 5):  # the same for rows of several words
        rows = rng.integers(0, 1 << 63, (n, row_words), dtype=np.uint64)
        r_dev = to_dev(torch, rows.reshape(-1)) if n else torch.zeros(1, dtype=torch.int64, device="cuda")
        dst = torch.full((n * row_words + 5,), SENT64, dtype=torch.int64, device="cuda")
        ctx.shard_permute_rows(r_dev.data_ptr(), perm.data_ptr(), n, row_words, dst.data_ptr())
        d = dst.cpu().numpy()
        assert (d[n * row_words:] == SENT64).all()
        assert (d[:n * row_words].view(np.uint64).reshape(n, row_words)[p] == rows).all(), (n, W, row_words)


@pytest.mark.parametrize("W", [1, 2, 8, 64])
def test_route_and_permute(capi, torch, W):
    """perm is a bijection onto the slots, counts is the histogram of the owners, every slot lies in its owner's range, and
    permute64 puts every item where perm says -- for whole and partial chunks, several chunks per owner, skewed and absent owners."""
    ctx = capi.Context(0)
    try:
        ctx.shard_config(0, W)
        rng = np.random.default_rng(100 + W)
        for n in N_SMALL:
            for pattern in ("uniform", "last", "absent", "alternating"):
                if pattern == "absent" and W == 1:
                    continue
                check_route(ctx, torch, owners_of(pattern, n, W, rng), W, rng)
    finally:
        ctx.close()


def test_route_beyond_the_count_kernels_grid(capi, torch):
    ctx = capi.Context(0)
    try:
        ctx.shard_config(0, 8)
        rng = np.random.default_rng(7)
        check_route(ctx, torch, owners_of("absent", N_OVER_COUNT_GRID, 8, rng), 8, rng)
    finally:
        ctx.close()


def test_route_beyond_the_scatter_kernels_grid(capi, torch):
    """16.8 M items for 64 owners: every workgroup of the scatter kernel takes a second chunk and reserves slots twice."""
    ctx = capi.Context(0)
    try:
        ctx.shard_config(0, 64)
        rng = np.random.default_rng(8)
        check_route(ctx, torch, owners_of("uniform", N_OVER_SCATTER_GRID, 64, rng), 64, rng)
    finally:
        ctx.close()


def test_route_refuses_an_owner_outside_the_world(capi, torch):
    ctx = capi.Context(0)
    try:
        ctx.shard_config(0, 2)
        owner = np.array([0, 1, 1, 5, 0, 1, 0], dtype=np.int32)
        perm = torch.full((owner.size,), -1, dtype=torch.int32, device="cuda")
        with pytest.raises(RuntimeError, match="counted 6 of 7 items"):
            ctx.shard_route(to_dev(torch, owner).data_ptr(), owner.size, perm.data_ptr(), 2)
        assert (perm.cpu().numpy() == -1).all()  # refused before the scatter
        owner[3] = 1
        assert ctx.shard_route(to_dev(torch, owner).data_ptr(), owner.size, perm.data_ptr(), 2) == [3, 4]
    finally:
        ctx.close()


# ================================================================================================ a. selection
def hits_of(rng, total, density):
    if density == 0:
        return np.zeros(total, dtype=np.uint8)
    if density == 1:
        return np.ones(total, dtype=np.uint8)
    return (rng.random(total) < density).astype(np.uint8)


def selection_inputs(torch, rng, n, fc, density, with_perm, sid=None):
    """(sid, keep, device sid / hit / perm pointer holders): answers in send order, a random bijection as the send order."""
    if sid is None:
        sid = rng.integers(0, max(1, n // 3) + 1, n).astype(np.uint64) * np.uint64(8) + rng.integers(0, 8, n).astype(np.uint64)  # duplicated ids
    hit = hits_of(rng, n * fc, density)
    perm = rng.permutation(n * fc).astype(np.uint32) if with_perm else None
    keep = R.all_hit(hit, n, fc, perm)
    one64 = torch.zeros(1, dtype=torch.int64, device="cuda")
    d = {"sid": to_dev(torch, sid) if n else one64, "hit": to_dev(torch, hit) if n else torch.zeros(4, dtype=torch.uint8, device="cuda"),
         "perm": to_dev(torch, perm) if with_perm and n else None}
    if with_perm and not n:
        d["perm"] = torch.zeros(1, dtype=torch.int32, device="cuda")
    d["perm_ptr"] = d["perm"].data_ptr() if d["perm"] is not None else 0  # 0: the natural order
    return sid, keep, d


def check_select(ctx, torch, rng, n, fc, density, with_perm):
    sid, keep, d = selection_inputs(torch, rng, n, fc, density, with_perm)
    out = torch.full((n + 3,), SENT64, dtype=torch.int64, device="cuda")
    m = ctx.shard_select(d["sid"].data_ptr(), n, fc, d["hit"].data_ptr(), d["perm_ptr"], out.data_ptr())
    got = out.cpu().numpy()
    assert m == int(keep.sum()), (n, fc, density, with_perm, m, int(keep.sum()))
    assert (got[m:] == SENT64).all()
    assert (np.sort(got[:m].view(np.uint64)) == np.sort(sid[keep])).all(), (n, fc, density, with_perm)


@pytest.mark.parametrize("fc", [1, 2, 3, 4, 5, 7, 8, 15])
def test_select(capi, torch, fc):
    """The kept ids are exactly those whose fc answers are all 1 -- answers in natural order (four of them: one 32-bit compare) and
    behind a send order -- as a multiset, with the count, and nothing written behind them."""
    ctx = capi.Context(0)
    try:
        rng = np.random.default_rng(200 + fc)
        for density in (0, 0.5, 0.97, 1):
            for n in N_SMALL:
                for with_perm in (False, True):
                    check_select(ctx, torch, rng, n, fc, density, with_perm)
    finally:
        ctx.close()


@pytest.mark.parametrize("fc,with_perm", [(4, False), (3, True)])
def test_select_beyond_its_grid(capi, torch, fc, with_perm):
    ctx = capi.Context(0)
    try:
        check_select(ctx, torch, np.random.default_rng(300 + fc), N_OVER_SELECT_GRID, fc, 0.97, with_perm)
    finally:
        ctx.close()


# ================================================================================================ texts and planned contexts
def random_records(seed, lengths, n_run=50):
    """Random records, a run of N in the second one."""
    rng = np.random.default_rng(seed)
    recs = [rng.integers(0, 4, n).astype(np.uint8) for n in lengths]
    if len(recs) > 1 and n_run:
        a = int(rng.integers(200, lengths[1] - 200 - n_run))
        recs[1][a:a + n_run] = 4
    return recs


def definite_windows(codes, k):
    """definite[g]: T[g .. g+k-1] lies inside the text and holds no N."""
    bad = np.concatenate([[0], np.cumsum(codes > 3)])
    ok = np.zeros(codes.size, dtype=bool)
    m = codes.size - k + 1
    ok[:m] = (bad[k:k + m] - bad[:m]) == 0
    return ok


class Ranks:
    """W contexts on one text: parameters, upload, shard_config, filter_reset, the query's plan."""

    def __init__(self, capi, torch, recs, k, L, q, W, options, seed=SEED, only=None):
        self.capi, self.torch, self.k, self.L, self.q, self.W = capi, torch, k, L, q, W
        self.text = capi.PackedText.from_codes(recs)
        self.n_text = self.text.length
        self.codes = text_codes(np.asarray(self.text.bases), np.asarray(self.text.nmask), self.n_text)
        self.table = capi.seed_table(q, L, seed=seed)
        self.n_tiles = R.text_tiles(self.n_text)
        self.ctxs = [None] * W  # (only: the ranks to open; the others stay None)
        for r in (range(W) if only is None else only):
            c = self.ctxs[r] = capi.Context(0)
            for name, val in options.items():
                c.set_option(name, val)
            c.shard_config(r, W)  # (before the parameters: the filter is then allocated once, at its sharded size)
            c.set_params(k, L, q, self.table)
            c.seq_upload(self.text)
            c.shard_config(r, W)
            c.filter_reset()
        self._ref = {}

    def open(self):
        return [c for c in self.ctxs if c is not None]

    def close(self):
        for c in self.open():
            c.close()
        self.text.close()

    def plan_query(self):
        geoms = [c.shard_plan(QUERY) for c in self.open()]
        assert all(g == geoms[0] for g in geoms)
        self.geom = geoms[0]
        self.per, self.batches = self.geom["tiles_per_rank"], self.geom["batches"]
        return self.geom

    def batch_range(self, r, b):
        """[base, end) of the positions rank r hashes in batch b (empty: base >= end)."""
        chunk = (self.n_tiles + self.W - 1) // self.W
        c1 = min(self.n_tiles, min(self.n_tiles, r * chunk) + chunk)
        base = R.chunk_base(self.n_tiles, r, self.W, self.per, b)
        end = min(c1, base // R.TILE_POSITIONS + self.per) * R.TILE_POSITIONS
        return base, end

    def establish(self, r, b):
        """A shard_apply of batch b with nothing received: no survivors; it sets the base the ids of rank r are relative to."""
        torch, g = self.torch, self.geom
        regions = torch.zeros(max(16, self.W * g["region_block_bytes"]), dtype=torch.uint8, device="cuda")
        counts = torch.zeros(max(16, self.W * g["count_block_bytes"]), dtype=torch.uint8, device="cuda")
        assert self.ctxs[r].shard_apply(QUERY, b, regions.data_ptr(), counts.data_ptr()) == 0

    def mask(self, r):
        c = self.ctxs[r]
        m = self.torch.zeros(c.mask_words(), dtype=self.torch.int32, device="cuda")
        c.mask_export(m.data_ptr())
        return u32(m)

    def addresses(self, g, e):
        """Reference addresses [n, q] of the edges (g[i], e[i]), each distinct edge hashed once."""
        out = np.zeros((len(g), self.q), dtype=np.uint64)
        for i, key in enumerate(zip(g.tolist(), e.tolist())):
            a = self._ref.get(key)
            if a is None:
                a = self._ref[key] = np.array(R.edge_hashes(self.codes, key[0], key[1], self.k, self.L, self.table), dtype=np.uint64)
            out[i] = a
        return out


@pytest.fixture(scope="class")
def planned(capi, torch):
    """Two planned and established query contexts on one small text: the only rank of one, and rank 2 of four (its ids carry
    source bits, its base is not 0)."""
    recs = random_records(11, (30000, 25000, 20000))  # 5 tiles: rank 2 of 4 owns tile 4
    one = Ranks(capi, torch, recs, 25, 20, 5, 1, {"slice_bits": 10})
    four = Ranks(capi, torch, recs, 25, 20, 5, 4, {"slice_bits": 10}, only=[2])
    out = []
    for rk, r in ((one, 0), (four, 2)):
        rk.plan_query()
        assert rk.batches == 1
        rk.establish(r, 0)
        base, end = rk.batch_range(r, 0)
        assert base < rk.n_text and (r == 0 or base > 0)
        out.append({"ranks": rk, "ctx": rk.ctxs[r], "rank": r, "W": rk.W, "base": base, "span": min(end, rk.n_text) - base})
    yield out
    one.close()
    four.close()


def marking_ids(rng, n, p):
    """n survivor ids of rank p["rank"]: positions of its batch (a vertex often twice: in- and out-edge), its own source bits."""
    rel = rng.integers(0, min(p["span"], max(1, n // 2) + 1), n)
    if n > 2:
        rel[0], rel[1] = 0, p["span"] - 1
    lw = p["W"].bit_length() - 1
    field = (np.uint64(p["rank"]) << np.uint64(30 - lw)) | rel.astype(np.uint64)
    return (field << np.uint64(3)) | rng.integers(0, 8, n).astype(np.uint64), rel


def random_mask(rng, words):
    m = rng.integers(0, 1 << 32, words, dtype=np.uint64).astype(np.uint32)
    return m & rng.integers(0, 1 << 32, words, dtype=np.uint64).astype(np.uint32) & rng.integers(0, 1 << 32, words, dtype=np.uint64).astype(np.uint32)


def check_finish(p, torch, rng, n, fc, density, with_perm):
    ctx = p["ctx"]
    sid, rel = marking_ids(rng, n, p)
    sid, keep, d = selection_inputs(torch, rng, n, fc, density, with_perm, sid=sid)
    before = random_mask(rng, ctx.mask_words())
    ctx.mask_import(to_dev(torch, before).data_ptr())
    marked = ctx.shard_finish(d["sid"].data_ptr(), n, fc, d["hit"].data_ptr(), d["perm_ptr"])
    after = p["ranks"].mask(p["rank"])
    assert marked == int(keep.sum()), (n, fc, density, with_perm, marked, int(keep.sum()))  # survivors, not bits
    assert (after == R.mask_with_bits(before, p["base"] + rel[keep])).all(), (n, fc, density, with_perm)


class TestMarksAndMasks:
    """On the two planned contexts of the class-scoped fixture `planned` (closed again before the address cases open up to eight)."""

    @pytest.mark.parametrize("fc", [1, 2, 3, 4, 5, 7, 8, 15])
    def test_finish(self, planned, torch, fc):
        """The mask after tpc_shard_finish is the mask before with the positions of the kept survivors set, bit for bit; n_marked
        counts the kept survivors, duplicates and already set bits included."""
        rng = np.random.default_rng(400 + fc)
        for p in planned:
            for density in (0, 0.5, 0.97, 1):
                for n in N_SMALL:
                    for with_perm in (False, True):
                        check_finish(p, torch, rng, n, fc, density, with_perm)


    @pytest.mark.parametrize("fc,with_perm", [(4, False), (3, True)])
    def test_finish_beyond_its_grid(self, planned, torch, fc, with_perm):
        check_finish(planned[1], torch, np.random.default_rng(500 + fc), N_OVER_SELECT_GRID, fc, 0.97, with_perm)


    def test_mark(self, planned, torch):
        rng = np.random.default_rng(600)
        for p in planned:
            ctx = p["ctx"]
            for n in N_SMALL + [4096 * 256 + 5]:  # (the last: beyond k_v_mark's grid)
                sid, rel = marking_ids(rng, n, p)
                before = random_mask(rng, ctx.mask_words())
                ctx.mask_import(to_dev(torch, before).data_ptr())
                ctx.shard_mark((to_dev(torch, sid) if n else torch.zeros(1, dtype=torch.int64, device="cuda")).data_ptr(), n)
                assert (p["ranks"].mask(p["rank"]) == R.mask_with_bits(before, p["base"] + rel)).all(), n


    @pytest.mark.parametrize("W", [1, 2, 8, 64])
    def test_survivor_sources(self, capi, torch, W):
        """src[i] = the top log2(W) bits of the 30-bit position field, both ends of the field included."""
        rk = Ranks(capi, torch, random_records(12, (9000, 5000)), 25, 26, 5, 1, {"slice_bits": 14})
        try:
            ctx = rk.ctxs[0]
            ctx.shard_config(0, W)
            ctx.shard_plan(QUERY)
            rng = np.random.default_rng(700 + W)
            for n in (1, 255, 4097, 4096 * 256 + 7):
                field = rng.integers(0, 1 << 30, n).astype(np.uint64)
                field[0] = (1 << 30) - 1
                if n > 1:
                    field[1] = 0
                sid = (field << np.uint64(3)) | rng.integers(0, 8, n).astype(np.uint64)
                src = torch.full((n + 3,), -7, dtype=torch.int32, device="cuda")
                ctx.shard_survivor_sources(to_dev(torch, sid).data_ptr(), n, src.data_ptr())
                got = src.cpu().numpy()
                assert (got[n:] == -7).all()
                assert (got[:n] == ((sid >> np.uint64(3)) >> np.uint64(30 - (W.bit_length() - 1))).astype(np.int32)).all()
                assert (got[:n] == R.sid_parts(sid, W)[0].astype(np.int32)).all()
        finally:
            rk.close()


    def test_mask_calls(self, planned, torch):
        """export_padded zero-fills its tail and stops at total_words; or_blocks and merge are the OR of their blocks; import / export round-trip."""
        ctx = planned[0]["ctx"]
        rng = np.random.default_rng(800)
        nw = ctx.mask_words()
        assert nw == (planned[0]["ranks"].n_text >> 5) + 1
        mask = random_mask(rng, nw)
        ctx.mask_import(to_dev(torch, mask).data_ptr())
        assert (planned[0]["ranks"].mask(0) == mask).all()
        for total in (nw, nw + 37):
            out = torch.full((total + 9,), -1, dtype=torch.int32, device="cuda")
            ctx.mask_export_padded(out.data_ptr(), total)
            got = u32(out)
            assert (got[:nw] == mask).all() and (got[nw:total] == 0).all() and (got[total:] == 0xFFFFFFFF).all()
        with pytest.raises(RuntimeError):
            ctx.mask_export_padded(torch.zeros(nw, dtype=torch.int32, device="cuda").data_ptr(), nw - 1)
        words = 1000 + 3  # no multiple of the OR kernel's 256
        for count in (1, 2, 5):
            blocks = np.stack([random_mask(rng, words) for _ in range(count)])
            out = torch.full((words + 9,), -1, dtype=torch.int32, device="cuda")
            ctx.mask_or_blocks(to_dev(torch, blocks.reshape(-1)).data_ptr(), count, words, out.data_ptr())
            got = u32(out)
            assert (got[:words] == np.bitwise_or.reduce(blocks, axis=0)).all() and (got[words:] == 0xFFFFFFFF).all(), count
        for count in (0, 1, 3):
            ctx.mask_import(to_dev(torch, mask).data_ptr())
            blocks = np.stack([random_mask(rng, nw) for _ in range(max(count, 1))])
            ctx.mask_merge(to_dev(torch, blocks.reshape(-1)).data_ptr(), count)
            want = mask if count == 0 else mask | np.bitwise_or.reduce(blocks[:count], axis=0)
            assert (planned[0]["ranks"].mask(0) == want).all(), count


# ================================================================================================ b. addresses
def fn0_tie_candidates(codes, k, L, table):
    """(g, e) of the edges on which function 0's two strand hashes are equal, found with prefix XORs over the whole text; only a way to
    FIND them -- what the test asserts about them comes from shard_verify_reference."""
    lm = np.uint64((1 << L) - 1)

    def rotl(x, r):
        r = (np.asarray(r, dtype=np.int64) % L).astype(np.uint64)
        return ((x << r) & lm) | (x >> (np.uint64(L) - r))

    x = np.minimum(codes.astype(np.int64), 3)
    j = np.arange(x.size, dtype=np.int64)
    h = np.asarray(table[0][:4], dtype=np.uint64)
    su = np.concatenate([[np.uint64(0)], np.bitwise_xor.accumulate(rotl(h[x], -j))])
    sv = np.concatenate([[np.uint64(0)], np.bitwise_xor.accumulate(rotl(h[3 - x], j))])
    g = np.nonzero(definite_windows(codes, k))[0]
    pos, neg = rotl(su[g + k] ^ su[g], k - 1 + g), rotl(sv[g + k] ^ sv[g], -g)
    found = []
    for c in range(4):
        hc, hr = h[c], h[3 - c]
        tie_in = (rotl(hc, k) ^ pos) == (rotl(neg, 1) ^ hr)
        tie_out = (rotl(pos, 1) ^ hc) == (neg ^ rotl(hr, k))
        found += [(int(a), c) for a in g[tie_in]] + [(int(a), 4 + c) for a in g[tie_out]]
    return sorted(found)


def choose_edges(rk, r, b, distinct, rng):
    """Distinct (g, e) of rank r's batch b: the first and last definite window of the batch, the last window of the text when it lies
    there, windows at g mod 32 = 0, 1 and 31, every e, and random ones up to `distinct`."""
    base, end = rk.batch_range(r, b)
    end = min(end, rk.n_text)
    ok = np.nonzero(rk.definite[base:end])[0] + base
    assert ok.size > 100
    must = [ok[0], ok[-1]] + [ok[ok % 32 == m][i] for m in (0, 1, 31) for i in (0, -1)]
    edges = {(int(g), e) for g in must for e in range(8)}
    last = rk.n_text - 1 - rk.k  # the window that ends at the text's last letter
    if base <= last < end:
        assert rk.definite[last] and not rk.definite[last + 1]
        edges |= {(last, e) for e in range(8)}
    edges |= {t for t in rk.ties if base <= t[0] < end}
    while len(edges) < distinct:
        edges.add((int(ok[rng.integers(0, ok.size)]), int(rng.integers(0, 8))))
    g, e = np.array(sorted(edges)).T
    return base, g, e


# name: k, L, q, W, slice_bits, levels, record lengths, distinct edges per rank, further options
ADDR_CASES = {
    "k9_L14_q5_w1": (9, 14, 5, 1, 6, 0, (9000, 5000, 3000), 1500, {}),
    "k9_L14_q1_w2": (9, 14, 1, 2, 8, 0, (20000, 9000, 5000), 1000, {}),
    "k25_L14_q2_w4_3lv_empty_rank": (25, 14, 2, 4, 6, 3, (30000, 25000, 20000), 700, {}),  # 5 tiles on 4 ranks: 2, 2, 1 (partly text), 0
    "k31_L14_q8_w8": (31, 14, 8, 8, 6, 0, (60000, 40000, 25000), 300, {}),
    "k32_L14_q1_w8": (32, 14, 1, 8, 6, 0, (60000, 40000, 25000), 300, {}),
    "k33_L14_q5_w4": (33, 14, 5, 4, 8, 0, (30000, 25000, 20000), 500, {}),
    "k65_L14_q9_w1": (65, 14, 9, 1, 6, 0, (9000, 5000, 3000), 600, {}),
    "k9_L14_q16_w2_3lv": (9, 14, 16, 2, 6, 3, (20000, 9000, 5000), 500, {}),
    "k25_L26_q5_w1_over_grid": (25, 26, 5, 1, 14, 0, (9000, 5000, 3000), 1500, {}),
    "k25_L26_q5_w4_batches": (25, 26, 5, 4, 14, 0, (70000, 50000, 40000), 500, {"part_min_tiles": 1, "part_budget_bytes": 1 << 20}),
    "k31_L26_q16_w2": (31, 26, 16, 2, 14, 0, (20000, 9000, 5000), 400, {}),
    "k9_L26_q9_w8_3lv": (9, 26, 9, 8, 14, 3, (60000, 40000, 25000), 200, {}),
    "k32_L26_q5_w2": (32, 26, 5, 2, 12, 0, (20000, 9000, 5000), 800, {}),
    "k64_L26_q2_w1_3lv": (64, 26, 2, 1, 14, 3, (9000, 5000, 3000), 1000, {}),
    "k64_L26_q16_w8": (64, 26, 16, 8, 14, 0, (60000, 40000, 25000), 100, {}),
    "k97_L26_q8_w4": (97, 26, 8, 4, 14, 0, (30000, 25000, 20000), 250, {}),
    "k33_L26_q5_w4_3lv": (33, 26, 5, 4, 10, 3, (30000, 25000, 20000), 500, {}),
    "k65_L34_q5_w2": (65, 34, 5, 2, 20, 0, (20000, 9000, 5000), 500, {}),
    "k31_L34_q1_w1_3lv": (31, 34, 1, 1, 20, 3, (9000, 5000, 3000), 1500, {}),
    "k25_L34_q2_w8_3lv": (25, 34, 2, 8, 20, 3, (60000, 40000, 25000), 300, {}),
}


def plant_palindrome(recs, k):
    """k odd: a (k+1)-mer equal to its reverse complement in the first record -- both strands hash alike under every function."""
    if k % 2 == 0:
        return
    half = recs[0][1000:1000 + (k + 1) // 2].copy()
    recs[0][1000 + half.size:1000 + k + 1] = 3 - half[::-1]


def addr_case_records(name):
    k = ADDR_CASES[name][0]
    recs = random_records(sum(ord(ch) for ch in name), ADDR_CASES[name][6])
    plant_palindrome(recs, k)
    return recs


@pytest.mark.parametrize("name", list(ADDR_CASES))
def test_verify_addrs_and_send(capi, torch, name):
    """tpc_shard_verify_addrs for every (fn, cnt) and tpc_shard_verify_send for the round shapes, on every rank: owner and local
    address of each probe are owner_local(edge_hashes(...)) of the reference."""
    k, L, q, W, sb, levels, lengths, distinct, extra = ADDR_CASES[name]
    rk = Ranks(capi, torch, addr_case_records(name), k, L, q, W, dict({"slice_bits": sb, "part_levels": levels}, **extra))
    try:
        geom = rk.plan_query()
        assert (geom["b3"] > 0) == (levels == 3) and geom["slice_bits"] == sb
        if extra:
            assert rk.batches > 1
        rk.definite = definite_windows(rk.codes, k)
        rk.ties = fn0_tie_candidates(rk.codes, k, L, rk.table) if L == 14 else []
        rk.tie_set = set(rk.ties)
        rng = np.random.default_rng(len(name))
        depth_seen, empty_ranks = [], 0
        for r in range(W):
            ctx = rk.ctxs[r]
            nonempty = [b for b in range(rk.batches) if rk.batch_range(r, b)[0] < min(rk.batch_range(r, b)[1], rk.n_text)]
            if not nonempty:
                empty_ranks += 1  # (nothing is asked of a rank that hashes nothing)
                continue
            assert ctx.shard_chunk()[0] == R.chunk_base(rk.n_tiles, r, W, rk.per, 0)
            for b in sorted({nonempty[0], nonempty[-1]}):
                rk.establish(r, b)
                base, g, e = choose_edges(rk, r, b, distinct, rng)
                # the base first: the id with field 0 marks exactly the batch's first position
                before = rk.mask(r)
                ctx.shard_mark(to_dev(torch, np.array([R.make_sid(r, 0, 5, W)], dtype=np.uint64)).data_ptr(), 1)
                assert base == R.chunk_base(rk.n_tiles, r, W, rk.per, b)
                assert (rk.mask(r) == R.mask_with_bits(before, [base])).all(), (r, b, base)
                depth_seen += [R.tie_depth(rk.codes, gg, ee, k, L, rk.table) for gg, ee in zip(g.tolist(), e.tolist()) if (gg, ee) in rk.tie_set]
                check_rank_addresses(rk, r, base, g, e, rng, big=name.endswith("over_grid"))
        # ranks whose chunk begins at or behind the last tile hash nothing: their chunk is the empty one at the end of the text
        chunk = (rk.n_tiles + W - 1) // W
        empty = [r for r in range(W) if r * chunk >= rk.n_tiles]
        assert empty_ranks == len(empty) and (len(empty) == 1 or "empty_rank" not in name)
        for r in empty:
            assert rk.ctxs[r].shard_chunk()[0] == R.chunk_base(rk.n_tiles, r, W, rk.per, 0) == rk.n_tiles * R.TILE_POSITIONS
        if L == 14:
            # the tie chain is really taken: function 0 ties on some edges, later functions decide them -- or none does (a palindrome)
            assert len(depth_seen) > 0 and min(depth_seen) >= 1, name
            if q > 1:
                assert any(d < q for d in depth_seen), name
            if k % 2:
                assert any(d == q for d in depth_seen), name
    finally:
        rk.close()


def check_rank_addresses(rk, r, base, g, e, rng, big):
    torch, ctx, q, W = rk.torch, rk.ctxs[r], rk.q, rk.W
    A = rk.addresses(g, e)
    assert A.max() < (1 << rk.L)
    owner, local = R.owner_local(A, rk.geom, W)
    if W == 1:
        assert (local == A).all()
    # ids with repetition, in random order, this rank's source bits on top
    n_all = int(max(g.size, min(3000, 3 * g.size)))
    pick = np.concatenate([np.arange(g.size), rng.integers(0, g.size, n_all - g.size)])
    rng.shuffle(pick)
    lw = W.bit_length() - 1
    sid_all = (((np.uint64(r) << np.uint64(30 - lw)) | (g[pick] - base).astype(np.uint64)) << np.uint64(3)) | e[pick].astype(np.uint64)
    assert int((g - base).max()) < (1 << (30 - lw))
    sid_dev = to_dev(torch, sid_all)

    def addrs(fn, cnt, n, sids=sid_dev):
        addr = torch.full((n * cnt + 3,), SENT64, dtype=torch.int64, device="cuda")
        own = torch.full((n * cnt + 3,), -7, dtype=torch.int32, device="cuda")
        ctx.shard_verify_addrs(fn, cnt, sids.data_ptr(), n, addr.data_ptr(), own.data_ptr())
        a, o = addr.cpu().numpy(), own.cpu().numpy()
        assert (a[n * cnt:] == SENT64).all() and (o[n * cnt:] == -7).all()
        return a[:n * cnt].view(np.uint64).reshape(n, cnt), o[:n * cnt].reshape(n, cnt)

    for fn in range(q):
        for cnt in range(1, q - fn + 1):
            a, o = addrs(fn, cnt, n_all)
            assert (a == local[pick, fn:fn + cnt]).all(), (r, fn, cnt)
            assert (o == owner[pick, fn:fn + cnt]).all(), (r, fn, cnt)
    for n in (1, 255, 257):
        a, o = addrs(q - 1, 1, n)
        assert (a[:, 0] == local[pick[:n], q - 1]).all() and (o[:, 0] == owner[pick[:n], q - 1]).all(), (r, n)
    # refused before anything runs
    for fn, cnt in ((0, q + 1), (q - 1, 2), (q, 1), (0, 0), (-1, 1)):
        addr = torch.full((n_all * (q + 1),), SENT64, dtype=torch.int64, device="cuda")
        own = torch.full((n_all * (q + 1),), -7, dtype=torch.int32, device="cuda")
        with pytest.raises(RuntimeError):
            ctx.shard_verify_addrs(fn, cnt, sid_dev.data_ptr(), n_all, addr.data_ptr(), own.data_ptr())
        assert (addr.cpu().numpy() == SENT64).all() and (own.cpu().numpy() == -7).all()
    # the round shapes through the fused call: addresses already in owner-major send order
    shapes = {(0, q), (0, 1)} | ({(1, q - 1), (1, 1)} if q > 1 else set()) | ({(2, q - 2)} if q > 2 else set())
    for fn, cnt in sorted(shapes):
        check_verify_send(rk, r, sid_dev, n_all, fn, cnt, A[pick, fn:fn + cnt], owner[pick, fn:fn + cnt], local[pick, fn:fn + cnt])
    with pytest.raises(RuntimeError):
        ctx.shard_verify_send(0, 0, sid_dev.data_ptr(), n_all, 0, 0, 0, W)
    if big:  # more ids than the address kernel's grid has threads: each distinct id many times over
        n = N_OVER_ADDR_GRID
        pick2 = rng.integers(0, g.size, n)
        sid2 = (((np.uint64(r) << np.uint64(30 - lw)) | (g[pick2] - base).astype(np.uint64)) << np.uint64(3)) | e[pick2].astype(np.uint64)
        a, o = addrs(1, q - 1, n, to_dev(torch, sid2))
        assert (a == local[pick2, 1:]).all() and (o == owner[pick2, 1:]).all()


def check_verify_send(rk, r, sid_dev, n, fn, cnt, A, owner, local):
    torch, ctx, W = rk.torch, rk.ctxs[r], rk.W
    total = n * cnt
    send = torch.full((total + 3,), SENT64, dtype=torch.int64, device="cuda")
    if W == 1:  # the natural order is the send order: untagged, unpermuted, the plain hash addresses
        counts = ctx.shard_verify_send(fn, cnt, sid_dev.data_ptr(), n, 0, send.data_ptr(), 0, 1)
        s = send.cpu().numpy()
        assert counts == [total] and (s[total:] == SENT64).all()
        assert (s[:total].view(np.uint64) == A.reshape(-1)).all(), (fn, cnt)
        return None, u64(send)[:total]
    tmp = torch.zeros(total, dtype=torch.int64, device="cuda")
    perm = torch.full((total + 3,), -1, dtype=torch.int32, device="cuda")
    counts = ctx.shard_verify_send(fn, cnt, sid_dev.data_ptr(), n, tmp.data_ptr(), send.data_ptr(), perm.data_ptr(), W)
    s, p = send.cpu().numpy(), u32(perm)
    assert (s[total:] == SENT64).all() and (p[total:] == 0xFFFFFFFF).all()
    p = p[:total].astype(np.int64)
    assert R.route_violations(p, owner.reshape(-1), counts, W) == [], (r, fn, cnt, counts)  # counts, a bijection, grouped by owner
    assert (s[:total].view(np.uint64)[p] == local.reshape(-1)).all(), (r, fn, cnt)  # (no owner tag left on the address)
    return p, s[:total].view(np.uint64)


# ================================================================================================ c. the protocol, by hand
WALK_K, WALK_L, WALK_Q, WALK_SB = 25, 20, 5, 10


@pytest.fixture(scope="module")
def walk_case():
    """Three copies of one random sequence with a few substitutions (true junctions), an N run; the oracle's filter and round mask."""
    rng = np.random.default_rng(31)
    base = rng.integers(0, 4, 11500).astype(np.uint8)
    recs = []
    for i in range(3):
        s = base.copy()
        at = rng.integers(30, s.size - 30, 35)
        s[at] = (s[at] + rng.integers(1, 4, at.size)) % 4
        recs.append(s.astype(np.uint8))
    recs[1][5000:5040] = 4
    o = O.Oracle(WALK_K, WALK_L, WALK_Q, O.seed_table(SEED, WALK_Q, WALK_L))
    letters = np.frombuffer(b"ACGTN", dtype=np.uint8)
    for s in recs:
        o.add_record(letters[s].tobytes())
    o.fill_only()
    marks = o.check_only()
    case = {"recs": recs, "filter": o.filter.copy(), "round_mask": o.round_mask.copy(), "marks": marks, "table": o.table.copy(), "hashes": {}}
    o.close()
    return case


def exchange_equal(torch, sends, W):
    """Block o of rank r's buffer becomes block r of rank o's."""
    blocks = [s.view(W, -1) for s in sends]
    return [torch.stack([blocks[r][o] for r in range(W)]).contiguous().view(-1) for o in range(W)]


def exchange_var(torch, sends, counts, W):
    """The counts[r][o] items of rank r for rank o, in rank order, on rank o; also where each came from (r, slot in r's buffer)."""
    out, origin = [], []
    for o in range(W):
        parts, orig = [], []
        for r in range(W):
            off = sum(counts[r][:o])
            parts.append(sends[r][off:off + counts[r][o]])
            orig.append((r, off, counts[r][o]))
        out.append(torch.cat(parts).contiguous() if parts else sends[0][:0])
        origin.append(orig)
    return out, origin


def run_pass(rk, which, walk_stats=None):
    """One pass (insert or the first probe of the query) over all batches; yields (batch, survivors per rank) after each apply."""
    torch, W = rk.torch, rk.W
    geoms = [c.shard_plan(which) for c in rk.ctxs]
    assert all(g == geoms[0] for g in geoms)
    geom = rk.geom = geoms[0]
    rk.per = geom["tiles_per_rank"]
    if which == INSERT:
        for c in rk.ctxs:
            c.filter_reset()
    for b in range(geom["batches"]):
        sends_r = [torch.zeros(W * geom["region_block_bytes"], dtype=torch.uint8, device="cuda") for _ in range(W)]
        sends_c = [torch.zeros(W * geom["count_block_bytes"], dtype=torch.uint8, device="cuda") for _ in range(W)]
        n_ovf = [rk.ctxs[r].shard_hash(which, b, sends_r[r].data_ptr(), sends_c[r].data_ptr()) for r in range(W)]
        assert max(n_ovf) < (1 << 62)
        recv_r, recv_c = exchange_equal(torch, sends_r, W), exchange_equal(torch, sends_c, W)
        if max(n_ovf) > 0:  # the overflow lists of all ranks, concatenated, on every rank (AddressSharded._exchange)
            eb = geom["overflow_entry_bytes"]
            lists = []
            for r in range(W):
                mine = torch.zeros(max(n_ovf[r] * eb, 8), dtype=torch.uint8, device="cuda")
                rk.ctxs[r].shard_overflow_get(which, mine.data_ptr(), n_ovf[r])
                lists.append(mine[:n_ovf[r] * eb])
            cat = torch.cat(lists).contiguous()
            for c in rk.ctxs:
                c.shard_overflow_set(which, cat.data_ptr(), cat.numel() // eb)
        yield b, [rk.ctxs[r].shard_apply(which, b, recv_r[r].data_ptr(), recv_c[r].data_ptr()) for r in range(W)]


def oracle_bits(case, A):
    A = np.asarray(A, dtype=np.uint64)
    return ((case["filter"][(A >> np.uint64(5)).astype(np.int64)] >> (A & np.uint64(31)).astype(np.uint32)) & np.uint32(1)).astype(np.uint8)


def walk_addresses(rk, case, sid, r, b):
    """Reference addresses [n, q] of survivor ids that are home on rank r in batch b; equal (k+1)-mers are hashed once for all walks."""
    src, rel, e = R.sid_parts(sid, rk.W)
    assert (src == r).all()
    g = (R.chunk_base(rk.n_tiles, r, rk.W, rk.per, b) + rel).astype(np.int64)
    out = np.zeros((sid.size, rk.q), dtype=np.uint64)
    for i, (gg, ee) in enumerate(zip(g.tolist(), e.tolist())):
        key = (rk.codes[gg:gg + rk.k].tobytes(), ee)
        a = case["hashes"].get(key)
        if a is None:
            a = case["hashes"][key] = np.array(R.edge_hashes(rk.codes, gg, ee, rk.k, rk.L, rk.table), dtype=np.uint64)
        out[i] = a
    return out


@pytest.mark.parametrize("W", [1, 2, 4])
def test_protocol_walk(capi, torch, walk_case, W):
    """Insert, first probe, survivors home, and the verification by hand in both pinned round shapes (what TPC_VERIFY_ROUNDS = eager /
    lazy make of dist.py's _verify): every probe answer is the oracle filter's bit at the reference's address, every round keeps exactly
    the ids whose probes all hit, the ranks' masks together are the oracle's round mask.  One rank goes through tpc_shard_verify_send
    and the calls without a send order (TPC_VERIFY_ROUTED), eager: the 32-bit compare of four answers."""
    case, q = walk_case, WALK_Q
    rk = Ranks(capi, torch, case["recs"], WALK_K, WALK_L, q, W, {"slice_bits": WALK_SB})
    try:
        assert (rk.table == case["table"]).all() and rk.n_tiles == 3  # on four ranks: 1, 1, 1 (partly text) and 0 tiles
        for _ in run_pass(rk, INSERT):
            pass
        for shape in ([(1, q - 1)], [(1, 1), (2, q - 2)]):
            total_marked, seen_survivors = 0, 0
            for b, n_surv in run_pass(rk, QUERY):
                # survivors: as they lie, and grouped by the rank that hashed them
                homes, counts = [], []
                for r in range(W):
                    n = n_surv[r]
                    plain = torch.full((n + 3,), SENT64, dtype=torch.int64, device="cuda")
                    rk.ctxs[r].shard_survivors(plain.data_ptr())
                    home = torch.full((n + 3,), SENT64, dtype=torch.int64, device="cuda")
                    tmp = torch.zeros(max(n, 1), dtype=torch.int64, device="cuda")
                    cnt = rk.ctxs[r].shard_survivors_home(tmp.data_ptr(), home.data_ptr(), W)
                    a, h = plain.cpu().numpy(), home.cpu().numpy()
                    assert (a[n:] == SENT64).all() and (h[n:] == SENT64).all()
                    a, h = a[:n].view(np.uint64), h[:n].view(np.uint64)
                    assert (np.sort(a) == np.sort(h)).all()
                    src = R.sid_parts(h, W)[0].astype(np.int64)
                    assert cnt == np.bincount(src, minlength=W).tolist() and (np.diff(src) >= 0).all(), (r, cnt)
                    homes.append(home[:n])
                    counts.append(cnt)
                    seen_survivors += n
                sids, _ = exchange_var(torch, homes, counts, W)
                for ri, (fn, cnt) in enumerate(shape):
                    last = ri + 1 == len(shape)
                    sends, perms, scounts, G = [], [], [], []
                    for r in range(W):
                        n = sids[r].numel()
                        sid = u64(sids[r])
                        A = walk_addresses(rk, case, sid, r, b)[:, fn:fn + cnt]
                        owner, local = R.owner_local(A, rk.geom, W)
                        sd = sids[r] if n else torch.zeros(1, dtype=torch.int64, device="cuda")
                        if n == 0:
                            cts, p, s = [0] * W, np.zeros(0, dtype=np.int64), torch.zeros(0, dtype=torch.int64, device="cuda")
                            assert rk.ctxs[r].shard_verify_send(fn, cnt, sd.data_ptr(), 0, 0, 0, 0, W) == cts
                        else:
                            send = torch.full((n * cnt,), SENT64, dtype=torch.int64, device="cuda")
                            perm = torch.full((n * cnt,), -1, dtype=torch.int32, device="cuda")
                            tmp = torch.zeros(n * cnt, dtype=torch.int64, device="cuda")
                            cts = rk.ctxs[r].shard_verify_send(fn, cnt, sd.data_ptr(), n, tmp.data_ptr() if W > 1 else 0, send.data_ptr(),
                                                               perm.data_ptr() if W > 1 else 0, W)
                            s = send
                            p = u32(perm).astype(np.int64) if W > 1 else np.arange(n * cnt)
                            assert R.route_violations(p, owner.reshape(-1), cts, W) == []
                            assert (u64(send)[p] == local.reshape(-1)).all()
                        slot_addr = np.zeros(n * cnt, dtype=np.uint64)  # the global address asked in every slot of the send buffer
                        slot_addr[p] = A.reshape(-1)
                        sends.append(s); perms.append(p); scounts.append(cts); G.append(slot_addr)
                    reqs, origin = exchange_var(torch, sends, scounts, W)
                    hits = []
                    for o in range(W):
                        m = reqs[o].numel()
                        hit = torch.full((m + 4,), 9, dtype=torch.uint8, device="cuda")
                        rk.ctxs[o].shard_probe((reqs[o] if m else torch.zeros(1, dtype=torch.int64, device="cuda")).data_ptr(), m, hit.data_ptr())
                        got = hit.cpu().numpy()
                        want = np.concatenate([oracle_bits(case, G[r][off:off + c]) for r, off, c in origin[o]]) if m else np.zeros(0, dtype=np.uint8)
                        assert (got[m:] == 9).all() and (got[:m] == want).all(), (o, fn, cnt)
                        hits.append(hit[:m])
                    # the answers go back the way the questions came: rank r's answers in the order of its send buffer
                    back, _ = exchange_var(torch, hits, [[scounts[r][o] for r in range(W)] for o in range(W)], W)
                    nxt = []
                    for r in range(W):
                        n = sids[r].numel()
                        sid = u64(sids[r])
                        keep = R.all_hit(back[r].cpu().numpy(), n, cnt, perms[r] if W > 1 else None)
                        assert (keep == (oracle_bits(case, walk_addresses(rk, case, sid, r, b)[:, fn:fn + cnt]) == 1).all(axis=1)).all()
                        sd = sids[r] if n else torch.zeros(1, dtype=torch.int64, device="cuda")
                        bk = torch.zeros(max(4, back[r].numel()), dtype=torch.uint8, device="cuda")
                        bk[:back[r].numel()] = back[r]
                        perm_dev = to_dev(torch, perms[r].astype(np.uint32)) if W > 1 and n else None
                        perm_ptr = perm_dev.data_ptr() if perm_dev is not None else 0
                        if last:
                            rel = R.sid_parts(sid, W)[1]
                            before = rk.mask(r)
                            marked = rk.ctxs[r].shard_finish(sd.data_ptr(), n, cnt, bk.data_ptr(), perm_ptr)
                            assert marked == int(keep.sum())
                            base = R.chunk_base(rk.n_tiles, r, W, rk.per, b)
                            assert (rk.mask(r) == R.mask_with_bits(before, base + rel[keep].astype(np.int64))).all()
                            total_marked += marked
                        else:
                            out = torch.full((n + 3,), SENT64, dtype=torch.int64, device="cuda")
                            m = rk.ctxs[r].shard_select(sd.data_ptr(), n, cnt, bk.data_ptr(), perm_ptr, out.data_ptr())
                            got = out.cpu().numpy()
                            assert m == int(keep.sum()) and (got[m:] == SENT64).all()
                            assert (np.sort(got[:m].view(np.uint64)) == np.sort(sid[keep])).all()
                            nxt.append(out[:m])
                    sids = nxt
            union = np.bitwise_or.reduce(np.stack([rk.mask(r) for r in range(W)]), axis=0)
            assert (union == case["round_mask"]).all(), shape
            assert seen_survivors > 1000 and 0 < total_marked < seen_survivors  # both false positives and true second edges were seen
            if W == 1:
                walked = union
        if W == 1:  # the same mask from the one-rank shortcut on a second context
            rk2 = Ranks(capi, torch, case["recs"], WALK_K, WALK_L, q, 1, {"slice_bits": WALK_SB})
            try:
                for _ in run_pass(rk2, INSERT):
                    pass
                for _ in run_pass(rk2, QUERY):
                    rk2.ctxs[0].shard_verify_local()
                assert (rk2.mask(0) == walked).all()
            finally:
                rk2.close()
    finally:
        rk.close()
