"""GPU (-m gpu): the second pass at every key width, abundance cut and sharded road, against the oracle on the same text and seed.

The second-pass kernels (k_filter2 / k_filter2_rec, k_scan2_write, k_mark_records, k_table_records, k_idtab_build, k_emit, the key sort)
are templated on the key width C = (k + 35) / 32 words, 1..19 (include/twopaco_hip.h: tpc_key_words), and on COUNTED (an abundance cut
applies).  Each width runs here at its first k (32C - 35, the revcomp shift of 70 bits), at 32(C - 1) (a shift of whole words), at its
last odd k (32C - 5) and at its last k (32C - 4, the last word holding 28 letters).  Small filters (L = 8, 9) saturate the Bloom filter:
nearly every position is a mark, function 0's two strand hashes tie often enough to run the letter tie-break, and the optimistic first
exact-filter table (marks / 4 slots) overflows.  Even k adds planted palindromes.  The sharded roads (positions, records, aggregated
records) are emulated with up to three contexts on one device.  Everything is compared exactly: counters, keys, ids, de_bruijn.bin bytes."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

LETTERS = np.frombuffer(b"ACGTN", dtype=np.uint8)
SEED = 8088
SEED_K3 = 49  # (under SEED no 3-mer ties with its reverse complement at L = 8; under 49 four of the 64 do)
Q = 5
MAXU = (1 << 64) - 1
CTXS = 3  # contexts open at once in this module (the first also serves the single-GPU road)


def width_of(k):
    return (k + 35) // 32


def widths_ks(C):
    """k = 32C - 35 (3 for C = 1), 32(C - 1) (even, not for C = 1), 32C - 5 and 32C - 4."""
    return sorted({3 if C == 1 else 32 * C - 35, 32 * C - 5, 32 * C - 4} | ({32 * (C - 1)} if C > 1 else set()))


SPARSE_C = (1, 2, 3, 4, 9, 19)


def revcomp(codes):
    return (3 - codes[::-1]).astype(np.uint8)


def palindrome(rng, k):
    half = rng.integers(0, 4, k // 2).astype(np.uint8)
    return np.concatenate([half, revcomp(half)])


def planted(rng, kmer, times, flank=40):
    """`kmer` `times` times between random flanks whose letters next to it differ from one site to the next: a junction from two sites on."""
    parts = [rng.integers(0, 4, flank).astype(np.uint8)]
    for t in range(times):
        parts[-1][-1] = t % 4
        parts += [kmer, rng.integers(0, 4, flank).astype(np.uint8)]
        parts[-1][0] = (t + 1) % 4
    return np.concatenate(parts)


def width_text(k, n=9000, seed=0, m=None):
    """Codes (A0 C1 G2 T3 N4): two copies of a random sequence with substitutions every 2k letters or 1 % of them (N runs in one), so that
    the copies share k-mers at every k, an unrelated record, records of
    k - 1, k and k + 1 letters; at even k two palindromes (one planted at three sites, one at two) and one seen once; m: a random k-mer
    planted m times, one twice and one three times (junctions of known multiplicity).  Returns (records, planted k-mers)."""
    rng = np.random.default_rng(7919 * k + seed)
    base = rng.integers(0, 4, n).astype(np.uint8)
    recs = []
    for _ in range(2):
        s = base.copy()
        hits = rng.random(n) < min(0.01, 0.5 / k)
        s[hits] = (s[hits] + rng.integers(1, 4, int(hits.sum()))) % 4
        recs.append(s.astype(np.uint8))
    for _ in range(3):
        a = int(rng.integers(0, n - 100))
        recs[0][a:a + int(rng.integers(1, 40))] = 4
    recs.append(rng.integers(0, 4, 3000).astype(np.uint8))
    recs += [rng.integers(0, 4, max(1, k - 1)).astype(np.uint8), rng.integers(0, 4, k).astype(np.uint8), rng.integers(0, 4, k + 1).astype(np.uint8)]
    extra = []
    if k % 2 == 0:
        p1, p2, p3 = palindrome(rng, k), palindrome(rng, k), palindrome(rng, k)
        recs += [planted(rng, p1, 3), planted(rng, p2, 2), planted(rng, p3, 1)]
        extra += [p1, p2, p3]
    if m:
        for kmer, times in ((rng.integers(0, 4, k).astype(np.uint8), m), (rng.integers(0, 4, k).astype(np.uint8), 2),
                            (rng.integers(0, 4, k).astype(np.uint8), 3)):
            recs.append(planted(rng, kmer, times))
            extra.append(kmer)
    return recs, extra


def kmer_strings(keys, k):
    """Rows of packed keys (2 bits per letter, letter i in word i / 32) -> k-mer strings."""
    if len(keys) == 0:
        return []
    i = np.arange(k)
    codes = (keys[:, i >> 5] >> (2 * (i & 31)).astype(np.uint64)) & np.uint64(3)
    return [r.tobytes().decode() for r in LETTERS[codes.astype(np.uint8)]]


def rc_string(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def strand_hashes(text, g, k, L, h0):
    """Function 0's hash of the k-mer at each position of g and of its reverse complement (CyclicHash, the canonical-strand choice of
    candidateoccurence.h:34), in closed form: with u_j = rotl(h0[x_j], -j) and v_j = rotl(h0[3 - x_j], j),
    H(fw at g) = rotl(u_g ^ .. ^ u_(g+k-1), k - 1 + g) and H(rc at g) = rotl(v_g ^ .. ^ v_(g+k-1), -g) -- prefix XORs."""
    lm = np.uint64((1 << L) - 1)

    def rotl(x, r):
        r = (np.asarray(r, dtype=np.int64) % L).astype(np.uint64)
        return ((x << r) & lm) | (x >> (np.uint64(L) - r))

    x = np.minimum(text.astype(np.int64), 3)  # (N never sits inside a marked k-mer)
    j = np.arange(x.size, dtype=np.int64)
    h = np.asarray(h0[:4], dtype=np.uint64)
    u = rotl(h[x], -j)
    v = rotl(h[3 - x], j)
    su = np.concatenate([[np.uint64(0)], np.bitwise_xor.accumulate(u)])
    sv = np.concatenate([[np.uint64(0)], np.bitwise_xor.accumulate(v)])
    g = np.asarray(g, dtype=np.int64)
    hp = rotl(su[g + k] ^ su[g], k - 1 + g)
    hn = rotl(sv[g + k] ^ sv[g], -g)
    return hp, hn


def mask_positions(words):
    bits = np.unpackbits(np.asarray(words, dtype=np.uint32).view(np.uint8), bitorder="little")
    return np.nonzero(bits)[0].astype(np.uint64)


def first_cap(n):
    """tpc_capi_pass2.hip: the first exact-filter table has the power of two >= max(1024, marks / 4 + 2) slots."""
    cap = 1024
    while cap < n // 4 + 2:
        cap <<= 1
    return cap


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


@pytest.fixture(scope="module")
def ctxs(capi):
    cs = [capi.Context(0) for _ in range(CTXS)]
    yield cs
    for c in cs:
        c.close()


class Case:
    """One text on the first context (set_params, upload, first pass) and the oracle on the same text and seed table."""

    def __init__(self, capi, torch, ctxs, k, L, recs, abundance=MAXU, seed=SEED):
        self.capi, self.torch, self.ctxs, self.k, self.L = capi, torch, ctxs, k, L
        self.C = width_of(k)
        self.table = capi.seed_table(Q, L, seed=seed)
        self.text = capi.PackedText.from_codes(recs)
        self.o = O.Oracle(k, L, Q, O.seed_table(seed, Q, L))
        assert (self.o.table == self.table).all()
        for r in recs:
            self.o.add_record(LETTERS[r].tobytes())
        self.loaded = set()
        c0 = self.load(0)
        c0.filter_reset()
        c0.pass1_insert()
        self.n_marks = c0.pass1_query()
        self.full = torch.empty(c0.mask_words(), dtype=torch.int32, device="cuda")
        c0.mask_export(self.full.data_ptr())
        self.set_abundance(abundance)
        assert self.n_marks == self.want_stats["marks"]
        self.marks = mask_positions(self.o.round_mask)
        assert self.marks.size == self.n_marks
        self.ogtext = self.o.text

    def load(self, i):
        c = self.ctxs[i]
        if i not in self.loaded:
            c.set_params(self.k, self.L, Q, self.table)
            c.seq_upload(self.text)
            assert c.key_words() == self.C
            self.loaded.add(i)
        c.run_begin()
        if hasattr(self, "full"):  # (the aggregated road leaves a chunk of it)
            c.mask_import(self.full.data_ptr())
        return c

    def set_abundance(self, a):
        self.a = a
        self.o.enumerate(rounds=1, abundance=a)
        self.want_stats = self.o.round_stats(0)
        self.want = {"true": self.want_stats["true"], "false": self.want_stats["false"], "table": self.want_stats["table"]}

    def counted(self, n, records=False, aggregated=False):
        """Which exact-filter instantiation the call must take (tpc_capi_pass2.hip: pass2_filter_impl)."""
        return int((records and self.a < (1 << 40)) or (not aggregated and self.a < n))

    # ------------------------------------------------------------------ checks after a road
    def check_keys_and_emit(self, c, tag, stream=True):
        J = c.junctions_finalize()
        assert J == len(self.o.keys), tag
        keys = c.junction_keys()
        assert keys.shape == self.o.keys.shape and (keys == self.o.keys).all(), ("junction keys", tag)
        self.check_emit([c], tag)
        if stream:
            data, _ = c.emit_stream(self.text.rec_start, self.text.rec_length)
            want = self.oracle_bin()
            assert data == want, ("de_bruijn.bin bytes", tag, len(data), len(want))

    def check_emit(self, cs, tag):
        gs, idss = [], []
        for c in cs:
            c.emit()
            g, ids = c.emit_fetch()
            gs.append(g)
            idss.append(ids)
        g, ids = np.concatenate(gs), np.concatenate(idss)
        seq, pos, oid = self.o.records
        J = len(self.o.keys)
        real = np.abs(oid) <= J
        og = self.o.rec_start[seq[real]] + pos[real].astype(np.uint64)
        valid = ids != self.capi.INVALID_VERTEX
        assert int(valid.sum()) == int(real.sum()), ("valid ids", tag, int(valid.sum()), int(real.sum()))
        order = np.argsort(g[valid], kind="stable")
        assert (g[valid][order] == og).all() and (ids[valid][order] == oid[real]).all(), ("emit", tag)

    def oracle_bin(self):
        if not hasattr(self, "_bin") or self._bin[0] != self.a:
            import tempfile
            with tempfile.NamedTemporaryFile(suffix=".bin") as f:
                self.o.write_bin(f.name)
                self._bin = (self.a, open(f.name, "rb").read())
        return self._bin[1]

    # ------------------------------------------------------------------ roads
    def single(self, tag):
        c = self.load(0)
        st = c.pass2_filter(self.a)
        assert st == self.want, ("single", tag, st, self.want)
        assert c.stat("filter2_counted") == self.counted(self.n_marks), tag
        if st["table"] > first_cap(self.n_marks):
            assert c.stat("filter2_retries") == 1, ("no retry with more keys than the first table holds", tag, st)
        self.check_keys_and_emit(c, tag)
        return st

    def install_union(self, owners, into, tag):
        """The owners' keys, exported to device buffers, imported on `into` (dist.py's union of the junction keys)."""
        torch, C = self.torch, self.C
        bufs = []
        for c in owners:
            n = c.junction_keys_export(0, 0)
            b = torch.empty(max(n, 1) * C, dtype=torch.int64, device="cuda")
            assert c.junction_keys_export(b.data_ptr(), n) == n
            bufs.append((b, n))
        for tgt in into:
            for i, (b, n) in enumerate(bufs):
                tgt.junction_keys_import(b.data_ptr(), n, append=i > 0)

    def sum_check(self, sts, tag):
        tot = {n: sum(s[n] for s in sts) for n in ("true", "false", "table")}
        assert tot == self.want, (tag, tot, self.want, sts)

    def positions(self, W, tag):
        torch = self.torch
        c0 = self.load(0)
        n = c0.pass2_marks()
        assert n == self.n_marks
        pos = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
        owner = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
        c0.pass2_mark_owners(W, pos.data_ptr(), owner.data_ptr())
        assert (pos[:n].cpu().numpy().astype(np.uint64) == self.marks).all(), tag
        own = owner[:n].cpu().numpy()
        assert own.min() >= 0 and own.max() < W
        sts, cs = [], []
        for d in range(W):
            c = c0 if d == 0 else self.load(d)
            if d:
                c.pass2_marks()
            sel = pos[:n][owner[:n] == d].contiguous()
            sts.append(c.pass2_filter_positions(sel.data_ptr(), sel.numel(), self.a))
            assert c.stat("filter2_counted") == self.counted(sel.numel()), (tag, d)
            cs.append(c)
        self.sum_check(sts, ("positions",) + tag)
        self.install_union(cs, [c0], tag)
        self.check_keys_and_emit(c0, ("positions",) + tag)

    def records(self, W, tag, check_rows=True):
        torch, C = self.torch, self.C
        rw = C + 1
        c0 = self.load(0)
        n = c0.pass2_marks()
        rec = torch.empty(max(n, 1) * rw, dtype=torch.int64, device="cuda")
        owner = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
        c0.pass2_mark_records(W, rec.data_ptr(), owner.data_ptr())
        send, starts = self.route(c0, rec, owner, n, rw, W, check_rows)
        if check_rows:  # the canonical keys of the records: the oracle's keys are among them
            rows = rec[:n * rw].view(n, rw).cpu().numpy().view(np.uint64)
            keyset = {r.tobytes() for r in np.ascontiguousarray(rows[:, :C])}
            assert all(np.ascontiguousarray(kk).tobytes() in keyset for kk in self.o.keys), tag
        sts, cs = [], []
        for d in range(W):
            c = c0 if d == 0 else self.load(d)
            if d:
                c.pass2_marks()
            m = starts[d + 1] - starts[d]
            sts.append(c.pass2_filter_records(send.data_ptr() + 8 * rw * starts[d], m, self.a))
            assert c.stat("filter2_counted") == self.counted(m, records=True), (tag, d)
            cs.append(c)
        self.sum_check(sts, ("records",) + tag)
        self.install_union(cs, [c0], tag)
        self.check_keys_and_emit(c0, ("records",) + tag)

    def route(self, c, rec, owner, n, rw, W, check_rows=True):
        """Rows grouped by owner (a stable order) with tpc_shard_permute_rows; checked against a numpy gather."""
        torch = self.torch
        own = owner[:n].cpu().numpy()
        order = np.argsort(own, kind="stable")
        perm = np.empty(n, dtype=np.uint32)
        perm[order] = np.arange(n, dtype=np.uint32)
        dperm = torch.from_numpy(perm.view(np.int32)).to("cuda")
        send = torch.empty(max(n, 1) * rw, dtype=torch.int64, device="cuda")
        c.shard_permute_rows(rec.data_ptr(), dperm.data_ptr(), n, rw, send.data_ptr())
        if check_rows:
            src = rec[:n * rw].view(n, rw).cpu().numpy()
            assert (send[:n * rw].view(n, rw).cpu().numpy() == src[order]).all(), "permute_rows"
        starts = [0] + np.cumsum(np.bincount(own, minlength=W)).tolist()
        return send, starts

    def chunk_bounds(self, W):
        T = int(self.ogtext.size)
        return [(T * r // W, T * (r + 1) // W) for r in range(W)]

    def aggregated(self, W, tag, mixed=False):
        """Each rank keeps the marks of its own chunk of the text, aggregates them (tpc_pass2_aggregate_records) and the owners merge
        what they receive (tpc_pass2_filter_aggregated; mixed: tpc_pass2_filter_records, which takes aggregated records too)."""
        torch, C = self.torch, self.C
        rw = C + 1
        per_rank, stats, received = [], [], []
        retried = False
        for r, (lo, hi) in enumerate(self.chunk_bounds(W)):
            c = self.load(r)
            mine = torch.empty(c.mask_words(), dtype=torch.int32, device="cuda")
            c.mask_export(mine.data_ptr())  # the whole round mask: clear every bit outside [lo, hi) on the device
            sh = torch.arange(32, dtype=torch.int64, device="cuda")
            bit = torch.arange(mine.numel() * 32, dtype=torch.int64, device="cuda").view(-1, 32)
            bits = ((mine.to(torch.int64).unsqueeze(1) >> sh) & 1) * ((bit >= lo) & (bit < hi))
            w = (bits << sh).sum(1)
            mine = torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32).contiguous()
            c.mask_import(mine.data_ptr())
            n = c.pass2_marks()
            want = self.marks[(self.marks >= lo) & (self.marks < hi)]
            assert n == want.size, (tag, r, n, want.size)
            rec = torch.empty(max(n, 1) * rw, dtype=torch.int64, device="cuda")
            owner = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
            nr = c.pass2_aggregate_records(W, rec.data_ptr(), owner.data_ptr(), self.a)
            stats.append((("aggregate", r), c.stat("filter2_counted"), int(self.a < (1 << 40))))
            if nr > first_cap(n):  # more distinct keys than the first table holds
                stats.append((("aggregate retries", r, nr, n), c.stat("aggregate_retries"), 1))
                retried = True
            send, starts = self.route(c, rec, owner, nr, rw, W)
            per_rank.append((send, starts))
        sts, cs = [], []
        for d in range(W):
            c = self.ctxs[d]
            parts = [send[starts[d] * rw:starts[d + 1] * rw] for send, starts in per_rank]
            recv = torch.cat(parts).contiguous()
            m = recv.numel() // rw
            received.append(m)
            if mixed:
                sts.append(c.pass2_filter_records(recv.data_ptr(), m, self.a))
                stats.append((("filter_records", d, m), c.stat("filter2_counted"), self.counted(m, records=True)))
            else:
                sts.append(c.pass2_filter_aggregated(recv.data_ptr(), m, self.a))
                stats.append((("filter_aggregated", d, m), c.stat("filter2_counted"), self.counted(m, records=True, aggregated=True)))
            cs.append(c)
        self.sum_check(sts, ("mixed" if mixed else "aggregated",) + tag)
        self.install_union(cs, cs, tag)
        for c in cs:
            assert c.junctions_finalize() == len(self.o.keys), tag
        assert (cs[0].junction_keys() == self.o.keys).all(), tag
        self.check_emit(cs, ("aggregated emit",) + tag)  # every rank's ids of its own chunk
        for what, got, want in stats:
            assert got == want, (what, tag, got, want)
        return retried, received

    def close(self):
        self.o.close()
        self.text.close()


def tie_count(case):
    """Marked k-mers whose function-0 strand hashes tie, from the seed table in numpy (checked on a sample against the oracle)."""
    hp, hn = strand_hashes(case.ogtext, case.marks, case.k, case.L, case.table[0])
    for i in np.linspace(0, case.marks.size - 1, 6).astype(np.int64):
        pn, _ = case.o.hash_dump(int(case.marks[i]))
        assert (int(pn[0, 0]), int(pn[0, 1])) == (int(hp[i]), int(hn[i])), "strand hashes of function 0"
    return hp == hn


# ---------------------------------------------------------------------------------------------------------------- 1. the width sweep
@pytest.mark.parametrize("C", range(1, 20))
def test_every_key_width_matches_oracle(capi, torch, ctxs, C):
    """All four k of width C on a saturated filter (and on a sparse one for C in 1, 2, 3, 4, 9, 19): counters, keys, ids (junction keys,
    their reverse complements, palindromes, tie k-mers), emit and the de_bruijn.bin bytes == the oracle's."""
    for i, k in enumerate(widths_ks(C)):
        assert width_of(k) == C
        recs, extra = width_text(k)
        for L in ([8 + i % 2] + ([22] if C in SPARSE_C else [])):
            tag = (C, k, L)
            case = Case(capi, torch, ctxs, k, L, recs, seed=SEED_K3 if k == 3 else SEED)
            c0 = ctxs[0]
            st = case.single(tag)
            small = L < 12
            ties = tie_count(case)
            print("C=%d k=%d L=%d key_words=%d marks=%d keys=%d strand ties=%d filter2_retries=%d" % (
                C, k, L, c0.key_words(), case.n_marks, len(case.o.keys), int(ties.sum()), c0.stat("filter2_retries")))
            if small:
                assert int(ties.sum()) >= 24, ("strand ties", tag, int(ties.sum()))
                if k >= 27:  # the distinct keys cannot fit the first table: one retry at full size
                    assert st["table"] > first_cap(case.n_marks) and c0.stat("filter2_retries") == 1, (tag, st, case.n_marks)
            # ids: every junction key and its reverse complement, the planted palindromes, marked k-mers whose strand hashes tie
            strs = kmer_strings(case.o.keys, k)
            for s in strs:
                for t in (s, rc_string(s)):
                    assert c0.get_id(t) == case.o.get_id(t) != capi.INVALID_VERTEX, (tag, t)
            for p in extra:
                s = LETTERS[p].tobytes().decode()
                assert s == rc_string(s)
                assert c0.get_id(s) == case.o.get_id(s), (tag, "palindrome")
            tie_pos = case.marks[ties][:40].astype(np.int64)
            for g in tie_pos:
                s = LETTERS[case.ogtext[g:g + k]].tobytes().decode()
                assert c0.get_id(s) == case.o.get_id(s), (tag, "tie", int(g))
            if k % 2 == 0 and small:
                pal = set(LETTERS[p].tobytes().decode() for p in extra[:2])
                assert pal <= set(strs), (tag, "planted palindromes are junctions")
            if k % 2 == 1 and k <= 61 and small:  # the reference's own --test definition (test.cpp:71-160), seed free
                chrs = [LETTERS[r].tobytes().decode() for r in recs]
                junction, _ = O.naive_junction_marks(chrs, k)
                assert set(strs) | set(rc_string(s) for s in strs) == junction, (tag, "naive junctions")
            case.close()


def test_key_width_limits(capi, ctxs):
    """k = 604 is the last k of 19 words; k = 605 is refused with the reference's message."""
    c = ctxs[0]
    t = capi.seed_table(Q, 12, seed=SEED)
    c.set_params(604, 12, Q, t)
    assert c.key_words() == 19
    with pytest.raises(RuntimeError, match="The value of K is too big"):
        c.set_params(605, 12, Q, t)


# ---------------------------------------------------------------------------------------------------------- 2. abundance-cut edges
M = 5


@pytest.mark.parametrize("C", SPARSE_C)
def test_abundance_cut_edges(capi, torch, ctxs, C):
    """A k-mer planted M times (and others twice and three times) under every cut around M, around the number of marks (the counted
    switch of the single-context filter) and around 2^40 (that of the aggregated records): counters, keys and emit on the single
    context and on the aggregated road; which exact-filter instantiation ran is asserted each time."""
    k = 32 * C - 5
    recs, extra = width_text(k, n=4000, seed=1, m=M)
    case = Case(capi, torch, ctxs, k, 20, recs)
    strs = set(kmer_strings(case.o.keys, k))
    assert LETTERS[extra[-3]].tobytes().decode() in strs or rc_string(LETTERS[extra[-3]].tobytes().decode()) in strs
    n = case.n_marks
    cuts = [0, 1, 2, M - 1, M, M + 1, n - 1, n, (1 << 40) - 1, 1 << 40, MAXU]
    seen = set()
    for a in cuts:
        case.set_abundance(a)
        case.single((C, k, a))
        seen.add(case.ctxs[0].stat("filter2_counted"))
        case.aggregated(2, (C, k, a))
    assert seen == {0, 1}, seen
    case.close()


# --------------------------------------------------------------------------------------------------------- 3. the sharded roads
@pytest.mark.parametrize("C", range(1, 20))
def test_sharded_roads_every_width(capi, torch, ctxs, C):
    """Positions, records and aggregated records at W = 2 or 3 emulated ranks, with and without a cut: per-owner counters add up to
    the oracle's, the union of the owners' keys installed through device buffers is the oracle's key set, emit and bytes match."""
    k = 32 * C - 4 if C % 2 else 32 * C - 5
    W = 2 + C % 2
    recs, _ = width_text(k, n=5000, seed=2)
    case = Case(capi, torch, ctxs, k, 9, recs)
    retried = False
    for a in (MAXU, 2 + C % 2):
        case.set_abundance(a)
        tag = (C, k, W, a)
        case.positions(W, tag)
        case.records(W, tag)
        retried = case.aggregated(W, tag)[0] or retried
    if k >= 27:
        assert retried, "no aggregate_records retry"
    case.close()


# ------------------------------------------------------------------------------------------------------ 4. mixed records contract
@pytest.mark.parametrize("C", [1, 2, 4])
def test_filter_records_takes_aggregated_records(capi, torch, ctxs, C):
    """tpc_pass2_filter_records with aggregated records under a cut n <= a < 2^40 (n = records an owner receives): a key seen twice on one
    rank only must stay a junction, a key whose summed count exceeds a must be cut -- the oracle's result, as tpc_pass2_filter_aggregated."""
    k = 32 * C - 5
    rng = np.random.default_rng(31 + C)
    base = rng.integers(0, 4, 3000).astype(np.uint8)
    base[2200:2900] = 0  # poly-A tracts in both ranks' chunks: one key counted about 2700 times, sent by both ranks
    twin = base.copy()
    twin[1500] = (twin[1500] + 1) % 4  # both copies in the first rank's chunk: their junctions are seen twice there only
    tail = rng.integers(0, 4, 3000).astype(np.uint8)
    tail[1000:1000 + 1400] = 0
    recs = [base, twin, tail]
    case = Case(capi, torch, ctxs, k, 22, recs)
    case.set_abundance(MAXU)
    seq, pos, oid = case.o.records
    real = np.abs(oid) <= len(case.o.keys)
    g = (case.o.rec_start[seq] + pos.astype(np.uint64))[real]
    jid = np.abs(oid[real])
    (lo0, hi0), _ = case.chunk_bounds(2)
    ids, counts = np.unique(jid, return_counts=True)
    twice_one_rank = [i for i, n in zip(ids, counts) if n == 2 and (g[jid == i] < hi0).all()]
    assert twice_one_rank, "no key seen twice on one rank only"
    big = int(counts.max())
    a = big - 1
    assert a < (1 << 40) and big > 2000
    case.set_abundance(a)
    _, received = case.aggregated(2, (C, k, a), mixed=True)
    assert max(received) <= a, received  # n <= a on every owner: the records alone could not tell that a key exceeds the cut
    case.aggregated(2, (C, k, a))
    case.close()
