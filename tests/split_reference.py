"""The split pass (rounds > 1) by its definition, without a device: what tpc_pass1_split_hist must return for a text, and what it may.

The pass (csrc/tpc_pass1.hip: k_split_emask, k_split<Q>; csrc/tpc_pass1_anyq.hip: k_split_anyq; csrc/tpc_capi.hip:
tpc_pass1_split_hist) takes every (k+1)-mer of 'N' + record + 'N' of the records with at least k letters, canonical edge by canonical
edge, and bumps for each DISTINCT edge the bins of its two endpoint vertex hashes.  "Distinct" is decided by a ballot over the edge's
q Bloom addresses in a scratch filter: in phase i (one launch each) every occurrence that has not won yet does one atomic OR on
address i of its edge; the occurrence that flips the bit wins, is counted, sets the edge's other q - 1 bits and leaves.

Everything here is built from oracle.Oracle.hash_dump(g, c), which gives the q canonical edge addresses and the vertex hashes of a
position, and from the record layout of PackedText: position 0 is a separator, record 0 starts at 1, one separator follows every
record.  An "edge" below is one distinct tuple of q addresses (for k + 1 <= L that is one canonical (k+1)-mer up to a hash
coincidence in all q functions at once; for k + 1 > L different (k+1)-mers can share the tuple, see same_edge_everywhere).

What holds under every schedule of the device, and why:

  1. An edge wins at most once.  All its occurrences share their q addresses.  To win in phase i an occurrence must flip bit a_i,
     and one atomic OR at most flips a bit.  The winner sets all q bits before the next launch starts, so no later phase flips one.
  2. A must-win edge wins.  must_win(p): one of its first p addresses, a_i, is an address of no OTHER edge.  Bit a_i is then set by
     this edge's occurrences only, and only by a winner or by the phase-i OR itself.  If the edge has not won before phase i the bit
     is clear when phase i starts, so the first OR of phase i flips it.
  3. sum(bins) = 2 x winners.  A winner adds one to the bin of the vertex at g and one to the bin of the vertex at g + 1 (twice to
     one bin when they agree), nobody else adds, and no bin comes near the saturation at 2^31 - 1.
  4. After q phases the scratch filter equals union_filter exactly.  Only addresses of edges are ever set, so filter <= union.  An
     edge that never wins has seen every one of its q bits already set when it tried, and bits are never cleared; an edge that wins
     sets all q.  Either way all q bits of every edge are set.
  5. After p < q phases the filter lies between the bits of the must_win(p) edges (they won: 2) and union_filter (4, first half).
  6. Per bin, lower_hist(p) <= bins <= upper_hist: the must-win edges are counted (2), and every edge at most once (1).

When every edge is must_win(p) the bounds meet: bins == distinct_hist bin for bin, under any schedule -- the exact cases below.
"""
import numpy as np

from oracle import oracle as O

LETTERS = np.frombuffer(b"ACGTN", dtype=np.uint8)
SEED = 4711
TILE = 8192          # positions of one workgroup of k_split (csrc/tpc_device.h: TPC_TILE_POS)
BINS = 1 << 24       # VE.h:471
K_MAX = 604          # the largest k tpc_set_params accepts: (k + 4 + 31) / 32 < 20 key words


def layout(recs):
    """(rec_start, rec_len, n_text) of PackedText.from_codes(recs): T = N rec0 N rec1 N ..."""
    ln = np.array([len(r) for r in recs], dtype=np.uint64)
    start = np.ones(ln.size, dtype=np.uint64)
    if ln.size > 1:
        start[1:] += np.cumsum(ln[:-1] + np.uint64(1))
    return start, ln, int(1 + (ln + np.uint64(1)).sum())


def positions(rec_start, rec_len, k):
    """The positions the occurrence mask must hold: g in [start - 1, start + len - k] of every record with len >= k, ascending."""
    s, n = np.asarray(rec_start, dtype=np.int64), np.asarray(rec_len, dtype=np.int64)
    keep = n >= k
    s, n = s[keep], n[keep]
    if s.size == 0:
        return np.zeros(0, dtype=np.int64)
    cnt = n - k + 2
    first = np.repeat(s - 1, cnt)
    within = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return first + within


def bin_size(L):
    return max(1, (1 << L) >> 24)   # VE.h:169


def phases_of(q, n_text, L):
    """The ballot launches of tpc_pass1.hip:launch_split_q: q when q < 3 or when more than an eighth of the bits could be set."""
    assert q * n_text != (1 << L) >> 3, "a case exactly on the boundary of `crowded`: move it"
    return q if (q < 3 or q * n_text > ((1 << L) >> 3)) else 3


def kernel_of(q, force_anyq=False):
    return 4 if (q > 16 or force_anyq) else 0   # the stat "split_kernel"


class SplitReference:
    """The edges of a text and what follows from them.  recs: uint8 code arrays (A0 C1 G2 T3 N4)."""

    def __init__(self, recs, k, L, q, seed=SEED):
        self.k, self.L, self.q, self.recs = k, L, q, recs
        self.rec_start, self.rec_len, self.n_text = layout(recs)
        self.pos = positions(self.rec_start, self.rec_len, k)
        o = O.Oracle(k, L, q, O.seed_table(seed, q, L))
        for r in recs:
            o.add_record(LETTERS[np.asarray(r, dtype=np.uint8)].tobytes())
        assert (o.rec_start == self.rec_start).all() and (o.rec_len == self.rec_len).all() and len(o.text) == self.n_text
        text = o.text
        self.text = text
        n = self.pos.size
        addr = np.zeros((n, q), dtype=np.uint64)
        vh = {}   # vertex hash of position g: min(pos[0], neg[0])
        for j, g in enumerate(self.pos.tolist()):
            pn, ad = o.hash_dump(g, int(text[g + k]))
            addr[j] = ad
            vh[g] = int(pn[0].min())
        for g in (self.pos + 1).tolist():
            if g not in vh:
                vh[g] = int(o.hash_dump(g)[0][0].min())
        o.close()
        bs = bin_size(L)
        b = np.array([[vh[g] // bs, vh[g + 1] // bs] for g in self.pos.tolist()], dtype=np.int64).reshape(n, 2)
        self.pos_addr, self.pos_bins = addr, b
        if n:
            self.edge_addr, first, self.edge_of_pos = np.unique(addr, axis=0, return_index=True, return_inverse=True)
            self.edge_of_pos = self.edge_of_pos.reshape(-1)
            self.edge_bins = b[first]
        else:
            self.edge_addr, self.edge_of_pos, self.edge_bins = np.zeros((0, q), dtype=np.uint64), np.zeros(0, dtype=np.int64), np.zeros((0, 2), dtype=np.int64)
        self.n_edges = self.edge_addr.shape[0]
        # held[e, i]: address i of edge e is also an address (any of the q) of another edge
        if self.n_edges:
            flat = self.edge_addr.reshape(-1)
            owner = np.repeat(np.arange(self.n_edges), q)
            pairs = np.unique(np.stack([flat, owner.astype(np.uint64)], axis=1), axis=0)   # an edge may hold one address twice
            vals, counts = np.unique(pairs[:, 0], return_counts=True)
            self.held = (counts[np.searchsorted(vals, flat)] > 1).reshape(self.n_edges, q)
        else:
            self.held = np.zeros((0, q), dtype=bool)

    # ---- the conditions the tests put on their inputs
    def same_edge_everywhere(self):
        """True when all positions of one address tuple hold the same canonical (k+1)-mer (compared as letters): no two different
        edges share all q addresses, which k + 1 > L allows (cyclichash.h:29-35: letters L apart are rotated alike)."""
        k, t = self.k, self.text
        comp = np.array([3, 2, 1, 0, 4], dtype=np.uint8)
        seen = {}
        for g, e in zip(self.pos.tolist(), self.edge_of_pos.tolist()):
            w = t[g:g + k + 1]
            f, r = w.tobytes(), comp[w[::-1]].tobytes()
            key = min(f, r)
            if seen.setdefault(e, key) != key:
                return False
        return True

    def bins_agree(self):
        """All positions of one edge name the same two bins (in either order: the other strand walks the edge backwards)."""
        a, e = np.sort(self.pos_bins, axis=1), np.sort(self.edge_bins, axis=1)
        return bool((a == e[self.edge_of_pos]).all())

    def must_win(self, phases):
        """bool per edge: one of its first `phases` addresses is held by no other edge."""
        return ~self.held[:, :min(phases, self.q)].all(axis=1)

    # ---- what the device must or may return
    def _hist(self, sel):
        return np.bincount(self.edge_bins[sel].reshape(-1), minlength=BINS).astype(np.int64)

    def distinct_hist(self):
        return self._hist(np.ones(self.n_edges, dtype=bool))

    upper_hist = distinct_hist

    def lower_hist(self, phases):
        return self._hist(self.must_win(phases))

    def filter_words(self):
        return max(1, (1 << self.L) >> 5)

    def _filter(self, sel):
        bits = np.zeros(self.filter_words() * 32, dtype=np.uint8)
        bits[self.edge_addr[sel].reshape(-1).astype(np.int64)] = 1
        return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)

    def union_filter(self):
        return self._filter(np.ones(self.n_edges, dtype=bool))

    def lower_filter(self, phases):
        return self._filter(self.must_win(phases))

    def mask_words(self):
        """The occurrence mask as 32-bit words (bit g % 32 of word g / 32)."""
        bits = np.zeros((self.n_text + 31) // 32 * 32, dtype=np.uint8)
        bits[self.pos] = 1
        return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)


# ------------------------------------------------------------------------------------------------ generated texts
def _rand(rng, n):
    return rng.integers(0, 4, int(n)).astype(np.uint8)


def revcomp(r):
    r = np.asarray(r, dtype=np.uint8)
    return np.array([3, 2, 1, 0, 4], dtype=np.uint8)[r[::-1]]


def split_text(k, seed=0, n=10000):
    """About three tiles, after text_records() of test_gpu_hash_counts.py: two mutated copies of a random sequence (N runs in one, a
    poly-A head on the other, a (CA)n tract across the first tile border), an unrelated record, one shorter than k, one of exactly k,
    one of k + 1."""
    rng = np.random.default_rng(5000 + 7 * k + seed)
    base = _rand(rng, n)
    recs = []
    for _ in range(2):
        s = base.copy()
        hits = rng.random(s.size) < 0.02
        s[hits] = _rand(rng, hits.sum())
        recs.append(s)
    for _ in range(4):
        a = int(rng.integers(0, n - 100))
        recs[0][a:a + int(rng.integers(1, 60))] = 4
    at = min(TILE - 1 - 150, n - 400)   # record 0 starts at position 1
    recs[0][at:at + 300] = np.resize(np.array([1, 0], dtype=np.uint8), 300)
    recs[1][:300] = 0
    recs.append(_rand(rng, 2500))
    recs.append(_rand(rng, max(1, k - 1)))
    recs.append(_rand(rng, k))
    recs.append(_rand(rng, k + 1))
    return recs


def _filler(rng, gap, k):
    """Records shorter than k (never dispatched) that take exactly `gap` positions, separators included."""
    out = []
    top = max(2, min(k, 40))   # positions of the largest filler record: len <= k - 1
    assert gap == 0 or gap >= 2 and k >= 3, (gap, k)
    while gap:
        take = top if gap >= top + 2 or gap == top else (gap if gap <= top else gap - 2)
        out.append(_rand(rng, take - 1))
        gap -= take
    return out


class _Builder:
    def __init__(self, k, seed):
        self.k, self.rng, self.recs, self.at = k, np.random.default_rng(seed), [], 1   # at: where the next record starts

    def real(self, ln):
        self.recs.append(_rand(self.rng, ln))
        self.at += ln + 1
        return self

    def fill_to(self, start):
        f = _filler(self.rng, start - self.at, self.k)
        self.recs += f
        self.at = start
        return self

    def real_at(self, start, ln):
        return self.fill_to(start).real(ln)


def total_text(total, k=25, seed=1):
    """Dispatched records only, n_text == total: the text ends 1 short of, on and 1 past a tile border."""
    b = _Builder(k, 100 + seed + total)
    b.real(3000).real(k).real(2 * k + 1)
    b.real(total - b.at - 1)
    assert layout(b.recs)[2] == total
    return b.recs


def tile_edge_text(k, seed=2):
    """Four tiles and the start of a fifth.  Tile 0: a record; one whose k + 1 windows straddle the border 0 | 1; fillers (records
    shorter than k) to the end of tile 1 but for a record whose trailing separator is the last position of tile 1; tile 2: fillers
    only, no edge in any thread word (em == 0); tile 3: a record from its first position and one whose last letter is the last position
    of the tile; then a last dispatched record that ends the text."""
    b = _Builder(k, 200 + 11 * k + seed)
    b.real(k + 40)
    b.real_at(TILE - (k + 1) // 2 - 5, k + 30)
    ln = k + 7
    b.real_at(2 * TILE - 1 - ln, ln)          # start + len == 2 * TILE - 1: the separator closes the tile
    b.real_at(3 * TILE + 1, k + 50)           # its first window starts on the tile's first position
    b.real_at(4 * TILE - ln, ln)              # start + len - 1 == 4 * TILE - 1: the last letter closes the tile
    b.real(k + 2)
    return b.recs


def mask_layout_text(k, seed=3):
    """The layouts of k_split_emask, ranges [a, b] = [start - 1, start + len - k]: fillers (records shorter than k) first; nine records
    of length k .. k + 2 from position 32 on -- at k = 3 the first one's range is bit 31 of word 0 and bit 0 of word 1, and eight ranges
    meet word 1; one range that is exactly bits 0 .. 31 of a word; one that begins on bit 31; one that ends on bit 0; a record over
    several words; fillers between dispatched records; the last record is dispatched and ends the text."""
    b = _Builder(k, 300 + 13 * k + seed)
    b.fill_to(32)
    for ln in (k, k, k + 1, k, k, k + 2, k, k, k):
        b.real(ln)
    w = b.at // 32 + 2
    b.real_at(32 * w + 1, k + 30)               # a = 32 w, b = 32 w + 31
    w = b.at // 32 + 2
    b.real_at(32 * w + 32, k + 5)               # a = 32 w + 31
    w = b.at // 32 + 3
    b.real_at(32 * w - 9, k + 9)                # b = 32 w
    b.real_at(b.at + 7, k + 150)                # over several words
    b.fill_to(b.at + 45)
    b.real(k + 1)
    return b.recs


def short_only_text(k, seed=4):
    """No record of length >= k at all."""
    rng = np.random.default_rng(400 + seed)
    return [_rand(rng, 1 + (i % max(1, k - 1))) for i in range(40)]


def strand_text(both, k=25):
    """A small split_text; with `both`, followed by the reverse complement of every record."""
    recs = split_text(k, 1, n=3000)
    return recs + [revcomp(r) for r in recs] if both else recs


def recs_of_fasta(path):
    """The records of a FASTA file as code arrays, read the way the oracle reads them."""
    o = O.Oracle(5, 20, 1, O.seed_table(1, 1, 20))
    o.add_fasta(path)
    t, s, n = o.text, o.rec_start, o.rec_len
    o.close()
    return [t[int(a):int(a + b)].copy() for a, b in zip(s, n)]


def crowded_text(n, seed=5):
    """One random record, a copy of a piece of it and the reverse complement of another piece: most edges once, some thrice."""
    rng = np.random.default_rng(500 + seed)
    a = _rand(rng, n)
    return [a, a[n // 3:n // 3 + n // 8].copy(), revcomp(a[n // 2:n // 2 + n // 8])]


# ------------------------------------------------------------------------------------------------ the cases
# name -> (text function, its arguments, k, L, q, force_anyq).  The exact cases: every edge must be must_win(phases_of(...)).
def _case(fn, args, k, L, q, force=False):
    return {"fn": fn, "args": args, "k": k, "L": L, "q": q, "force_anyq": force}


EXACT = {}
for _q in list(range(1, 17)) + [17, 33, 64]:
    EXACT["q%d" % _q] = _case(split_text, (25, 0), 25, 32 if _q <= 2 else 30, _q)
EXACT["q7_anyq"] = _case(split_text, (25, 0), 25, 30, 7, True)
# k + 1 > L = 30: letters 30 apart are rotated alike, so two windows that differ by a swap of such letters share all q addresses (the two
# flanks of the tract, a mutation in each copy 30 apart).  The seeds are the first ones whose text holds no such pair
# (test_split_reference_cpu.py: same_edge_everywhere).
WIDTH_SEEDS = {3: 0, 31: 3, 33: 5, 63: 1, 65: 2, 129: 0, 603: 0, K_MAX: 0}
for _k, _seed in WIDTH_SEEDS.items():
    for _q in (5, 3):
        EXACT["k%d_q%d" % (_k, _q)] = _case(split_text, (_k, _seed), _k, 30, _q)
for _t in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
    EXACT["total%d" % _t] = _case(total_text, (_t,), 25, 30, 5)
for _k in (3, 603):
    EXACT["tile_edges_k%d" % _k] = _case(tile_edge_text, (_k,), _k, 30, 5)
EXACT["mask_k3"] = _case(mask_layout_text, (3,), 3, 30, 5)
EXACT["mask_k3_anyq"] = _case(mask_layout_text, (3,), 3, 30, 5, True)
EXACT["mask_k25"] = _case(mask_layout_text, (25,), 25, 30, 5)
EXACT["short_only"] = _case(short_only_text, (25,), 25, 30, 5)

def crowded_L(q, n_text):
    """The largest L at which launch_split_q still calls the filter crowded: q n_text > 2^L / 8."""
    L = 2
    while q * n_text > (1 << (L + 1)) >> 3:
        L += 1
    return L


# the mask layouts again under the largest filter that still takes q phases: the filter left behind is compared bit for bit
MASK_CROWDED = {}
for _name, _fn, _k in (("mask_k3", mask_layout_text, 3), ("mask_k25", mask_layout_text, 25), ("tile_edges_k3", tile_edge_text, 3)):
    MASK_CROWDED[_name] = _case(_fn, (_k,), _k, crowded_L(5, layout(_fn(_k))[2]), 5)

# crowded filter, q phases: >= 20 % of the edges with address 0 held by another edge, <= 5 % not must-win
CROWDED = {
    "q2": _case(crowded_text, (6600,), 25, 16, 2),
    "q5": _case(crowded_text, (9000,), 25, 17, 5),
    "q16": _case(crowded_text, (9000,), 25, 18, 16),
    "q17": _case(crowded_text, (9000,), 25, 18, 17),
}

# sparse filter, 3 phases, fill near 10 %: >= 1000 edges with address 0 held, >= 50 with 0 and 1 held, <= 1 % not must-win
SPARSE = {
    "q5": _case(crowded_text, (19500,), 25, 20, 5),
    "q8": _case(crowded_text, (19500,), 25, 21, 8),
    "q16": _case(crowded_text, (19500,), 25, 22, 16),
}

# one text, two filter sizes: on either side of `crowded`
BOUNDARY = {"crowded": _case(total_text, (TILE + 1,), 25, 18, 4), "sparse": _case(total_text, (TILE + 1,), 25, 19, 4)}

STRANDS = {"one": _case(strand_text, (False,), 25, 30, 5), "both": _case(strand_text, (True,), 25, 30, 5)}

HOST_QS = (1, 3, 16, 17)   # through capi.Enumerator(rounds=3): the text of EXACT["q<n>"]

_REFS = {}


def case_recs(case):
    return case["fn"](*case["args"])


def reference(case):
    """The SplitReference of a case, computed once per process."""
    key = (case["fn"].__name__, case["args"], case["k"], case["L"], case["q"], case.get("seed", SEED))
    if key not in _REFS:
        _REFS[key] = SplitReference(case_recs(case), case["k"], case["L"], case["q"], case.get("seed", SEED))
    return _REFS[key]


def case_phases(case):
    return phases_of(case["q"], layout(case_recs(case))[2], case["L"])
