"""The wire format of the combined exchange's set-bit lists (csrc/tpc_lists.h, the header comment of tpc_combine_* in
include/twopaco_hip.h) stated plainly in numpy, for the tests of the list reader and the merge.

A filter slice of 2^slice_bits bits is cut into windows of 2^16 bits (one window of 2^slice_bits bits below that).  The set bits of a
window travel as 16-bit offsets, in no particular order, every list starting on a 16-byte unit of 8 entries.  A BLOCK is the lists of
one source; its directory holds, per (slice key, window), `unit << 24 | n`: the list's first unit inside the block and its length.
Block s starts at unit src_base[s] of the payload buffer and its directory at entry s * dir_stride.  Which sources list a permuted
slice sp = (b1 << b2_bits) | b2, and under which key, is said by n_owner:
    n_owner = W > 0   the sources (b1 mod W) + i W, i < n_src / W, under key [b1 / W][b2]  (the blocks of tpc_combine_export and the
                      merged blocks of tpc_combine_merge)
    n_owner = 0       every source, under the slice's index in the consumer's grid: sp itself for tpc_combine_import, and for the
                      merge on rank r of a world W -- whose grid is the slices of the buckets b1 mod W = r -- again [b1 / W][b2]
Permuted slice sp is filter slice (sp * PERM_INV) mod 2^F (csrc/tpc_bins.h:pt_make_perm).

A cell is one list: the mapping (source, permuted slice, window) -> array of offsets."""
from dataclasses import dataclass

import numpy as np

PERM_MULT = 0x9E3779B1
PERM_INV = pow(PERM_MULT, -1, 1 << 32)
WINDOW_BITS = 16
UNIT = 8           # entries of a 16-byte unit
SENTINEL = 0xFFFF  # every payload entry that is no list's: bit 65535 of a window, which a reader running past n would set


def geometry(L, slice_bits, b1=None, b2=None):
    """Two bucket levels over the F = L - slice_bits slice bits, as the planner splits them (or as tpc_combine_info reported them)."""
    F = L - slice_bits
    if b1 is None:
        b1, b2 = (F + 1) // 2, F // 2
    assert b1 + b2 == F
    return {"L": L, "slice_bits": slice_bits, "b1": b1, "b2": b2, "slices": 1 << F, "windows": 1 << max(0, slice_bits - WINDOW_BITS)}


def geometry_of(info, L):
    g = geometry(L, info["slice_bits"], info["b1"], info["b2"])
    assert g["slices"] == info["slices"] and g["windows"] == info["windows"], (g, info)
    return g


def window_size(geom):
    return 1 << min(geom["slice_bits"], WINDOW_BITS)


@dataclass
class Layout:
    """The keying of the blocks (n_src, n_owner; rank and world of a merge) and what a correct reader must not depend on."""
    n_src: int
    n_owner: int
    rank: int = 0
    world: int = 1
    shuffle_lists: bool = False    # lists placed in shuffled order inside a block
    gaps: bool = False             # unused units between lists
    shuffle_blocks: bool = False   # blocks in any order inside the payload buffer
    unaligned: bool = False        # blocks at odd unit offsets, unused units between them
    shuffle_entries: bool = False  # entries inside a list in any order
    seed: int = 0

    def divisor(self):
        return self.n_owner if self.n_owner else self.world

    def dir_stride(self, geom):
        return geom["slices"] // self.divisor() * geom["windows"]

    def key_of(self, geom, sp):
        sp = np.asarray(sp, dtype=np.int64)
        W = self.divisor()
        if W == 1:
            return sp
        b1, b2 = sp >> geom["b2"], sp & ((1 << geom["b2"]) - 1)
        return ((b1 // W) << geom["b2"]) | b2

    def lists_slice(self, geom, source, sp):
        """Does block `source` have directory entries for permuted slice sp?"""
        b1 = np.asarray(sp, dtype=np.int64) >> geom["b2"]
        if self.n_owner:
            return b1 % self.n_owner == source % self.n_owner
        return b1 % self.world == self.rank

    def sources_of(self, geom, sp):
        """The sources a reader visits for permuted slice sp, in its order."""
        if self.n_owner:
            return list(range((sp >> geom["b2"]) % self.n_owner, self.n_src, self.n_owner))
        return list(range(self.n_src))

    def block_slices(self, geom, source):
        """Permuted slice behind every key of block `source`."""
        key = np.arange(self.dir_stride(geom) // geom["windows"], dtype=np.int64)
        W = self.divisor()
        if W == 1:
            return key
        d = source % self.n_owner if self.n_owner else self.rank
        return ((((key >> geom["b2"]) * W) + d) << geom["b2"]) | (key & ((1 << geom["b2"]) - 1))


def encode_blocks(cells, geometry, layout):
    """payload (uint16), dirs (uint64, n_src * dir_stride), src_base (unit of every block), units (used units of every block) of the
    cells, laid out as `layout` says.  Everything in the payload that is not one of a list's n entries is SENTINEL."""
    geom, lay = geometry, layout
    rng = np.random.default_rng(lay.seed)
    n_win, stride, wsize = geom["windows"], lay.dir_stride(geom), window_size(geom)
    per_src = [[] for _ in range(lay.n_src)]
    for (s, sp, w), offs in cells.items():
        offs = np.asarray(offs, dtype=np.int64)
        if offs.size == 0:
            continue
        assert 0 <= s < lay.n_src and 0 <= w < n_win and 0 <= sp < geom["slices"]
        assert lay.lists_slice(geom, s, sp), "source %d does not list permuted slice %d" % (s, sp)
        assert offs.min() >= 0 and offs.max() < wsize and np.unique(offs).size == offs.size
        per_src[s].append((int(lay.key_of(geom, sp)) * n_win + w, offs))
    dirs = np.zeros(lay.n_src * stride, dtype=np.uint64)
    blocks, units = [], []
    for s in range(lay.n_src):
        lists = per_src[s]
        idx = np.array([i for i, _ in lists], dtype=np.int64)
        assert np.unique(idx).size == idx.size
        n = np.array([o.size for _, o in lists], dtype=np.int64)
        order = rng.permutation(len(lists)) if lay.shuffle_lists else np.argsort(idx, kind="stable")
        gap = rng.integers(0, 3, len(lists)) if lay.gaps else np.zeros(len(lists), dtype=np.int64)
        ulen = (n + UNIT - 1) // UNIT
        first = np.zeros(len(lists), dtype=np.int64)
        first[order] = np.cumsum(gap + ulen[order]) - ulen[order]
        used = int((gap + ulen).sum()) + (int(rng.integers(0, 3)) if lay.gaps and len(lists) else 0)
        assert used < (1 << 24) and n.max(initial=0) < (1 << 24)
        block = np.full(used * UNIT, SENTINEL, dtype=np.uint16)
        if len(lists):
            data = np.concatenate([o for _, o in lists])
            start = np.cumsum(n) - n
            within = np.arange(data.size) - np.repeat(start, n)
            if lay.shuffle_entries:  # (descending from a random entry of the list, around its end: cheap, and no order a reader may lean on)
                within = (np.repeat(rng.integers(0, 1 << 30, len(lists)), n) - within) % np.repeat(n, n)
            block[np.repeat(first * UNIT, n) + within] = data
            dirs[s * stride + idx] = (first.astype(np.uint64) << np.uint64(24)) | n.astype(np.uint64)
        blocks.append(block)
        units.append(used)
    src_base, at, parts = [0] * lay.n_src, 0, []
    for s in (rng.permutation(lay.n_src) if lay.shuffle_blocks else range(lay.n_src)):
        pad = 1 + 2 * int(rng.integers(0, 3)) if lay.unaligned else 0
        parts.append(np.full(pad * UNIT, SENTINEL, dtype=np.uint16))
        src_base[s] = at + pad
        parts.append(blocks[s])
        at += pad + units[s]
    if lay.unaligned:
        parts.append(np.full(3 * UNIT, SENTINEL, dtype=np.uint16))
    payload = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint16)
    return {"payload": payload, "dirs": dirs, "src_base": src_base, "units": units, "dir_stride": stride}


def decode_block(payload, dirs, base, used, geometry, slices):
    """(permuted slice, window, offset) of every entry of ONE block -- its directory `dirs`, its first unit `base` in `payload`, its
    used units, the permuted slice behind every key -- after the layout checks of decode_export: lists inside the used prefix, no
    two lists sharing a unit, offsets inside their window."""
    n_win, wsize = geometry["windows"], window_size(geometry)
    dirs = np.asarray(dirs, dtype=np.uint64)
    assert dirs.size == len(slices) * n_win
    idx = np.arange(dirs.size, dtype=np.int64)
    n = (dirs & np.uint64(0xFFFFFF)).astype(np.int64)
    first = (dirs >> np.uint64(24)).astype(np.int64)
    assert n.max(initial=0) <= wsize
    live = n > 0
    idx, n, first = idx[live], n[live], first[live]
    ulen = (n + UNIT - 1) // UNIT
    assert (first + ulen <= used).all(), "a list beyond its block's used units"
    order = np.argsort(first, kind="stable")
    assert (first[order][1:] >= (first + ulen)[order][:-1]).all(), "two lists share a unit"
    total = int(n.sum())
    at = np.repeat((base + first) * UNIT - (np.cumsum(n) - n), n) + np.arange(total, dtype=np.int64)
    vals = np.asarray(payload)[at].astype(np.int64)
    assert (vals < wsize).all(), "an offset outside its window"
    return np.repeat(np.asarray(slices, dtype=np.int64)[idx // n_win], n), np.repeat(idx % n_win, n), vals


def cells_of(source, sp, win, vals):
    """The decoded entries of a block as cells, every list sorted."""
    out = {}
    order = np.lexsort((vals, win, sp))
    sp, win, vals = sp[order], win[order], vals[order]
    cut = np.flatnonzero((np.diff(sp) != 0) | (np.diff(win) != 0)) + 1
    for lo, hi in zip(np.concatenate([[0], cut]), np.concatenate([cut, [sp.size]])):
        if hi > lo:
            out[(source, int(sp[lo]), int(win[lo]))] = vals[lo:hi]
    return out


def addresses(geometry, sp, win, vals):
    """Filter addresses of entries: the slice permutation undone."""
    sb, F = geometry["slice_bits"], geometry["L"] - geometry["slice_bits"]
    phys = (np.asarray(sp).astype(np.uint64) * np.uint64(PERM_INV)) & np.uint64((1 << F) - 1)
    return (phys << np.uint64(sb)) | (np.asarray(win, dtype=np.int64) * (1 << WINDOW_BITS) + np.asarray(vals, dtype=np.int64)).astype(np.uint64)


def words_of(addr, L):
    """Filter words (2^L / 32 and the spare one) with exactly the bits `addr` set."""
    out = np.zeros(max(1, (1 << L) >> 5) + 1, dtype=np.uint32)
    addr = np.unique(np.asarray(addr, dtype=np.uint64))
    if addr.size:
        word = (addr >> np.uint64(5)).astype(np.int64)
        bit = np.left_shift(np.uint32(1), (addr & np.uint64(31)).astype(np.uint32))
        starts = np.concatenate([[0], np.flatnonzero(np.diff(word)) + 1])
        out[word[starts]] = np.add.reduceat(bit, starts)  # (distinct powers of two of one word: the sum is the OR)
    return out


def union_filter(cells, geometry, L, before=None):
    """The dense filter words a consumer of the cells must produce: their OR, over `before` when given."""
    assert L == geometry["L"]
    parts = [addresses(geometry, np.full(len(o), sp), np.full(len(o), w), o) for (_, sp, w), o in cells.items() if len(o)]
    out = words_of(np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64), L)
    return out if before is None else out | np.asarray(before, dtype=np.uint32)


def filter_bits(filter_words, geometry):
    """(address, permuted slice, window, offset) of every set bit of the filter, by ascending address."""
    sb, L = geometry["slice_bits"], geometry["L"]
    F = L - sb
    w = np.ascontiguousarray(np.asarray(filter_words, dtype=np.uint32)[:max(1, (1 << L) >> 5)])
    addr = np.flatnonzero(np.unpackbits(w.view(np.uint8), bitorder="little")).astype(np.int64)
    sp = ((addr >> sb) * PERM_MULT) & ((1 << F) - 1)
    inside = addr & ((1 << sb) - 1)
    return addr, sp, inside >> WINDOW_BITS, inside & ((1 << WINDOW_BITS) - 1)


def split_bits(filter_words, geometry, n_src, n_owner, rng, forced=None):
    """Deals the set bits of the filter to the sources: every bit to a random non-empty subset of the sources allowed to list its
    slice (one of them, and each one again with probability 1 / max(4, sources): duplicates across sources).  forced: {(source, permuted slice,
    window): n} -- that cell is exactly the first n bits of its window.  The union of the cells is the filter."""
    lay = Layout(n_src, n_owner)
    addr, sp, win, off = filter_bits(filter_words, geometry)
    c = n_src // n_owner if n_owner else n_src  # sources per slice; local source i of slice sp is sources_of(sp)[i]
    assert 1 <= c <= 32
    mask = np.left_shift(np.uint32(1), rng.integers(0, c, addr.size, dtype=np.uint32))
    for i in range(c):
        mask |= (rng.integers(0, max(4, c), addr.size, dtype=np.uint8) == 0).astype(np.uint32) << np.uint32(i)
    by_window = {}
    for (s, fsp, fw), n in (forced or {}).items():
        srcs = lay.sources_of(geometry, fsp)
        assert s in srcs, "source %d does not list permuted slice %d" % (s, fsp)
        by_window.setdefault((fsp, fw), {})[srcs.index(s)] = n
    sb, F = geometry["slice_bits"], geometry["L"] - geometry["slice_bits"]
    for (fsp, fw), want in by_window.items():
        a0 = ((((fsp * PERM_INV) & ((1 << F) - 1)) << sb) + (fw << WINDOW_BITS))
        lo, hi = np.searchsorted(addr, a0), np.searchsorted(addr, a0 + window_size(geometry))
        count = hi - lo
        free = [i for i in range(c) if i not in want]
        assert all(n <= count for n in want.values()), "the window holds %d bits, forced %r" % (count, want)
        assert free or max(want.values()) == count, "every source of the window is forced and none holds all of its bits"
        m = mask[lo:hi]
        for i, n in want.items():
            m[:n] |= np.uint32(1 << i)
            m[n:] &= ~np.uint32(1 << i)
        rest = m == 0
        if rest.any():
            assert free
            m[rest] = np.uint32(1 << free[0])
    cells = {}
    stride = n_owner if n_owner else 1
    wid = addr >> min(sb, WINDOW_BITS)  # (ascending with the address: the bits of a window are one run)
    for i in range(c):
        sel = np.flatnonzero(mask & np.uint32(1 << i))
        cut = np.flatnonzero(np.diff(wid[sel])) + 1
        for lo, hi in zip(np.concatenate([[0], cut]).tolist(), np.concatenate([cut, [sel.size]]).tolist()):
            if hi > lo:
                csp, cw = int(sp[sel[lo]]), int(win[sel[lo]])
                cells[(((csp >> geometry["b2"]) % n_owner if n_owner else 0) + i * stride, csp, cw)] = off[sel[lo:hi]]
    return cells


# ---- the checks of tests/test_gpu_combine_lists.py on a whole export (one block per destination, every block cap units long)
def decode_export(info, n_dest, L, payload, dirs, units):
    """Filter addresses of every entry of an export, after checking the block layout: lists inside the used prefix of their block,
    no two lists sharing a unit, offsets inside their window."""
    sb, log_nb2, n_win, cap = info["slice_bits"], info["b2"], info["windows"], info["cap_units"]
    F = L - sb
    spd = info["slices"] // n_dest
    assert dirs.size == info["slices"] * n_win
    idx = np.arange(dirs.size, dtype=np.int64)
    dest = idx // (spd * n_win)
    key = (idx // n_win) % spd
    win = idx % n_win
    b1 = (key >> log_nb2) * n_dest + dest  # (the block of destination d holds the slices of the level-1 buckets b1 = d mod n_dest)
    sp = (b1 << log_nb2) | (key & ((1 << log_nb2) - 1))
    n = (dirs & 0xFFFFFF).astype(np.int64)
    base = (dirs >> 24).astype(np.int64)
    assert n.max(initial=0) <= 1 << min(sb, WINDOW_BITS)
    live = n > 0
    dest, win, sp, n, base = dest[live], win[live], sp[live], n[live], base[live]
    ulen = (n + 7) // 8
    used = np.asarray(units, dtype=np.int64)
    assert (base + ulen <= used[dest]).all(), "a list beyond its block's used units"
    order = np.lexsort((base, dest))
    d_s, b_s, e_s = dest[order], base[order], (base + ulen)[order]
    same = d_s[1:] == d_s[:-1]
    assert (b_s[1:][same] >= e_s[:-1][same]).all(), "two lists share a unit"
    total = int(n.sum())
    first = np.cumsum(n) - n
    at = np.repeat((dest * cap + base) * 8 - first, n) + np.arange(total, dtype=np.int64)
    vals = payload[at].astype(np.int64)
    assert (vals < (1 << min(sb, WINDOW_BITS))).all()
    phys = (np.repeat(sp, n).astype(np.uint64) * np.uint64(PERM_INV)) & np.uint64((1 << F) - 1)
    return (phys << np.uint64(sb)) | (np.repeat(win, n) * (1 << WINDOW_BITS) + vals).astype(np.uint64)


def assert_bits_are_filter(addr, filt):
    """The addresses, one per entry, are exactly the set bits of filt: per word, as many entries as set bits and their powers of two
    summing to the word -- which also rules out any address listed twice (a sum of c powers of two has c bits only when they differ)."""
    words = (addr >> np.uint64(5)).astype(np.int64)
    bits = np.left_shift(np.uint64(1), addr & np.uint64(31)).astype(np.float64)
    assert words.max(initial=0) < filt.size
    cnt = np.bincount(words, minlength=filt.size)
    sums = np.bincount(words, weights=bits, minlength=filt.size)
    assert (cnt == np.bitwise_count(filt)).all(), "entries per filter word differ from its set bits"
    assert (sums.astype(np.uint64) == filt.astype(np.uint64)).all(), "the lists are not the oracle's filter"
