"""tests/lists_reference.py against itself and by hand, and the preconditions of tests/test_gpu_lists.py against the oracle: the
texts of its import cases really put the forced list lengths into the windows it forces them in.  No GPU."""

import numpy as np
import pytest

import lists_cases as C
import lists_reference as R

SWITCHES = ["shuffle_lists", "gaps", "shuffle_blocks", "unaligned", "shuffle_entries"]
LAYOUTS = [()] + [(s,) for s in SWITCHES] + [tuple(SWITCHES)]


def random_cells(geom, lay, rng, fill=0.3, most=40):
    """Cells of random lengths 0 .. most (never offset 65535), in about `fill` of the (source, slice, window) places the layout allows."""
    cells, wsize = {}, R.window_size(geom)
    for s in range(lay.n_src):
        for sp in range(geom["slices"]):
            if not lay.lists_slice(geom, s, sp):
                continue
            for w in range(geom["windows"]):
                if rng.random() < fill:
                    cells[(s, sp, w)] = np.sort(rng.choice(min(wsize, 65535), int(rng.integers(0, min(most, wsize) + 1)), replace=False))
    return cells


def decode_all(enc, geom, lay):
    out = {}
    for s in range(lay.n_src):
        d = enc["dirs"][s * enc["dir_stride"]:(s + 1) * enc["dir_stride"]]
        out.update(R.cells_of(s, *R.decode_block(enc["payload"], d, enc["src_base"][s], enc["units"][s], geom, lay.block_slices(geom, s))))
    return out


def same_cells(a, b):
    a = {k: v for k, v in a.items() if len(v)}
    return a.keys() == b.keys() and all((np.sort(a[k]) == b[k]).all() for k in a)


@pytest.mark.parametrize("switches", LAYOUTS, ids=lambda s: "+".join(s) or "plain")
@pytest.mark.parametrize("keying", [(1, 0, 0, 1), (5, 0, 0, 1), (3, 1, 0, 1), (8, 4, 0, 1), (6, 2, 0, 1), (4, 0, 1, 4), (2, 0, 1, 2)], ids=str)
@pytest.mark.parametrize("L,slice_bits", [(14, 8), (20, 16), (22, 18)])
def test_decode_inverts_encode(L, slice_bits, keying, switches):
    n_src, n_owner, rank, world = keying
    geom = R.geometry(L, slice_bits)
    lay = R.Layout(n_src, n_owner, rank=rank, world=world, seed=L + n_src, **{s: True for s in switches})
    rng = np.random.default_rng(n_src * 100 + L)
    cells = random_cells(geom, lay, rng)
    enc = R.encode_blocks(cells, geom, lay)
    assert same_cells(cells, decode_all(enc, geom, lay))
    # whatever is not a list's entry is the sentinel: as many other values as entries
    assert int((enc["payload"] != R.SENTINEL).sum()) == sum(len(v) for v in cells.values())
    if "shuffle_entries" not in switches and "shuffle_lists" not in switches and "gaps" not in switches:
        assert enc["units"] == [sum((len(v) + 7) // 8 for (s, _, _), v in cells.items() if s == src) for src in range(n_src)]


def test_a_block_by_hand():
    """One source, four slices of one window (L = 18, slice_bits = 16), three lists back to back:
         slice 0: offsets 3, 65534      -> unit 0, entries 0 .. 1, directory entry 0 = 0 << 24 | 2
         slice 1: nothing               -> directory entry 1 = 0
         slice 2: offsets 10 .. 18      -> units 1 and 2 (nine entries), entries 8 .. 16, directory entry 2 = 1 << 24 | 9
         slice 3: offset 100            -> unit 3, entry 24, directory entry 3 = 3 << 24 | 1
       four units = 32 entries, every other one 0xFFFF."""
    geom = R.geometry(18, 16)
    assert (geom["b1"], geom["b2"], geom["slices"], geom["windows"]) == (1, 1, 4, 1)
    cells = {(0, 0, 0): [3, 65534], (0, 2, 0): list(range(10, 19)), (0, 3, 0): [100]}
    enc = R.encode_blocks(cells, geom, R.Layout(1, 1))
    want = np.full(32, 0xFFFF, dtype=np.uint16)
    want[0:2] = [3, 65534]
    want[8:17] = np.arange(10, 19)
    want[24] = 100
    assert (enc["payload"] == want).all()
    assert enc["dirs"].tolist() == [2, 0, (1 << 24) | 9, (3 << 24) | 1]
    assert enc["src_base"] == [0] and enc["units"] == [4] and enc["dir_stride"] == 4
    # F = 2: the permutation's multiplier 0x9E3779B1 is 1 mod 4, so permuted slice s is filter slice s; slice 2's bit 10 is filter bit
    # 2 * 65536 + 10 = word 4096, bit 10
    f = R.union_filter(cells, geom, 18)
    assert f.size == (1 << 13) + 1 and f[4096] == sum(1 << b for b in range(10, 19)) and f[0] == 1 << 3 and f[2047] == 1 << 30
    assert f[3 * 2048 + 3] == 1 << 4 and int(np.bitwise_count(f).sum()) == 12


def test_the_keys_by_hand():
    """L = 20, slice_bits = 16: sixteen slices, b1 and b2 of two bits.  Permuted slice 13 is b1 = 3, b2 = 1.
       n_owner = 2 of 4 sources: listed by sources 1 and 3 (3 mod 2 = 1) under key [3 / 2][1] = 1 << 2 | 1 = 5 of a directory of
       16 / 2 = 8 entries: entries 1 * 8 + 5 = 13 and 3 * 8 + 5 = 29.
       n_owner = 0 of 4 sources: every source, key 13 of 16 entries: source 2's entry is 2 * 16 + 13 = 45.
       the merge on rank 1 of a world of 2: key 5 of 8 again, for every source: source 0's entry is 5."""
    geom = R.geometry(20, 16)
    owner = R.Layout(4, 2)
    assert owner.sources_of(geom, 13) == [1, 3]
    enc = R.encode_blocks({(1, 13, 0): [7], (3, 13, 0): [8, 9]}, geom, owner)
    assert enc["dir_stride"] == 8 and np.flatnonzero(enc["dirs"]).tolist() == [13, 29]
    assert enc["dirs"][13] == 1 and enc["dirs"][29] == 2 and enc["src_base"] == [0, 0, 1, 1] and enc["units"] == [0, 1, 0, 1]
    with pytest.raises(AssertionError):
        R.encode_blocks({(0, 13, 0): [7]}, geom, owner)
    enc = R.encode_blocks({(2, 13, 0): [7]}, geom, R.Layout(4, 0))
    assert enc["dir_stride"] == 16 and np.flatnonzero(enc["dirs"]).tolist() == [45]
    enc = R.encode_blocks({(0, 13, 0): [7]}, geom, R.Layout(2, 0, rank=1, world=2))
    assert enc["dir_stride"] == 8 and np.flatnonzero(enc["dirs"]).tolist() == [5]
    assert R.Layout(2, 0, rank=1, world=2).block_slices(geom, 0).tolist() == [4, 5, 6, 7, 12, 13, 14, 15]
    with pytest.raises(AssertionError):
        R.encode_blocks({(0, 9, 0): [7]}, geom, R.Layout(2, 0, rank=1, world=2))  # b1 = 2 is rank 0's


def test_decode_block_rejects_a_broken_layout():
    geom = R.geometry(18, 16)
    payload = np.arange(64, dtype=np.uint16)
    slices = np.arange(4)
    ok = np.array([(0 << 24) | 9, (2 << 24) | 1, 0, (3 << 24) | 8], dtype=np.uint64)
    sp, win, vals = R.decode_block(payload, ok, 2, 4, geom, slices)
    assert sp.tolist() == [0] * 9 + [1] + [3] * 8 and vals.tolist() == list(range(16, 25)) + [32] + list(range(40, 48))
    overlap = ok.copy()
    overlap[1] = (1 << 24) | 1  # unit 1 is the second unit of the first list
    with pytest.raises(AssertionError, match="share a unit"):
        R.decode_block(payload, overlap, 2, 4, geom, slices)
    with pytest.raises(AssertionError, match="beyond"):
        R.decode_block(payload, ok, 2, 3, geom, slices)  # the last list ends at unit 4
    small = R.geometry(12, 8)
    with pytest.raises(AssertionError):
        R.decode_block(np.array([256] * 8, dtype=np.uint16), np.array([1] + [0] * 15, dtype=np.uint64), 0, 1, small, np.arange(16))


@pytest.mark.parametrize("n_src,n_owner", C.PAIRS)
def test_split_bits_is_a_partition_with_overlap(n_src, n_owner):
    geom = R.geometry(20, 16)
    rng = np.random.default_rng(n_src)
    f = np.zeros((1 << 15) + 1, dtype=np.uint32)
    a, b, c3 = (rng.integers(0, 1 << 32, 1 << 15, dtype=np.uint64).astype(np.uint32) for _ in range(3))
    f[:-1] = a & (b | c3)  # three bits of eight: ~24 k of a window's 65536
    forced = C.forced_cells(f, geom, n_src, n_owner)
    cells = R.split_bits(f, geom, n_src, n_owner, rng, forced)
    assert (R.union_filter(cells, geom, 20) == f).all()
    lay = R.Layout(n_src, n_owner)
    assert all(lay.lists_slice(geom, s, sp) for s, sp, _ in cells)
    addr, sp, win, off = R.filter_bits(f, geom)
    for (s, fsp, fw), n in forced.items():
        first = off[(sp == fsp) & (win == fw)][:n]
        assert (cells.get((s, fsp, fw), np.zeros(0)) == first).all(), (s, fsp, fw, n)
    c = n_src // n_owner if n_owner else n_src
    listed = sum(len(v) for v in cells.values())
    assert listed == addr.size if c == 1 else listed > addr.size  # duplicates across sources
    if c > 1:
        assert sorted(set(forced.values()))[:5] == [0, 1, 7, 8, 9] and 16 * 1024 + 3 in forced.values()


@pytest.mark.parametrize("name", list(C.TEXTS))
def test_the_texts_reach_the_densities_the_gpu_tests_rely_on(name):
    L, slice_bits, _ = C.TEXTS[name]
    geom = R.geometry(L, slice_bits)
    o = C.oracle_for(name)
    try:
        o.fill_only()
        f = o.filter
    finally:
        o.close()
    _, sp, win, _ = R.filter_bits(f, geom)
    _, count = np.unique(sp * geom["windows"] + win, return_counts=True)
    T = 1024 // geom["windows"]
    pairs = dict(C.FMT6 + C.FMT8)[name]
    for n_src, n_owner in pairs:
        forced = C.forced_cells(f, geom, n_src, n_owner)
        c = n_src // n_owner if n_owner else n_src
        for (s, fsp, fw), n in forced.items():
            have = int(((sp == fsp) & (win == fw)).sum())
            assert n <= have, (name, n_src, n_owner, fsp, fw, n, have)
        if c > 1 and name in C.DENSE:
            # every forced length exists, the streaming one of 2 * T * 8 + 3 entries among them, in a window that holds that many bits
            assert sorted(set(forced.values()))[:9] == C.lengths(geom["windows"], None)[:9], (name, n_src, n_owner)
            assert 2 * T * 8 + 3 in forced.values()
        if c > 1 and name != "skewed6":  # (the skewed text's repeats leave a handful of bits per 4096-bit window)
            assert {0, 1, 7, 8, 9} <= set(forced.values())
    if name in C.DENSE:
        assert count.max() > 16 * T + 3
    if name == "dense8":
        assert count.min() > 32768  # more than half of every window
    if name.startswith("sparse"):
        assert 50 < count.mean() < 400  # the m2_like density
