"""GPU (-m gpu): the round mask's compaction and the exchange's region packing against their definitions, at every form.

Both are a prefix sum followed by a move, both were rewritten for speed, and both ran only behind whole pipelines on whatever a real
hash produced.  Here they are driven directly with masks and counts of the test's own choosing.

A  mask -> ordered mark list (k_mask_count, k_scan_sums, k_scan_sums_seg, k_scan_sums_wide, k_mask_scatter behind compact_mask):
   marks == flatnonzero(bits of the mask) as uint64, n_marks == its length (mask_cases.marks_of; on the device by nonzero over the
   unpacked words where the list is long, tied to the numpy definition at every small length and on every sparse mask).
     forms    text lengths with nb = 1, 1, 1, 2, 2, 4096, 4097, 4097, 8193 blocks of 256 words (the second 4097: 33 554 532 positions, 100 of
              them in the second segment, which at 33 554 432 exists and holds none), each with the option test_mask_scan at 0 (by
              size) and 2 (the segmented pair: one segment with base 0 on the small texts), nb = 4097 / 8193 also at 1 (the single
              workgroup's loop turns over twice / three times and carries).  "mask_scan_form" is asserted after every count.
     masks    empty, position 0, position n_text - 1, every position (at 67 M positions: density 0.5), one full block of 8192 marks
              between two empty ones, marks in block 4095 / 4096 / the last block alone, the last word of a block with the first of the
              next (blocks 0|1, 4095|4096 = the segment border, the last two), densities 1e-4, 0.03, 0.5.  Where a length has no such
              block the mask is left out (mask_cases.case_names; tests/test_mask_cases_cpu.py checks the placement): "full_block" and
              "border_last" need a position in a third block, "border0" one in a second, "block4096" / "border4095" exist from
              33 554 532 positions on -- at 33 554 432 the 4097th block holds no position.
     context  one per text length, used for nothing else: k = 9, L = 16, q = 1, a text of one record (the letters do not matter:
              tpc_pass2_mark_owners(world = 1) copies the list and answers owner 0).  The densest mask comes first and sizes the list
              (ensure() never shrinks it); the outputs are poisoned and a few words longer than n: the tail must stay untouched.
              Before that the densest mask is compacted ONCE under the other scan form, list unread: should a scan be wrong, the
              entries a too low offset leaves unwritten then hold positions of the text, not whatever the allocation held -- the owner
              kernel loads the k-mer at every entry of the list.
     cached   after a partitioned query (query_path == 2, one batch and several) tpc_pass2_marks reuses the query's block sums: the
              list == the set bits of mask_download(); then, each after a fresh query that left the sums valid, the mask is rewritten
              by tpc_mask_import (a strict subset), tpc_mask_merge (one block) and tpc_shard_periodic_copy (one rank, option set) and
              compacted again.  The copy cannot change a mask the query itself has just copied (it is a fixed point), so that one
              call shows no missing reset; the other two do.
     run-wide three rounds of tpc_mask_import (random subsets of a real query's candidate mask) + tpc_pass2_filter: mask_download(True) is
              their OR (first round: the copy, later rounds: k_mask_or) and tpc_emit counts as many marked positions as it has bits.
B  tpc_shard_pack (k_region_offsets, k_region_pack): packed == the used prefixes of the regions in region order, bytes_per_dest[d] ==
   the counts of destination d's block x entry size, nothing written behind the total; W = 2, 4 emulated ranks, insert (4-byte) and
   query (8-byte) entries, counts all zero / all full / random multiples of the flush group; n = 4 regions (a lone partly filled wave),
   n = 1184 and 608 (ragged 128- and 64-count segments, the last wave partly filled, six idle) and n = 16384 (all 16 waves).

Not covered: texts beyond 2^31 positions by size (the return to the single workgroup beyond 64 segments is reached through the
option, at three iterations, not at 65 segments).

That the tests bite -- three changes planted one at a time, each can only lower offsets or counts; the narrowest test, once on an MI355X:
   1  k_scan_sums_wide ignores the totals of the segments before it   test_compaction_equals_the_definition[67108864-scan2] fails on its
                                                                      first mask: 16 777 273 of 33 557 026 entries differ, entry 0 holds 33 554 433
   2  k_scan_sums does not carry across loop iterations               test_compaction_equals_the_definition[67108864-scan1] fails the same way
   3  tpc_mask_import no longer clears rmask_sums_valid               test_rewritten_mask_after_the_query fails: n_marks 29 901 (the query's) for
                                                                      a subset of 15 027 bits
(At 33 554 432 positions the second segment holds no position, so 1 and 2 change nothing there; 33 554 532 and 67 108 864 see them.)

Wall time per test on an MI355X (32 tests, 6.8 s together): 1.4 s for [67108864-scan0] and 0.7 to 0.8 s for [33554431-scan0],
[33554432-scan0] and [33554532-scan0], which draw their length's masks on the host (the forced forms reuse them: 0.02 to 0.04 s each),
0.6 s for the file's first test (the code objects load; its setup imports torch: 1.5 s), 0.11 s for the first tpc_shard_pack case, at most
0.03 s for every other one."""
import functools
import os

import numpy as np
import pytest

import helpers as H
import mask_cases as M

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A5A5A5A5A
OWNER_POISON = 0x5A5A5A5A
PAD = 8
SEED = 20240229


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


class FlatText:
    """What Context.seq_upload reads: n_text positions, the separator N at both ends, the letter A between them."""

    def __init__(self, n_text):
        nw = (n_text + 31) // 32
        self.length = n_text
        self.bases = np.zeros(nw, dtype=np.uint64)
        self.nmask = np.zeros(nw, dtype=np.uint32)
        self.nmask[0] |= np.uint32(1)
        self.nmask[(n_text - 1) >> 5] |= np.uint32(1 << ((n_text - 1) & 31))


def to_device(torch, words):
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.int32)).cuda()


def device_marks(torch, dev_words):
    """The definition on the device: nonzero over the unpacked words (int64 positions, ascending)."""
    sh = torch.arange(32, device="cuda", dtype=torch.int32)
    bits = ((dev_words.unsqueeze(1) >> sh) & 1).to(torch.bool)
    return bits.reshape(-1).nonzero().squeeze(1)


@functools.lru_cache(maxsize=None)
def host_marks(n_text, name):
    """(popcount, the numpy definition's list or None where it is long) of a generated mask."""
    m = M.mask(n_text, name)
    n = int(np.unpackbits(m.view(np.uint8)).sum(dtype=np.int64))
    return n, (M.marks_of(m) if n <= (1 << 21) else None)


def read_list(torch, ctx, n):
    """The context's list and its owners through tpc_pass2_mark_owners(world = 1), into poisoned buffers PAD words longer than n."""
    pos = torch.full((n + PAD,), POISON, dtype=torch.int64, device="cuda")
    own = torch.full((n + PAD,), OWNER_POISON, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.pass2_mark_owners(1, pos.data_ptr(), own.data_ptr())
    assert bool((pos[n:] == POISON).all()), "the list was written behind its n entries"
    assert bool((own[n:] == OWNER_POISON).all()), "the owners were written behind their n entries"
    assert not bool(own[:n].any()), "an owner other than 0 with one rank"
    return pos[:n]


def assert_same(torch, got, want, tag):
    assert got.numel() == want.numel(), ("list length", got.numel(), want.numel()) + tag
    bad = (got != want).nonzero().squeeze(1)
    if bad.numel():
        i = int(bad[0])
        raise AssertionError("the list differs from the definition at %d of %d entries, first at entry %d (block %d of the sums): device %d, "
                             "definition %d; %r" % (bad.numel(), want.numel(), i, int(want[i]) // M.BLOCK, int(got[i]), int(want[i]), tag))


def check_mask(torch, ctx, n_text, name, option):
    tag = (n_text, name, option)
    words = M.mask(n_text, name)
    dev = to_device(torch, words)
    torch.cuda.synchronize()
    ctx.mask_import(dev.data_ptr())
    n = ctx.pass2_marks()
    assert ctx.stat("mask_scan_form") == M.scan_form(M.n_blocks(n_text), option), ("the count took the other scan form",) + tag
    n_host, list_host = host_marks(n_text, name)
    assert n == n_host, ("n_marks", n, n_host) + tag
    got = read_list(torch, ctx, n)
    assert_same(torch, got, device_marks(torch, dev), tag)
    if list_host is not None:   # the device's reference is the numpy definition
        assert (got.cpu().numpy().view(np.uint64) == list_host).all(), ("the numpy definition",) + tag


COMPACTION = [(n, 0) for n in M.LENGTHS] + [(n, 2) for n in M.LENGTHS] + [(n, 1) for n in M.LENGTHS if M.NB[n] > M.SEG]


@pytest.mark.parametrize("n_text,option", COMPACTION, ids=["%d-scan%d" % c for c in COMPACTION])
def test_compaction_equals_the_definition(capi, torch, n_text, option):
    """Every mask of the length on one context, under the scan form the option asks for."""
    nb = M.n_blocks(n_text)
    assert nb == M.NB[n_text]
    ctx = capi.Context(0)
    try:
        ctx.set_params(9, 16, 1, capi.seed_table(1, 16, seed=SEED))
        ctx.seq_upload(FlatText(n_text))
        assert ctx.mask_words() == M.mask_words(n_text)
        names = M.case_names(n_text)
        # the list is sized and written once by the other form (see the file's docstring); the list is not read
        other = 2 if M.scan_form(nb, option) == 1 else 1
        ctx.set_option("test_mask_scan", other)
        dev = to_device(torch, M.mask(n_text, names[0]))
        torch.cuda.synchronize()
        ctx.mask_import(dev.data_ptr())
        assert ctx.pass2_marks() == host_marks(n_text, names[0])[0] and ctx.stat("mask_scan_form") == other
        ctx.set_option("test_mask_scan", option)
        for name in names:
            check_mask(torch, ctx, n_text, name, option)
        check_mask(torch, ctx, n_text, names[0], option)   # a long list again behind the short ones
    finally:
        ctx.set_option("test_mask_scan", 0)  # process-wide
        ctx.close()


def test_scan_form_by_size(capi, torch):
    """With the option at 0 the single workgroup serves nb <= 4096 and the segmented pair 4097 and 8193; a value outside 0..2 means 0."""
    forms = {}
    for n_text in (8193, 33554431, 33554432, 33554532, 67108864):
        ctx = capi.Context(0)
        try:
            ctx.set_option("test_mask_scan", 7)
            ctx.set_params(9, 16, 1, capi.seed_table(1, 16, seed=SEED))
            ctx.seq_upload(FlatText(n_text))
            dev = to_device(torch, M.mask(n_text, "last"))
            torch.cuda.synchronize()
            ctx.mask_import(dev.data_ptr())
            assert ctx.pass2_marks() == 1
            forms[n_text] = ctx.stat("mask_scan_form")
            assert int(read_list(torch, ctx, 1)[0]) == n_text - 1
        finally:
            ctx.close()
    assert forms == {8193: 1, 33554431: 1, 33554432: 2, 33554532: 2, 67108864: 2}


# ------------------------------------------------------------------------------------------------------------------ the cached sums
QUERY = (("insert_mode", 2), ("query_mode", 2), ("part_min_tiles", 1), ("shard_periodic_skip", 1))
K, L, Q = 25, 28, 5   # the golden case tr_k25_L28


def query_ctx(capi, torch, extra=()):
    """A context over the golden text with tracts, the partitioned query forced, its list sized by the densest mask there is."""
    text = capi.PackedText.from_fasta([os.path.join(H.GOLDEN, "tracts.fa")])
    ctx = capi.Context(0)
    for name, val in QUERY + tuple(extra):
        ctx.set_option(name, val)
    ctx.set_params(K, L, Q, capi.seed_table(Q, L, seed=SEED))
    ctx.seq_upload(text)
    n_text = text.length
    assert ctx.mask_words() == M.mask_words(n_text)
    full = M.clip(np.full(ctx.mask_words(), 0xFFFFFFFF, dtype=np.uint32), n_text)
    dev = to_device(torch, full)
    torch.cuda.synchronize()
    ctx.mask_import(dev.data_ptr())
    assert ctx.pass2_marks() == n_text
    return ctx, n_text


def query(ctx):
    ctx.filter_reset()
    ctx.pass1_insert()
    n = ctx.pass1_query()
    assert ctx.stat("query_path") == 2, "the partitioned query did not run (or overflowed): its block sums are not kept"
    return n


def assert_list_is_the_mask(torch, ctx, tag):
    """tpc_pass2_marks now: n and the list equal the definition over mask_download().  Returns the mask's words."""
    n = ctx.pass2_marks()
    words = ctx.mask_download()
    want = M.marks_of(words)
    assert n == want.size, ("n_marks", n, want.size, tag)
    got = read_list(torch, ctx, n).cpu().numpy().view(np.uint64)
    assert (got == want).all(), ("the list is not the set bits of the mask", int(np.flatnonzero(got != want)[0]), tag)
    return words


@pytest.mark.parametrize("extra,batched", [((), False), ((("part_budget_bytes", 64 << 10),), True)], ids=["one-batch", "batches"])
def test_marks_right_after_the_query(capi, torch, extra, batched):
    """The shortcut itself: tpc_pass2_marks right after tpc_pass1_query scatters behind the query's own block sums.  With several tile
    batches every batch's window count has written the same sums buffer before the final count."""
    ctx, n_text = query_ctx(capi, torch, extra)
    try:
        for rep in range(2):
            n = query(ctx)
            assert (ctx.stat("query_batches") > 1) == batched, ctx.stat("query_batches")
            words = assert_list_is_the_mask(torch, ctx, ("after the query", rep, extra))
            assert 0 < n == M.marks_of(words).size < n_text
            assert_list_is_the_mask(torch, ctx, ("a second compaction of the same mask", rep, extra))   # (the sums were consumed: counted again)
    finally:
        ctx.close()


def test_rewritten_mask_after_the_query(capi, torch):
    """Each call that rewrites the round mask after a query has left its sums valid must make the next compaction count again."""
    ctx, n_text = query_ctx(capi, torch)
    rng = np.random.default_rng(11)
    nw = ctx.mask_words()
    try:
        # tpc_mask_import of a strict subset
        n = query(ctx)
        m0 = ctx.mask_download()
        sub = m0 & rng.integers(0, 1 << 32, nw, dtype=np.uint64).astype(np.uint32)
        n_sub = M.marks_of(sub).size
        assert 0 < n_sub < n and n == M.marks_of(m0).size
        dev = to_device(torch, sub)
        torch.cuda.synchronize()
        ctx.mask_import(dev.data_ptr())
        got = assert_list_is_the_mask(torch, ctx, "mask_import of a subset")
        assert (got == sub).all()
        # tpc_mask_merge of one block
        assert query(ctx) == n and (ctx.mask_download() == m0).all()
        extra = M.words_of_positions(rng.integers(1, n_text - K - 1, 3000), n_text)
        assert (extra & ~m0).any()
        dev = to_device(torch, extra)
        torch.cuda.synchronize()
        ctx.mask_merge(dev.data_ptr(), 1)
        got = assert_list_is_the_mask(torch, ctx, "mask_merge of one block")
        assert (got == (m0 | extra)).all() and M.marks_of(got).size > n
        # tpc_shard_periodic_copy on a one-rank context with the option set
        assert query(ctx) == n
        assert ctx.stat("periodic_any_query") == 1, "the golden text has no copying position: the copy would not run"
        ctx.shard_periodic_copy()
        got = assert_list_is_the_mask(torch, ctx, "shard_periodic_copy")
        assert (got == m0).all()   # the query has copied already: a fixed point
    finally:
        ctx.close()


def test_run_wide_mask_over_three_rounds(capi, torch):
    """tpc_pass2_filter merges every round's mask into the run-wide one (round 1 copies, rounds 2 and 3 run k_mask_or), and tpc_emit
    compacts that one.  The rounds' masks are subsets of a real query's candidates: positions the exact filter is built for."""
    ctx, n_text = query_ctx(capi, torch)
    rng = np.random.default_rng(12)
    nw = ctx.mask_words()
    try:
        ctx.run_begin()
        query(ctx)
        m0 = ctx.mask_download()
        union = np.zeros(nw, dtype=np.uint32)
        for rnd in range(3):
            sub = m0 & rng.integers(0, 1 << 32, nw, dtype=np.uint64).astype(np.uint32) & rng.integers(0, 1 << 32, nw, dtype=np.uint64).astype(np.uint32)
            assert (sub & ~union).any(), "the round adds nothing new"
            dev = to_device(torch, sub)
            torch.cuda.synchronize()
            ctx.mask_import(dev.data_ptr())
            ctx.pass2_filter()
            assert ctx.stat("round_marks") == M.marks_of(sub).size
            union |= sub
            assert (ctx.mask_download(True) == union).all(), ("run-wide mask after round", rnd)
        assert (union != m0).any() and M.marks_of(union).size > M.marks_of(sub).size
        ctx.junctions_finalize()
        n_marked, n_valid = ctx.emit()
        assert n_marked == M.marks_of(union).size and n_valid <= n_marked
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------------ tpc_shard_pack
# name: (positions of the text as tiles of 16384 per rank, L, slice_bits, regions of the insert, regions of the query).  A rank hashes
# `tiles` 512-word tiles; the level-1 regions number nwg1 << b1 with b1 = (L - slice_bits + 1) / 2, nwg1 = min(256, (tiles + 1) / 2)
# workgroups for the insert and min(256, tiles) for the query (csrc/tpc_partition.hip, tpc_qpartition.hip)
GEOMETRY = {
    "lone-wave": (1, 16, 12, 4, 4),          # fewer than 64 counts: wave 0 alone, partly filled
    "ragged": (37, 20, 10, 608, 1184),       # (n + 15) / 16 = 38 and 74: segments of 64 and 128, the last wave partly filled, the rest idle
    "16-waves": (256, 24, 12, 8192, 16384),  # every wave owns a whole segment of 512 / 1024 counts
}
PACK = [(g, w) for g in GEOMETRY for w in (2, 4)]


def segment(n):
    return ((n + 15) // 16 + 63) & ~63


@pytest.mark.parametrize("geometry,W", PACK, ids=["%s-W%d" % p for p in PACK])
def test_shard_pack_equals_the_definition(capi, torch, geometry, W):
    tiles, L_, slice_bits, n_insert, n_query = GEOMETRY[geometry]
    n_text = tiles * W * 16384 - 100 if tiles > 1 else 5000
    ctx = capi.Context(0)
    try:
        ctx.set_option("slice_bits", slice_bits)
        ctx.shard_config(0, W)
        ctx.set_params(K, L_, Q, capi.seed_table(Q, L_, seed=SEED))
        ctx.seq_upload(FlatText(n_text))
        seen = []
        for which, eb, n_want, dtype in ((0, 4, n_insert, torch.int32), (1, 8, n_query, torch.int64)):
            g = ctx.shard_plan(which)
            assert g["batches"] == 1 and g["tiles_per_rank"] == tiles, g
            n = W * g["count_block_bytes"] // 4
            assert n == n_want and n % W == 0, (n, n_want, g)
            cap1 = W * g["region_block_bytes"] // (n * eb)
            group = 128 // eb
            assert cap1 * n * eb == W * g["region_block_bytes"] and cap1 % group == 0 and cap1 >= 2 * group, (cap1, g)
            seen.append(n)
            gen = torch.Generator(device="cuda")
            gen.manual_seed(n + eb)
            regions = torch.randint(-(1 << 31), 1 << 31, (n, cap1), dtype=torch.int64, device="cuda", generator=gen).to(dtype) if eb == 4 else \
                torch.randint(-(1 << 62), 1 << 62, (n, cap1), dtype=torch.int64, device="cuda", generator=gen)
            col = torch.arange(cap1, device="cuda", dtype=torch.int64).unsqueeze(0)
            for kind in ("zeros", "full", "random"):
                counts_host = M.pack_counts(kind, n, cap1, group, seed=W)
                counts = torch.from_numpy(counts_host.view(np.int32).copy()).cuda()
                total = int(counts_host.sum(dtype=np.int64))
                packed = torch.full((n * cap1 * eb + 64,), 0x5A, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                per_dest = ctx.shard_pack(which, regions.data_ptr(), counts.data_ptr(), packed.data_ptr(), W)
                tag = (geometry, W, "insert" if which == 0 else "query", kind, n, cap1)
                block = n // W
                assert per_dest == [int(counts_host[d * block:(d + 1) * block].sum(dtype=np.int64)) * eb for d in range(W)], ("bytes_per_dest",) + tag
                assert sum(per_dest) == total * eb
                assert bool((packed[total * eb:] == 0x5A).all()), ("bytes behind the total were written",) + tag
                want = regions[col < counts.to(torch.int64).unsqueeze(1)]   # row-major: the used prefixes in region order
                got = packed[:total * eb].view(dtype)
                assert got.numel() == want.numel() == total
                bad = (got != want).nonzero().squeeze(1)
                if bad.numel():
                    i = int(bad[0])
                    off = np.concatenate([[0], np.cumsum(counts_host.astype(np.int64))])
                    r = int(np.searchsorted(off, i, side="right")) - 1
                    raise AssertionError("packed differs at %d of %d entries, first at entry %d = entry %d of region %d (wave %d of the offsets' scan, "
                                         "segments of %d counts): %r" % (bad.numel(), total, i, i - off[r], r, r // segment(n), segment(n), tag))
                if n <= 64:   # the same by the numpy definition
                    ref = M.pack_reference(regions.cpu().numpy(), counts_host)
                    assert (got.cpu().numpy() == ref).all(), ("the numpy definition",) + tag
        if geometry == "lone-wave":
            assert max(seen) < 64
        elif geometry == "ragged":
            assert all(((n + 15) // 16) % 64 for n in seen) and all(n % segment(n) for n in seen)
        else:
            assert max(seen) >= 16384 and max(seen) == 16 * segment(max(seen))
    finally:
        ctx.close()
