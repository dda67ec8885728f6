"""CPU: the masks of tests/mask_cases.py hold what tests/test_gpu_mask_compaction.py relies on -- the block counts of the text
lengths, the block of every planted mark, no bit at or past n_text -- and the numpy definition of the compaction agrees with a
bit-by-bit loop.  The 67 M-position masks are the slow ones here (a second each to draw)."""
import numpy as np
import pytest

import mask_cases as M


def test_block_counts_of_the_lengths():
    """nb = ceil(((n_text >> 5) + 1) / 256) of every text length, and the form each nb takes by size and when forced."""
    assert [M.n_blocks(n) for n in M.LENGTHS] == [1, 1, 1, 2, 2, 4096, 4097, 4097, 8193]
    assert all(M.n_blocks(n) == M.NB[n] for n in M.LENGTHS)
    assert M.mask_words(8191) == 256 and M.mask_words(8192) == 257 and M.mask_words(31) == 1 and M.mask_words(2) == 1
    assert [M.scan_form(M.NB[n]) for n in M.LENGTHS] == [1, 1, 1, 1, 1, 1, 2, 2, 2]
    assert all(M.scan_form(M.NB[n], 1) == 1 and M.scan_form(M.NB[n], 2) == 2 for n in M.LENGTHS)
    # by size the single workgroup comes back beyond 64 segments, and the option cannot force the pair there (64 words of scratch)
    assert M.scan_form(64 * M.SEG) == 2 and M.scan_form(64 * M.SEG + 1) == 1 and M.scan_form(64 * M.SEG + 1, 2) == 1
    # the block behind the text's last position exists and is empty at the two lengths that are multiples of 8192
    assert M.last_block(8192) == 0 and M.last_block(8193) == 1 and M.last_block(33554431) == 4095 and M.last_block(33554432) == 4095
    assert M.last_block(33554532) == 4096 and M.last_block(67108864) == 8191


@pytest.mark.parametrize("n_text", M.LENGTHS)
def test_masks_place_what_they_claim(n_text):
    names = M.case_names(n_text)
    assert len(set(names)) == len(names)
    assert names[0] == ("rand0.5" if n_text == 67108864 else "full")
    assert {"empty", "first", "last", "last_block", "rand0.0001", "rand0.03", "rand0.5"} <= set(names)
    lb = M.last_block(n_text)
    assert ("full_block" in names) == (lb >= 2) and ("border0" in names) == (lb >= 1)
    assert ("block4095" in names) == (n_text >= 33554431) and ("block4096" in names) == (n_text >= 33554532) == ("border4095" in names)
    sizes = {}
    for name in names:
        m = M.mask(n_text, name)
        assert m.size == M.mask_words(n_text) and m.dtype == np.uint32
        pos = M.marks_of(m).astype(np.int64)
        sizes[name] = pos.size
        assert pos.size == 0 or pos[-1] < n_text, (name, "a bit at or past n_text")
        blocks = np.unique(pos // M.BLOCK)
        if name == "empty":
            assert pos.size == 0
        elif name == "first":
            assert pos.tolist() == [0]
        elif name == "last":
            assert pos.tolist() == [n_text - 1]
        elif name == "full":
            assert pos.size == n_text and pos[0] == 0 and pos[-1] == n_text - 1
        elif name == "full_block":
            b = M.full_block_index(n_text)
            assert 1 <= b < lb and pos.size == M.BLOCK and blocks.tolist() == [b]
        elif name in ("block4095", "block4096", "last_block"):
            b = {"block4095": 4095, "block4096": 4096, "last_block": lb}[name]
            lo, hi = M.block_range(b, n_text)
            assert blocks.tolist() == [b] and pos[0] == lo and pos[-1] == hi - 1
            assert hi - lo <= 2 or 2 <= pos.size < hi - lo or hi - lo < 8
        elif name.startswith("border"):
            b = {"border0": 0, "border4095": 4095, "border_last": lb - 1}[name]
            assert pos.tolist() == [(b + 1) * M.BLOCK - 1, (b + 1) * M.BLOCK]
            assert (pos // 32 % M.BLOCK_WORDS).tolist() == [M.BLOCK_WORDS - 1, 0] and blocks.tolist() == [b, b + 1]
        else:
            d = float(name[4:])
            want = n_text * d
            assert abs(pos.size - want) <= 6 * np.sqrt(want) + 1, (name, pos.size, want)
            if n_text >= 33554431:   # every block, every segment and the borders between them take part
                per_block = np.bincount(pos // M.BLOCK, minlength=M.n_blocks(n_text))
                assert per_block[:lb].min() >= (1 if d >= 0.03 else 0) and per_block[lb + 1:].sum() == 0   # (every whole block)
                # (the 100 positions of 33 554 532's second segment: only density 0.5 is sure to mark some)
                assert all(per_block[s * M.SEG:(s + 1) * M.SEG].sum() > 0 for s in range(lb // M.SEG + 1) if d == 0.5 or n_text - s * M.SEG * M.BLOCK >= M.BLOCK)
    assert max(sizes.values()) == sizes[names[0]], "the first mask is the densest: it sizes the list for the others"


def test_the_definition_against_a_bit_by_bit_loop():
    rng = np.random.default_rng(5)
    for n_text in (2, 31, 33, 8191, 8192, 8193, 20000):
        for name in M.case_names(n_text):
            m = M.mask(n_text, name)
            assert (M.marks_of(m) == M.marks_bit_by_bit(m)).all() and M.marks_of(m).dtype == np.uint64, (n_text, name)
    w = rng.integers(0, 1 << 32, 300, dtype=np.uint64).astype(np.uint32)
    got = M.marks_of(w)
    assert (got == M.marks_bit_by_bit(w)).all() and (np.diff(got.astype(np.int64)) > 0).all()
    assert got.size == sum(bin(int(x)).count("1") for x in w)
    assert M.marks_of(np.array([0x80000001, 0, 2], dtype=np.uint32)).tolist() == [0, 31, 65]


def test_pack_reference_and_counts():
    rng = np.random.default_rng(9)
    for group, cap1, n in ((32, 96, 7), (16, 160, 70)):
        regions = rng.integers(0, 1 << 30, (n, cap1))
        for kind in ("zeros", "full", "random"):
            c = M.pack_counts(kind, n, cap1, group)
            assert c.dtype == np.uint32 and (c % group == 0).all() and (c <= cap1).all()
            want = [int(regions[r, i]) for r in range(n) for i in range(int(c[r]))]
            assert M.pack_reference(regions, c).tolist() == want
        c = M.pack_counts("random", 4000, cap1, group)
        assert (c == 0).sum() > 800 and (c == cap1).sum() > 100 and np.unique(c).size == cap1 // group + 1
