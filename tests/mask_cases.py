"""The mask compaction by its definition, and the masks and text lengths at which its kernels change form: shared by
tests/test_gpu_mask_compaction.py (the device) and tests/test_mask_cases_cpu.py (that the generators place what they claim).

A round mask is an array of 32-bit words, bit b of word w = text position 32 w + b, of (n_text >> 5) + 1 words (csrc/tpc_capi.hip:
tpc_seq_upload).  The compaction counts 256 words = 8192 positions per workgroup (a block), scans the block sums in segments of 4096
(csrc/tpc_pass2.hip: SCAN_SEG) and scatters every block's positions behind its offset."""
import functools

import numpy as np

BLOCK_WORDS = 256
BLOCK = BLOCK_WORDS * 32   # positions of one workgroup of k_mask_count / k_mask_scatter
SEG = 4096                 # block sums of one scan segment, and of one loop iteration of k_scan_sums

# text lengths, the smallest at which each form exists: one word; one block, then two (8192 is the first length with 257 words,
# 8193 the first with a position in the second block); nb = 4096, the last size of one workgroup in one loop iteration; 4097, two
# segments (the second one holds no position yet: whatever offset its one block gets, nothing is written there), the same nb with 100
# positions in the second segment (the first length at which a lost segment total or a lost carry shows); 8193, three segments
SMALL = (2, 31, 8191, 8192, 8193)
LARGE = (33554431, 33554432, 33554532, 67108864)
LENGTHS = SMALL + LARGE
NB = {2: 1, 31: 1, 8191: 1, 8192: 2, 8193: 2, 33554431: 4096, 33554432: 4097, 33554532: 4097, 67108864: 8193}
DENSITIES = (1e-4, 0.03, 0.5)


def mask_words(n_text):
    return (n_text >> 5) + 1


def n_blocks(n_text):
    return -(-mask_words(n_text) // BLOCK_WORDS)


def scan_form(nb, option=0):
    """What tpc_launch_mask_count takes for nb block sums under option test_mask_scan: 1 = the single workgroup, 2 = the segmented pair."""
    segs = -(-nb // SEG)
    if option == 1 or segs > 64:
        return 1
    return 2 if segs >= (1 if option == 2 else 2) else 1


def marks_of(words):
    """THE DEFINITION: the positions of the set bits of the mask, ascending, as uint64."""
    bits = np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")
    return np.flatnonzero(bits).astype(np.uint64)


def marks_bit_by_bit(words):
    """The same, one bit after the other (the check of marks_of; small masks only)."""
    out = []
    for w, x in enumerate(np.asarray(words).tolist()):
        for b in range(32):
            if (x >> b) & 1:
                out.append(32 * w + b)
    return np.array(out, dtype=np.uint64)


def words_of_positions(pos, n_text):
    bits = np.zeros(mask_words(n_text) * 32, dtype=np.uint8)
    bits[np.asarray(pos, dtype=np.int64)] = 1
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)


def clip(words, n_text):
    """Clears every bit at or past n_text."""
    words = words.copy()
    w, b = n_text >> 5, n_text & 31
    words[w] &= np.uint32((1 << b) - 1)
    words[w + 1:] = 0
    return words


def last_block(n_text):
    """The last block that holds a position of the text (at n_text = 8192 and 33554432 the block behind it exists and is empty)."""
    return (n_text - 1) // BLOCK


def block_range(b, n_text):
    return b * BLOCK, min((b + 1) * BLOCK, n_text)


def _random(n_text, density, seed):
    rng = np.random.default_rng(seed)
    if density == 0.5:
        return clip(rng.integers(0, 1 << 32, mask_words(n_text), dtype=np.uint64).astype(np.uint32), n_text)
    if n_text * density < 1e6 and n_text > 1 << 20:  # sparse over a long text: draw the positions
        return words_of_positions(rng.integers(0, n_text, int(n_text * density)), n_text)
    return words_of_positions(np.flatnonzero(rng.random(n_text) < density), n_text)


def _in_block(b, n_text, seed):
    """Marks of density 0.3 inside block b alone, its first and its last position among them."""
    lo, hi = block_range(b, n_text)
    rng = np.random.default_rng(seed)
    pos = lo + np.flatnonzero(rng.random(hi - lo) < 0.3)
    return words_of_positions(np.concatenate([pos, [lo, hi - 1]]), n_text)


def full_block_index(n_text):
    """The block that "full_block" sets: whole, an empty block before it and one behind (texts with a position in a third block)."""
    return max(1, last_block(n_text) // 2)


def case_names(n_text):
    """The masks of a text length, the densest first (it sizes the context's list for all that follow)."""
    nb, lb = n_blocks(n_text), last_block(n_text)
    names = ["rand0.5" if n_text >= 67108864 else "full", "empty", "first", "last", "last_block", "rand0.0001", "rand0.03"]
    if n_text < 67108864:
        names.append("rand0.5")
    if lb >= 2:
        names.append("full_block")
    if lb >= 1:
        names.append("border0")              # last word of block 0 + first word of block 1
    if lb >= SEG:
        names += ["border4095", "block4096"]  # the segment border
    if lb >= SEG - 1:
        names.append("block4095")
    if lb >= 2:
        names.append("border_last")
    return names


@functools.lru_cache(maxsize=None)
def mask(n_text, name):
    """The mask `name` of a text of n_text positions: uint32 words, no bit at or past n_text.  Cached: the forced forms reuse them."""
    nb, lb = n_blocks(n_text), last_block(n_text)
    nw = mask_words(n_text)
    if name == "empty":
        m = np.zeros(nw, dtype=np.uint32)
    elif name == "first":
        m = words_of_positions([0], n_text)
    elif name == "last":
        m = words_of_positions([n_text - 1], n_text)
    elif name == "full":
        m = clip(np.full(nw, 0xFFFFFFFF, dtype=np.uint32), n_text)
    elif name == "full_block":   # 8192 marks between two empty blocks
        b = full_block_index(n_text)
        m = np.zeros(nw, dtype=np.uint32)
        m[b * BLOCK_WORDS:(b + 1) * BLOCK_WORDS] = 0xFFFFFFFF
    elif name == "block4095":
        m = _in_block(4095, n_text, 4095)
    elif name == "block4096":
        m = _in_block(4096, n_text, 4096)
    elif name == "last_block":
        m = _in_block(lb, n_text, 7)
    elif name.startswith("border"):
        b = {"border0": 0, "border4095": 4095, "border_last": lb - 1}[name]
        m = words_of_positions([(b + 1) * BLOCK - 1, (b + 1) * BLOCK], n_text)
    elif name.startswith("rand"):
        d = float(name[4:])
        m = _random(n_text, d, int(d * 10000) + n_text % 1000)
    else:
        raise KeyError(name)
    assert m.dtype == np.uint32 and m.size == nw and nb == NB.get(n_text, nb)
    m.setflags(write=False)
    return m


# ---------------------------------------------------------------------------------------------- the exchange packing (tpc_shard_pack)
def pack_reference(regions, counts):
    """regions [n, cap1] entries, counts [n]: the used prefixes in region order."""
    return np.concatenate([regions[r, :c] for r, c in enumerate(np.asarray(counts).tolist())] + [regions[:0, 0]])


def pack_counts(kind, n, cap1, group, seed=0):
    """Counts the writer may leave (csrc/tpc_bins.h, tpc_rbins.h: a region's count is a whole number of flush groups, at most its
    capacity, itself a multiple of the group): all zero, all full, random multiples -- a third of them zero, a few full."""
    assert cap1 % group == 0
    if kind == "zeros":
        return np.zeros(n, dtype=np.uint32)
    if kind == "full":
        return np.full(n, cap1, dtype=np.uint32)
    rng = np.random.default_rng(seed + n)
    c = rng.integers(0, cap1 // group + 1, n) * group
    c[rng.random(n) < 0.33] = 0
    c[rng.random(n) < 0.05] = cap1
    return c.astype(np.uint32)
