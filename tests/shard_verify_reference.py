"""The sharded verification by its definitions, in plain Python / numpy: no GPU and none of the project's kernels.

What the kernels of csrc/tpc_qpartition.hip behind tpc_shard_verify_* / _route / _select / _finish / _mark must compute
(DESIGN section 5.2), written down once so that tests/test_gpu_shard_verify.py can compare each of them below the end-to-end
results.  tests/test_shard_verify_reference_cpu.py holds these definitions against the oracle and against assemble() of
tests/test_gpu_addr_shard.py.

Survivor ids: sid = (field << 3) | e.  field is 30 bits: the top log2(world) bits name the rank that hashed the position, the
rest is the position relative to that rank's batch (chunk_base).  e < 4: the in-edge c + T[g .. g+k-1] with c = e; e >= 4: the
out-edge T[g .. g+k-1] + c with c = e & 3."""
import numpy as np

TILE_POSITIONS = 16384  # positions of one 512-word tile of the packed text
FIELD_BITS = 30


# ------------------------------------------------------------------------------------------------ hashing
def _rotl1(x, L):
    return ((x << 1) & ((1 << L) - 1)) | (x >> (L - 1))


def _eat(letters, row, L):
    """CyclicHash of a word, one letter after the other: h = rotl(h, 1) ^ table[letter]."""
    h = 0
    for x in letters:
        h = _rotl1(h, L) ^ row[x]
    return h


def edge_letters(text, g, e, k):
    """The k + 1 letter codes (0..3, 4 = N) of the edge (g, e)."""
    w = [int(x) for x in text[g:g + k]]
    assert len(w) == k
    return [e] + w if e < 4 else w + [e & 3]


def strand_hashes(letters, L, table):
    """[(positive, negative)] per hash function: the hash of the word and of its reverse complement (N stays N)."""
    rc = [x if x == 4 else 3 - x for x in reversed(letters)]
    out = []
    for row in table:
        row = [int(v) for v in row]
        out.append((_eat(letters, row, L), _eat(rc, row, L)))
    return out


def pick_negative(pairs):
    """The canonical strand: the first function whose two values differ decides, the smaller wins; all equal: positive."""
    for p, n in pairs:
        if p != n:
            return n < p
    return False


def edge_hashes(text, g, e, k, L, table):
    """The q filter addresses in [0, 2^L) of the (k+1)-mer named by position g and edge code e (all of one strand: the canonical one)."""
    pairs = strand_hashes(edge_letters(text, g, e, k), L, table)
    neg = pick_negative(pairs)
    return [n if neg else p for p, n in pairs]


def tie_depth(text, g, e, k, L, table):
    """How many leading functions have equal strand hashes on this edge (0: function 0 decides; q: the positive strand by default)."""
    d = 0
    for p, n in strand_hashes(edge_letters(text, g, e, k), L, table):
        if p != n:
            break
        d += 1
    return d


def sid_parts(sid, world):
    """(source rank, position relative to the source's batch, e) of survivor ids (ints or a uint64 array)."""
    lw = int(world).bit_length() - 1
    field = (sid >> 3) & ((1 << FIELD_BITS) - 1)
    return field >> (FIELD_BITS - lw), field & ((1 << (FIELD_BITS - lw)) - 1), sid & 7


def make_sid(source, rel, e, world):
    lw = int(world).bit_length() - 1
    return (((int(source) << (FIELD_BITS - lw)) | int(rel)) << 3) | int(e)


# ------------------------------------------------------------------------------------------------ geometry
def owner_local(A, geom, world):
    """(owner rank, bit address inside the owner's shard) of filter addresses A under a shard_plan geometry (dict with slice_bits,
    b1, b2, b3, perm_mult).  Accepts an int or an array; returns uint64 / int64 arrays of A's shape."""
    A = np.asarray(A, dtype=np.uint64)
    sb, low = int(geom["slice_bits"]), int(geom["b2"]) + int(geom.get("b3", 0))
    F = int(geom["b1"]) + low
    u = np.uint64
    sp = ((A >> u(sb)) * u(int(geom["perm_mult"]))) & u((1 << F) - 1)
    bv = sp >> u(low)
    owner = (bv & u(world - 1)).astype(np.int64)
    if world == 1:
        return owner, A.copy()
    lw = int(world).bit_length() - 1
    local = ((((bv >> u(lw)) << u(low)) | (sp & u((1 << low) - 1))) << u(sb)) | (A & u((1 << sb) - 1))
    return owner, local


def chunk_base(n_tiles, rank, world, per, batch):
    """First text position of batch `batch` of rank `rank`: ranks own contiguous chunks of ceil(n_tiles / world) tiles, `per` tiles a batch."""
    chunk = (n_tiles + world - 1) // world
    return (min(n_tiles, rank * chunk) + batch * per) * TILE_POSITIONS


def text_tiles(n_text):
    """512-word tiles of a packed text of n_text positions (one more than the words need when n_text is a multiple of 16384)."""
    return (n_text // 32 + 512) // 512


# ------------------------------------------------------------------------------------------------ routing
def route_is_bijection(perm, n):
    """perm maps the n items onto the slots [0, n), each taken once."""
    perm = np.asarray(perm, dtype=np.int64)
    if perm.size != n:
        return False
    if n == 0:
        return True
    if perm.min() < 0 or perm.max() >= n:
        return False
    return bool((np.bincount(perm, minlength=n) == 1).all())


def route_counts_match(counts, owner, world):
    """counts[o] is the number of items of owner o, for every rank of the world."""
    owner = np.asarray(owner, dtype=np.int64)
    return len(counts) == world and [int(c) for c in counts] == np.bincount(owner, minlength=world).tolist()


def route_slots_in_ranges(perm, owner, counts):
    """Every item's slot lies in its owner's range of the exclusive prefix sum of counts (the order inside a range is not defined)."""
    perm, owner = np.asarray(perm, dtype=np.int64), np.asarray(owner, dtype=np.int64)
    end = np.cumsum(np.asarray(counts, dtype=np.int64))
    begin = end - np.asarray(counts, dtype=np.int64)
    return bool(((perm >= begin[owner]) & (perm < end[owner])).all())


def route_violations(perm, owner, counts, world):
    """Names of the routing properties a result breaks (empty: a valid owner-major routing of the items)."""
    bad = []
    if not route_is_bijection(perm, len(owner)):
        bad.append("bijection")
    if not route_counts_match(counts, owner, world):
        bad.append("counts")
    elif len(np.asarray(perm)) == len(owner) and not route_slots_in_ranges(perm, owner, counts):
        bad.append("ranges")
    return bad


# ------------------------------------------------------------------------------------------------ selection and marks
def all_hit(hit, n, fn_count, perm=None):
    """keep[i]: the fn_count answers of survivor i are all 1.  The answer of probe j = i * fn_count + t sits at hit[perm[j]];
    perm None: at hit[j]."""
    hit = np.asarray(hit, dtype=np.uint8)
    j = np.arange(n * fn_count, dtype=np.int64)
    a = hit[j] if perm is None else hit[np.asarray(perm, dtype=np.int64)[j]]
    return (a.reshape(n, fn_count) == 1).all(axis=1)


def mask_with_bits(before, positions):
    """The mask words after setting the given bit positions (bit b of word w = position 32 w + b)."""
    out = np.array(before, dtype=np.uint32)
    p = np.asarray(positions, dtype=np.int64)
    np.bitwise_or.at(out, p >> 5, (np.uint32(1) << (p & 31).astype(np.uint32)))
    return out
