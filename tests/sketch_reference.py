"""The distinct-edge sketch of tpc_distinct_sketch (include/twopaco_hip.h) by its definition, in numpy: every window is
evaluated directly from its letters -- nothing rolls -- and the estimate and the exact count it is compared with sit beside it.

With n = k + 1 and h[0..3] the first four outputs of splitmix64 from state 0x5457504143, every window w = T[g .. g + n) without
an 'N' contributes
    F = XOR_t rotl64(h[w_t], (n - 1 - t) mod 64)        R = XOR_t rotl64(h[3 - w_t], t mod 64)
    x = mix64(min(F, R));  idx = x >> 50;  v = x << 14;  rank = 51 if v == 0 else clz64(v) + 1;  reg[idx] = max(reg[idx], rank)."""
import numpy as np

P = 14
M = 1 << P
MASK64 = (1 << 64) - 1
U = np.uint64


def mix64_int(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def letter_hashes():
    state, out = 0x5457504143, []
    for _ in range(4):
        state = (state + 0x9E3779B97F4A7C15) & MASK64
        out.append(mix64_int(state))
    return out


def mix64(z):
    """tpc_mix64 on a uint64 array (array products wrap modulo 2^64)."""
    z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
    return z ^ (z >> U(31))


def rotl(x, r):
    r %= 64
    return x if r == 0 else (x << U(r)) | (x >> U(64 - r))


def window_hashes(codes, k):
    """(valid, x): for every g with a whole window in the text, whether T[g .. g + k + 1) is free of 'N' (code 4), and
    mix64(min(F, R)) of it (meaningless where not valid)."""
    codes = np.asarray(codes, dtype=np.uint8)
    n = k + 1
    W = codes.size - n + 1
    if W <= 0:
        return np.zeros(0, dtype=bool), np.zeros(0, dtype=np.uint64)
    isn = np.concatenate([[0], np.cumsum(codes > 3)])
    valid = (isn[n:n + W] - isn[:W]) == 0
    h = np.array(letter_hashes(), dtype=np.uint64)
    c = np.minimum(codes, 3)           # an 'N' reads as any letter: its windows are not valid
    fwd, rev = h[c], h[3 - c]
    F = np.zeros(W, dtype=np.uint64)
    R = np.zeros(W, dtype=np.uint64)
    for t in range(n):
        F ^= rotl(fwd[t:t + W], n - 1 - t)
        R ^= rotl(rev[t:t + W], t)
    return valid, mix64(np.minimum(F, R))


def sketch_reference(codes, k):
    """(registers uint8[16384], contributing windows) of the text with these position codes (0..3 = ACGT, 4 = 'N' and separators)."""
    reg = np.zeros(M, dtype=np.uint8)
    valid, x = window_hashes(codes, k)
    x = x[valid]
    if x.size == 0:
        return reg, 0
    idx = (x >> U(64 - P)).astype(np.int64)
    u = x & U((1 << (64 - P)) - 1)     # v = x << 14 is u shifted up: clz64(v) = 50 - bit_length(u); exact in float64 (u < 2^53)
    bit_length = np.frexp(u.astype(np.float64))[1]
    rank = np.where(u == 0, 64 - P + 1, 64 - P + 1 - bit_length).astype(np.uint8)
    np.maximum.at(reg, idx, rank)
    return reg, int(x.size)


def hll_estimate(reg):
    reg = np.asarray(reg, dtype=np.int64)
    m = reg.size
    zeros = int((reg == 0).sum())
    if zeros == m:
        return 0.0
    alpha = 0.7213 / (1 + 1.079 / m)
    e = alpha * m * m / float(np.sum(np.ldexp(1.0, -reg)))
    if e <= 2.5 * m and zeros > 0:
        return m * float(np.log(m / zeros))
    return e


def exact_distinct(codes, k):
    """The number of distinct canonical (k+1)-mers: a Python set of min(window, reverse complement) over the N-free windows."""
    codes = np.asarray(codes, dtype=np.uint8)
    n = k + 1
    text = bytes(np.frombuffer(b"ACGTN", dtype=np.uint8)[np.minimum(codes, 4)])
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    seen = set()
    for piece_start, piece in _pieces(text):
        rc = piece.translate(comp)[::-1]
        L = len(piece)
        for g in range(L - n + 1):
            a, b = piece[g:g + n], rc[L - g - n:L - g]
            seen.add(a if a <= b else b)
    return len(seen)


def _pieces(text):
    pos = 0
    for piece in text.split(b"N"):
        if piece:
            yield pos, piece
        pos += len(piece) + 1


def revcomp_codes(codes):
    c = np.asarray(codes, dtype=np.uint8)[::-1].copy()
    c[c < 4] = 3 - c[c < 4]
    return c


def fasta_codes(path):
    """Position codes of the global text N rec0 N rec1 N ... of a FASTA file (any letter other than ACGT, either case, is 'N')."""
    lut = np.full(256, 4, dtype=np.uint8)
    for i, ch in enumerate(b"ACGT"):
        lut[ch] = i
        lut[ch + 32] = i
    recs, cur = [], None
    with open(path, "rb") as f:
        for line in f:
            if line[:1] == b">":
                cur = []
                recs.append(cur)
            elif cur is not None:
                cur.append(line.strip())
    parts = [np.array([4], dtype=np.uint8)]
    for r in recs:
        parts += [lut[np.frombuffer(b"".join(r), dtype=np.uint8)], np.array([4], dtype=np.uint8)]
    return np.concatenate(parts)
