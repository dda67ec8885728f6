"""Shared helpers of the test-suite."""
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


# full-size synthetic workloads: minutes of work and GiBs of filter each -- dedicated tests, not the parametrised sweeps
BIG = ("m1_full", "m2_full", "m2_s05_f38", "m3_f38", "m2_x15", "m2r_full", "m2r2_full")


def golden_cases():
    with open(os.path.join(GOLDEN, "cases.json")) as f:
        return json.load(f)


def case_files(case, tmpdir):
    """FASTA paths of a golden case (synthetic workloads are regenerated into tmpdir)."""
    if case.get("fasta"):
        return [os.path.join(GOLDEN, case["fasta"])]
    from twopaco_amd import synth
    s = case["synth"]
    recs, p = synth.workload(s["workload"], seed=s["seed"], scale=s["scale"])
    return synth.fasta_files(recs, p, tmpdir, prefix=case["name"] + "_")  # one record per file, or a genome's contigs per file (m2r)


def sha256_file(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 20), b""):
            h.update(blk)
    return h.hexdigest()


def parse_log(log):
    import re
    rounds = []
    for m in re.finditer(r"Round (\d+), (\d+):(\d+)", log):
        rounds.append({"low": int(m.group(2)), "high": int(m.group(3))})
    for key, pat in [("true", r"True junctions count = (\d+)"), ("false", r"False junctions count = (\d+)"),
                     ("table", r"Hash table size = (\d+)"), ("marks", r"Candidate marks count = (\d+)")]:
        for i, m in enumerate(re.finditer(pat, log)):
            rounds[i][key] = int(m.group(1))
    tm = re.search(r"True marks count: (\d+)", log)
    return {"rounds": rounds, "true_marks": int(tm.group(1)) if tm else None}


def text_codes(bases, nmask, length):
    g = np.arange(length, dtype=np.uint64)
    codes = ((bases[g >> np.uint64(5)] >> (np.uint64(2) * (g & np.uint64(31)))) & np.uint64(3)).astype(np.uint8)
    isn = ((nmask[g >> np.uint64(5)] >> (g & np.uint64(31)).astype(np.uint32)) & np.uint32(1)).astype(bool)
    codes[isn] = 4
    return codes


_BAND = {}


def band_case():
    """A random text of 16 M positions (almost every k-mer distinct) under a 2^30-bit filter of 16384 slices of 2^16 bits: each of two
    ranks exports about 2400 distinct bits per slice -- the list density at which the long-lived export used to claim more than the
    block size tpc_combine_info promised.  The FASTA file and the oracle's results are made once per test session."""
    if _BAND:
        return _BAND
    import tempfile

    from oracle import oracle as O
    k, L, q, seed = 25, 30, 5, 7
    d = tempfile.mkdtemp(prefix="tpc_band_")
    path = os.path.join(d, "band.fa")
    rng = np.random.default_rng(2400)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(path, "wb") as f:
        for r in range(4):
            lines = letters[rng.integers(0, 4, 4000000)].reshape(-1, 80)
            f.write(b">band%d\n" % r)
            f.write(np.hstack([lines, np.full((lines.shape[0], 1), ord("\n"), dtype=np.uint8)]).tobytes())
    o = O.Oracle(k, L, q, O.seed_table(seed, q, L))
    o.add_fasta(path)
    o.fill_only()
    marks = o.check_only()
    filt, mask = o.filter.copy(), o.round_mask.copy()
    o.enumerate(rounds=1)
    seqs, pos, ids = o.records
    start = np.asarray(o.rec_start, dtype=np.int64)
    want = sorted((int(start[s] + p), int(i)) for s, p, i in zip(seqs.tolist(), pos.tolist(), ids.tolist()) if abs(i) <= len(o.keys))
    o.write_bin(os.path.join(d, "oracle.bin"))
    with open(os.path.join(d, "oracle.bin"), "rb") as f:
        out = f.read()
    _BAND.update(files=[path], k=k, L=L, q=q, seed=seed, marks=marks, filter=filt, round_mask=mask, junctions=len(o.keys), want=want, bin=out)
    o.close()
    return _BAND


# ---------------------------------------------------------------------------------------------- periodic windows: the definition
PER_MAXP = 63      # periods 1 .. 63 (csrc/tpc_internal.h: TPC_PER_MAXP)
PER_TILE = 16384   # positions of a 512-word tile: its first PER_MAXP positions never copy


def periodic_reference(codes, k, lo=0, hi=None):
    """The periodic-window masks of a text by their definition (csrc/tpc_qpartition.hip: k_periodic_build), in numpy.

    codes: the position codes of the global text (0..3, 4 = N and every separator).  A context that holds only the characters
    [lo, hi) sees every other one as 4; so does everything before the text and behind it.  With
        eq_p[j] = T[j] < 4 and T[j - p] < 4 and T[j] == T[j - p]          p = 1 .. 63
    ins[i]  = some p with eq_p true on all of i .. i + k       (the k + 1 characters of the out-edge repeat: the insert adds nothing)
    qs[i]   = some p with eq_p true on all of i - 1 .. i + k   (the k + 2 characters of the vertex repeat: it takes the verdict of
              position i - p), and i mod 16384 >= 63 (a copy never leaves its tile); dist[i] = the smallest such p, 0 where qs is clear.
    Returns (qs bool, dist uint8, ins bool), one entry per position."""
    T = np.array(codes, dtype=np.uint8)
    n = T.size
    hi = n if hi is None else min(int(hi), n)
    T[:max(0, int(lo))] = 4
    T[hi:] = 4
    idx = np.arange(n, dtype=np.int64)
    ins = np.zeros(n, dtype=bool)
    qs = np.zeros(n, dtype=bool)
    dist = np.zeros(n, dtype=np.uint8)
    if n <= k:
        return qs, dist, ins
    for p in range(PER_MAXP, 0, -1):   # descending: the smallest period is written last
        eq = np.zeros(n, dtype=bool)
        eq[p:] = (T[p:] == T[:n - p]) & (T[p:] < 4)
        # run[j] = length of the stretch of true eq that ends at j (0 where eq[j] is false)
        run = idx - np.maximum.accumulate(np.where(eq, -1, idx))
        end = run[k:]                   # end[i] = run at the window's last character i + k; windows past the text's end hold a 4
        ins[:n - k] |= end >= k + 1
        two = end >= k + 2
        qs[:n - k] |= two
        dist[:n - k][two] = p
    tile = (idx % PER_TILE) >= PER_MAXP
    qs &= tile
    dist[~qs] = 0
    return qs, dist, ins


def periodic_reference_bruteforce(codes, k, lo=0, hi=None):
    """The same definition by comparing windows of the text as strings, one position and one period at a time (the check of
    periodic_reference; a few thousand positions at most)."""
    n = len(codes)
    hi = n if hi is None else min(int(hi), n)
    s = "".join("ACGT"[c] if c < 4 and lo <= j < hi else "N" for j, c in enumerate(np.asarray(codes).tolist()))
    pad = "N" * (PER_MAXP + 1)
    s = pad + s + "N" * (k + 2)
    qs = np.zeros(n, dtype=bool)
    dist = np.zeros(n, dtype=np.uint8)
    ins = np.zeros(n, dtype=bool)
    for i in range(n):
        a = i + len(pad)
        edge, vertex = s[a:a + k + 1], s[a - 1:a + k + 1]
        for p in range(1, PER_MAXP + 1):
            if "N" not in edge and edge == s[a - p:a - p + k + 1]:
                ins[i] = True
            if "N" not in vertex and vertex == s[a - 1 - p:a - p + k + 1] and i % PER_TILE >= PER_MAXP and not qs[i]:
                qs[i] = True
                dist[i] = p
    return qs, dist, ins


def periodic_copy_reference(marks, qs, dist):
    """k_periodic_copy's result, one position after the other: for i ascending, where qs[i], mark[i] = mark[i - dist[i]]."""
    m = np.array(marks, dtype=bool)
    d = dist.astype(np.int64)
    for i in np.nonzero(qs)[0].tolist():
        m[i] = m[i - d[i]]
    return m


def bits_of_words(words, n):
    """One bool per position from a mask of 32-bit words (bit b of word w = position 32 w + b)."""
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")[:n].astype(bool)


def words_of_bits(bits, n_words):
    b = np.zeros(n_words * 32, dtype=np.uint8)
    b[:len(bits)] = np.asarray(bits, dtype=np.uint8)
    return np.packbits(b, bitorder="little").view("<u4").astype(np.uint32)
