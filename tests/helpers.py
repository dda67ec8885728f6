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
