"""The segment colour table by its definition, from the text of a gfa1 graph -- the oracle of test_colors_cpu.py and
test_gpu_colors.py.  Nothing here goes through the project's own colour code: the input is what the serial
`graphdump -f gfa1` prints (pinned to the reference's bytes by tests/golden/graphdump.json),
    S <sequence> * UR:Z:<file>      one per input sequence, in order: sequence -> file
    S <segment> <body>              a row, in this order; length = len(body)
    C <segment> <strand> <sequence> + <pos>   one occurrence of the row <segment> in <sequence>
and the output is the arrays and the TSV of include/twopaco_hip.h's tpc_segments_colors_* group."""
import hashlib
import json
import os
import subprocess

import numpy as np

from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPHDUMP = os.path.join(ROOT, "twopaco_amd", "bin", "graphdump")
TWOPACO = os.path.join(ROOT, "twopaco_amd", "bin", "twopaco")
FRESH = 1 << 34   # 'N'-named segments
GFA1_VECTORS = [v for v in json.load(open(os.path.join(GOLDEN, "graphdump.json"))) if v["case"] != "cli" and v["args"][2] == "gfa1"]
GOOD_VECTORS = [v for v in GFA1_VECTORS if v["rc"] == 0]
# the real reference's graphdump on tracts.fa (the hot row), recorded the same way: graphdump.json has no vector of that input
TRACTS_VECTORS = json.load(open(os.path.join(GOLDEN, "graphdump_tracts.json")))


def vector_id(v):
    return v["case"] + ("_prefix" if "--prefix" in v["args"] else "")


def vector_of(case):
    return [v for v in GFA1_VECTORS if v["case"] == case and "--prefix" not in v["args"]][0]


def colors_args(v):
    """The arguments of a gfa1 vector without its `-f gfa1`."""
    a = list(v["args"])
    i = a.index("-f")
    return a[:i] + a[i + 2:]


def run_graphdump(args, cwd=GOLDEN):
    return subprocess.run([GRAPHDUMP] + list(args), cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


_GFA1 = {}


def golden_gfa1(v):
    """The serial gfa1 of a golden vector, checked against the reference's sha256; made once per session."""
    key = vector_id(v)
    if key not in _GFA1:
        r = run_graphdump(v["args"])
        assert r.returncode == 0 and r.stderr == b"", r.stderr
        assert len(r.stdout) == v["stdout_bytes"] and hashlib.sha256(r.stdout).hexdigest() == v["stdout_sha256"], key
        _GFA1[key] = r.stdout
    return _GFA1[key]


def case_vector(case):
    """The gfa1 vector of the real reference for a golden CASE (tests/golden/cases.json), without --prefix."""
    return [v for v in GFA1_VECTORS + TRACTS_VECTORS if v["case"] == case["name"] and "--prefix" not in v["args"]][0]


class Gfa1:
    """What the colour table needs of a gfa1 text."""

    def __init__(self, text):
        self.seq_name, self.seq_file = [], []
        self.row_name, self.row_length = [], []
        occ = []          # (segment name, forward, sequence name)
        for line in text.decode().split("\n"):
            f = line.split("\t")
            if f[0] == "S" and len(f) == 4 and f[2] == "*" and f[3].startswith("UR:Z:"):
                self.seq_name.append(f[1])
                self.seq_file.append(f[3][5:])
            elif f[0] == "S":
                assert len(f) == 3, line
                self.row_name.append(int(f[1]))
                self.row_length.append(len(f[2]))
            elif f[0] == "C":
                assert len(f) == 6 and f[2] in "+-" and f[4] == "+", line
                occ.append((int(f[1]), f[2] == "+", f[3]))
        assert len(set(self.seq_name)) == len(self.seq_name), "the oracle tells sequences apart by their names"
        index = {n: i for i, n in enumerate(self.seq_name)}
        self.occ_name = np.array([o[0] for o in occ], dtype=np.int64)
        self.occ_forward = np.array([o[1] for o in occ], dtype=bool)
        self.occ_seq = np.array([index[o[2]] for o in occ], dtype=np.int64)
        assert len(set(self.row_name)) == len(self.row_name)


def color_map(g, by, files=None):
    """(color_of_seq, labels): one colour per file as given, or per sequence."""
    if by == "sequence":
        return list(range(len(g.seq_name))), ["%d\t%s" % (s + 1, f) for s, f in enumerate(g.seq_file)]
    files = list(dict.fromkeys(g.seq_file)) if files is None else list(files)
    return [files.index(f) for f in g.seq_file], files


def table(g, color_of_seq, n_colors):
    """dict of arrays, one entry per row: name, length, occurrences, forward, n_colors, presence (bool [rows, n_colors]);
    and hist_segments / hist_bases [n_colors + 1]."""
    row_of = {n: r for r, n in enumerate(g.row_name)}
    rows = len(g.row_name)
    occ = np.zeros(rows, dtype=np.int64)
    fwd = np.zeros(rows, dtype=np.int64)
    presence = np.zeros((rows, n_colors), dtype=bool)
    color = np.asarray(color_of_seq, dtype=np.int64)
    for name, forward, seq in zip(g.occ_name.tolist(), g.occ_forward.tolist(), g.occ_seq.tolist()):
        r = row_of[name]
        occ[r] += 1
        fwd[r] += forward
        presence[r, color[seq]] = True
    ncol = presence.sum(axis=1).astype(np.int64)
    length = np.array(g.row_length, dtype=np.int64)
    hist_segments = np.bincount(ncol, minlength=n_colors + 1).astype(np.int64)
    hist_bases = np.bincount(ncol, weights=length, minlength=n_colors + 1).astype(np.int64)
    return {"name": np.array(g.row_name, dtype=np.int64), "length": length, "occurrences": occ, "forward": fwd, "n_colors": ncol, "presence": presence,
            "hist_segments": hist_segments, "hist_bases": hist_bases, "events": len(g.occ_name), "colors": n_colors}


def presence_words(presence):
    """bool [rows, C] -> uint32 [rows, ceil(C / 32)]: bit c % 32 of word c // 32."""
    rows, c = presence.shape
    w = (c + 31) // 32
    bits = np.zeros((rows, w * 32), dtype=np.uint8)
    bits[:, :c] = presence
    return np.packbits(bits, axis=1, bitorder="little").view("<u4").reshape(rows, w).astype(np.uint32)


def hex_of(bits):
    """ceil(C / 4) lower-case hex digits: digit j from the left holds colours 4j .. 4j + 3, colour 4j + b has the value 1 << b."""
    out = []
    for j in range(0, len(bits), 4):
        out.append("0123456789abcdef"[sum(1 << b for b, v in enumerate(bits[j:j + 4]) if v)])
    return "".join(out)


def render(t, by, k, labels):
    lines = ["#twopaco-colors\t1\tby=%s\tk=%d\tcolors=%d\tsegments=%d\tevents=%d" % (by, k, t["colors"], len(t["name"]), t["events"])]
    lines += ["#color\t%d\t%s" % (c, label) for c, label in enumerate(labels)]
    for r in range(len(t["name"])):
        lines.append("%d\t%d\t%d\t%d\t%d\t%s" % (t["name"][r], t["length"][r], t["occurrences"][r], t["forward"][r], t["n_colors"][r], hex_of(t["presence"][r].tolist())))
    lines += ["#hist\t%d\t%d\t%d" % (n, t["hist_segments"][n], t["hist_bases"][n]) for n in range(1, t["colors"] + 1) if t["hist_segments"][n]]
    return ("\n".join(lines) + "\n").encode()


def tsv(gfa1_text, by, k, files=None):
    g = Gfa1(gfa1_text)
    color_of_seq, labels = color_map(g, by, files)
    t = table(g, color_of_seq, len(labels))
    return render(t, by, k, labels), t


# ---------------------------------------------------------------------------------------------- word boundaries of presence
BOUNDARY_COLORS = (1, 31, 32, 33, 64, 65)
BOUNDARY_K, BOUNDARY_L, BOUNDARY_Q, BOUNDARY_SEED = 11, 20, 5, 11


def boundary_records():
    """65 records: overlapping windows (2000 bp, starts below 400) of one random 3-kbp base, each with three substitutions
    outside the stretch [1000, 1200) every window holds unchanged -- so one segment lies in every record, whatever the cut --
    records 3 and 40 reverse-complemented, record 7 with a run of N."""
    rng = np.random.default_rng(20261017)
    base = rng.integers(0, 4, 3000)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
    recs = []
    for r in range(65):
        start = int(rng.integers(0, 400))
        w = base[start:start + 2000].copy()
        for _ in range(3):
            p = int(rng.integers(20, 1980))
            if 1000 - 20 <= start + p < 1200 + 20:
                continue
            w[p] = (w[p] + 1 + int(rng.integers(0, 3))) % 4
        s = "".join("ACGT"[c] for c in w)
        if r == 7:
            at = 1500 - start
            s = s[:at] + "N" * 9 + s[at + 9:]
        if r in (3, 40):
            s = "".join(comp[c] for c in reversed(s))
        recs.append(s)
    return recs


def boundary_fasta(path, n_records):
    recs = boundary_records()[:n_records]
    with open(path, "w") as f:
        for r, s in enumerate(recs):
            f.write(">w%d\n" % r)
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + "\n")
    return path
