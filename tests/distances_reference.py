"""The genome distance matrices by their definition, from the text of a gfa1 graph -- the oracle of test_distances_cpu.py and
test_gpu_distances.py.  Nothing here goes through the project's own code for the matrices: the input is what the serial
`graphdump -f gfa1` prints (pinned to the reference's bytes by tests/golden/graphdump.json), read by colors_reference.Gfa1 / table
into the S x C 0/1 matrix P, and
    weight[r]  = len(body of row r) - k          the (k+1)-mers the segment spells
    segments   = P.T @ P
    edges      = P.T @ (P * weight[:, None])     both in int64
as include/twopaco_hip.h's tpc_segments_distances_* group defines them.  The TSV and the PHYLIP text are rendered here."""
import numpy as np

import colors_reference as R


def matrices(t, k):
    """(segments, edges): int64 [C, C] of a colors_reference.table."""
    p = t["presence"].astype(np.int64)
    weight = t["length"].astype(np.int64) - k
    assert (weight >= 0).all()
    return p.T @ p, p.T @ (p * weight[:, None])


def render(segments, edges, by, k, labels, rows):
    c = len(labels)
    assert segments.shape == (c, c) and edges.shape == (c, c)
    lines = ["#twopaco-distances\t1\tby=%s\tk=%d\tcolors=%d\tsegments=%d" % (by, k, c, rows)]
    lines += ["#color\t%d\t%s" % (i, label) for i, label in enumerate(labels)]
    lines += ["#self\t%d\t%d\t%d" % (i, segments[i, i], edges[i, i]) for i in range(c)]
    lines += ["%d\t%d\t%d\t%d" % (i, j, segments[i, j], edges[i, j]) for i in range(c) for j in range(i + 1, c)]
    return ("\n".join(lines) + "\n").encode()


def phylip(edges, labels):
    """The relaxed PHYLIP square matrix of the Jaccard distances over edges: one correctly rounded division per value."""
    c = len(labels)
    lines = ["%d" % c]
    for i in range(c):
        name = "".join("_" if ch <= 0x20 else chr(ch) for ch in labels[i].encode("latin-1"))
        row = []
        for j in range(c):
            shared = int(edges[i, j])
            u = int(edges[i, i]) + int(edges[j, j]) - shared
            row.append(" %.6f" % (0.0 if i == j or u == 0 else (u - shared) / u))
        lines.append(name + "".join(row))
    return ("\n".join(lines) + "\n").encode()


def tsv(gfa1_text, by, k, files=None):
    """(TSV bytes, PHYLIP bytes, segments, edges, the colour table) of a gfa1 text."""
    g = R.Gfa1(gfa1_text)
    color_of_seq, labels = R.color_map(g, by, files)
    t = R.table(g, color_of_seq, len(labels))
    segments, edges = matrices(t, k)
    return render(segments, edges, by, k, labels, len(t["name"])), phylip(edges, labels), segments, edges, t


def parse(text):
    """(segments, edges) int64 [C, C] read back from a TSV, symmetric: for identities that need the matrix, not its bytes."""
    lines = text.decode().split("\n")
    c = int([f for f in lines[0].split("\t") if f.startswith("colors=")][0][7:])
    segments, edges = np.zeros((c, c), dtype=np.int64), np.zeros((c, c), dtype=np.int64)
    for line in lines[1:]:
        f = line.split("\t")
        if f[0] == "#self":
            segments[int(f[1]), int(f[1])], edges[int(f[1]), int(f[1])] = int(f[2]), int(f[3])
        elif line and line[0] != "#":
            i, j = int(f[0]), int(f[1])
            segments[i, j] = segments[j, i] = int(f[2])
            edges[i, j] = edges[j, i] = int(f[3])
    return segments, edges


# ---------------------------------------------------------------------------------------------- generated inputs
def twins_fasta(path, n=300, seed=20261018):
    """Three records: one random sequence twice (two identical colours by sequence: distance 0) and another one once."""
    rng = np.random.default_rng(seed)
    a = "".join("ACGT"[c] for c in rng.integers(0, 4, n))
    b = "".join("ACGT"[c] for c in rng.integers(0, 4, n))
    with open(path, "w") as f:
        for name, s in (("first", a), ("twin", a), ("other", b)):
            f.write(">%s\n" % name)
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + "\n")
    return path


def long_pair_fasta(path, n=(3 << 16) + 4321, seed=20261019):
    """One unique random sequence of more than 2^17 + 2^16 bases, twice, in two records: by sequence two colours share one segment
    whose weight has the bits 16 and 17 set."""
    rng = np.random.default_rng(seed)
    s = "".join("ACGT"[c] for c in rng.integers(0, 4, n))
    with open(path, "w") as f:
        for name in ("one", "two"):
            f.write(">%s\n" % name)
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + "\n")
    return path
