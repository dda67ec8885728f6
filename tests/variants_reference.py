"""The variants by their definition (include/twopaco_hip.h, the tpc_segments_variants_* group) -- the oracle of test_variants_cpu.py and
test_gpu_variants.py.  Nothing here goes through the project's own variant code.  Two statements:

  Variants      PART 1, from the text the serial `graphdump -f gfa1` prints (pinned to the reference's bytes by
                tests/golden/graphdump.json), the lengths and, for the VCF, the letters of the FASTA records.  The events are read as
                anchors_reference.Anchors reads them, the superbubble rows come from superbubbles_reference.Superbubbles (the set
                definition) and the colours from colors_reference.  Plain loops over the events; an allele is kept as the TUPLE of the
                sides a traversal reads between entrance and exit, never as a mask: that the set of sides says as much as the tuple is
                asserted, not assumed.  The TSV and the VCF are rendered here with code of its own.
  check_files   PART 2, which needs no graph: from the program's TSV, its VCF and the FASTA alone -- REF equals the reference's letters
                at POS; every allele's span, spelled from the FASTA (reverse-complemented on '-'), begins and ends with its site's two
                k-mers; the alleles of a site without an N spell pairwise different strings; equal edges imply edges >= k + 1; for every sample with one
                allele in GT, left flank + allele + right flank occurs in one of that colour's sequences or their reverse complements."""
import numpy as np

import anchors_reference as A
import colors_reference as C
import superbubbles_reference as S
from anchors_reference import fasta_of, k_of, lengths_of  # noqa: F401
from superbubbles_reference import (GFA1_VECTORS, GOOD_VECTORS, GRAPHDUMP, TWOPACO, SB_HUB, case_vector, SB_K, SB_L, SB_Q, SB_RECORDS, SB_SEED, golden_gfa1, golden_superbubbles,  # noqa: F401
                                    oracle_stream, plain, read_fasta, rev, reverse_complement, run_graphdump, simple_rows, superbubble_fasta, superbubble_records,
                                    superbubbles_args, vector_id, vector_of)

NONE = 0xFFFFFFFF
variants_args = superbubbles_args   # the arguments of a gfa1 vector without its `-f gfa1`


def label_of(label):
    """A colour's label as a sample name: every byte <= ' ' an underscore (the PHYLIP matrix's labels)."""
    return "".join("_" if ord(ch) <= 32 else ch for ch in label)


class Variants:
    """ref: the reference colour, None = none.  lengths: the letters of every input sequence, in input order; records: the letters
    themselves, for the VCF.  sb: the Superbubbles of the same text, k, by and max_inside, if the caller has them."""

    def __init__(self, gfa1_text, k, lengths, by="file", ref=None, max_inside=S.DEFAULT_MAX_INSIDE, records=None, sb=None, color_of_seq=None, labels=None):
        a = A.Anchors(gfa1_text, k, lengths, by, 0, color_of_seq=color_of_seq, labels=labels)
        self.k, self.by, self.ref, self.max_inside, self.records = k, by, ref, max_inside, records
        self.seq_name, self.seq_length, self.color_of_seq, self.labels, self.n_colors = a.seq_name, a.seq_length, a.color_of_seq, a.labels, a.n_colors
        self.begin, self.end, self.seq = a.begin, a.end, a.seq
        assert ref is None or 0 <= ref < self.n_colors
        self.sb = sb = S.Superbubbles(gfa1_text, k, by, max_inside=max_inside, color_of_seq=color_of_seq) if sb is None else sb
        assert sb.max_inside == max_inside and sb.k == k
        row_of = {n: r for r, n in enumerate(sb.g.row_name)}
        self.segments = len(sb.g.row_name)
        self.side = side = [row_of[n] * 2 + (0 if fw else 1) for n, fw in zip(a.name, a.forward)]
        n = len(side)
        row_of_entrance = {}
        for b, r in enumerate(sb.rows):
            assert r["entrance"] not in row_of_entrance, "a side is the entrance of at most one row"
            row_of_entrance[r["entrance"]] = b
        self.strays = 0
        self.traversals = []     # (start, last, d, row, the tuple of the sides read inside, edges)
        for e in range(n):
            for d in (0, 1):
                b = row_of_entrance.get(side[e] ^ d)
                if b is None:
                    continue
                r = sb.rows[b]
                inside, path, x = set(r["members"]), [], e
                while True:
                    x += -1 if d else 1
                    if x < 0 or x >= n or self.seq[x] != self.seq[e]:
                        break                                   # the sequence ends inside the superbubble
                    read = side[x] ^ d
                    if read == r["exit"]:
                        lo, hi = min(e, x), max(e, x)
                        edges = abs(self.begin[hi] - self.end[lo])
                        assert len(path) <= r["inside"] <= max_inside and len(set(path)) == len(path)
                        self.traversals.append((e, x, d, b, tuple(path), edges))
                        break
                    if read not in inside:
                        self.strays += 1
                        break
                    path.append(read)
        # the alleles: the traversals of one row that read the same sides
        groups = {}
        for t, (_, _, _, b, path, _) in enumerate(self.traversals):
            groups.setdefault((b, path), []).append(t)
        by_set = {}
        for b, path in groups:
            assert by_set.setdefault((b, frozenset(path)), path) == path, "the sides of a path determine the path"
        self.alleles = sorted(((b, ts[0], path, ts) for (b, path), ts in groups.items()))   # ascending by (row, first)
        self.allele_of = {}
        for i, (b, _, path, ts) in enumerate(self.alleles):
            for t in ts:
                self.allele_of[t] = i
        nb = len(sb.rows)
        self.allele_offset = [0] * (nb + 1)
        for b, _, _, _ in self.alleles:
            self.allele_offset[b + 1] += 1
        for b in range(nb):
            self.allele_offset[b + 1] += self.allele_offset[b]
        self.site_traversals = [0] * nb
        self.ref_traversal = [None] * nb        # the smallest traversal of the reference colour
        self.ref_traversals = [0] * nb
        for t, (e, _, _, b, _, _) in enumerate(self.traversals):
            self.site_traversals[b] += 1
            if ref is not None and self.color_of(t) == ref:
                if self.ref_traversals[b] == 0:
                    self.ref_traversal[b] = t
                self.ref_traversals[b] += 1
        self.ref_allele = [NONE if t is None else self.allele_of[t] for t in self.ref_traversal]

    def color_of(self, t):
        return self.color_of_seq[self.seq[self.traversals[t][0]]]

    def sites(self):
        return sum(1 for b in range(len(self.sb.rows)) if self.allele_offset[b + 1] > self.allele_offset[b])

    def presence(self, i):
        p = [False] * self.n_colors
        for t in self.alleles[i][3]:
            p[self.color_of(t)] = True
        return p

    def mask(self, b, path):
        members = self.sb.rows[b]["members"]
        return sum(1 << members.index(u) for u in path)

    def hist(self):
        n = [self.allele_offset[b + 1] - self.allele_offset[b] for b in range(len(self.sb.rows))]
        h = [0] * (max(n + [0]) + 1)
        for x in n:
            if x:
                h[x] += 1
        return h

    def span(self, t):
        """(sequence, begin, end in bases, strand) of traversal t."""
        e, x, d, _, _, _ = self.traversals[t]
        lo, hi = min(e, x), max(e, x)
        return self.seq[e], self.end[lo], self.begin[hi] + self.k, "-" if d else "+"

    def check(self):
        """The consequences the definition promises, on the oracle's own results."""
        assert self.strays == 0
        for i, (b, first, path, ts) in enumerate(self.alleles):
            assert len({self.traversals[t][5] for t in ts}) == 1 and first == min(ts)
        for b, r in enumerate(self.sb.rows):
            n = self.allele_offset[b + 1] - self.allele_offset[b]
            assert n <= int(r["paths"])
            assert sum(len(self.alleles[i][3]) for i in range(self.allele_offset[b], self.allele_offset[b + 1])) == self.site_traversals[b]

    # ------------------------------------------------------------------------------------------ what the C-ABI fetches
    def arrays(self):
        t = self.traversals
        u32, u64 = np.uint32, np.uint64
        trav = [np.array([x[i] for x in t], dtype=u32) for i in (0, 1, 2, 3, 5)] + [np.array([self.mask(x[3], x[4]) for x in t], dtype=u64)]
        al = self.alleles
        presence = np.array([self.presence(i) for i in range(len(al))], dtype=bool).reshape(len(al), self.n_colors)
        alle = [np.array([a[0] for a in al], dtype=u32), np.array([len(a[2]) for a in al], dtype=u32), np.array([t[a[1]][5] for a in al], dtype=u32),
                np.array([a[1] for a in al], dtype=u32), presence.sum(axis=1).astype(u32), np.array([self.mask(a[0], a[2]) for a in al], dtype=u64),
                np.array([len(a[3]) for a in al], dtype=u64)]
        sites = [np.array(self.allele_offset, dtype=u32), np.array(self.site_traversals, dtype=u64), np.array(self.ref_allele, dtype=u32), np.array(self.ref_traversals, dtype=u64)]
        return trav, alle, C.presence_words(presence), sites, np.array(self.hist(), dtype=u64)

    # ------------------------------------------------------------------------------------------ the two files
    def tsv(self):
        sb = self.sb
        out = ["#twopaco-variants\t1\tby=%s\tk=%d\tcolors=%d\tsegments=%d\tsuperbubbles=%d\tmax_inside=%d\tref=%s\tsites=%d\talleles=%d\ttraversals=%d" % (
            self.by, self.k, self.n_colors, self.segments, len(sb.rows), self.max_inside, "none" if self.ref is None else str(self.ref), self.sites(), len(self.alleles),
            len(self.traversals))]
        out += ["#color\t%d\t%s" % (c, label) for c, label in enumerate(self.labels)]
        out += ["#sequence\t%d\t%d\t%d\t%s" % (s, self.color_of_seq[s], self.seq_length[s], self.seq_name[s]) for s in range(len(self.seq_name))]
        out += ["#alleles\t%d\t%d" % (n, c) for n, c in enumerate(self.hist()) if c]
        for i, (b, first, path, ts) in enumerate(self.alleles):
            r = sb.rows[b]
            p = self.presence(i)
            s, begin, end, strand = self.span(first)
            out.append("%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%s\t%d" % (b, sb.spelled(r["entrance"]), sb.spelled(r["exit"]), i - self.allele_offset[b], len(ts), len(path),
                                                                         self.traversals[first][5], sum(p), C.hex_of(p), s, begin, end, strand,
                                                                         1 if self.ref is not None and self.ref_allele[b] == i else 0))
        return ("\n".join(out) + "\n").encode()

    def spelled(self, t):
        """The letters of traversal t in the superbubble's orientation, entrance to exit."""
        s, begin, end, strand = self.span(t)
        letters = plain(self.records[s][begin:end])
        return letters if strand == "+" else reverse_complement(letters)

    def records_of_vcf(self):
        """(sequence, pos, site, ref text, [alt texts], [record-local allele -> index among all alleles])."""
        k, got = self.k, []
        for b in range(len(self.sb.rows)):
            mine = list(range(self.allele_offset[b], self.allele_offset[b + 1]))
            rt = self.ref_traversal[b]
            if rt is None or len(mine) < 2:
                continue
            local = [self.ref_allele[b]] + [i for i in mine if i != self.ref_allele[b]]
            edges = [self.traversals[self.alleles[i][1]][5] for i in local]
            flip = self.traversals[rt][2] == 1
            # all edges equal: then they are k + 1 at least in a graph of all (k+1)-mers (check_files asserts it); under an abundance cut
            # smaller ones exist and take the anchored form
            equal = len(set(edges)) == 1 and edges[0] >= k + 1
            texts = []
            for j, i in enumerate(local):
                letters = self.spelled(rt if j == 0 else self.alleles[i][1])
                letters = reverse_complement(letters) if flip else letters      # to the reference traversal's stored orientation
                assert len(letters) == edges[j] + k
                if equal:
                    texts.append(letters[k:edges[j]])
                else:
                    texts.append(letters[k - 1:edges[j] + k - min(k, min(edges))])
            s, begin, _, _ = self.span(rt)
            pos = begin + k + 1 if equal else begin + k
            got.append((s, pos, b, texts[0], texts[1:], local))
        return sorted(got, key=lambda r: r[:3])

    def vcf(self):
        assert self.ref is not None and self.records is not None
        out = ["##fileformat=VCFv4.2", "##source=twopaco variants k=%d by=%s ref=%d max_inside=%d" % (self.k, self.by, self.ref, self.max_inside)]
        out += ["##contig=<ID=%s,length=%d>" % (self.seq_name[s], self.seq_length[s]) for s in range(len(self.seq_name)) if self.color_of_seq[s] == self.ref]
        out += ['##INFO=<ID=AC,Number=A,Type=Integer,Description="Traversals of each ALT allele">', '##INFO=<ID=AN,Number=1,Type=Integer,Description="Traversals of the site">',
                '##INFO=<ID=NS,Number=1,Type=Integer,Description="Colours with a traversal of the site">', '##INFO=<ID=INS,Number=1,Type=Integer,Description="Sides inside the superbubble">',
                '##FORMAT=<ID=GT,Number=1,Type=String,Description="Alleles the colour walks">']
        out.append("\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + [label_of(x) for x in self.labels]))
        for s, pos, b, ref_text, alts, local in self.records_of_vcf():
            held = [self.presence(i) for i in local]
            ns = sum(any(h[c] for h in held) for c in range(self.n_colors))
            info = "AC=%s;AN=%d;NS=%d;INS=%d" % (",".join(str(len(self.alleles[i][3])) for i in local[1:]), self.site_traversals[b], ns, self.sb.rows[b]["inside"])
            gts = ["/".join(str(j) for j, h in enumerate(held) if h[c]) or "." for c in range(self.n_colors)]
            out.append("\t".join([self.seq_name[s], str(pos), "sb%d" % b, ref_text, ",".join(alts), ".", ".", info, "GT"] + gts))
        return ("\n".join(out) + "\n").encode()


_VARIANTS = {}


def golden_variants(v, by="file", ref=None, max_inside=S.DEFAULT_MAX_INSIDE):
    key = (vector_id(v), by, ref, max_inside)
    if key not in _VARIANTS:
        records = [s for f in fasta_of(v) for _, s in read_fasta(A.os.path.join(A.GOLDEN, f))]
        _VARIANTS[key] = Variants(golden_gfa1(v), k_of(v), [len(s) for s in records], by, ref, max_inside, records=records, sb=golden_superbubbles(v, by, max_inside))
    return _VARIANTS[key]


# ------------------------------------------------------------------------------------------------------------------ part 2
def check_files(tsv, vcf, records, cut=False):
    """On the program's two files and the letters of the input alone (vcf may be None).  cut: the graph was built with an abundance cut,
    where one name covers different bodies (rand6_k9_a3, as test_bubbles_cpu.py says): the letters of two alleles may then be equal,
    and equal edges small.  Returns (alleles, VCF records) checked."""
    text = tsv.decode().split("\n")
    assert text[-1] == ""
    head = dict(f.split("=") for f in text[0].split("\t")[2:])
    k, colors = int(head["k"]), int(head["colors"])
    seqs = {int(f[1]): (int(f[2]), int(f[3]), f[4]) for f in (line.split("\t") for line in text if line.startswith("#sequence\t"))}
    hist = {int(f[1]): int(f[2]) for f in (line.split("\t") for line in text if line.startswith("#alleles\t"))}
    rows = [line.split("\t") for line in text if line and not line.startswith("#")]
    assert int(head["alleles"]) == len(rows)
    sites = {}
    for r in rows:
        assert len(r) == 16, r
        site, allele, traversals, sides, edges, n = int(r[0]), int(r[5]), int(r[6]), int(r[7]), int(r[8]), int(r[9])
        s, begin, end = int(r[11]), int(r[12]), int(r[13])
        assert n == sum(bin(int(d, 16)).count("1") for d in r[10]) and 1 <= n <= colors and len(r[10]) == (colors + 3) // 4 and traversals >= n
        assert end - begin == edges + k and 0 <= begin and end <= seqs[s][1]
        letters = plain(records[s][begin:end])
        letters = letters if r[14] == "+" else reverse_complement(letters)
        mine = sites.setdefault(site, [])
        assert allele == len(mine)
        mine.append({"letters": letters, "edges": edges, "traversals": traversals, "presence": r[10], "is_ref": r[15] == "1", "sides": sides})
    assert int(head["sites"]) == len(sites) and sum(hist.values()) == len(sites)
    assert int(head["traversals"]) == sum(a["traversals"] for alleles in sites.values() for a in alleles)
    for site, alleles in sites.items():
        first = alleles[0]["letters"]
        assert cut or all(a["letters"][:k] == first[:k] and a["letters"][-k:] == first[-k:] for a in alleles), site     # the site's two k-mers
        # pairwise different, as far as the letters are known: an 'N'-named segment is a row of its own at every occurrence, so two
        # alleles through such rows may print the same letters around their N
        spelled = [a["letters"] for a in alleles if "N" not in a["letters"]]
        assert cut or len(set(spelled)) == len(spelled), site
        if len(alleles) > 1 and len({a["edges"] for a in alleles}) == 1:
            assert cut or "N" in "".join(a["letters"] for a in alleles) or alleles[0]["edges"] >= k + 1, site
        assert sum(a["is_ref"] for a in alleles) <= (0 if head["ref"] == "none" else 1)
    for n, c in hist.items():
        assert c == sum(1 for alleles in sites.values() if len(alleles) == n)
    if vcf is None:
        return len(rows), 0
    ref = int(head["ref"])
    lines = vcf.decode().split("\n")
    assert lines[-1] == "" and lines[0] == "##fileformat=VCFv4.2"
    contigs = [line[len("##contig=<ID="):-1].rsplit(",length=", 1) for line in lines if line.startswith("##contig=")]
    assert contigs == [[name, str(length)] for _, (colour, length, name) in sorted(seqs.items()) if colour == ref]
    index_of = {name: s for s, (colour, _, name) in seqs.items() if colour == ref}
    body = [line.split("\t") for line in lines[:-1] if not line.startswith("#")]
    header = [line for line in lines if line.startswith("#CHROM")][0].split("\t")
    assert len(header) == 9 + colors
    by_colour = {c: [plain(records[s]) for s, (colour, _, _) in seqs.items() if colour == c] for c in range(colors)}
    order = []
    for f in body:
        assert len(f) == 9 + colors and f[2].startswith("sb") and f[8] == "GT", f
        s, pos, site = index_of[f[0]], int(f[1]), int(f[2][2:])
        order.append((s, pos, site))
        alleles = sites[site]
        ref_allele = [a for a in alleles if a["is_ref"]]
        assert len(ref_allele) == 1 and len(alleles) >= 2
        texts = [f[3]] + f[4].split(",")
        known = [x for x in texts if "N" not in x]
        assert len(texts) == len(alleles) and all(texts) and (cut or len(set(known)) == len(known))
        assert plain(records[s])[pos - 1:pos - 1 + len(f[3])] == f[3], f[:4]                                    # REF is the reference at POS
        info = dict(x.split("=") for x in f[7].split(";"))
        others = [a for a in alleles if not a["is_ref"]]
        assert info["AC"] == ",".join(str(a["traversals"]) for a in others) and int(info["AN"]) == sum(a["traversals"] for a in alleles)
        local = ref_allele + others
        equal = len({a["edges"] for a in alleles}) == 1 and alleles[0]["edges"] >= k + 1
        least = min(a["edges"] for a in alleles)
        # the flanks, in the reference's stored orientation: found from the reference allele's own span
        whole = [a["letters"] for a in local]
        if whole[0][k - (0 if equal else 1):][:len(texts[0])] != texts[0]:      # the reference walks the site on its other strand
            whole = [reverse_complement(w) for w in whole]
        trim = (k, k) if equal else (k - 1, min(k, least))
        for w, text in zip(whole, texts):
            assert cut or w[trim[0]:len(w) - trim[1]] == text, (f[:3], text)
        for c in range(colors):
            gt = f[9 + c]
            want = "/".join(str(j) for j, a in enumerate(local) if int(a["presence"][c // 4], 16) >> (c % 4) & 1) or "."
            assert gt == want, (f[:3], c)
            if gt != "." and "/" not in gt:
                hap = whole[int(gt)]
                assert cut or any(hap in s2 or reverse_complement(hap) in s2 for s2 in by_colour[c]), (f[:3], c)
    assert order == sorted(order)
    return len(rows), len(body)


# ------------------------------------------------------------------------------------------------------------------ the generated inputs
def duplicated_records():
    """A genome that walks one site twice with two different alleles: g0 holds a region of 120 letters twice, once with each letter of
    a substitution; g1 and g2 hold it once, with one letter each.  By sequence, with g0 the reference: GT 0/1 and ref_traversals 2."""
    rng = np.random.default_rng(20261021)

    def letters(n):
        return "".join("ACGT"[c] for c in rng.integers(0, 4, n))

    left, mid, right, region = letters(150), letters(150), letters(150), letters(121)
    a = region[:60] + "A" + region[61:]
    c = region[:60] + "C" + region[61:]
    return [("g0", left + a + mid + c + right), ("g1", left + a + right), ("g2", mid + c + right)]


HOT_RECORDS, HOT_K = 600, 21


def hot_records():
    """600 short records carrying one of 3 alleles of one substitution: one site, three alleles of 200 traversals each."""
    rng = np.random.default_rng(20261022)
    base = "".join("ACGT"[c] for c in rng.integers(0, 4, 101))
    return [("r%d" % r, base[:50] + "ACG"[r % 3] + base[51:]) for r in range(HOT_RECORDS)]


def edge_records():
    """Where a walk meets the ends of its sequence: two genomes with one substitution between 90 letters at each side; between them a
    record of exactly k letters, which is one junction and no event -- a sequence without events between two that have some; a record
    that begins inside the left flank and ends inside the right one, so that its first event is the entrance and its last the exit
    (a '+' walk that ends on the last event of its sequence); and the reverse complement of such a record with the other letter (a
    '-' walk that starts on the last event of its sequence and ends on the first)."""
    rng = np.random.default_rng(20261023)

    def letters(n):
        return "".join("ACGT"[c] for c in rng.integers(0, 4, n))

    left, right, lone = letters(90), letters(90), letters(HOT_K)
    return [("full_a", left + "A" + right), ("lone", lone), ("full_c", left + "C" + right), ("inner_a", left[30:] + "A" + right[:50]),
            ("inner_c_rc", reverse_complement(left[30:] + "C" + right[:50]))]


def write_fasta(path, records):
    with open(path, "w") as f:
        for name, s in records:
            f.write(">%s\n" % name)
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + "\n")
    return path
