"""The EVENT TABLE of a junction stream by its definition (include/twopaco_hip.h, the tpc_segments_* group), in Python: what
the device builds and what host/graphformat.h formats from.  Shared by the CPU and the GPU tests of `twopaco --graph`."""
import struct

import numpy as np


def read_fasta(path):
    """Records as the parser gives them to graphdump: upper-cased letters, whitespace dropped."""
    recs = []
    for line in open(path):
        if line.startswith(">"):
            recs.append([])
        else:
            recs[-1].append("".join(line.split()).upper())
    return ["".join(r) for r in recs]


def event_table(data, seqs, k):
    """name / first / begin / end per event in file order and seq_event_begin[0 .. len(seqs)] of a junction stream.
    An event is a pair of consecutive records with no separator between them; its sequence id is the number of separator
    slots before it (a slot is a separator when its position OR its id field says so); its name is SegmentNamer::Name
    (reference graphdump.cpp:44-113), restated; first = no earlier event has this |name|; begin / end = the position
    fields of its two records; seq_event_begin[s] = the events with a sequence id below s."""
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    name, begin, end, seq_of = [], [], [], []
    fresh, seq, prev = 1 << 34, 0, None
    for slot in range(len(data) // 12):
        pos, ident = struct.unpack_from("<Iq", data, slot * 12)
        if pos == 0xFFFFFFFF or ident == (1 << 63) - 1:
            seq, prev = seq + 1, None
            continue
        if prev is not None:
            lp, lid = prev
            left, right = abs(lid), abs(ident)
            forward = left < right or (left == right and left > 0)
            nxt = seqs[seq][lp + k] if forward else comp.get(seqs[seq][pos - 1], "N")
            start = lid if forward else -ident
            if nxt == "N":
                n = fresh
                fresh += 1
            else:
                n = "ACGT".index(nxt) if nxt in "ACGT" else -1
                if n >= 0:
                    n |= (4 | abs(start) << 3) if start < 0 else start << 3
                n = -n if start != lid else n   # reverse, but not between two ids of 0 (graphdump.cpp:88-91)
            name.append(n)
            begin.append(lp)
            end.append(pos)
            seq_of.append(seq)
        prev = (pos, ident)
    seen, first = set(), []
    for n in name:
        first.append(abs(n) not in seen)
        seen.add(abs(n))
    seq_of = np.array(seq_of, dtype=np.int64)
    seq_event_begin = [int((seq_of < s).sum()) for s in range(len(seqs) + 1)]
    return (np.array(name, dtype=np.int64), np.array(first, dtype=bool), np.array(begin, dtype=np.uint32), np.array(end, dtype=np.uint32),
            np.array(seq_event_begin, dtype=np.uint32))


def vector_parts(v):
    """(bin, format, k, fasta files, prefix) of a vector's command line: <bin> -f <fmt> -k <k> -s <fasta> ... [--prefix]"""
    a = v["args"]
    assert a[1] == "-f" and a[3] == "-k"
    files, rest, i = [], [], 5
    while i < len(a):
        if a[i] == "-s":
            files.append(a[i + 1])
            i += 2
        else:
            rest.append(a[i])
            i += 1
    assert files and rest in ([], ["--prefix"]), a
    return a[0], a[2], int(a[4]), files, rest == ["--prefix"]
