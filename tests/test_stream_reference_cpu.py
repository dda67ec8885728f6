"""CPU: tests/stream_reference.py, the sequential statement of the junction stream that tests/test_gpu_stream.py holds the kernels of
csrc/tpc_stream.hip against.  It has to reproduce the real reference's files from their own real-id records, write a few streams small
enough to be listed by hand, and its annotation has to give the sharded calls' quantities the properties the host relies on."""
import os

import numpy as np
import pytest

import stream_reference as R
from helpers import GOLDEN, golden_cases
from oracle import oracle as O

SEP = (R.SEPARATOR_POS, R.INVALID)
COMMITTED = [c for c in golden_cases() if c.get("bin") and c.get("fasta") and os.path.exists(os.path.join(GOLDEN, c["bin"]))
             and os.path.exists(os.path.join(GOLDEN, c["fasta"]))]


def golden_input(case):
    """(bytes of the golden file, k, J, rec_len, marks, ids): the marks are the file's own real-id records."""
    with open(os.path.join(GOLDEN, case["bin"]), "rb") as f:
        data = f.read()
    rec_len = [len(r) for r in O.read_fasta_records(os.path.join(GOLDEN, case["fasta"]))]
    start = R.rec_starts(rec_len)
    real = R.parse(data, case["distinct"])
    return data, case["k"], case["distinct"], rec_len, [start[s] + p for s, p, _ in real], [i for _, _, i in real]


def test_reproduces_every_committed_golden_file():
    """The writer fed the real-id records of each golden file and the lengths of its FASTA records gives the file back byte for byte."""
    checked = stubs = short = exact = 0
    for case in COMMITTED:
        data, k, J, rec_len, marks, ids = golden_input(case)
        s = R.write(k, J, rec_len, marks, ids)
        assert s.bytes == data, case["name"]
        assert s.n_records == case["true_marks"], case["name"]
        checked += 1
        stubs += int(np.count_nonzero((s.kind == R.STUB_FIRST) | (s.kind == R.STUB_LAST)))
        short += sum(1 for n in rec_len if n < k)
        exact += sum(1 for n in rec_len if n == k)
    assert checked >= 43, checked           # a case that silently drops out cannot hide a failure
    assert stubs > 0 and short > 0 and exact > 0, (stubs, short, exact)


def test_invalid_marks_change_no_byte():
    """INVALID marks on k-mer starts the file does not mark -- among them first and last k-mers that get stubs -- are skipped."""
    rng = np.random.default_rng(11)
    on_stub = checked = 0
    for case in COMMITTED:
        data, k, J, rec_len, marks, ids = golden_input(case)
        start = R.rec_starts(rec_len)
        have = set(marks)
        extra = set()
        for first, n in zip(start, rec_len):
            if n < k:
                continue
            ends = [g for g in {first, first + n - k} if g not in have]
            extra.update(ends)              # every end k-mer that gets a stub
            on_stub += len(ends)
            inner = [first + int(p) for p in rng.integers(0, n - k + 1, 3)]
            extra.update(g for g in inner if g not in have)
        both = sorted([(g, i) for g, i in zip(marks, ids)] + [(g, R.INVALID) for g in extra])
        s = R.write(k, J, rec_len, [g for g, _ in both], [i for _, i in both])
        assert s.bytes == data, case["name"]
        checked += 1
    assert checked >= 43 and on_stub > 0


# k = 3, sequences of 0, 2, 3, 3, 7 and 1 bases: they start at 1, 2, 5, 9, 13 and 21; the 7-base one has k-mers at 13 .. 17
LENS = [0, 2, 3, 3, 7, 1]
HAND = {
    # leading short sequences cost a separator each once something follows; the length-k sequence with a real id, the one without (stub);
    # stubs at both ends of the long one around a record; the INVALID mark on its last k-mer is skipped; the trailing short one: nothing
    "mixed": (5, [5, 15, 17], [4, -2, R.INVALID],
              [SEP, SEP, (0, 4), SEP, (0, 47), SEP, (0, 48), (2, -2), (4, 49)],
              [1, 4, 5, 8, 9, 12, 13, 15, 17]),
    # no mark at all: one stub for each length-k sequence, two for the long one, numbered in emission order
    "unmarked": (5, [], [], [SEP, SEP, (0, 47), SEP, (0, 48), SEP, (0, 49), (4, 50)], [1, 4, 5, 8, 9, 12, 13, 17]),
    # a length-k sequence whose only k-mer is marked INVALID (stub), one with a real id, both ends of the long one real: one stub in all
    "ends_real": (0, [5, 9, 13, 17], [R.INVALID, 1, 3, -3], [SEP, SEP, (0, 42), SEP, (0, 1), SEP, (0, 3), (4, -3)], [1, 4, 5, 8, 9, 12, 13, 17]),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_written_streams(name):
    J, marks, ids, want, owners = HAND[name]
    s = R.write(3, J, LENS, marks, ids)
    assert s.rec_start == [1, 2, 5, 9, 13, 21]
    assert s.records() == want
    assert s.owner.tolist() == owners
    assert s.n_records == sum(1 for w in want if w != SEP) and len(s.bytes) == 12 * len(want)
    assert s.bytes == b"".join(int(p).to_bytes(4, "little") + int(i).to_bytes(8, "little", signed=True) for p, i in want)


def test_hand_written_all_short_and_trailing():
    """Only sequences shorter than k: no byte.  Short sequences behind the last emitting one get no separator; a single sequence none either."""
    assert R.write(3, 7, [0, 2, 1], [], []).bytes == b""
    assert R.write(3, 7, [3, 2, 0, 1], [1], [6]).records() == [(0, 6)]
    assert R.write(3, 7, [2, 4], [4, 5], [-1, 2]).records() == [SEP, (0, -1), (1, 2)]
    assert R.write(3, 7, [5], [2], [3]).records() == [(0, 49), (1, 3), (2, 50)]


def test_contract_violations_are_refused():
    for marks in ([1], [2], [3], [6], [22], [15, 15], [15, 14]):   # in a short sequence, past a last k-mer, on a separator, behind the text, not ascending
        with pytest.raises(ValueError):
            R.write(3, 5, LENS, marks, [1] * len(marks))


def random_layout(rng, k, n_rec):
    rec_len = [int(x) for x in rng.choice([0, 1, k - 1, k, k + 1, 2 * k, 40], n_rec)]
    start = R.rec_starts(rec_len)
    marks, ids = [], []
    for first, n in zip(start, rec_len):
        for g in range(first, first + n - k + 1):
            if rng.random() < 0.4:
                marks.append(g)
                ids.append(R.INVALID if rng.random() < 0.3 else int(rng.integers(1, 10)) * (1 if rng.random() < 0.5 else -1))
    return rec_len, marks, ids


def random_cuts(rng, s, w):
    end = s.rec_start[-1] + s.rec_len[-1] + 2
    return sorted(int(c) for c in rng.integers(0, end, w - 1))


@pytest.mark.parametrize("seed", range(6))
def test_owners_ascend_and_rank_ranges_tile_the_file(seed):
    rng = np.random.default_rng(seed)
    rec_len, marks, ids = random_layout(rng, 4, 60)
    s = R.write(4, 9, rec_len, marks, ids)
    assert s.n_slots > 100 and (np.diff(s.owner.astype(np.int64)) >= 0).all()
    # each annotation agrees with the slot's own fields
    sep = s.kind == R.SEPARATOR
    assert ((s.pos == R.SEPARATOR_POS) == sep).all() and ((s.id == R.INVALID) == sep).all()
    assert (s.owner[~sep] == np.array(s.rec_start, dtype=np.uint64)[s.seq[~sep]] + s.pos[~sep]).all()
    assert (s.owner[sep] == np.array(s.rec_start, dtype=np.uint64)[s.seq[sep] + 1] - 1).all()
    for w in (1, 2, 3, 4, 8):
        cuts = random_cuts(rng, s, w)
        if w == 4:
            cuts[1] = cuts[0]               # an empty chunk
            cuts.sort()
        d = R.shard(s, cuts)
        at = 0
        for slot0, n in zip(d["slot0"], d["n_slots"]):
            assert slot0 == at
            at += n
        assert at == s.n_slots


@pytest.mark.parametrize("seed", range(6))
def test_derived_quantities_keep_the_hosts_identities(seed):
    rng = np.random.default_rng(100 + seed)
    rec_len, marks, ids = random_layout(rng, 5, 80)
    if seed == 0:
        marks, ids = [], []
    if seed == 1:
        rec_len, marks, ids = [0, 3, 4, 1], [], []   # no sequence of k bases: an empty stream
    s = R.write(5, 3, rec_len, marks, ids)
    n = len(rec_len)
    for w in (2, 3, 8):
        d = R.shard(s, random_cuts(rng, s, w))
        records = int(d["e_scan"][n])
        assert records == s.n_records
        assert sum(d["n_slots"]) == (records + d["r_last"] if records else 0) == s.n_slots
        total = np.zeros(n, dtype=np.uint64)
        for r in range(w):
            assert (d["before"][r] == total).all()      # before[r] = cnt of the ranks in front of r
            total += d["cnt"][r]
        real = sum(1 for i in ids if i != R.INVALID)
        assert int(total.sum()) == real
        long_enough = np.array([x >= 5 for x in rec_len])
        assert (((d["gflags"] & 4) != 0) == long_enough).all()
        assert (np.diff(d["e_scan"].astype(np.int64)) >= long_enough).all() and (np.diff(d["s_scan"].astype(np.int64)) <= 2).all()
        assert d["r_last"] == (max(i for i in range(n) if long_enough[i]) if long_enough.any() else 0)
        # a first / last k-mer holds a real id on exactly one rank, and the stubs are the ends that hold none
        firsts = sum((f & 1).astype(np.int64) for f in d["flags"])
        lasts = sum(((f >> 1) & 1).astype(np.int64) for f in d["flags"])
        assert firsts.max(initial=0) <= 1 and lasts.max(initial=0) <= 1
        exact = np.array([x == 5 for x in rec_len])
        stubs = (long_enough & (firsts == 0)).astype(np.int64) + (long_enough & ~exact & (lasts == 0)).astype(np.int64)
        assert (np.diff(d["s_scan"].astype(np.int64)) == stubs).all()
