"""GPU (-m gpu): the periodic-window masks and the verdict copy against their definition.

The first pass skips a position whose window of the text equals the window p = 1 .. 63 positions earlier: k_periodic_build flags
it (behind the cheap necessary condition periodic_may_flag), the hash kernels drop its insert (per_i) and its probes (per_qs), and
k_periodic_copy gives it its twin's verdict.  End to end a detector that flags too little, or too much where the verdict happens to
agree, or a copy from a multiple of the period, is invisible.  Here:

  masks   tpc_periodic_download == helpers.periodic_reference at EVERY position (not a subset, not a superset), on one constructed
          text per k (periodic_cases.constructed_case: every period, the four lengths around the threshold, every word offset, 32
          tile boundaries, N and separators inside tracts, the text's ends, runs beyond 1023), on plain random text, on m2r2, on the
          four windows of a text cut over four ranks, after a change of k and after a second upload; the detection-only launch;
  copy    k_periodic_copy alone (tpc_mask_import + tpc_shard_periodic_copy on a one-rank context) over random marks == the
          sequential definition mark[i] = mark[i - dist[i]];
  users   every hash kernel that reads the masks, with marks that vary inside the tracts: filter, mask and count == the oracle's.

The reference is checked on the CPU against string comparison (tests/test_periodic_reference_cpu.py), and every case asserts from
the reference alone that it holds what it was built to hold.

That the tests bite -- ten changes planted in tpc_qpartition.hip, one at a time (each can only produce wrong bits), once through this
file on an MI355X; tests that failed, of 42:
   1  T2 = k + 1 where k + 2 is meant                 34: constructed[every k], random text, m2r2, detection-only, windowed, copy, ...
   2  PER_CBITS = 9                                     2: constructed[603], copy[603-constructed]
   3  periodic_may_flag: false for off >= 20           10: constructed[18, 19, 25, 29], m2r2[25, 19], option off/on, change of k, copy[25-*]
   4  `four` always false                               7: constructed[18, 19, 25, 29], option off/on, change of k, copy[25-constructed]
   5  the pre-test's N test removed                     0: see below
   6  the tile rule's 63 -> 64                         30: constructed[every k], m2r2, windowed, copy, ...
   7  __ffsll -> the highest set bit                   31: constructed[every k], random text, m2r2, windowed, copy, ...
   8  plane 5 of the distance dropped                  37: the same and every hash-kernel case (a verdict copied from 32 positions off)
   9  the walk's zeros == PER_MAXP -> 62                3: copy[5-constructed], copy[5-copy], copy[25-copy]
  10  mh not masked                                     0: see below
5 and 10 change no output for any input, so no test of outputs can see them.  5: a flagged position's window holds a whole tested
block that equals its twin p back, both definite (that is the pre-test's own argument), so that block passes whether or not an N
elsewhere in the 63 + B characters returned early: the N test only makes the pre-test pass more words to the detector, which then
flags nothing in them.  10: the mask clears bit 63 of mh alone, and the walk reads bit d - 1 <= 62."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import periodic_cases as C
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTERS = np.frombuffer(b"ACGTN", dtype=np.uint8)
SEED = 2357


@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


def open_ctx(capi, k, L=20, q=1, options=()):
    ctx = capi.Context(0)
    for name, val in options:
        ctx.set_option(name, val)
    ctx.set_params(k, L, q, capi.seed_table(q, L, seed=SEED))
    return ctx


def packed(capi, records, flat=None):
    text = capi.PackedText.from_codes(records)
    codes = H.text_codes(text.bases, text.nmask, text.length)
    if flat is not None:
        assert text.length == len(flat) and (codes == flat).all(), "the packed text is not the text the case was laid out as"
    return text, codes


def padded(ref, n):
    out = []
    for a in ref:
        b = np.zeros(n, dtype=a.dtype)
        b[:len(a)] = a
        out.append(b)
    return out


def assert_masks(got, ref, codes, k, tag):
    """qs, dist and ins equal at every position; the message names the first position that differs, its window and its word offset."""
    ref = padded(ref, len(got[0]))
    for name, g, r in zip(("qs", "dist", "ins"), got, ref):
        bad = np.nonzero(g != r)[0]
        if bad.size:
            i = int(bad[0])
            win = "".join("ACGTN"[c] for c in codes[max(0, i - 66):i + k + 1])
            raise AssertionError("%s differs at %d positions, first at %d (word %d, offset %d, position %d of its tile): device %d, definition %d; "
                                 "device qs/dist/ins %d/%d/%d, definition %d/%d/%d; text[i - 66 .. i + k] = %s; %r"
                                 % (name, bad.size, i, i // 32, i % 32, i % H.PER_TILE, int(g[i]), int(r[i]), got[0][i], got[1][i], got[2][i],
                                    ref[0][i], ref[1][i], ref[2][i], win, tag))


# ------------------------------------------------------------------------------------------------------------------ masks
@pytest.mark.parametrize("k", C.KS)
def test_constructed_masks_equal_the_definition(capi, k):
    """One constructed text per k over the pre-test's branches (k < 18: off; B = 10 .. 15: k = 18 .. 29, reads of three and of four
    words; B = 16; the tiling switch at k = 61 / 62 / 63; k = 603).  check_constructed asserts from the reference alone that every
    case of the list is there; then the device's masks equal the definition at every position."""
    case = C.constructed_case(k)
    C.check_constructed(case)
    text, codes = packed(capi, case["records"], case["flat"])
    ctx = open_ctx(capi, k)
    try:
        ctx.seq_upload(text)
        got = ctx.periodic_download()
        assert_masks(got, (case["qs"], case["dist"], case["ins"]), codes, k, ("constructed", k))
        assert ctx.stat("periodic_any_query") == 1 and ctx.stat("periodic_any_insert") == 1 and ctx.stat("periodic_skip") == 1
    finally:
        ctx.close()


_RANDOM = {}


def random_text(capi):
    if not _RANDOM:
        rng = np.random.default_rng(77)
        recs = [rng.integers(0, 4, n).astype(np.uint8) for n in (120000, 90001, 60000, 29999)]
        for r in recs[:2]:
            r[rng.integers(0, r.size, 6)] = 4
        text, codes = packed(capi, recs)
        _RANDOM.update(text=text, codes=codes)
    return _RANDOM["text"], _RANDOM["codes"]


def test_random_text_masks_equal_the_definition(capi):
    """300 k positions of plain random text, no planted tract, every k on one upload: only chance repeats are flagged -- a few
    positions in a thousand at k = 5, nearly none from k = 18 on, where the pre-test rejects nearly every word.  A pre-test that says
    no too often on real-looking input shows here, where the planted tracts of the constructed text would still pass it."""
    text, codes = random_text(capi)
    ctx = open_ctx(capi, C.KS[0])
    try:
        ctx.seq_upload(text)
        for k in C.KS:
            ctx.set_params(k, 20, 1, capi.seed_table(1, 20, seed=SEED))
            ref = H.periodic_reference(codes, k)
            share = ref[0].sum() / len(codes)
            print("random text k=%d: %d copying, %d dropped inserts (%.2e of the positions)" % (k, ref[0].sum(), ref[2].sum(), share))
            if k == 5:
                assert 1e-3 < share < 1e-2 and len(set(ref[1].tolist())) > 40
            elif k >= 18:
                assert share < 1e-5
            assert_masks(ctx.periodic_download(), ref, codes, k, ("random", k))
            assert ctx.stat("periodic_any_query") == int(ref[0].any()) and ctx.stat("periodic_any_insert") == int(ref[2].any()), k
    finally:
        ctx.close()


@pytest.mark.parametrize("k", [25, 19, 62])
def test_m2r2_masks_equal_the_definition(capi, k):
    """The workload with tracts of every kind (homopolymers, microsatellites, minisatellite units of 7 .. 60 letters), small."""
    from twopaco_amd import synth
    recs, _ = synth.workload("m2r2", scale=0.001)
    text, codes = packed(capi, recs)
    ref = H.periodic_reference(codes, k)
    assert 200000 < len(codes) < 500000 and ref[0].sum() > 500 and (ref[1] > 6).sum() > 100 and len(set(ref[1].tolist())) > 8, (len(codes), ref[0].sum())
    ctx = open_ctx(capi, k)
    try:
        ctx.seq_upload(text)
        assert_masks(ctx.periodic_download(), ref, codes, k, ("m2r2", k))
    finally:
        ctx.close()


def small_text(rng, k, kind):
    """3000 random positions with: 'insert_only' one tract of exactly k + 1 + p letters (one dropped insert, nothing copies);
    'neither' nothing; 'both' one of k + 2 + p."""
    p = 7
    a = rng.integers(0, 4, 3000).astype(np.uint8)
    if kind != "neither":
        t = C.tract(rng, C.primitive_unit(rng, p), k + p + (1 if kind == "insert_only" else 2))
        a[1500:1500 + len(t)] = t
    return [a]


@pytest.mark.parametrize("k", [19, 25, 62])
def test_detection_only_launch(capi, k):
    """The launch without outputs decides whether anything is allocated and which mask a hash kernel is handed: its two answers equal
    the reference's qs.any() / ins.any(), also on a text with dropped inserts and no copying position, and on one with neither."""
    rng = np.random.default_rng(300 + k)
    want = {"insert_only": (False, True), "neither": (False, False), "both": (True, True)}
    ctx = open_ctx(capi, k)
    try:
        for kind in ("insert_only", "neither", "both", "neither"):
            text, codes = packed(capi, small_text(rng, k, kind))
            ref = H.periodic_reference(codes, k)
            assert (bool(ref[0].any()), bool(ref[2].any())) == want[kind], (kind, k)
            if kind == "insert_only":
                assert ref[2].sum() == 1
            ctx.seq_upload(text)
            got = ctx.periodic_download()
            assert (ctx.stat("periodic_any_query"), ctx.stat("periodic_any_insert")) == (int(ref[0].any()), int(ref[2].any())), (kind, k)
            assert_masks(got, ref, codes, k, (kind, k))
    finally:
        ctx.close()


def test_option_off_reads_zero(capi):
    k = 25
    case = C.constructed_case(k, tiles=1)
    text, codes = packed(capi, case["records"], case["flat"])
    ctx = open_ctx(capi, k, options=(("periodic_skip", 0),))
    try:
        ctx.seq_upload(text)
        got = ctx.periodic_download()
        assert not got[0].any() and not got[1].any() and not got[2].any()
        assert ctx.stat("periodic_any_query") == 0 and ctx.stat("periodic_any_insert") == 0 and ctx.stat("periodic_skip") == 0
        ctx.set_option("periodic_skip", 1)
        assert_masks(ctx.periodic_download(), (case["qs"], case["dist"], case["ins"]), codes, k, "option back on")
    finally:
        ctx.close()


def test_masks_follow_a_change_of_k_and_a_second_upload(capi):
    """set_params with another k on the same upload, then another text: the read-out is that of the text and k at hand, not stale."""
    a, b = C.constructed_case(19, tiles=2), C.constructed_case(62, seed=1, tiles=1)
    ta, ca = packed(capi, a["records"], a["flat"])
    tb, cb = packed(capi, b["records"], b["flat"])
    ctx = open_ctx(capi, 19)
    try:
        ctx.seq_upload(ta)
        assert_masks(ctx.periodic_download(), (a["qs"], a["dist"], a["ins"]), ca, 19, "first")
        for k in (62, 5, 19):
            ctx.set_params(k, 20, 1, capi.seed_table(1, 20, seed=SEED))
            ref = H.periodic_reference(ca, k)
            assert (ref[0] != a["qs"]).any() or k == 19
            assert_masks(ctx.periodic_download(), ref, ca, k, ("k changed", k))
        ctx.seq_upload(tb)   # (shorter: fewer mask words)
        ref = H.periodic_reference(cb, 19)
        assert_masks(ctx.periodic_download(), ref, cb, 19, "second upload")
        ctx.set_params(62, 20, 1, capi.seed_table(1, 20, seed=SEED))
        assert_masks(ctx.periodic_download(), (b["qs"], b["dist"], b["ins"]), cb, 62, "second upload, k changed")
    finally:
        ctx.close()


@pytest.mark.parametrize("k", [25, 62, 127])
def test_windowed_contexts(capi, k):
    """Four ranks, each holding only the packed words of its tiles and their halo (options text_window, shard_periodic_skip): the
    masks of a rank equal the definition with every character outside its words read as N, and are zero outside.  A tract lies across
    each edge of each window."""
    world = 4
    rng = np.random.default_rng(800 + k)
    n = 9 * H.PER_TILE + 1000
    opts = (("text_window", 1), ("shard_periodic_skip", 1))

    def windows(text):
        out = []
        for rank in range(world):
            ctx = capi.Context(0)
            for name, val in opts:
                ctx.set_option(name, val)
            ctx.shard_config(rank, world)
            ctx.set_params(k, 20, 1, capi.seed_table(1, 20, seed=SEED))
            ctx.seq_upload(text)
            out.append((ctx, ctx.stat("text_word_begin"), ctx.stat("text_word_end")))
        return out

    a = rng.integers(0, 4, n).astype(np.uint8)
    text, _ = packed(capi, [a])
    ws = windows(text)
    try:
        edges = sorted({32 * w for _, w0, w1 in ws for w in (w0, w1) if 0 < 32 * w < n})
        for ctx, w0, w1 in ws:
            assert ctx.stat("text_words") == w1 - w0 and 0 <= w0 < w1
            ctx.close()
        assert ws[0][1] == 0 and all(ws[r][2] > ws[r + 1][1] for r in range(world - 1)) and 32 * ws[-1][2] > n  # the windows cover the text, with a halo
        assert max(w1 - w0 for _, w0, w1 in ws) < (n // 32) // 2 and len(edges) >= 6                             # and each is a window
        for j, e in enumerate(edges):   # a tract across every edge (the text's position e is the record's letter e - 1)
            p = (1, 3, 7, 31, 63, 2, 5, 11)[j % 8]
            t = C.tract(rng, C.primitive_unit(rng, p), 2 * (k + p + 60))
            a[e - 1 - len(t) // 2:e - 1 - len(t) // 2 + len(t)] = t
        text, codes = packed(capi, [a])
        ws = windows(text)
        whole = H.periodic_reference(codes, k)
        for rank, (ctx, w0, w1) in enumerate(ws):
            ref = H.periodic_reference(codes, k, 32 * w0, 32 * w1)
            lo, hi = 32 * w0, min(32 * w1, len(codes))
            assert not ref[2][:lo].any() and not ref[2][hi:].any() and ref[0][lo:hi].sum() > 100
            assert any((whole[0][e - 70:e + 70] & ~ref[0][e - 70:e + 70]).any() for e in (lo, hi) if 0 < e < len(codes)), "no tract is cut by this window's edge"
            assert_masks(ctx.periodic_download(), ref, codes, k, ("window", rank, w0, w1))
    finally:
        for ctx, _, _ in ws:
            ctx.close()


# ------------------------------------------------------------------------------------------------------------------ copy
def copy_text(k):
    """Beyond the constructed text: a tract of 40 k positions (a walk of hundreds of words, across tile boundaries), tracts 62, 63 and
    64 probing positions apart (63 probing positions in a row end a segment), two tracts whose ends share a packed word, a tract that
    runs to the text's end."""
    rng = np.random.default_rng(4000 + k)
    lay = C.Layout(rng)
    lay.filler(300)
    lay.put("long", 3, C.tract(rng, C.primitive_unit(rng, 3), 40000))
    lay.put("long", 11, C.tract(rng, C.primitive_unit(rng, 11), 3000))
    for gap in (62, 63, 64, 62, 63, 64):
        # the last copying position of a tract of ln letters from s is s + ln - 1 - k, the first one s + p + 1: `gap` probing positions between
        p1, p2 = 2, 3
        t1, t2 = C.tract(rng, C.primitive_unit(rng, p1), k + 60), C.tract(rng, C.primitive_unit(rng, p2), k + 60)
        between = gap - k - p2 - 1 - 2   # (random letters between the two letters that break the periods)
        assert between >= 0
        s = lay.put("gap_first", gap, t1, flank=True)
        lay.parts.pop()          # (drop the right flank: the second tract follows `between` letters behind the first)
        lay.n -= C.FLANK
        lay.filler(between)
        lay.put("gap_second", gap, t2, flank=False)
        lay.filler(C.FLANK)
    for off in (3, 17, 30):
        lay.filler(C.FLANK)
        t1, t2 = C.tract(rng, np.array([0, 1], dtype=np.uint8), k + 50), C.tract(rng, np.array([2, 3, 3], dtype=np.uint8), k + 50)
        lay.pad_to(len(t1) - 1 - k - 1, 32, off)   # the first tract's last copying position at offset `off` of its word
        lay.put("shared_word", off, np.concatenate([t1[:-1], t2[1:]]), flank=False)
    lay.filler(C.FLANK)
    lay.put("tail", 5, np.concatenate([[3], np.resize(np.array([1, 2, 2, 3, 0], dtype=np.uint8), k + 500)]), flank=False)
    flat = lay.finish()
    qs, dist, ins = H.periodic_reference(flat, k)
    pos = np.nonzero(qs)[0]
    gaps = set((np.diff(pos) - 1).tolist())
    assert {62, 63, 64} <= gaps, sorted(gaps)[-8:]
    for kind, tag, s, e in lay.cases:
        if kind == "long":
            assert qs[s + tag + 2:e - 1 - k].sum() > (e - s) * 0.98 and ((e - s) < 5000 or not qs[s:e][(np.arange(s, e) % H.PER_TILE) < 63].any())
        if kind == "shared_word":
            w = (s + 50) // 32
            d = dist[32 * w:32 * w + 32]
            assert qs[s + 50] and not qs[s + 51] and (s + 50) % 32 == tag
            if k <= 8 and tag < 20:   # (the second tract's first copying position is k + 5 behind the first one's last)
                assert {2, 3} <= set(d.tolist()) and (d == 0).any(), ("two tracts in one word", tag, d)
    n = len(flat)
    assert (qs | (np.arange(n) % H.PER_TILE < 63))[n - 400:n - 1 - k].all() and not qs[n - 1 - k:].any()
    return dict(k=k, flat=flat, splits=[], records=C.records_of(flat, []), qs=qs, dist=dist, ins=ins, cases=lay.cases)


def random_marks(rng, case, density):
    """Marks of the given density at the probing positions, none at the copying ones; where a tract's first copying position has
    period p >= 2, its p sources get both values, so that the copies inside the tract are not all the same."""
    qs, dist = case["qs"], case["dist"]
    m = (rng.random(len(qs)) < density) & ~qs
    m[case["flat"] == 4] = False
    pos = np.nonzero(qs)[0]
    firsts = pos[np.concatenate([[True], np.diff(pos) > 1])]
    varied = 0
    for f in firsts.tolist():
        p = int(dist[f])
        if p >= 2 and not qs[f - p:f].any() and (dist[f:f + p] == p).all():
            m[f - p:f] = rng.random(p) < 0.5
            m[f - 1], m[f - 2] = True, False
            varied += 1
    return m, firsts, varied


def run_copy(capi, ctx, marks):
    import torch
    nw = ctx.mask_words()
    words = H.words_of_bits(marks, nw)
    dev = torch.from_numpy(words.view(np.int32).copy()).cuda()
    ctx.mask_import(dev.data_ptr())
    ctx.shard_periodic_copy()
    return H.bits_of_words(ctx.mask_download(False), nw * 32)


@pytest.mark.parametrize("k,which", [(5, "constructed"), (25, "constructed"), (62, "constructed"), (603, "constructed"), (5, "copy"), (25, "copy")])
def test_copy_over_random_marks(capi, k, which):
    """k_periodic_copy alone: import a random round mask (density 0.5 and 0.02 at the probing positions, zero at the copying ones),
    run the copy, download: equal to mark[i] = mark[i - dist[i]] taken in ascending order, at every position, probing positions
    unchanged.  A distance that is a wrong multiple, a lost word where a walk changes words, a walk that stops one position early,
    a segment that starts where it must not: all show under random marks -- the marks a tract copies are asserted not to be constant."""
    case = C.constructed_case(k) if which == "constructed" else copy_text(k)
    text, codes = packed(capi, case["records"], case["flat"])
    ctx = open_ctx(capi, k, options=(("shard_periodic_skip", 1),))
    try:
        ctx.seq_upload(text)
        assert_masks(ctx.periodic_download(), (case["qs"], case["dist"], case["ins"]), codes, k, ("copy", which, k))
        for density in (0.5, 0.02):
            rng = np.random.default_rng(int(density * 100) + k)
            marks, firsts, varied = random_marks(rng, case, density)
            want = H.periodic_copy_reference(marks, case["qs"], case["dist"])
            assert varied >= 10 and (want & case["qs"]).sum() > 100 and (~want & case["qs"]).sum() > 100
            # every stretch of copying positions that starts with period >= 2 holds both values
            pos = np.nonzero(case["qs"])[0]
            run_id = np.cumsum(np.concatenate([[True], np.diff(pos) > 1])) - 1
            ones = np.bincount(run_id, weights=want[pos].astype(np.float64))
            size = np.bincount(run_id)
            for r, f in enumerate(firsts.tolist()):
                p = int(case["dist"][f])
                if p >= 2 and not case["qs"][f - p:f].any() and (case["dist"][f:f + p] == p).all():
                    assert 0 < ones[r] < size[r], ("constant marks in a tract", f, p)
            got = run_copy(capi, ctx, marks)
            want = padded([want], len(got))[0]
            bad = np.nonzero(got != want)[0]
            if bad.size:
                i = int(bad[0])
                raise AssertionError("the copy differs at %d positions, first at %d (word %d, offset %d, position %d of its tile): device %d, definition %d, "
                                     "qs %d, dist %d, imported %d, the 64 marks before it %s; copying positions among the 64 before: %s; density %.2f"
                                     % (bad.size, i, i // 32, i % 32, i % H.PER_TILE, got[i], want[i], case["qs"][i], case["dist"][i], marks[i],
                                        "".join(str(int(x)) for x in want[max(0, i - 64):i]), "".join(str(int(x)) for x in case["qs"][max(0, i - 64):i]), density))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------------ users
def junction_text(k, n=70000, seed=0):
    """Random text with tracts of periods 2 .. 63 (some across the tile boundaries at 16384 and 32768, one with an N inside, one at a
    record's start, one at its end) and, elsewhere, a copy of one k-mer of every tract followed by a letter the tract does not have
    there: that phase of the tract is a junction, the other phases are not, so the verdicts a tract's positions copy differ."""
    rng = np.random.default_rng(600 + 13 * k + seed)
    a = rng.integers(0, 4, n).astype(np.uint8)
    tracts = []
    at = 400
    for t, p in enumerate((2, 3, 5, 7, 13, 31, 60, 63, 4, 6, 9, 17)):
        ln = k + p + 300 + 37 * t
        if t in (3, 7):
            at = H.PER_TILE * (1 if t == 3 else 2) - 1 - ln // 2  # (record 0 starts at text position 1)
        body = C.tract(rng, C.primitive_unit(rng, p), ln)
        a[at:at + len(body)] = body
        tracts.append((at + 2, ln, p))   # (text position of the tract's first letter: record 0 starts at 1, the breaking letter at `at`)
        at += len(body) + 900
    assert at < n - 4000
    a[tracts[4][0] - 1 + tracts[4][1] // 2] = 4
    plant = n - 3000
    for s, ln, p in tracts:
        j = s - 1 + p + 3
        a[plant:plant + k] = a[j:j + k]
        a[plant + k] = (a[j + k] + 1) % 4
        a[plant + k + 1] = 4   # (an N behind every plant: the plants do not run into each other)
        plant += k + 2
    assert plant < n - 700
    second = rng.integers(0, 4, 9000).astype(np.uint8)
    second[:k + 200] = np.resize(np.array([1, 0, 0], dtype=np.uint8), k + 200)
    second[-(k + 150):] = np.resize(np.array([2, 3], dtype=np.uint8), k + 150)
    return [a, second, rng.integers(0, 4, max(1, k - 2)).astype(np.uint8)], tracts


def users_case(capi, q, k, L, options, want_insert, want_query, ranges=None, batched=False):
    """Insert and query with periodic_skip 1 and 0, whole range and two gated halves, against the oracle; the path and the kernels that
    ran are asserted.  Returns nothing: raises on the first difference."""
    recs, tracts = junction_text(k)
    text, codes = packed(capi, recs)
    ref = H.periodic_reference(codes, k)
    o = O.Oracle(k, L, q, O.seed_table(SEED, q, L))
    for r in recs:
        o.add_record(LETTERS[r].tobytes())
    half = 1 << (L - 1)
    ranges = ranges or ((0, 1 << L), (0, half - 1), (half, (1 << L) - 1))
    closed = q > 16
    try:
        for skip in (1, 0):
            ctx = capi.Context(0)
            try:
                for name, val in (("insert_mode", 2), ("query_mode", 2), ("periodic_skip", skip)) + tuple(options):
                    ctx.set_option(name, val)
                ctx.set_params(k, L, q, capi.seed_table(q, L, seed=SEED))
                ctx.seq_upload(text)
                for ri, (lo, hi) in enumerate(ranges):
                    o.fill_only(lo, hi)
                    marks = o.check_only(lo, hi)
                    ctx.filter_reset()
                    ctx.pass1_insert(lo, hi)
                    got = ctx.pass1_query(lo, hi)
                    st = {s: ctx.stat(s) for s in ("insert_path", "query_path", "insert_hash_kernel", "query_hash_kernel", "insert_batches", "query_batches",
                                                   "query_b1", "query_b2", "periodic_skip")}
                    tag = (q, k, L, options, skip, lo, hi, st)
                    if ri == 0 and skip:   # the verdicts inside the tracts differ: a copy from a wrong phase changes the mask
                        mask = H.bits_of_words(o.round_mask, len(codes))
                        for s, ln, p in tracts:
                            if s == tracts[4][0]:
                                continue   # (the one with an N inside)
                            sl = slice(s + p + 1, s + ln - k)
                            assert ref[0][sl][(np.arange(sl.start, sl.stop) % H.PER_TILE) >= 63].all(), ("tract not copying", s, p)
                            if p >= 5:   # (the tract's two ends make a junction of one phase each, the plant of a third)
                                assert 0 < mask[sl].sum() < (sl.stop - sl.start), ("constant verdicts in a tract", s, ln, p, int(mask[sl].sum()))
                    if closed:
                        assert st["insert_path"] == 1 and st["query_path"] == 1, tag
                    else:
                        assert st["insert_path"] in (2, 3) and st["query_path"] in (2, 3), tag
                    assert st["insert_hash_kernel"] == want_insert and st["query_hash_kernel"] == want_query, tag
                    assert st["periodic_skip"] == skip, tag
                    if batched:
                        assert st["insert_batches"] > 1 and st["query_batches"] > 1, tag
                    assert got == marks, ("marks", got, marks) + tag
                    assert (ctx.mask_download(False) == o.round_mask).all(), ("candidate mask",) + tag
                    assert (ctx.filter_download() == o.filter).all(), ("filter bitmap",) + tag
                    yield st
            finally:
                ctx.close()
    finally:
        o.close()


USERS = [
    # q, k, L, options, insert kernel, query kernel, batched
    pytest.param(5, 25, 22, (("slice_bits", 9), ("part_levels", 2)), 1, 1, False, id="lean-seed-table"),
    pytest.param(5, 47, 22, (("slice_bits", 9), ("part_levels", 2)), 2, 1, False, id="lean-no-seed-table"),
    pytest.param(5, 31, 34, (), 1, 1, False, id="L34"),
    pytest.param(5, 25, 26, (("slice_bits", 8), ("part_levels", 2)), 1, 1, False, id="512-bins"),
    pytest.param(3, 25, 23, (("slice_bits", 8), ("part_levels", 3)), 1, 1, False, id="three-levels"),
    pytest.param(5, 25, 22, (("slice_bits", 9), ("part_levels", 2), ("part_min_tiles", 1), ("part_budget_bytes", 64 << 10)), 1, 1, True, id="batches"),
    pytest.param(17, 25, 20, (), 4, 4, False, id="closed-form-q17"),
]


@pytest.mark.parametrize("q,k,L,options,want_insert,want_query,batched", USERS)
def test_hash_kernels_that_read_the_masks(capi, q, k, L, options, want_insert, want_query, batched):
    """Every hash kernel that is handed per_i / per_qs (and the closed form of q = 17, which skips nothing while the copy still runs):
    filter, mask and count equal the oracle's with the skip on and off, on a text whose tracts hold junctions at one phase only."""
    stats = list(users_case(capi, q, k, L, options, want_insert, want_query, batched=batched))
    assert len(stats) == 6
    if dict(options).get("part_levels") == 3:
        assert all(st["insert_path"] == 3 and st["query_path"] == 3 for st in stats)
    if L == 26:
        assert all(st["query_b1"] == 9 for st in stats), stats   # 512 bins: two rounds per position in k_q_hash2
    print("kernels:", stats[0])


def no_lean_sweep():
    """Under TPC_NO_LEAN=1 (a fresh process: the knob is read once): k_part_hash and the ring query hash k_q_hash, at 2^7 and 2^9 bins."""
    from twopaco_amd import capi
    rows = []
    for q, k, L, options in ((5, 25, 22, (("slice_bits", 9), ("part_levels", 2))), (2, 33, 26, (("slice_bits", 8), ("part_levels", 2)))):
        rows += list(users_case(capi, q, k, L, options, 3, 2))
    return rows


def test_hash_kernels_without_the_lean_ones():
    env = dict(os.environ, TPC_NO_LEAN="1")
    code = "import json, sys; sys.path[:0] = [%r, %r]; import test_gpu_periodic as t; print(json.dumps(t.no_lean_sweep()))" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    rows = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(rows) == 12 and all(st["insert_hash_kernel"] == 3 and st["query_hash_kernel"] == 2 for st in rows), rows
    assert {st["query_b1"] for st in rows} == {7, 9}, rows
