"""CPU: the numpy definition of the periodic-window masks (tests/helpers.py: periodic_reference), which tests/test_gpu_periodic.py
holds the device against, equals a comparison of windows of the text as strings -- and the generators of that file build, by the
reference alone, every case they promise (no GPU needed for either)."""
import numpy as np
import pytest

import helpers as H


def _text(rng, n, k):
    """A few thousand positions: random letters, tracts of periods 1 .. 70 (some with an N inside, some back to back), scattered N,
    separators (N as well: the global text has one code for both), a tract at either end."""
    a = rng.integers(0, 4, n).astype(np.uint8)
    for t in range(40):
        p = int(rng.integers(1, 71))
        ln = int(rng.integers(k + p, k + p + 160))
        at = int(rng.integers(0, n - ln))
        a[at:at + ln] = np.resize(rng.integers(0, 4, p).astype(np.uint8), ln)
        if t % 4 == 0:
            a[at + int(rng.integers(0, ln))] = 4
    a[rng.integers(0, n, 12)] = 4
    a[1:k + 40] = np.resize(np.array([2, 1, 1], dtype=np.uint8), k + 39)
    a[n - k - 30:n - 1] = 3
    a[0] = a[-1] = 4
    return a


@pytest.mark.parametrize("k", [1, 5, 17, 31, 64, 127])
def test_reference_equals_string_comparison(k):
    rng = np.random.default_rng(500 + k)
    a = _text(rng, 4000, k)
    got = H.periodic_reference(a, k)
    want = H.periodic_reference_bruteforce(a, k)
    for name, g, w in zip(("qs", "dist", "ins"), got, want):
        assert (g == w).all(), (name, k, np.nonzero(g != w)[0][:10])
    assert got[0].sum() > 100 and got[2].sum() > got[0].sum() and len(set(got[1].tolist())) > 5, (got[0].sum(), got[2].sum(), len(set(got[1].tolist())))
    assert not (got[0] & ~got[2]).any()  # a k + 2 window that repeats holds a k + 1 window that does


def test_reference_tile_rule_and_window():
    """The first 63 positions of a 16384-position tile never copy (their insert is still dropped); a context that holds the
    characters [lo, hi) sees N outside."""
    k = 9
    a = np.zeros(16384 + 400, dtype=np.uint8)
    a[0] = a[-1] = 4
    a[15000:15800] = np.resize(np.array([0, 1, 3], dtype=np.uint8), 800)
    a[:15000][1:] = np.random.default_rng(1).integers(0, 4, 14999)
    a[15800:-1] = 2
    qs, dist, ins = H.periodic_reference(a, k)
    b = H.periodic_reference_bruteforce(a[14900:], k)  # (the slice starts at 14900: its tile boundary is not the text's)
    assert ins[16384 - 5:16384 + 70].all() and not qs[16384:16384 + 63].any() and qs[16384 + 63:16384 + 70].all() and qs[16384 - 5:16384].all()
    assert (ins[15100:] == b[2][200:]).all()
    lo, hi = 15360, 16000
    w = H.periodic_reference(a, k, lo, hi)
    wb = H.periodic_reference_bruteforce(a, k, lo, hi)
    for g, x in zip(w, wb):
        assert (g == x).all()
    assert not w[2][:lo + 3].any() and not w[2][hi - k:].any() and w[0][lo + 5:hi - k - 1].sum() > 300


def test_copy_reference_follows_chains():
    qs = np.zeros(40, dtype=bool)
    dist = np.zeros(40, dtype=np.uint8)
    qs[10:30] = True
    dist[10:30] = 3
    m = np.zeros(40, dtype=bool)
    m[8] = True
    out = H.periodic_copy_reference(m, qs, dist)
    assert out.nonzero()[0].tolist() == [8, 11, 14, 17, 20, 23, 26, 29]
    w = H.words_of_bits(out, 2)
    assert (H.bits_of_words(w, 40) == out).all()


@pytest.mark.parametrize("k", [5, 18, 25, 62, 603])
def test_constructed_text_holds_its_cases(k):
    """The constructed text of the GPU tests: every assertion it makes from the reference alone holds (periods seen, exact counts at the
    four tract lengths, both fourth-word branches of the pre-test, ...), so a failure on the GPU is the device's."""
    import periodic_cases as C
    case = C.constructed_case(k)
    C.check_constructed(case)
