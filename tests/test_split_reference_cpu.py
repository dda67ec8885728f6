"""No device: tests/split_reference.py against the oracle, and every condition tests/test_gpu_split_pass.py puts on its inputs.

The reference's distinct_hist must be Oracle.split_bins() bin for bin wherever no edge is ever falsely "already seen": on the three
collision-free goldens and on every generated exact case.  The conditions (every edge must-win, the shares of held addresses of the
crowded and sparse cases, the layouts of the mask cases) are assertions here, with the measured count in the message, so that a
generated text that stops meeting its condition fails before any device is involved."""
import os

import numpy as np
import pytest

import split_reference as S
from helpers import GOLDEN, golden_cases
from oracle import oracle as O

GOLDENS = ("rand6_k9_L24_r4", "c2_k29_L26_r3", "lk_k603_r2")


def oracle_bins(recs, k, L, q, seed=S.SEED):
    o = O.Oracle(k, L, q, O.seed_table(seed, q, L))
    for r in recs:
        o.add_record(S.LETTERS[np.asarray(r, dtype=np.uint8)].tobytes())
    bins = o.split_bins().astype(np.int64)
    o.close()
    return bins


def check_exact(case, ref):
    """The exact condition and what follows from it."""
    ph = S.phases_of(case["q"], ref.n_text, case["L"])
    lost = int((~ref.must_win(ph)).sum())
    assert lost == 0, "%d of %d edges are not must-win in %d phases" % (lost, ref.n_edges, ph)
    assert ref.bins_agree(), "the occurrences of one address tuple name different bins"
    assert ref.same_edge_everywhere(), "two different (k+1)-mers share all %d addresses" % case["q"]
    want = oracle_bins(ref.recs, case["k"], case["L"], case["q"], case.get("seed", S.SEED))
    got = ref.distinct_hist()
    assert int(got.sum()) == 2 * ref.n_edges
    assert (got == want).all(), np.nonzero(got != want)[0][:10]
    assert (ref.lower_hist(ph) == got).all()


@pytest.mark.parametrize("name", GOLDENS)
def test_reference_is_the_oracle_on_the_collision_free_goldens(name):
    c = [c for c in golden_cases() if c["name"] == name][0]
    case = {"k": c["k"], "L": c["L"], "q": c["q"], "seed": c["seed"]}
    ref = S.SplitReference(S.recs_of_fasta(os.path.join(GOLDEN, c["fasta"])), c["k"], c["L"], c["q"], c["seed"])
    assert ref.n_edges > 0
    check_exact(case, ref)


@pytest.mark.parametrize("name", sorted(S.EXACT))
def test_exact_cases_meet_their_condition_and_the_oracle(name):
    case = S.EXACT[name]
    ref = S.reference(case)
    if name == "short_only":
        assert ref.pos.size == 0 and ref.n_edges == 0 and not ref.distinct_hist().any() and (ref.rec_len < case["k"]).all() and ref.rec_len.size > 1
    else:
        assert ref.pos.size >= ref.n_edges > 0, (ref.pos.size, ref.n_edges)
    check_exact(case, ref)
    assert S.kernel_of(case["q"], case["force_anyq"]) == (4 if case["q"] > 16 or name.endswith("_anyq") else 0)


def test_positions_are_the_ranges_of_the_dispatched_records():
    for name in ("mask_k3", "tile_edges_k3", "q5", "short_only"):
        ref = S.reference(S.EXACT[name])
        want = [g for s, n in zip(ref.rec_start.tolist(), ref.rec_len.tolist()) if n >= ref.k for g in range(s - 1, s + n - ref.k + 1)]
        assert ref.pos.tolist() == want, name
        assert int(np.unpackbits(ref.mask_words().view(np.uint8)).sum()) == len(want)
        assert not want or (ref.text[ref.pos[0]] == 4 and want[-1] + ref.k < ref.n_text)


@pytest.mark.parametrize("q", [1, 5, 16, 17, 64])
def test_hash_count_text_has_its_features(q):
    """About three tiles; N runs, a poly-A head, a tract across the first tile border, records of k - 1, k and k + 1 letters."""
    case = S.EXACT["q%d" % q]
    ref, k = S.reference(case), case["k"]
    assert 2 * S.TILE < ref.n_text <= 3 * S.TILE, ref.n_text
    assert ref.rec_len.tolist()[-3:] == [k - 1, k, k + 1]
    t = ref.text
    assert (t[1:-1] == 4).sum() > len(ref.recs) and (t[S.TILE - 100:S.TILE + 100].reshape(-1, 2) == t[S.TILE - 100:S.TILE - 98]).all()
    s1 = int(ref.rec_start[1])
    assert (t[s1:s1 + 300] == 0).all()
    assert ref.pos.size - ref.n_edges > 1000, "edges that occur more than once: %d" % (ref.pos.size - ref.n_edges)


@pytest.mark.parametrize("total", [S.TILE - 1, S.TILE, S.TILE + 1, 2 * S.TILE + 1])
def test_total_texts_have_their_length(total):
    ref = S.reference(S.EXACT["total%d" % total])
    assert ref.n_text == total and (ref.rec_len >= ref.k).all()
    assert ref.pos[-1] + ref.k == total - 1, "the last window ends on the text's last position"


@pytest.mark.parametrize("k", [3, 603])
def test_tile_edge_text_has_its_edges(k):
    ref = S.reference(S.EXACT["tile_edges_k%d" % k])
    T = S.TILE
    s, n = ref.rec_start.astype(np.int64), ref.rec_len.astype(np.int64)
    real = n >= k
    ends = (s + n)[real]          # the position of the separator behind a dispatched record
    assert (ends == 2 * T - 1).any(), "a last window that ends on the last position of a tile, on the separator"
    assert (ends - 1 == 4 * T - 1).any(), "... on the record's last letter"
    straddle = ref.pos[(ref.pos < T) & (ref.pos + k >= T)]
    assert straddle.size >= min(k, 20), "k + 1 windows across the border 0 | 1: %d" % straddle.size
    assert not ((ref.pos >= 2 * T) & (ref.pos < 3 * T)).any(), "tile 2 holds no edge"
    assert (ref.pos == 3 * T).any() and (ref.pos >= 4 * T).any()
    assert real[-1]
    if k > 3:   # (k = 3: positions share the few 4-mers there are; the k = 603 text shows every single position)
        assert ref.n_edges == ref.pos.size, (ref.n_edges, ref.pos.size)


@pytest.mark.parametrize("k", [3, 25])
def test_mask_layout_text_has_its_layouts(k):
    ref = S.reference(S.EXACT["mask_k%d" % k])
    s, n = ref.rec_start.astype(np.int64), ref.rec_len.astype(np.int64)
    real = n >= k
    a, b = (s - 1)[real], (s + n - k)[real]
    if k > 3:   # (k = 3 has 136 canonical 4-mers of letters: positions share edges, and only the k = 25 text shows every single one)
        assert ref.n_edges == ref.pos.size, "every position has an edge of its own, so a dropped or an extra one shows: %d edges, %d positions" % (ref.n_edges, ref.pos.size)
    per_word = max(int(((a <= 32 * w + 31) & (b >= 32 * w)).sum()) for w in range(ref.n_text // 32 + 1))
    assert per_word >= (8 if k == 3 else 2), "ranges that meet one word: %d" % per_word
    assert set((n[real][:9] - k).tolist()) == {0, 1, 2}
    assert ((a % 32 == 0) & (b - a == 31)).any(), "a range that is one whole word"
    assert (a % 32 == 31).any() and (b % 32 == 0).any() and ((b >> 5) - (a >> 5) >= 3).any()
    i = np.nonzero(real)[0]
    assert not real[0] and (np.diff(i) > 1).any() and real[-1], "fillers first and between dispatched records, a dispatched record last"
    words = ref.mask_words()
    assert (words == 0xFFFFFFFF).any()
    assert ref.pos[-1] + k == ref.n_text - 1


@pytest.mark.parametrize("name", sorted(S.MASK_CROWDED))
def test_mask_cases_run_q_phases_in_their_crowded_form(name):
    case = S.MASK_CROWDED[name]
    n_text = S.layout(S.case_recs(case))[2]
    assert S.phases_of(case["q"], n_text, case["L"]) == case["q"] and S.phases_of(case["q"], n_text, case["L"] + 1) == 3
    assert case["L"] >= 11


@pytest.mark.parametrize("name", sorted(S.CROWDED))
def test_crowded_cases_meet_their_conditions(name):
    case = S.CROWDED[name]
    ref, q, L = S.reference(case), case["q"], case["L"]
    assert 16 <= L <= 18 and q * ref.n_text > (1 << L) / 8 and S.phases_of(q, ref.n_text, L) == q
    held0 = int(ref.held[:, 0].sum())
    lost = int((~ref.must_win(q)).sum())
    assert held0 >= 0.20 * ref.n_edges, "first address held by another edge: %d of %d edges" % (held0, ref.n_edges)
    assert lost <= 0.05 * ref.n_edges, "not must-win: %d of %d edges" % (lost, ref.n_edges)
    assert ref.pos.size - ref.n_edges > 500, "repeated occurrences: %d" % (ref.pos.size - ref.n_edges)
    assert (ref.lower_hist(q) <= ref.upper_hist()).all() and ref.bins_agree() and ref.same_edge_everywhere()


@pytest.mark.parametrize("name", sorted(S.SPARSE))
def test_sparse_cases_meet_their_conditions(name):
    case = S.SPARSE[name]
    ref, q, L = S.reference(case), case["q"], case["L"]
    assert q * ref.n_text <= (1 << L) / 8 and S.phases_of(q, ref.n_text, L) == 3
    fill = float(np.unpackbits(ref.union_filter().view(np.uint8)).mean())
    assert 0.05 <= fill <= 0.125, "fill %.4f" % fill
    held0 = int(ref.held[:, 0].sum())
    held01 = int(ref.held[:, :2].all(axis=1).sum())
    lost = int((~ref.must_win(3)).sum())
    assert held0 >= 1000, "address 0 held by another edge: %d edges" % held0
    assert held01 >= 50, "addresses 0 and 1 both held: %d edges" % held01
    assert lost <= 0.01 * ref.n_edges, "not must-win: %d of %d edges" % (lost, ref.n_edges)
    lo, hi = ref.lower_filter(3), ref.union_filter()
    assert not (lo & ~hi).any() and (lo != hi).any() == (lost > 0)
    assert ref.bins_agree() and ref.same_edge_everywhere()


def test_boundary_cases_lie_on_either_side_of_crowded():
    c, s = S.BOUNDARY["crowded"], S.BOUNDARY["sparse"]
    assert c["args"] == s["args"] and c["q"] == s["q"] == 4 and s["L"] == c["L"] + 1
    assert S.case_phases(c) == 4 and S.case_phases(s) == 3


def test_both_strands_give_the_histogram_of_one():
    one, both = S.reference(S.STRANDS["one"]), S.reference(S.STRANDS["both"])
    check_exact(S.STRANDS["one"], one)
    check_exact(S.STRANDS["both"], both)
    assert both.n_text == 2 * one.n_text - 1 and both.n_edges == one.n_edges
    assert (both.distinct_hist() == one.distinct_hist()).all()


def test_host_cases_are_exact_cases():
    for q in S.HOST_QS:
        assert "q%d" % q in S.EXACT
