"""CPU: the generated walks of test_gpu_anchors.py without a device -- every small builder runs, the numpy statement of the
definition (anchors_reference.direct) equals the oracle over the serial gfa1 text (part 1) on it, and each case holds the property it
is named after, asserted from the references alone.  The device tests compare the kernels with the numpy statement; this file is
what pins that statement."""
import numpy as np
import pytest

import anchors_reference as R
import graph_walks as G
import test_gpu_anchors as T


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
@pytest.mark.parametrize("n", [1, 63, 257])
def test_one_block(n, reverse):
    rng = np.random.default_rng(1000 + n)
    letters, (pos, ids) = T.reference_walk(rng, n)
    q_letters, q = T.copy_of(letters, ids, 0, n, reverse)
    case = T.walk_case("block%d" % n, [letters, q_letters], [(pos, ids), q], [0, 1], 2)
    o = T.pinned(case)
    assert o.blocks == [(n, 2 * n - 1, 0, n - 1, reverse)] and o.shared[1] == [1, n, G.GAP * n, G.GAP * n if reverse else 0] and o.same_length


def test_the_hot_row():
    case, hot = T.hot_case()
    o = T.pinned(case)
    assert len(o.blocks) == 1 and o.blocks[0][:2] == (hot + 4, hot + 5) and max(len(ev) for ev in o.count.values()) == hot


def test_two_reference_sequences():
    case, m, n = T.two_reference_sequences_case()
    o = T.pinned(case)
    assert [b[:4] for b in o.blocks] == [(n, n + m - 1, 0, m - 1), (n + m, 2 * n - 1, m, n - 1)]
    assert o.mate[n + m] == o.mate[n + m - 1] + 1 and o.seq[o.mate[n + m]] != o.seq[o.mate[n + m - 1]]


def test_the_flag_flips():
    case, n, triples = T.flag_flip_case()
    o = T.pinned(case)
    assert len(o.blocks) == 2 * len(triples) and all(b[0] == b[1] for b in o.blocks)
    for first, second in zip(o.blocks[0::2], o.blocks[1::2]):
        assert second[0] == first[0] + 1 and o.seq[second[0]] == o.seq[first[0]] and o.mate[second[0]] == o.mate[first[0]] - 1 and (first[4], second[4]) == (False, True)


@pytest.mark.parametrize("n_colors", [2, 33])
def test_the_fan(n_colors):
    colours = [1] * 70 if n_colors == 2 else [1 + ((s // 2) * 37) % (n_colors - 1) for s in range(70)]
    o = T.pinned(T.fan_case(n_colors, colours))
    assert len(o.blocks) == 70 and sum(s[1] for s in o.shared) == 280 and [b[4] for b in o.blocks[:4]] == [False, True, False, True]


def test_the_singles_by_the_numpy_statement():
    """70 000 rows are too many for the text oracle to be quick; the same builder at 700 rows is pinned instead."""
    n = 700
    rng = np.random.default_rng(8)
    letters, (pos, ids) = T.reference_walk(rng, n)
    q_ids = np.arange(1, n + 2, 2, dtype=np.int64)
    q_letters = G.LETTERS[rng.integers(0, 4, G.GAP * q_ids.size)]
    q_letters[G.GAP * np.arange(q_ids.size - 1) + G.K] = letters[G.GAP * (q_ids[:-1] - 1) + G.K]
    case = T.walk_case("singles", [letters, q_letters], [(pos, ids), (T.positions(q_ids.size), q_ids)], [0, 1], 2)
    o = T.pinned(case)
    assert len(o.blocks) == n // 2 and all(b[0] == b[1] for b in o.blocks)
