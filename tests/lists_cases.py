"""Input texts, source counts and forced list lengths shared by tests/test_gpu_lists.py and tests/test_lists_reference_cpu.py: the
GPU tests rely on list lengths that the CPU test checks against the oracle's filter of the very same texts."""
import numpy as np

import lists_reference as R
from oracle import oracle as O
from test_gpu_combine_lists import LETTERS, _random_records, _skewed_records

K, Q, SEED = 25, 5, 11

# (n_src, n_owner) of tpc_combine_import: 1 .. 16 sources per slice, every residue mod 4 (the reader's groups of four); (64, 8) is
# the all-gather of eight ranks' exports
PAIRS = [(1, 0), (3, 0), (5, 0), (2, 1), (3, 1), (4, 1), (5, 1), (7, 1), (9, 1), (16, 1), (4, 2), (6, 2), (8, 2), (8, 4), (16, 4), (64, 8)]
FEW_PAIRS = [(1, 0), (5, 1), (16, 4), (64, 8)]
STALE_PAIRS = [(5, 1), (8, 4)]  # repeated with fresh == 0

# name: (L, slice_bits, positions; 0 = the skewed text).  F = L - slice_bits decides the query's entries: b2 = F / 2 >= 4 takes the
# 6-byte entries (k_apply_lookup6), below that the planner keeps the 8-byte ones (k_apply_lookup)
TEXTS = {
    "dense6": (24, 16, 1100000),        # ~18 k of a window's 65536 bits: past 16 T + 3 = 16387 entries of a list (T = 1024 threads)
    "dense6_4win": (26, 18, 1000000),   # ~4.7 k bits per window, 16 T + 3 = 4099 (T = 256)
    "sparse6": (24, 16, 8000),          # the m2_like density: ~150 bits per window
    "small6": (16, 8, 3000),            # 256-bit windows
    "skewed6": (24, 12, 0),
    "dense8": (22, 16, 1000000),        # more than half of every window
    "dense8_16win": (26, 20, 500000),   # ~2.4 k bits per window, 16 T + 3 = 1027 (T = 64)
    "sparse8": (22, 16, 2000),
}
DENSE = ["dense6", "dense6_4win", "dense8", "dense8_16win"]  # every forced length exists in these
FMT6 = [("dense6", PAIRS), ("sparse6", PAIRS), ("dense6_4win", FEW_PAIRS), ("small6", FEW_PAIRS), ("skewed6", [(5, 1)])]
FMT8 = [("dense8", PAIRS), ("sparse8", PAIRS), ("dense8_16win", FEW_PAIRS)]


def records(name):
    L, _, n_pos = TEXTS[name]
    return _random_records(n_pos, seed=L + n_pos) if n_pos else _skewed_records()


def oracle_for(name):
    L = TEXTS[name][0]
    o = O.Oracle(K, L, Q, O.seed_table(SEED, Q, L))
    for r in records(name):
        o.add_record(LETTERS[r].tobytes())
    return o


def lengths(windows, full):
    """The list lengths to force, T = 1024 / windows threads reading a window: around one load of a thread (8 entries), around the
    first load of all of them (8 T), into the streaming branch (16 T + 3), and the whole window."""
    T = 1024 // windows
    return [0, 1, 7, 8, 9, 8 * T - 1, 8 * T, 8 * T + 1, 16 * T + 3, full]


def forced_cells(filter_words, geom, n_src, n_owner):
    """{(source, permuted slice, window): n} over the densest windows of the filter: at most three forced sources in a window and one
    left free (a window with a single source can only list all of its bits).  "The whole window" is every bit the window holds; a
    length the densest windows do not reach is left out."""
    lay = R.Layout(n_src, n_owner)
    _, sp, win, _ = R.filter_bits(filter_words, geom)
    count = np.bincount(sp * geom["windows"] + win, minlength=geom["slices"] * geom["windows"])
    cell = np.flatnonzero(count)
    count = count[cell]
    order = np.argsort(-count, kind="stable")
    c = n_src // n_owner if n_owner else n_src
    per_window = max(1, min(3, c - 1))
    forced, at = {}, 0
    todo = lengths(geom["windows"], None)
    if c == 1:
        todo = [None]
    for j in range(0, len(todo), per_window):
        if at >= order.size:
            break
        fsp, fw, have = int(cell[order[at]] // geom["windows"]), int(cell[order[at]] % geom["windows"]), int(count[order[at]])
        at += 1
        srcs = lay.sources_of(geom, fsp)
        for i, n in enumerate(todo[j:j + per_window]):
            n = have if n is None else n
            if n <= have:
                forced[(srcs[(i + j) % c], fsp, fw)] = n
    return forced
