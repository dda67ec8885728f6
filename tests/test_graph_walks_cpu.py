"""CPU: tests/graph_walks.py, the generated topologies that tests/test_gpu_graph_walks.py holds the six graph-table stages against.
Every builder runs here, so every property a builder asserts is checked without a device; the serial `graphdump -f gfa1` accepts every
small case (and prints the bytes of the reference's own graphdump, recorded in tests/golden/graph_walks.json and run again where its
binary is present); the vectorised tile writer equals segments_reference.build_stream; the tiling rule holds table for table; the
numpy reference of the large cases equals the oracles on small ones; and the serial program's own tables of forest and bound are the
oracles' bytes."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import bubbles_reference as B
import colors_reference as C
import components_reference as CM
import distances_reference as D
import graph_walks as G
import links_reference as L
import superbubbles_reference as S
from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPHDUMP_REF = os.path.join(ROOT, "oracle", "_ref", "graphdump_ref")
WALKS_GOLDEN = os.path.join(GOLDEN, "graph_walks.json")
SMALL = {"forest": lambda: forest(), "bound": lambda: bound(), "tile": lambda: G.tiles_case("tile", 1), "tiles_3": lambda: G.tiles_case("tiles_3", 3),
         "chain_up_1000": lambda: G.build_chain("chain_up_1000", 1000, "up"), "chain_down_1000": lambda: G.build_chain("chain_down_1000", 1000, "down"),
         "chain_shuffled_1000": lambda: G.build_chain("chain_shuffled_1000", 1000, "shuffled"), "late_hub_300": lambda: G.build_late_hub("late_hub_300", 300),
         "first_hub_300": lambda: G.build_late_hub("first_hub_300", 300, hub_first=True), "zero_start": lambda: G.case_of_ids("zero_start", [np.arange(0, 6)])}
_BUILT = {}


def small(name):
    if name not in _BUILT:
        _BUILT[name] = SMALL[name]()
    return _BUILT[name]


def forest():
    return G.build_forest()


def bound():
    return G.build_bound()


def run_walk(exe, c, d):
    fa, stream = c.files(d)
    return subprocess.run([exe, os.path.basename(stream), "-k", str(c.k), "-s", os.path.basename(fa), "-f", "gfa1"], cwd=d, capture_output=True, timeout=600)


# ---------------------------------------------------------------------------------------------------------------- the builders
@pytest.mark.parametrize("name", sorted(SMALL))
def test_the_real_walks_accept_the_case(tmp_path, name):
    """The builder's assertions hold, this project's serial graphdump prints the recorded bytes with an empty stderr, and so does the
    reference's graphdump where it has been built."""
    c = small(name)
    record = json.load(open(WALKS_GOLDEN))[name]
    for exe in [C.GRAPHDUMP] + ([GRAPHDUMP_REF] if os.path.exists(GRAPHDUMP_REF) else []):
        d = tmp_path / os.path.basename(exe)
        d.mkdir()
        r = run_walk(exe, c, str(d))
        assert r.returncode == 0 and r.stderr == b"", (exe, r.stderr[-400:])
        assert len(r.stdout) == record["stdout_bytes"] and hashlib.sha256(r.stdout).hexdigest() == record["stdout_sha256"], exe
    assert c.gfa1() == r.stdout


def test_the_recorded_walks_are_all_there():
    assert set(json.load(open(WALKS_GOLDEN))) == set(SMALL)


@pytest.mark.parametrize("order", ["up", "down", "shuffled"])
def test_the_large_chains_build(order):
    c = G.build_chain("chain_" + order, order=order)
    assert c.direct.rows == G.CHAIN_ROWS > 65536 and c.w.name.size >= G.CHAIN_ROWS


@pytest.mark.parametrize("hub_first", [False, True])
def test_the_large_hubs_build(hub_first):
    c = G.build_late_hub("hub", hub_first=hub_first)
    assert c.direct.rows == G.HUB_LEAVES + 1


def test_the_forest_takes_about_three_seconds():
    assert small("forest").oracle_seconds < 30


# ---------------------------------------------------------------------------------------------------------------- the vectorised writer
def test_the_vectorised_tiles_are_build_streams_bytes():
    a, b = G.tiles_case("a", 3), G.tiles_case("b", 3, vectorised=False)
    assert a.data == b.data and len(a.seqs) == len(b.seqs) and all((x == y).all() for x, y in zip(a.seqs, b.seqs)) and a.color_of_seq == b.color_of_seq
    assert a.color_of_seq[:8] == a.color_of_seq[8:16] == a.color_of_seq[16:] and set(a.color_of_seq) == {0, 1, 2}
    c = G.build_chain("c", 50, "shuffled")      # the group writer of the chains and hubs, against build_stream as well
    again = G.R.build_stream([(G.GAP * np.arange(2), ids) for ids in c.groups[0]] + [(G.GAP * np.arange(51), c.groups[1])], last_separator=True)
    assert c.data == again and len(c.seqs) == 51 and [len(x) for x in c.seqs] == [6] * 50 + [153]
    one = G.tiles_case("one", 1)
    assert a.data[:len(one.data)] == one.data and len(a.data) == 3 * len(one.data)


# ---------------------------------------------------------------------------------------------------------------- the tiling rule
@pytest.mark.parametrize("T", [3, 5])
def test_the_tiling_rule(T):
    """Every oracle table of the tile written T times == the arithmetic from one tile: links, colours, bubbles (rows, sides, histogram),
    components, superbubbles (exit[], rows, members, presence) and the distance matrices."""
    one = small("tile").oracles()
    assert G.tile_ok(one)
    real = (small("tiles_3") if T == 3 else G.tiles_case("tiles_5", 5)).oracles()
    want = G.tiled(one, T, G.TILE_IDS)
    assert G.same_arrays(G.arrays_of(real), G.arrays_of(want)) is None
    assert real.superbubbles.count() == T * one.superbubbles.count() >= 2 * T and real.components.count() == T * one.components.count()
    # and it is no identity: the shifted fields differ from a plain repeat
    assert int(want.components.component.max()) == T * one.components.count() - 1 and int(want.superbubbles.entrance.max()) > 2 * len(one.colors["name"])
    assert (want.colors["name"] >= G.R.FRESH).sum() == T and len(set(want.colors["name"].tolist())) == T * len(one.colors["name"])


def test_the_tile_counts_pass_every_grid_limit():
    one = small("tile").oracles()
    rows, links, events = len(one.colors["name"]), one.links.rows(), one.events
    T = G.tiles_for(one, "full")
    assert T * rows > G.TURN and T * links > G.TURN and T * events > G.TURN and 2 * T * links >= G.TURN       # rows, link rows, events, arc keys
    assert T * int((one.bubbles.deg >= 2).sum()) > G.TURN_SEARCH and 2 * T * rows > G.TURN_HIST and T * one.superbubbles.count() > G.TURN_REPORT
    assert (T - 1) * min(rows, links, events) <= G.TURN + 2 * min(rows, links, events)                           # and no larger than that takes
    assert G.tiles_for(one, "report") * one.superbubbles.count() > G.TURN_REPORT
    assert 8 * 4 * G.TILE_IDS * T < 1 << 28                                                                     # the first-sight table stays small


# ---------------------------------------------------------------------------------------------------------------- the numpy reference
@pytest.mark.parametrize("name", ["chain_up_1000", "chain_down_1000", "chain_shuffled_1000", "late_hub_300", "first_hub_300"])
def test_direct_equals_the_oracles(name):
    c = small(name)
    assert G.same_arrays(G.arrays_of(c.oracles()), G.arrays_of(c.direct)) is None


def test_label_propagation_equals_the_breadth_first_search():
    for name in ("forest", "chain_shuffled_1000", "tiles_3"):
        m = small(name).oracles().components
        a, b = np.array([p[0] for p in m.pairs], dtype=np.int64), np.array([p[1] for p in m.pairs], dtype=np.int64)
        assert G.classes_by_labels(m.rows, a, b).tolist() == CM.classes_of(m.rows, m.pairs)
    assert G.classes_by_labels(3, [], []).tolist() == [0, 1, 2]


# ---------------------------------------------------------------------------------------------------------------- the serial tables
@pytest.mark.parametrize("name", ["forest", "bound"])
def test_the_serial_tables_equal_the_oracles(tmp_path, name):
    """graphdump --links / --colors / --bubbles / --components / --superbubbles / --distances on the generated shapes."""
    c = small(name)
    d = str(tmp_path)
    fa, stream = c.files(d)
    args = [os.path.basename(stream), "-k", str(c.k), "-s", os.path.basename(fa)]
    text = c.gfa1()

    def serial(more):
        r = C.run_graphdump(args + more, cwd=d)
        assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
        return r.stdout

    assert serial(["--links"]) == L.Links(text).tsv(c.k)
    assert serial(["--colors", "file"]) == C.tsv(text, "file", c.k)[0]
    assert serial(["--bubbles", "file"]) == B.Bubbles(text, "file").tsv(c.k)
    assert serial(["--distances", "file"]) == D.tsv(text, "file", c.k)[0]
    assert serial(["--components", "file"]) == CM.Components(text, "file", k=c.k).tsv()
    for max_inside in (62,) if name == "forest" else (2, 8, 61, 62):
        members = os.path.join(d, "members_%d.tsv" % max_inside)
        want = S.Superbubbles(text, c.k, "file", max_inside=max_inside)
        assert serial(["--superbubbles", "file", "--superbubbles-members", members, "--superbubbles-max", str(max_inside)]) == want.tsv()
        assert open(members, "rb").read() == want.members_tsv()


def test_a_segment_named_0_drops_its_l_line_and_keeps_its_link(tmp_path):
    """Why no builder uses junction id 0.  Junction 0 read forward before an A names its segment 0, and 0 is the serial walk's (and the
    reference's) "no segment yet": the gfa1 text has no L line for the occurrence behind it, so the oracles, which read the L lines, do
    not know that link.  The link table's definition counts every event that is not the first of its sequence, and so does the serial
    `--links`: it holds one row more, 0+ -> 8+.  (A name of 0 cannot carry a strand either: -0 is 0.)"""
    c = small("zero_start")
    assert c.w.name.tolist() == [0, 8, 16, 24, 32]
    text = c.gfa1()
    want = L.Links(text)
    assert want.rows() == 3 and text.count(b"\nL\t") == 3 and want.events == 5
    fa, stream = c.files(str(tmp_path))
    r = C.run_graphdump([os.path.basename(stream), "-k", str(c.k), "-s", os.path.basename(fa), "--links"], cwd=str(tmp_path))
    assert r.returncode == 0 and r.stderr == b""
    lines, ref = r.stdout.decode().split("\n"), want.tsv(c.k).decode().split("\n")
    assert lines[0] == "#twopaco-links\t1\tk=3\tsegments=5\tlinks=4\toccurrences=4" and lines[1] == "0\t+\t8\t+\t1\t1" and lines[2:] == ref[1:]


# ---------------------------------------------------------------------------------------------------------------- recording
if __name__ == "__main__":
    # python tests/test_graph_walks_cpu.py : writes tests/golden/graph_walks.json from the reference's own graphdump
    import tempfile
    assert os.path.exists(GRAPHDUMP_REF), "the reference's graphdump has not been built (oracle/Makefile: ref)"
    out = {}
    for name in sorted(SMALL):
        with tempfile.TemporaryDirectory() as d:
            r = run_walk(GRAPHDUMP_REF, small(name), d)
        assert r.returncode == 0 and r.stderr == b"", (name, r.stderr)
        out[name] = {"stdout_bytes": len(r.stdout), "stdout_sha256": hashlib.sha256(r.stdout).hexdigest()}
    with open(WALKS_GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", len(out), "walks")
