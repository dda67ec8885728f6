"""GPU (-m gpu): the six graph-table stages behind the segment build -- colours (csrc/tpc_colors.hip), links (tpc_links.hip), simple
bubbles (tpc_bubbles.hip), connected components (tpc_components.hip), superbubbles (tpc_superbubbles.hip), distances
(tpc_distances.hip) -- on GENERATED TOPOLOGIES (tests/graph_walks.py): synthetic junction streams whose ids decide the graph, held
against the independent oracles where they can be afforded (forest, bound), against a numpy statement of the definition pinned to those
oracles (chains and hubs of 100 000 to 300 000 segments) and against one tile's oracles repeated by arithmetic (tiles: past 65 535
reported superbubbles; past 2 097 152 segments, links and events, which is past every other grid limit of these stages as well).
tests/test_graph_walks_cpu.py runs every builder and pins the three references to each other without a device.

Every case goes to a fresh Context(0): seq_upload, segments_build from the stream's bytes, then colours, links, bubbles, components,
superbubbles, distances, each compared in full and exactly -- every fetched array, every info[] field, segments_error() is None.  The
link, bubble, component and superbubble comparisons are the check_table bodies of the stages' own GPU tests.

Measured on an MI355X, two runs (kernel_ms of the stage; wall time of the whole test with its builder, packing and comparison):
    tiles_full      2 097 228 segments, 2 147 162 links, 2 646 502 events, 99 868 superbubbles: colours 0.18 ms, links 1.03, bubbles 0.42,
                    components 0.49, superbubbles 1.08, distances 0.46; the test 1.0 s, of which the tile writer and the arithmetic
                    reference 0.2 s, packing 399 472 records 0.6 s, upload, seven builds, every fetch and comparison 0.2 s: the host's
                    record-by-record packing dominates, not the device
    tiles_report    1 376 298 segments, 65 538 superbubbles, then the forest on the same context: the test 0.6 s
    chain_up / chain_down / chain_shuffled (300 000 segments)   components 0.5 .. 4.5 / 49 .. 89 / 0.55 ms; the tests 0.1 / 0.2 / 0.7 s
    late_hub / first_hub (100 001 segments)                     components 1.9 .. 2.6 / 1.4 ms; the tests 0.4 / 0.2 s
    forest 1.4 s (its oracles), bound 0.1 s for the four bounds; the whole file 5.6 s
The descending chain is the slow one -- every hook lands under the row before it and the finds walk long paths until halving catches
up -- and stays a factor of ten below the second of kernel time at which the union-find would be a finding: every case runs at its
full size."""
import time

import numpy as np
import pytest

import graph_walks as G
import segments_reference as R
import test_gpu_bubbles as TB
import test_gpu_components as TC
import test_gpu_links as TL
import test_gpu_superbubbles as TS
from colors_reference import presence_words

pytestmark = pytest.mark.gpu

_BUILT = {}
BUILDERS = {"forest": lambda: G.build_forest(), "bound": lambda: G.build_bound(),
            "chain_up": lambda: G.build_chain("chain_up", order="up"), "chain_down": lambda: G.build_chain("chain_down", order="down"),
            "chain_shuffled": lambda: G.build_chain("chain_shuffled", order="shuffled"),
            "late_hub": lambda: G.build_late_hub("late_hub"), "first_hub": lambda: G.build_late_hub("first_hub", hub_first=True),
            "tiles_report": lambda: G.build_tiles("tiles_report", G.tiles_for(G.tiles_case("tile", 1).oracles(), "report")),
            "tiles_full": lambda: G.build_tiles("tiles_full", G.tiles_for(G.tiles_case("tile", 1).oracles(), "full"))}


def case(name, keep=True):
    """Built once, shared, never changed (keep=False: built for one test and dropped, for the cases of hundreds of megabytes)."""
    if name in _BUILT:
        return _BUILT[name]
    c = BUILDERS[name]()
    if keep:
        _BUILT[name] = c
    return c


@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


def packed_text(capi, c):
    """The case's text (ACGTN only) as the host packs it."""
    lens = np.array([s.size for s in c.seqs], dtype=np.int64)
    codes = R.codes_of(np.concatenate(c.seqs))
    ends = np.cumsum(lens)
    text = capi.PackedText.from_codes([codes[a:b] for a, b in zip((ends - lens).tolist(), ends.tolist())])
    assert (text.rec_length.astype(np.int64) == lens).all()
    return text


def segments(capi, ctx, c):
    """The case's segment table on ctx; returns the build's counts."""
    text = packed_text(capi, c)
    ctx.seq_upload(text)
    counts = ctx.segments_build(c.data, c.k, text.rec_start, text.rec_length)
    assert ctx.segments_error() is None
    return counts


def check_colours(ctx, c, want):
    """Everything the device holds after a colour build == the reference's colour table."""
    t = want.colors
    rows, words = len(t["name"]), (c.n_colors + 31) // 32
    assert ctx.segments_colors_build(c.color_of_seq, c.n_colors) == {"rows": rows, "colors": c.n_colors, "words": words}
    first, occ, fwd, ncol = ctx.segments_colors_fetch_rows()
    assert first.dtype == occ.dtype == fwd.dtype == ncol.dtype == np.uint32 and first.size == rows
    assert (first == want.first_event).all() and (occ == t["occurrences"]).all() and (fwd == t["forward"]).all() and (ncol == t["n_colors"]).all()
    name, first_bits = ctx.segments_fetch()
    begin, end = ctx.segments_fetch_events()
    assert name.size == want.events and (np.nonzero(first_bits)[0] == want.first_event).all() and (np.abs(name[first]) == t["name"]).all()
    assert (end[first].astype(np.int64) - begin[first] + c.k == t["length"]).all()
    presence = ctx.segments_colors_fetch_presence()
    assert presence.dtype == np.uint32 and presence.shape == (rows, words) and (presence == presence_words(t["presence"])).all()
    seg, bases = ctx.segments_colors_fetch_hist()
    assert seg.dtype == bases.dtype == np.uint64 and (seg.astype(np.int64) == t["hist_segments"]).all() and (bases.astype(np.int64) == t["hist_bases"]).all()
    assert ctx.kernel_ms("colors") > 0


def check_distances(ctx, c, want):
    want_s, want_e = want.distances
    info = ctx.segments_distances_build()
    weights = want.colors["length"] - c.k
    assert (info["colors"], info["rows"], info["planes"]) == (c.n_colors, len(weights), int(weights.max()).bit_length())
    seg, edg = ctx.segments_distances_fetch()
    assert seg.dtype == edg.dtype == np.uint64 and seg.shape == edg.shape == (c.n_colors, c.n_colors)
    assert (seg.astype(np.int64) == want_s).all() and (edg.astype(np.int64) == want_e).all()
    assert ctx.kernel_ms("distances") > 0


STAGES = ("colors", "links", "bubbles", "components", "superbubbles", "distances")


def check_all(capi, ctx, c, want, counts):
    """The six stages in the order of the module's text, each compared in full; returns {stage: kernel_ms}."""
    rows = len(want.colors["name"])
    assert (counts["events"], counts["segments"], counts["n_named"]) == (want.events, rows, want.n_named)
    check_colours(ctx, c, want)
    TL.check_table(ctx, want.links)
    TB.check_table(ctx, want.bubbles)
    TC.check_table(ctx, want.components)
    TS.check_table(ctx, want.superbubbles)
    check_distances(ctx, c, want)
    assert ctx.segments_error() is None
    return {stage: ctx.kernel_ms(stage) for stage in STAGES}


def report(name, t0, ms, **more):
    print("\n%s: test %.1f s so far;" % (name, time.time() - t0), " ".join("%s %.3f ms" % kv for kv in ms.items()), " ".join("%s %s" % kv for kv in more.items()))


# ---------------------------------------------------------------------------------------------------------------- against the oracles
def test_forest_equals_the_oracles(capi):
    t0 = time.time()
    c = case("forest")
    ctx = capi.Context(0)
    try:
        ms = check_all(capi, ctx, c, c.oracles(), segments(capi, ctx, c))
    finally:
        ctx.close()
    report("forest", t0, ms)


@pytest.mark.parametrize("max_inside", [2, 8, 61, 62])
def test_bound_equals_the_oracles(capi, max_inside):
    """Superbubbles of 61, 62 and 63 sides inside and sides of out-degree 64 and 65 and in-degree 65, at every bound."""
    c = case("bound")
    want = c.oracles(max_inside)
    assert want.superbubbles.count() == {2: 0, 8: 0, 61: 1, 62: 2}[max_inside]
    ctx = capi.Context(0)
    try:
        check_all(capi, ctx, c, want, segments(capi, ctx, c))
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- chains and hubs
@pytest.mark.parametrize("name", ["chain_up", "chain_down", "chain_shuffled", "late_hub", "first_hub"])
def test_chains_and_hubs_equal_the_definition(capi, name):
    """One component of 100 001 or 300 000 segments that the union-find has to hook in row order, against it, in a random order, and
    all at one root: component[], root, every sum plane, presence and largest; link rows, counts and first bits; the bubble histogram
    with the hub in its 5+ bin and an empty bubble table; no superbubble.  Then again with test_components_step_limit set to the
    segment count: the build still succeeds -- path halving and hooking by roots keep every find far below the bound S + 1."""
    t0 = time.time()
    c = case(name, keep=False)
    want = c.direct
    ctx = capi.Context(0)
    try:
        ms = check_all(capi, ctx, c, want, segments(capi, ctx, c))
        assert ctx.segments_bubbles_info()["bubbles"] == 0 and ctx.segments_superbubbles_info()["superbubbles"] == 0
        assert ctx.segments_components_info()["components"] == 1 and ctx.segments_components_info()["largest"] == want.rows
        try:
            ctx.set_option("test_components_step_limit", want.rows)
            TC.check_table(ctx, want.components)
            limited = ctx.kernel_ms("components")
        finally:
            ctx.set_option("test_components_step_limit", 0)
    finally:
        ctx.close()
    report(name, t0, ms, components_limited_ms="%.3f" % limited, segments=want.rows)
    assert ms["components"] < 1000, "a second of kernel time for one chain: a finding about the union-find (DESIGN.md 3.11)"


# ---------------------------------------------------------------------------------------------------------------- past the grids
def check_windows(ctx, want, rows_at, sides_at, links_at, report_at):
    """The fetch ranges (r0, n) on windows that straddle the given items, off every word and wave boundary."""
    t, m, s, l, b = want.colors, want.components, want.superbubbles, want.links, want.bubbles
    for at in rows_at:
        r0, n = at - 70, 141
        got = ctx.segments_colors_fetch_rows(r0, n)
        for a, ref in zip(got, (want.first_event, t["occurrences"], t["forward"], t["n_colors"])):
            assert (a == ref[r0:r0 + n]).all()
        assert (ctx.segments_colors_fetch_presence(r0, n) == presence_words(t["presence"][r0:r0 + n])).all()
        assert (ctx.segments_components_fetch_members(r0, n) == m.component[r0:r0 + n]).all()
    for at in links_at:
        r0, n = at - 70, 141
        for a, ref in zip(ctx.segments_links_fetch_rows(r0, n), (l.first_event, l.count, l.same)):
            assert (a == ref[r0:r0 + n]).all()
    for at in sides_at:
        c0, n = at - 70, 141
        for a, ref in zip(ctx.segments_bubbles_fetch_sides(c0, n), (b.deg, b.lo, b.hi)):
            assert (a == ref[c0:c0 + n]).all()
        assert (ctx.segments_superbubbles_fetch_exits(c0, n) == s.exit[c0:c0 + n]).all()
    for at in report_at:
        b0 = at - 5
        n = min(10, s.count() - b0)
        assert n > 5
        got = ctx.segments_superbubbles_fetch_rows(b0, n)
        for a, ref in zip(got, (s.entrance, s.exits, s.inside, s.arcs, s.n_colors, s.paths, s.min_edges, s.max_edges)):
            assert (a.astype(np.uint64) == ref[b0:b0 + n].astype(np.uint64)).all()
        assert (ctx.segments_superbubbles_fetch_presence(b0, n) == presence_words(s.presence[b0:b0 + n])).all()


def test_tiles_past_the_report_grid_and_a_forest_behind_them(capi):
    """Just past 65 535 reported superbubbles (k_sb_report's rows), the window at row 65 535 -- and then the forest on the same
    context: every table and size is the forest's, nothing of the tiles is left."""
    t0 = time.time()
    c = case("tiles_report", keep=False)
    want = c.want
    assert G.TURN_REPORT < want.superbubbles.count() <= G.TURN_REPORT + 2 * c.tile.superbubbles.count()
    ctx = capi.Context(0)
    try:
        ms = check_all(capi, ctx, c, want, segments(capi, ctx, c))
        check_windows(ctx, want, (), (), (), (G.TURN_REPORT,))
        report("tiles_report", t0, ms, segments=len(want.colors["name"]), superbubbles=want.superbubbles.count())
        f = case("forest")
        check_all(capi, ctx, f, f.oracles(), segments(capi, ctx, f))
    finally:
        ctx.close()


def test_tiles_past_every_grid(capi):
    """Segments, links and events each past 2 097 152 (col_grid: events, link slots, link rows, segment rows; sides and arc keys are
    past it twice), which is past 524 288 superbubble candidates, 262 144 sides and 65 535 reported rows as well; the windows at item
    2 097 152 of the rows, the link rows and the sides (and at the sides of row 2 097 152) and at superbubble row 65 535."""
    t0 = time.time()
    c = case("tiles_full", keep=False)
    want, one = c.want, c.tile
    rows, links = len(want.colors["name"]), want.links.rows()
    assert min(rows, links, want.events) > G.TURN and want.superbubbles.n_arcs > G.TURN and want.superbubbles.count() > G.TURN_REPORT
    assert c.T * int((one.bubbles.deg >= 2).sum()) > G.TURN_SEARCH and 2 * rows > G.TURN_HIST
    t1 = time.time()
    text = packed_text(capi, c)
    t2 = time.time()
    ctx = capi.Context(0)
    try:
        ctx.seq_upload(text)
        counts = ctx.segments_build(c.data, c.k, text.rec_start, text.rec_length)
        t3 = time.time()
        ms = check_all(capi, ctx, c, want, counts)
        check_windows(ctx, want, (G.TURN,), (G.TURN, 2 * G.TURN), (G.TURN,), (G.TURN_REPORT,))
    finally:
        ctx.close()
    report("tiles_full", t0, ms, segments=rows, links=links, events=want.events, superbubbles=want.superbubbles.count(), build_s="%.1f" % (t1 - t0), pack_s="%.1f" % (t2 - t1),
           upload_and_segments_s="%.1f" % (t3 - t2), stages_and_compare_s="%.1f" % (time.time() - t3))
