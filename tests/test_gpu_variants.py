"""GPU (-m gpu): the variants on the device (csrc/tpc_variants.hip, the tpc_segments_variants_* group of include/twopaco_hip.h) against
their definition, restated in variants_reference.py: every array of the traversals, the alleles, their presence words, the sites, the
histogram and info[] through the C-ABI on a host stream and a resident stream, for all golden vectors and the generated inputs at
max_inside 62, 61, 8 and 2; the hot site and the cluster under one and two workgroups (past a grid turn); walks at the ends of their
sequences and a sequence without events; the word-boundary input at 1 .. 65 colours; the stages it leaves untouched, in both orders;
ranges and refusals; the bytes of `graphdump --variants --gpu` and `twopaco --variants`; m2r2 at scale 0.05 by sha256."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import variants_reference as R
from helpers import GOLDEN, case_files, golden_cases
from test_gpu_components import ambiguous_positions, cli, host_context, resident_context
from tracks_reference import BOUNDARY_COLORS, BOUNDARY_K, BOUNDARY_L, BOUNDARY_Q, BOUNDARY_SEED, boundary_fasta

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in golden_cases()}
MAXU = (1 << 64) - 1
GENERATED_CASE = {"k": R.SB_K, "L": R.SB_L, "q": R.SB_Q, "seed": R.SB_SEED, "rounds": [{"low": 0, "high": 1 << R.SB_L}], "n_rounds": 1, "abundance": None}
GENERATED = {"s11": lambda: R.superbubble_records()[:R.SB_RECORDS], "dup": R.duplicated_records, "hot": R.hot_records, "edge": R.edge_records}


@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """The generated inputs: FASTA, junction stream (from the CPU restatement of the pipeline, oracle/), the serial gfa1 and the
    records' letters, made once; the oracles are kept beside them."""
    d = tmp_path_factory.mktemp("variants")
    got = {"dir": str(d)}
    for name, records in GENERATED.items():
        recs = records()
        fa = R.write_fasta(str(d / (name + ".fa")), recs)
        stream = R.oracle_stream(fa, str(d / (name + ".bin")), R.SB_K, R.SB_L, R.SB_Q, R.SB_SEED)
        gfa1 = R.run_graphdump([os.path.basename(stream), "-k", str(R.SB_K), "-s", os.path.basename(fa), "-f", "gfa1"], cwd=str(d))
        assert gfa1.returncode == 0 and gfa1.stderr == b""
        got[name] = {"fasta": fa, "stream": stream, "gfa1": gfa1.stdout, "records": [s for _, s in recs], "oracle": {}}
    return got


def oracle_of(made, name, by="sequence", ref=None, max_inside=62):
    m = made[name]
    key = (by, ref, max_inside)
    if key not in m["oracle"]:
        sb = m["oracle"].get((by, "sb", max_inside))
        m["oracle"][key] = w = R.Variants(m["gfa1"], R.SB_K, [len(s) for s in m["records"]], by, ref, max_inside, records=m["records"], sb=sb)
        m["oracle"][(by, "sb", max_inside)] = w.sb
    return m["oracle"][key]


def generated_context(capi, made, name, source="host"):
    m = made[name]
    data = open(m["stream"], "rb").read()
    return host_context(capi, m["fasta"], data, R.SB_K) if source == "host" else resident_context(capi, dict(GENERATED_CASE, name=name), m["fasta"], data)


def prepare(ctx, want):
    """The three tables the stage reads, under the oracle's colours and bound."""
    ctx.segments_links_build()
    ctx.segments_colors_build(want.color_of_seq, want.n_colors)
    assert ctx.segments_superbubbles_build(want.max_inside)["superbubbles"] == want.sb.count()


def check_arrays(ctx, want, grid=0):
    """Everything the device holds after a variant build == the oracle's arrays.  grid: test_variants_grid for this build."""
    if grid:
        ctx.set_option("test_variants_grid", grid)
    info = ctx.segments_variants_build(want.color_of_seq, want.n_colors, want.ref)
    trav, alle, presence, sites, hist = want.arrays()
    peak = info.pop("peak_bytes")
    assert info == {"sites": want.sites(), "alleles": len(want.alleles), "traversals": len(want.traversals), "strays": 0, "colors": want.n_colors, "ref": want.ref,
                    "hist_bins": hist.size, "superbubbles": want.sb.count()}
    # what the header promises: 44 B per event during the call, 28 B per traversal and 36 B + 4 W B per allele kept
    assert peak >= 44 * ctx.segments_counts()["events"] + 28 * len(want.traversals) + (36 + 4 * presence.shape[1]) * len(want.alleles)
    got_trav = ctx.segments_variants_fetch_traversals()
    for a, ref in zip(got_trav, trav):
        assert a.dtype == ref.dtype and a.size == ref.size and (a == ref).all()
    got_alle = ctx.segments_variants_fetch_alleles()
    for a, ref in zip(got_alle, alle):
        assert a.dtype == ref.dtype and a.size == ref.size and (a == ref).all()
    got = ctx.segments_variants_fetch_presence()
    assert got.dtype == np.uint32 and got.shape == presence.shape and (got == presence).all()
    got_sites = ctx.segments_variants_fetch_sites()
    for a, ref in zip(got_sites, sites):
        assert a.dtype == ref.dtype and a.size == ref.size and (a == ref).all()
    got = ctx.segments_variants_fetch_hist()
    assert got.dtype == np.uint64 and got.size == hist.size and (got == hist).all()
    # the consequences, on the device's arrays alone: an allele's traversals have its edges; the traversals of a site sum to its
    # alleles' counts; alleles <= paths
    allele_of = {(int(r), int(m)): i for i, (r, m) in enumerate(zip(got_alle[0], got_alle[5]))}
    assert len(allele_of) == len(want.alleles)
    for r, m, e in zip(got_trav[3], got_trav[5], got_trav[4]):
        assert int(got_alle[2][allele_of[(int(r), int(m))]]) == int(e)
    off = got_sites[0].astype(np.int64)
    paths = ctx.segments_superbubbles_fetch_rows()[5]
    assert ((off[1:] - off[:-1]).astype(np.uint64) <= paths).all()
    assert [int(got_alle[6][off[b]:off[b + 1]].sum()) for b in range(want.sb.count())] == [int(x) for x in got_sites[1]]
    assert ctx.kernel_ms("variants") > 0 and ctx.segments_error() is None


# ------------------------------------------------------------------------------------------------ 1. the golden vectors
# (the resident stream is made by the plain pipeline of test_gpu_components.resident_context, which has no abundance cut)
VECTOR_SOURCES = [(v, source) for v in R.GOOD_VECTORS for source in ("host", "resident") if source == "host" or CASES[v["case"]]["abundance"] is None]


@pytest.mark.parametrize("v,source", VECTOR_SOURCES, ids=["%s-%s" % (R.vector_id(v), source) for v, source in VECTOR_SOURCES])
def test_variant_arrays_by_their_definition(capi, v, source):
    case = CASES[v["case"]]
    fasta, data = os.path.join(GOLDEN, case["fasta"]), open(os.path.join(GOLDEN, case["bin"]), "rb").read()
    ctx = host_context(capi, fasta, data, case["k"]) if source == "host" else resident_context(capi, case, fasta, data)
    assert ctx.segments_error() is None
    for by in ("sequence", "file"):
        none = R.golden_variants(v, by)
        prepare(ctx, none)
        check_arrays(ctx, none)
        check_arrays(ctx, none)   # a second build replaces the first
        for ref in sorted({0, none.n_colors - 1}):
            check_arrays(ctx, R.golden_variants(v, by, ref))
    ctx.close()


def test_no_event_at_all(capi):
    text = capi.PackedText.from_fasta([os.path.join(GOLDEN, "rand6.fa")])
    ctx = capi.Context(0)
    ctx.seq_upload(text)
    ctx.segments_build(b"", 9, text.rec_start, text.rec_length)
    n_seq = len(text.rec_start)
    ctx.segments_links_build()
    ctx.segments_colors_build([0] * n_seq, 1)
    ctx.segments_superbubbles_build()
    info = ctx.segments_variants_build([0] * n_seq, 1, 0)
    assert (info["sites"], info["alleles"], info["traversals"], info["strays"], info["hist_bins"], info["superbubbles"]) == (0, 0, 0, 0, 1, 0)
    assert all(a.size == 0 for a in ctx.segments_variants_fetch_traversals()) and all(a.size == 0 for a in ctx.segments_variants_fetch_alleles())
    assert ctx.segments_variants_fetch_sites()[0].tolist() == [0] and ctx.segments_variants_fetch_hist().tolist() == [0]
    ctx.close()


# ------------------------------------------------------------------------------------------------ 2. the generated inputs
@pytest.mark.parametrize("source", ["host", "resident"])
@pytest.mark.parametrize("max_inside", [62, 61, 8, 2])
def test_the_generated_input_at_every_bound(capi, made, max_inside, source):
    ctx = generated_context(capi, made, "s11", source)
    for ref in (None, 0, 5, 8):
        want = oracle_of(made, "s11", "sequence", ref, max_inside)
        if ref is None:
            prepare(ctx, want)
        check_arrays(ctx, want)
    inside = [r["inside"] for r in want.sb.rows]
    assert (max(inside) == 62) == (max_inside == 62) and want.sb.count() == {62: 10, 61: 9, 8: 9, 2: 4}[max_inside]
    if max_inside == 62:
        assert any(int(m) >> 61 & 1 for m in ctx.segments_variants_fetch_traversals()[5])
        by_file = oracle_of(made, "s11", "file", 0, 62)
        prepare(ctx, by_file)
        check_arrays(ctx, by_file)
    ctx.close()


@pytest.mark.parametrize("name", ["hot", "s11", "dup", "edge"])
def test_under_one_and_two_workgroups(capi, made, name):
    """One workgroup of 256 threads strides the 2 x events walks, the traversals and the alleles several times, two half as often: the
    hot site's 600 traversals of three alleles and the cluster's masks past a grid turn."""
    ctx = generated_context(capi, made, name)
    want = oracle_of(made, name, "sequence", 0)
    prepare(ctx, want)
    assert 2 * ctx.segments_counts()["events"] > 512 or name in ("dup", "edge")
    for grid in (0, 1, 2):
        check_arrays(ctx, want, grid)
    if name == "hot":
        assert ctx.segments_variants_fetch_alleles()[6].tolist() == [200, 200, 200] and ctx.segments_variants_fetch_hist().tolist() == [0, 0, 0, 1]
        assert ctx.segments_variants_fetch_presence().shape == (3, 19)
    if name == "dup":
        assert ctx.segments_variants_fetch_sites()[3].tolist() == [2]
    if name == "edge":
        start, last, d = (a.tolist() for a in ctx.segments_variants_fetch_traversals()[:3])
        seq_begin = ctx.segments_fetch_sequences(0, 6).tolist()
        first_of = {s: want.seq.index(s) for s in set(want.seq)}
        last_of = {s: len(want.seq) - 1 - want.seq[::-1].index(s) for s in set(want.seq)}
        assert 1 not in first_of and seq_begin[1] == seq_begin[2] and seq_begin[0] < seq_begin[1] < seq_begin[3]     # the sequence without events
        assert any(x == 0 and e == first_of[want.seq[e]] and l == last_of[want.seq[e]] for e, l, x in zip(start, last, d))
        assert any(x == 1 and e == last_of[want.seq[e]] and l == first_of[want.seq[e]] for e, l, x in zip(start, last, d))
    ctx.close()


# ------------------------------------------------------------------------------------------------ 3. the presence words' widths
@pytest.fixture(scope="module")
def boundary(tmp_path_factory):
    """{C: (fasta, stream, gfa1, records)} of the first C records of colors_reference's word-boundary input."""
    d = tmp_path_factory.mktemp("boundary")
    got = {}
    for c in BOUNDARY_COLORS:
        fa = boundary_fasta(str(d / ("w%d.fa" % c)), c)
        stream = R.oracle_stream(fa, str(d / ("w%d.bin" % c)), BOUNDARY_K, BOUNDARY_L, BOUNDARY_Q, BOUNDARY_SEED)
        gfa1 = R.run_graphdump([os.path.basename(stream), "-k", str(BOUNDARY_K), "-s", os.path.basename(fa), "-f", "gfa1"], cwd=str(d))
        assert gfa1.returncode == 0 and gfa1.stderr == b""
        got[c] = (fa, stream, gfa1.stdout, [s for _, s in R.read_fasta(fa)])
    return got


@pytest.mark.parametrize("c", BOUNDARY_COLORS)
def test_every_width_of_the_presence_words(capi, boundary, c):
    """One word, the last bit of a word, the first bit of the next, two words and three."""
    fa, stream, gfa1, records = boundary[c]
    ctx = host_context(capi, fa, open(stream, "rb").read(), BOUNDARY_K)
    sb = None
    for ref in (None, 0, c - 1):
        want = R.Variants(gfa1, BOUNDARY_K, [len(s) for s in records], "sequence", ref, records=records, sb=sb)
        sb = want.sb
        if ref is None:
            prepare(ctx, want)
            assert want.n_colors == c and (c == 1 or want.sites() >= 50)
            assert c == 1 or max(sum(want.presence(i)) for i in range(len(want.alleles))) >= c - 1     # an allele nearly every colour walks
        check_arrays(ctx, want)
    check_arrays(ctx, want, grid=1)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 4. opt-in
@pytest.mark.parametrize("order", ["variants_first", "variants_last"])
def test_the_other_tables_are_unchanged_by_a_variant_build(capi, order):
    v = R.vector_of("c2_k29")
    case = CASES["c2_k29"]
    fasta, data = os.path.join(GOLDEN, case["fasta"]), open(os.path.join(GOLDEN, case["bin"]), "rb").read()
    want = R.golden_variants(v, "sequence", 1)
    n_seq = want.n_colors
    colour_map = list(range(n_seq))

    def build_others(ctx):
        ctx.segments_distances_build()
        ctx.segments_components_build()
        ctx.segments_classes_build()
        ctx.segments_anchors_build(colour_map, n_seq, 0)
        ctx.segments_tracks_build(colour_map, n_seq)

    def outputs(ctx):
        name, first = ctx.segments_fetch()
        begin, end = ctx.segments_fetch_events()
        got = [name, first, begin, end]
        got += list(ctx.segments_colors_fetch_rows()) + [ctx.segments_colors_fetch_presence()] + list(ctx.segments_colors_fetch_hist())
        got += list(ctx.segments_links_fetch_rows()) + [ctx.segments_links_fetch_first()]
        got += list(ctx.segments_superbubbles_fetch_rows()) + list(ctx.segments_superbubbles_fetch_members()) + [ctx.segments_superbubbles_fetch_presence(), ctx.segments_superbubbles_fetch_exits()]
        got += list(ctx.segments_distances_fetch())
        got += [ctx.segments_components_fetch_members()] + list(ctx.segments_components_fetch_rows()) + [ctx.segments_components_fetch_presence()]
        got += [ctx.segments_classes_fetch_members()] + list(ctx.segments_classes_fetch_rows()) + [ctx.segments_classes_fetch_presence()]
        got += [ctx.segments_anchors_fetch_mates()] + list(ctx.segments_anchors_fetch_rows()) + list(ctx.segments_anchors_fetch_shared())
        got += list(ctx.segments_tracks_fetch_rows()) + list(ctx.segments_tracks_fetch_colors()) + list(ctx.segments_tracks_fetch_depth())
        counts = {key: n for key, n in ctx.segments_counts().items() if key != "peak_device_bytes"}
        sb_info = {key: n for key, n in ctx.segments_superbubbles_info().items() if key != "peak_bytes"}
        return counts, ctx.segments_error(), ctx.segments_colors_info(), ctx.segments_links_info(), sb_info, got

    alone = host_context(capi, fasta, data, case["k"])
    prepare(alone, want)
    build_others(alone)
    ref = outputs(alone)
    with pytest.raises(RuntimeError, match="tpc_segments_variants_build first"):    # a context that never calls the stage holds none of it
        alone.segments_variants_info()
    alone.close()
    ctx = host_context(capi, fasta, data, case["k"])
    prepare(ctx, want)
    if order == "variants_first":
        check_arrays(ctx, want)
        build_others(ctx)
    else:
        build_others(ctx)
        check_arrays(ctx, want)
    for _ in range(2):
        got = outputs(ctx)
        assert got[:5] == ref[:5]
        assert all(a.shape == b.shape and (a == b).all() for a, b in zip(got[5], ref[5]))
        check_arrays(ctx, R.golden_variants(v, "sequence", 2))
    # every other build leaves the variants where they are; a new superbubble build drops them
    build_others(ctx)
    assert (ctx.segments_variants_fetch_sites()[2] == R.golden_variants(v, "sequence", 2).arrays()[3][2]).all()
    ctx.segments_superbubbles_build(2)
    with pytest.raises(RuntimeError, match="tpc_segments_variants_build first"):
        ctx.segments_variants_fetch_traversals(0, 0)
    check_arrays(ctx, R.golden_variants(v, "sequence", 0, 2))
    ctx.close()


# ------------------------------------------------------------------------------------------------ 5. ranges and refusals
def test_fetch_ranges(capi):
    v = R.vector_of("c2_k29")
    case = CASES["c2_k29"]
    want = R.golden_variants(v, "sequence", 0)
    ctx = host_context(capi, os.path.join(GOLDEN, case["fasta"]), open(os.path.join(GOLDEN, case["bin"]), "rb").read(), case["k"])
    prepare(ctx, want)
    check_arrays(ctx, want)
    trav, alle, presence, sites, hist = want.arrays()
    n, a, b = len(want.traversals), len(want.alleles), want.sb.count()
    assert (n, a, b) == (86, 81, 29)
    for got, ref in zip(ctx.segments_variants_fetch_traversals(30, 41), trav):
        assert (got == ref[30:71]).all()
    for got, ref in zip(ctx.segments_variants_fetch_alleles(a - 1, 1), alle):
        assert (got == ref[a - 1:]).all()
    assert (ctx.segments_variants_fetch_presence(7, 9) == presence[7:16]).all()
    got = ctx.segments_variants_fetch_sites(5, 11)
    assert (got[0] == sites[0][5:17]).all() and all((x == ref[5:16]).all() for x, ref in zip(got[1:], sites[1:]))
    assert all(x.size == 0 for x in ctx.segments_variants_fetch_traversals(n, 0)) and ctx.segments_variants_fetch_presence(a, 0).shape == (0, 1)
    assert ctx.segments_variants_fetch_sites(b, 0)[0].tolist() == [a]
    for call, what, size in ((ctx.segments_variants_fetch_traversals, "traversal", n), (ctx.segments_variants_fetch_alleles, "allele", a),
                             (ctx.segments_variants_fetch_presence, "allele", a), (ctx.segments_variants_fetch_sites, "site", b)):
        for i0, m in ((size, 1), (size + 1, 0), (0, size + 1), (MAXU, 2)):
            with pytest.raises(RuntimeError, match="segment variants: bad %s range" % what):
                call(i0, m)
    # null pointers
    L, h = capi.hip(), ctx._h
    buf = np.zeros(4 * n + 8, dtype=np.uint64)
    p = buf.ctypes.data
    assert L.tpc_segments_variants_fetch_traversals(h, 0, 1, p, p, None, p, p, p) != 0 and b"bad traversal range" in L.tpc_last_error(h)
    assert L.tpc_segments_variants_fetch_traversals(h, 0, 1, p, p, p, p, p, None) != 0 and b"the masks are required" in L.tpc_last_error(h)
    assert L.tpc_segments_variants_fetch_traversals(h, 0, 0, None, None, None, None, None, None) == 0      # nothing asked for, nothing needed
    assert L.tpc_segments_variants_fetch_alleles(h, 0, 1, p, p, p, p, p, p, None) != 0 and b"the masks and the traversal counts" in L.tpc_last_error(h)
    assert L.tpc_segments_variants_fetch_presence(h, 0, 1, None) != 0 and b"bad allele range" in L.tpc_last_error(h)
    assert L.tpc_segments_variants_fetch_sites(h, 0, 1, None, p, p, p) != 0 and b"bad site range" in L.tpc_last_error(h)
    assert L.tpc_segments_variants_fetch_hist(h, None) != 0 and b"the histogram is required" in L.tpc_last_error(h)
    assert L.tpc_segments_variants_info(h, None) != 0
    check_arrays(ctx, want)   # still usable
    ctx.close()


def test_refusals(capi):
    v = R.vector_of("c2_k29")
    case = CASES["c2_k29"]
    fasta, data = os.path.join(GOLDEN, case["fasta"]), open(os.path.join(GOLDEN, case["bin"]), "rb").read()
    want = R.golden_variants(v, "sequence", 0)
    text = capi.PackedText.from_fasta([fasta])
    n_seq = want.n_colors
    colour_map = list(range(n_seq))
    ctx = capi.Context(0)
    with pytest.raises(RuntimeError, match="^twopaco_hip: segment variants: build the segment table first"):   # no table
        ctx.segments_variants_build(colour_map, n_seq)
    for call in (ctx.segments_variants_info, ctx.segments_variants_fetch_traversals, ctx.segments_variants_fetch_alleles, ctx.segments_variants_fetch_presence,
                 ctx.segments_variants_fetch_sites, ctx.segments_variants_fetch_hist):
        with pytest.raises(RuntimeError, match="^twopaco_hip: segment variants: tpc_segments_variants_build first"):
            call()
    # the context is usable: a table, then the three tables the stage reads, one after the other
    ctx.seq_upload(text)
    ctx.segments_build(data, case["k"], text.rec_start, text.rec_length, ambiguous_positions(fasta, text.rec_start))
    with pytest.raises(RuntimeError, match="^twopaco_hip: segment variants: build the colour table first"):
        ctx.segments_variants_build(colour_map, n_seq)
    ctx.segments_colors_build(colour_map, n_seq)
    with pytest.raises(RuntimeError, match="^twopaco_hip: segment variants: build the link table first"):
        ctx.segments_variants_build(colour_map, n_seq)
    ctx.segments_links_build()
    with pytest.raises(RuntimeError, match="^twopaco_hip: segment variants: build the superbubble table first"):
        ctx.segments_variants_build(colour_map, n_seq)
    assert ctx.segments_counts()["events"] > 0 and ctx.segments_error() is None
    ctx.segments_superbubbles_build()
    check_arrays(ctx, want)
    # a colour table of another colour count; a colour beyond the colours; a reference beyond them.  A refused build leaves no table.
    for args, text_of in (((colour_map, n_seq + 1), "the colour table holds %d colours, the caller gives %d" % (n_seq, n_seq + 1)),
                          (([0] * n_seq, 1), "the colour table holds %d colours, the caller gives 1" % n_seq),
                          ((colour_map[:-1] + [n_seq], n_seq), "sequence %d has colour %d, there are %d colours" % (n_seq - 1, n_seq, n_seq)),
                          ((colour_map, n_seq, n_seq), "the reference colour is %d, there are %d colours" % (n_seq, n_seq)),
                          ((colour_map, n_seq, 0xFFFFFFFE), "the reference colour is 4294967294, there are %d colours" % n_seq)):
        with pytest.raises(RuntimeError, match="^twopaco_hip: segment variants: " + text_of):
            ctx.segments_variants_build(*args)
        with pytest.raises(RuntimeError, match="tpc_segments_variants_build first"):
            ctx.segments_variants_info()
        assert ctx.segments_counts()["events"] > 0 and ctx.segments_colors_info()["colors"] == n_seq and ctx.segments_superbubbles_info()["superbubbles"] == want.sb.count()
        check_arrays(ctx, want)
    h = ctx._h
    assert capi.hip().tpc_segments_variants_build(h, None, n_seq, 0xFFFFFFFF) != 0 and capi.hip().tpc_last_error(h).startswith(b"segment variants: the colour of every one")
    check_arrays(ctx, want)
    # the option holds for one build, whichever way it returns
    ctx.set_option("test_variants_grid", 1)
    with pytest.raises(RuntimeError, match="^twopaco_hip: segment variants: the reference colour"):
        ctx.segments_variants_build(colour_map, n_seq, n_seq)
    check_arrays(ctx, want)
    # a new link build drops the superbubbles and the variants with them; a new segment build everything
    ctx.segments_links_build()
    with pytest.raises(RuntimeError, match="tpc_segments_variants_build first"):
        ctx.segments_variants_fetch_traversals(0, 0)
    with pytest.raises(RuntimeError, match="^twopaco_hip: segment variants: build the superbubble table first"):
        ctx.segments_variants_build(colour_map, n_seq)
    ctx.segments_build(b"", case["k"], text.rec_start, text.rec_length)
    with pytest.raises(RuntimeError, match="^twopaco_hip: segment variants: build the colour table first"):
        ctx.segments_variants_build(colour_map, n_seq)
    ctx.close()
    # a table whose walk failed
    bad = CASES["edge_k5"]
    ctx = host_context(capi, os.path.join(GOLDEN, bad["fasta"]), open(os.path.join(GOLDEN, bad["bin"]), "rb").read(), bad["k"])
    assert ctx.segments_error() is not None
    with pytest.raises(RuntimeError, match="^twopaco_hip: segment variants: the segment table holds the walk's error 1 at slot 3"):
        ctx.segments_variants_build([0], 1)
    with pytest.raises(RuntimeError, match="unknown option"):
        ctx.set_option("test_variant_grid", 1)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 6. bytes
def serial_bytes(args, by, tmp_path, cwd, ref=None, more=()):
    vcf = str(tmp_path / "serial.vcf")
    r = R.run_graphdump(args + ["--variants", by] + ([] if ref is None else ["--variants-ref", str(ref), "--variants-vcf", vcf]) + list(more), cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    return r.stdout, None if ref is None else open(vcf, "rb").read()


@pytest.mark.parametrize("by", ["file", "sequence"])
@pytest.mark.parametrize("name", ["rand6_k9_q1", "c2_k29", "example_k11", "s11", "dup"])
def test_the_programs_write_the_serial_bytes(tmp_path, made, name, by):
    if name in made:
        m = made[name]
        case = dict(GENERATED_CASE, name=name, fasta=os.path.basename(m["fasta"]))
        args, cwd, data = [os.path.basename(m["stream"]), "-k", str(R.SB_K), "-s", os.path.basename(m["fasta"])], made["dir"], open(m["stream"], "rb").read()
        want = oracle_of(made, name, by, 0)
        none = oracle_of(made, name, by, None)
    else:
        case = CASES[name]
        v = R.case_vector(case)
        args, cwd, data = R.variants_args(v), GOLDEN, open(os.path.join(GOLDEN, case["bin"]), "rb").read()
        want, none = R.golden_variants(v, by, 0), R.golden_variants(v, by)
    tsv, vcf_text = serial_bytes(args, by, tmp_path, cwd, 0)
    assert tsv == want.tsv() and vcf_text == want.vcf()
    tsv_none, _ = serial_bytes(args, by, tmp_path, cwd)
    assert tsv_none == none.tsv()
    tsv_8, vcf_8 = serial_bytes(args, by, tmp_path, cwd, 0, more=["--superbubbles-max", "8"])
    # graphdump --gpu
    stats, vcf = str(tmp_path / "stats.json"), str(tmp_path / "gpu.vcf")
    env = dict(os.environ, TWOPACO_GRAPHDUMP_STATS=stats)
    r = subprocess.run([R.GRAPHDUMP] + args + ["--variants", by, "--variants-ref", "0", "--variants-vcf", vcf, "--gpu", "--threads", "16"], cwd=cwd, capture_output=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert r.stdout == tsv and open(vcf, "rb").read() == vcf_text
    s = json.load(open(stats))
    assert s["path"] == "device" and s["variants_kernel_ms"] > 0 and s["variant_alleles"] == len(want.alleles)
    r = subprocess.run([R.GRAPHDUMP] + args + ["--variants", by, "--gpu"], cwd=cwd, capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == tsv_none
    r = subprocess.run([R.GRAPHDUMP] + args + ["--variants", by, "--variants-ref", "0", "--variants-vcf", vcf, "--superbubbles-max", "8", "--gpu"], cwd=cwd, capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == tsv_8 and open(vcf, "rb").read() == vcf_8
    # beside the other tables of the same colours: each what it is alone, the variant table last
    flags = ("--colors", "--distances", "--components", "--superbubbles", "--anchors", "--classes", "--tracks")
    alone = [R.run_graphdump(args + [flag, by], cwd=cwd).stdout for flag in flags]
    extra = [x for flag in flags for x in (flag, by)]
    r = R.run_graphdump(args + ["--variants", by, "--variants-ref", "0", "--gpu"] + extra, cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == b"".join(alone) + tsv
    # twopaco
    d = str(tmp_path / "twopaco")
    os.mkdir(d)
    out = {key: os.path.join(d, key + ".tsv") for key in ("variants", "vcf", "colors", "superbubbles", "tracks")}
    r = cli(case, ["--tmpdir", d, "--variants", by, "--variants-ref", "0", "--variants-out", out["variants"], "--variants-vcf", out["vcf"], "--colors", by, "--colors-out", out["colors"],
                   "--superbubbles", by, "--superbubbles-out", out["superbubbles"], "--tracks", by, "--tracks-out", out["tracks"], "-o", os.path.join(d, "j.bin")], cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert open(os.path.join(d, "j.bin"), "rb").read() == data
    assert open(out["variants"], "rb").read() == tsv and open(out["vcf"], "rb").read() == vcf_text
    for key, text in zip(("colors", "superbubbles", "tracks"), (alone[0], alone[3], alone[6])):
        assert open(out[key], "rb").read() == text, key
    assert sorted(os.listdir(d)) == sorted(["j.bin"] + [key + ".tsv" for key in out])
    # ... alone (the superbubble stage runs for it), and with the graph text rendered on the device
    r = cli(case, ["--tmpdir", d, "--variants", by, "--variants-out", out["variants"], "--superbubbles-max", "8", "--variants-ref", "0", "--variants-vcf", out["vcf"], "--graph", "gfa1",
                   "--graph-out", os.path.join(d, "g.gfa"), "--graph-text", "device", "-o", os.path.join(d, "j.bin")], cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert open(out["variants"], "rb").read() == tsv_8 and open(out["vcf"], "rb").read() == vcf_8


def test_twopaco_default_file_timing_lines_and_refusals(tmp_path):
    case = CASES["c2_k29"]
    fasta = os.path.join(GOLDEN, case["fasta"])
    want = R.golden_variants(R.case_vector(case), "file")
    d = str(tmp_path)
    r = cli(case, ["--tmpdir", d, "--variants", "file"], fasta, cwd=d, env=dict(os.environ, TWOPACO_TIMING="1"))
    assert r.returncode == 0, r.stderr[-400:]
    assert sorted(os.listdir(d)) == ["de_bruijn.bin", "de_bruijn.variants.tsv"]
    err = r.stderr.decode()
    assert "segment variants:" in err and "segment variants fetch:" in err and "variants_kernel_ms" in err and "variant table writing:" in err and "segment superbubbles:" in err
    got = open(os.path.join(d, "de_bruijn.variants.tsv"), "rb").read()
    assert got.split(b"\n")[0] == want.tsv().split(b"\n")[0] and got.split(b"\n")[2:] == want.tsv().split(b"\n")[2:]      # (the one colour's label is the file as given)
    os.unlink(os.path.join(d, "de_bruijn.bin"))
    os.unlink(os.path.join(d, "de_bruijn.variants.tsv"))
    r = cli(case, ["--tmpdir", d, "--variants", "file", "--gpus", "2"], fasta, cwd=d)
    assert r.returncode == 1 and r.stderr.decode().endswith("not with --gpus above 1 for arg (--variants)\n") and os.listdir(d) == []
    n_seq = len(want.seq_name)
    r = cli(case, ["--tmpdir", d, "--variants", "sequence", "--variants-ref", str(n_seq)], fasta, cwd=d)
    assert r.returncode == 1 and "The variant table's reference colour is %d, there are %d colours" % (n_seq, n_seq) in r.stderr.decode()
    assert not os.path.exists(os.path.join(d, "de_bruijn.variants.tsv"))


# ------------------------------------------------------------------------------------------------ 7. at size
M2R2_SCALE, M2R2_SEED = 0.05, 450


def test_m2r2_variants_equal_the_serial_graphdump(tmp_path):
    """synth m2r2 at scale 0.05, synth seed 450, k = 25, f = 32 (the workload of test_gpu_superbubbles.py: 62 files): sha256 and size of
    the two files of `twopaco --variants file --variants-ref 0` == those of the serial `graphdump` over the junction stream of the same
    command; the two files are checked against the letters of the input."""
    d = str(tmp_path)
    case = {"name": "m2r2_variants", "fasta": None, "synth": {"workload": "m2r2", "seed": M2R2_SEED, "scale": M2R2_SCALE}}
    files = case_files(case, d)
    assert len(files) == 62
    junctions, table, vcf = os.path.join(d, "m2r2.bin"), os.path.join(d, "variants.tsv"), os.path.join(d, "variants.vcf")
    r = subprocess.run([R.TWOPACO, "-k", "25", "-f", "32", "-t", "16", "--seed", "12345", "--tmpdir", d, "-o", junctions, "--variants", "file", "--variants-ref", "0",
                        "--variants-out", table, "--variants-vcf", vcf] + files, capture_output=True, timeout=900)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-800:]
    seqs = []
    for f in files:
        seqs += ["-s", f]
    serial, serial_vcf = os.path.join(d, "serial.tsv"), os.path.join(d, "serial.vcf")
    r = subprocess.run([R.GRAPHDUMP, junctions, "-k", "25", "--variants", "file", "--variants-ref", "0", "--variants-out", serial, "--variants-vcf", serial_vcf] + seqs,
                       capture_output=True, timeout=900)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    for mine, theirs in ((table, serial), (vcf, serial_vcf)):
        got, ref = open(mine, "rb").read(), open(theirs, "rb").read()
        assert len(got) == len(ref) and hashlib.sha256(got).hexdigest() == hashlib.sha256(ref).hexdigest()
    got = open(table, "rb").read()
    head = dict(f.split("=") for f in got.split(b"\n", 1)[0].decode().split("\t")[2:])
    assert (head["by"], head["k"], head["colors"], head["ref"]) == ("file", "25", "62", "0") and int(head["sites"]) > 1000
    records = [s for f in files for _, s in R.read_fasta(f)]
    alleles, n = R.check_files(got, open(vcf, "rb").read(), records)
    print("sites", head["sites"], "alleles", alleles, "traversals", head["traversals"], "records", n)
