"""GPU (-m gpu): the bounded superbubbles on the device (csrc/tpc_superbubbles.hip, the tpc_segments_superbubbles_* group of
include/twopaco_hip.h) against their set definition, stated in superbubbles_reference.py over the serial gfa1 text (pinned to the
real reference's sha256 by tests/golden/graphdump.json): the adjacency arrays, exit[] of every side, every plane of the rows, the
members, the presence words and info[] through the C-ABI on a host stream and a resident stream, at max_inside 62, 8 and 2, at
1 / 32 / 33 / 65 colours, the stages it leaves untouched, fetch ranges and refusals, the bytes of `graphdump --superbubbles --gpu`
and `twopaco --superbubbles`, and m2r2 at scale 0.05 by sha256 against the serial graphdump."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import superbubbles_reference as R
from colors_reference import presence_words
from helpers import GOLDEN, case_files, golden_cases

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in golden_cases()}
MAXU = (1 << 64) - 1
GENERATED_CASE = {"k": R.SB_K, "L": R.SB_L, "q": R.SB_Q, "seed": R.SB_SEED, "rounds": [{"low": 0, "high": 1 << R.SB_L}], "n_rounds": 1, "abundance": None}
GENERATED = {"s11": R.SB_RECORDS, "s81": R.SB_RECORDS + R.SB_HUB}
NAMES = ["s11", "s81", "short", "c2_k29", "rand6_k27", "rand6_k3", "tr_k25_L28", "example_k11"]


@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


def ambiguous_positions(fasta, rec_start):
    return [int(rec_start[r]) + i for r, (_, s) in enumerate(R.read_fasta(fasta)) for i, ch in enumerate(s) if ch not in "ACGTN"]


def host_context(capi, fasta, data, k):
    """A context used for nothing else, the table from the stream's bytes."""
    text = capi.PackedText.from_fasta([fasta])
    ctx = capi.Context(0)
    ctx.seq_upload(text)
    ctx.segments_build(data, k, text.rec_start, text.rec_length, ambiguous_positions(fasta, text.rec_start))
    return ctx


def resident_context(capi, case, fasta, data):
    """The whole path in this process up to tpc_emit_stream, the table from the device's own copy of the stream."""
    text = capi.PackedText.from_fasta([fasta])
    ctx = capi.Context(0)
    ctx.set_params(case["k"], case["L"], case["q"], capi.seed_table(case["q"], case["L"], seed=case["seed"]))
    ctx.seq_upload(text)
    for st in case["rounds"]:
        ctx.filter_reset()
        ctx.pass1_insert(st["low"], st["high"])
        ctx.pass1_query(st["low"], st["high"])
        ctx.pass2_filter()
    ctx.junctions_finalize()
    ctx.emit()
    stream, _ = ctx.emit_stream(text.rec_start, text.rec_length)
    assert stream == data
    ctx.segments_build(None, case["k"], text.rec_start, text.rec_length, ambiguous_positions(fasta, text.rec_start))
    return ctx


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """The generated inputs (superbubbles_reference.superbubble_fasta without and with the hub) and the link-free records: FASTA,
    junction stream (from the CPU restatement of the pipeline, oracle/) and the serial gfa1, made once; the oracles are kept beside
    them, and the generated input is checked to hold every kind."""
    d = tmp_path_factory.mktemp("superbubbles")
    got = {"dir": str(d)}
    for name in ("s11", "s81", "short"):
        fa = str(d / (name + ".fa"))
        if name == "short":
            R.B.few_events_fasta(fa, only_short=True)
        else:
            R.superbubble_fasta(fa, GENERATED[name])
        k = 11 if name == "short" else R.SB_K   # the link-free records are made for k = 11
        stream = R.oracle_stream(fa, str(d / (name + ".bin")), k, R.SB_L, R.SB_Q, R.SB_SEED)
        gfa1 = R.run_graphdump([stream, "-k", str(k), "-s", fa, "-f", "gfa1"], cwd=str(d))
        assert gfa1.returncode == 0 and gfa1.stderr == b""
        got[name] = {"fasta": fa, "stream": stream, "gfa1": gfa1.stdout, "k": k, "oracle": {}}
    full, at8, at2 = (oracle_of(got, "s81", max_inside=m) for m in (62, 8, 2))
    got["unmirrored"] = R.check_kinds(full, at8, at2)
    return got


_GOLDEN_ORACLES = {}


def oracle_of(made, name, by="file", max_inside=62):
    key = (name, by, max_inside)
    if name in made:
        m = made[name]
        if key not in m["oracle"]:
            m["oracle"][key] = R.Superbubbles(m["gfa1"], m["k"], by, max_inside=max_inside)
        return m["oracle"][key]
    if key not in _GOLDEN_ORACLES:
        case = CASES[name]
        _GOLDEN_ORACLES[key] = R.Superbubbles(R.golden_gfa1(R.case_vector(case)), case["k"], by, max_inside=max_inside)
    return _GOLDEN_ORACLES[key]


def inputs(name, made, by="file", max_inside=62):
    """(case, fasta, stream bytes, oracle)"""
    want = oracle_of(made, name, by, max_inside)
    if name in made:
        m = made[name]
        return dict(GENERATED_CASE, name=name, k=m["k"]), m["fasta"], open(m["stream"], "rb").read(), want
    case = CASES[name]
    return case, os.path.join(GOLDEN, case["fasta"]), open(os.path.join(GOLDEN, case["bin"]), "rb").read(), want


def color_map_of(want):
    """What tpc_segments_colors_build takes for the oracle's colours."""
    g = want.g
    if want.by == "sequence":
        return list(range(len(g.seq_name))), len(g.seq_name)
    files = list(dict.fromkeys(g.seq_file))
    return [files.index(f) for f in g.seq_file], len(files)


def check_table(ctx, want):
    """Everything the device holds after a superbubble build == the oracle's, element for element."""
    info = ctx.segments_superbubbles_build(want.max_inside)
    assert (info["superbubbles"], info["sides"], info["members"], info["unmirrored"], info["arcs"], info["max_inside"]) == (
        want.count(), want.sides, len(want.member_sides), want.unmirrored, want.n_arcs, want.max_inside)
    words = (want.colors["colors"] + 31) // 32
    assert info["peak_bytes"] >= 8 * want.sides + 4 * want.n_arcs + want.count() * (48 + 4 * words) + 4 * len(want.member_sides)
    off, heads = ctx.segments_superbubbles_fetch_adjacency()
    assert off.dtype == heads.dtype == np.uint32 and off.size == want.sides + 1 and heads.size == want.n_arcs
    assert (off == want.off).all() and (heads == want.heads).all()
    exits = ctx.segments_superbubbles_fetch_exits()
    assert exits.dtype == np.uint32 and exits.size == want.sides and (exits == want.exit).all()
    rows = ctx.segments_superbubbles_fetch_rows()
    assert all(a.dtype == np.uint32 for a in rows[:5]) and all(a.dtype == np.uint64 for a in rows[5:])
    for got, ref in zip(rows, (want.entrance, want.exits, want.inside, want.arcs, want.n_colors, want.paths, want.min_edges, want.max_edges)):
        assert got.size == ref.size and (got.astype(np.uint64) == ref.astype(np.uint64)).all()
    m_off, m_sides = ctx.segments_superbubbles_fetch_members()
    assert m_off.dtype == m_sides.dtype == np.uint32 and (m_off == want.member_off).all() and (m_sides == want.member_sides).all()
    presence = ctx.segments_superbubbles_fetch_presence()
    assert presence.dtype == np.uint32 and presence.shape == (want.count(), words)
    if want.count():
        assert (presence == presence_words(want.presence)).all()
    assert ctx.kernel_ms("superbubbles") > 0
    return info


# ------------------------------------------------------------------------------------------------ 1. the arrays by their definition
@pytest.mark.parametrize("source", ["host", "resident"])
@pytest.mark.parametrize("name", NAMES)
def test_superbubble_arrays_by_their_definition(capi, made, name, source):
    case, fasta, data, want = inputs(name, made)
    ctx = host_context(capi, fasta, data, case["k"]) if source == "host" else resident_context(capi, case, fasta, data)
    assert ctx.segments_error() is None
    assert ctx.segments_links_build()["rows"] == want.links
    ctx.segments_colors_build(*color_map_of(want))
    check_table(ctx, want)
    check_table(ctx, want)   # a second build replaces the first
    if name in GENERATED:
        # the cluster lies exactly at the bound: 62 sides inside, 2^11 paths
        assert want.count() == 10 and int(want.inside.max()) == 62 and int(want.paths.max()) == 2048 and made["unmirrored"] == 0
    if name == "s81":
        assert int(np.diff(want.off).max()) >= 20                       # the hub: many arcs leave one side
    if name == "tr_k25_L28":
        assert any(u in want.out[u] for u in range(want.sides))         # its self-loop
    if name == "rand6_k3":
        assert int((np.diff(want.off) >= 4).sum()) == 273               # almost nothing qualifies
    if name == "example_k11":
        assert want.count() == 0 and want.links > 0 and all(a.size == 0 for a in ctx.segments_superbubbles_fetch_rows())
    if name == "short":
        assert (want.links, want.n_arcs, want.count()) == (0, 0, 0) and want.sides > 0 and (want.exit == R.NONE).all()
    ctx.close()


def test_no_event_at_all(capi, made):
    fa = made["short"]["fasta"]
    text = capi.PackedText.from_fasta([fa])
    ctx = capi.Context(0)
    ctx.seq_upload(text)
    ctx.segments_build(b"", 11, text.rec_start, text.rec_length)
    ctx.segments_links_build()
    ctx.segments_colors_build([0] * len(text.rec_start), 1)
    info = ctx.segments_superbubbles_build()
    assert (info["superbubbles"], info["sides"], info["members"], info["arcs"]) == (0, 0, 0, 0)
    off, heads = ctx.segments_superbubbles_fetch_adjacency()
    assert off.tolist() == [0] and heads.size == 0 and ctx.segments_superbubbles_fetch_exits().size == 0
    assert ctx.segments_superbubbles_fetch_members()[0].tolist() == [0] and ctx.segments_superbubbles_fetch_presence().shape == (0, 1)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 2. the bound, the colours
@pytest.mark.parametrize("max_inside", [2, 8, 61, 62])
@pytest.mark.parametrize("name", ["s81", "c2_k29"])
def test_the_bound(capi, made, name, max_inside):
    """61 and 62: the cluster of the generated input holds exactly 62 sides inside, so it is there at 62 and gone at 61."""
    case, fasta, data, want = inputs(name, made, max_inside=max_inside)
    ctx = host_context(capi, fasta, data, case["k"])
    ctx.segments_links_build()
    ctx.segments_colors_build(*color_map_of(want))
    check_table(ctx, want)
    if name == "s81":
        assert want.count() == {2: 4, 8: 9, 61: 9, 62: 10}[max_inside]
    ctx.close()


@pytest.mark.parametrize("n_colors", [1, 32, 33, 65])
def test_presence_at_every_word_boundary(capi, made, n_colors):
    case, fasta, data, _ = inputs("s81", made)
    n_seq = len(R.read_fasta(fasta))
    color_of_seq = [s % n_colors for s in range(n_seq)]
    want = R.Superbubbles(made["s81"]["gfa1"], R.SB_K, color_of_seq=color_of_seq)
    assert want.colors["colors"] == n_colors and int(want.n_colors.max()) >= min(n_colors, 8) and int(want.n_colors.min()) >= min(n_colors, 2)
    ctx = host_context(capi, fasta, data, case["k"])
    ctx.segments_links_build()
    ctx.segments_colors_build(color_of_seq, n_colors)
    check_table(ctx, want)
    ctx.close()


def test_colours_by_sequence(capi, made):
    case, fasta, data, want = inputs("s81", made, "sequence")
    ctx = host_context(capi, fasta, data, case["k"])
    ctx.segments_links_build()
    ctx.segments_colors_build(*color_map_of(want))
    check_table(ctx, want)
    # the 4-allele site: four sides inside, each held by the two genomes with its letter
    four = [r for r in want.rows if r["inside"] == 4 and r["paths"] == 4]
    assert four and all(r["n_colors"] == 8 for r in four)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 3. opt-in
@pytest.mark.parametrize("order", ["last", "first"])
def test_the_other_tables_are_unchanged(capi, made, order):
    case, fasta, data, want = inputs("s81", made)
    n_seq = len(R.read_fasta(fasta))

    def outputs(ctx):
        name, first = ctx.segments_fetch()
        begin, end = ctx.segments_fetch_events()
        got = [name, first, begin, end, ctx.segments_fetch_sequences(0, n_seq + 1)]
        got += list(ctx.segments_colors_fetch_rows()) + [ctx.segments_colors_fetch_presence()] + list(ctx.segments_colors_fetch_hist())
        got += list(ctx.segments_links_fetch_rows()) + [ctx.segments_links_fetch_first()]
        got += list(ctx.segments_bubbles_fetch_rows()) + list(ctx.segments_bubbles_fetch_sides()) + [ctx.segments_bubbles_fetch_hist()]
        got += list(ctx.segments_distances_fetch())
        got += [ctx.segments_components_fetch_members()] + list(ctx.segments_components_fetch_rows()) + [ctx.segments_components_fetch_presence()]
        infos = (ctx.segments_error(), ctx.segments_colors_info(), ctx.segments_links_info(), ctx.segments_bubbles_info()["bubbles"], ctx.segments_components_info()["components"])
        return {key: n for key, n in ctx.segments_counts().items() if key != "peak_device_bytes"}, infos, got

    def others(ctx):
        ctx.segments_bubbles_build()
        ctx.segments_distances_build()
        ctx.segments_components_build()

    alone = host_context(capi, fasta, data, case["k"])
    alone.segments_colors_build(*color_map_of(want))
    alone.segments_links_build()
    others(alone)
    ref = outputs(alone)
    alone.close()
    ctx = host_context(capi, fasta, data, case["k"])
    ctx.segments_colors_build(*color_map_of(want))
    ctx.segments_links_build()
    if order == "first":
        check_table(ctx, want)
        others(ctx)
    else:
        others(ctx)
        check_table(ctx, want)
    for _ in range(2):
        got = outputs(ctx)
        assert got[:2] == ref[:2]
        assert all(a.shape == b.shape and (a == b).all() for a, b in zip(got[2], ref[2]))
        check_table(ctx, want)   # rebuilt: the same table, and the others once more
    # the other stages neither drop it nor are dropped by it
    others(ctx)
    assert (ctx.segments_superbubbles_fetch_rows()[0] == want.entrance).all()
    # a new link build drops it, and so does a new colour build
    ctx.segments_links_build()
    with pytest.raises(RuntimeError, match="tpc_segments_superbubbles_build first"):
        ctx.segments_superbubbles_info()
    check_table(ctx, want)
    ctx.segments_colors_build(*color_map_of(want))
    with pytest.raises(RuntimeError, match="tpc_segments_superbubbles_build first"):
        ctx.segments_superbubbles_fetch_exits()
    check_table(ctx, want)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 4. ranges and refusals
def test_fetch_ranges(capi, made):
    case, fasta, data, want = inputs("s81", made)
    ctx = host_context(capi, fasta, data, case["k"])
    ctx.segments_links_build()
    ctx.segments_colors_build(*color_map_of(want))
    n = ctx.segments_superbubbles_build()["superbubbles"]
    assert n == 10
    rows = ctx.segments_superbubbles_fetch_rows(3, 5)
    for got, ref in zip(rows, (want.entrance, want.exits, want.inside, want.arcs, want.n_colors, want.paths, want.min_edges, want.max_edges)):
        assert (got.astype(np.uint64) == ref[3:8].astype(np.uint64)).all()
    assert (ctx.segments_superbubbles_fetch_presence(3, 5) == presence_words(want.presence)[3:8]).all()
    assert all(a.size == 0 for a in ctx.segments_superbubbles_fetch_rows(n, 0)) and ctx.segments_superbubbles_fetch_presence(n, 0).shape == (0, 1)
    for b0, m in ((n, 1), (n + 1, 0), (0, n + 1), (MAXU, 2)):
        with pytest.raises(RuntimeError, match="bad row range"):
            ctx.segments_superbubbles_fetch_rows(b0, m)
        with pytest.raises(RuntimeError, match="bad row range"):
            ctx.segments_superbubbles_fetch_presence(b0, m)
    sides = want.sides
    assert (ctx.segments_superbubbles_fetch_exits(133, 71) == want.exit[133:204]).all()
    assert ctx.segments_superbubbles_fetch_exits(sides, 0).size == 0
    for c0, m in ((sides, 1), (sides + 1, 0), (0, sides + 1), (MAXU, 2)):
        with pytest.raises(RuntimeError, match="bad side range"):
            ctx.segments_superbubbles_fetch_exits(c0, m)
    ctx.close()


def test_refusals(capi, made):
    case, fasta, data, want = inputs("s11", made)
    text = capi.PackedText.from_fasta([fasta])
    ctx = capi.Context(0)
    ctx.seq_upload(text)
    with pytest.raises(RuntimeError, match="segment superbubbles: build the segment table first"):
        ctx.segments_superbubbles_build()
    with pytest.raises(RuntimeError, match="tpc_segments_superbubbles_build first"):
        ctx.segments_superbubbles_info()
    ctx.segments_build(data, case["k"], text.rec_start, text.rec_length, ambiguous_positions(fasta, text.rec_start))
    with pytest.raises(RuntimeError, match="segment superbubbles: build the link table first"):
        ctx.segments_superbubbles_build()
    ctx.segments_links_build()
    with pytest.raises(RuntimeError, match="segment superbubbles: build the colour table first"):
        ctx.segments_superbubbles_build()
    ctx.segments_colors_build(*color_map_of(want))
    for bad in (0, 1, 63, 64, 1 << 20):
        with pytest.raises(RuntimeError, match="max_inside = %d, allowed are 2 .. 62" % bad):
            ctx.segments_superbubbles_build(bad)
    with pytest.raises(RuntimeError, match="tpc_segments_superbubbles_build first"):   # a refused build leaves no table
        ctx.segments_superbubbles_fetch_members()
    check_table(ctx, want)                                                                # and the context usable
    with pytest.raises(RuntimeError, match="max_inside = 1, allowed"):
        ctx.segments_superbubbles_build(1)
    with pytest.raises(RuntimeError, match="tpc_segments_superbubbles_build first"):   # the table of before is gone as well
        ctx.segments_superbubbles_info()
    ctx.close()
    # a table whose walk failed: there are no segments to join, and the context goes on
    bad = CASES["edge_k5"]
    ctx = host_context(capi, os.path.join(GOLDEN, bad["fasta"]), open(os.path.join(GOLDEN, bad["bin"]), "rb").read(), bad["k"])
    assert ctx.segments_error() is not None
    with pytest.raises(RuntimeError, match="segment superbubbles: the segment table holds the walk's error 1 at slot 3"):
        ctx.segments_superbubbles_build()
    with pytest.raises(RuntimeError, match="tpc_segments_superbubbles_build first"):
        ctx.segments_superbubbles_info()
    bad_text = capi.PackedText.from_fasta([os.path.join(GOLDEN, bad["fasta"])])
    ctx.segments_build(b"", bad["k"], bad_text.rec_start, bad_text.rec_length)
    ctx.segments_links_build()
    ctx.segments_colors_build([0] * len(bad_text.rec_start), 1)
    assert ctx.segments_superbubbles_build()["superbubbles"] == 0
    ctx.close()


# ------------------------------------------------------------------------------------------------ 5. bytes
def program_inputs(name, made, by):
    """(case, fasta, stream bytes, oracle, graphdump's arguments, its directory)"""
    case, fasta, data, want = inputs(name, made, by)
    if name in made:
        return case, fasta, data, want, [made[name]["stream"], "-k", str(case["k"]), "-s", fasta], made["dir"]
    return case, fasta, data, want, R.superbubbles_args(R.case_vector(CASES[name])), GOLDEN


@pytest.mark.parametrize("by", ["file", "sequence"])
@pytest.mark.parametrize("name", NAMES)
def test_graphdump_gpu_writes_the_oracle_bytes(tmp_path, made, name, by):
    case, fasta, _, want, args, cwd = program_inputs(name, made, by)
    stats, members = str(tmp_path / "stats.json"), str(tmp_path / "members.tsv")
    env = dict(os.environ, TWOPACO_GRAPHDUMP_STATS=stats)
    r = subprocess.run([R.GRAPHDUMP] + args + ["--superbubbles", by, "--superbubbles-members", members, "--gpu", "--threads", "16"], cwd=cwd, capture_output=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert r.stdout == want.tsv(), name
    assert open(members, "rb").read() == want.members_tsv()
    s = json.load(open(stats))
    assert s["path"] == "device" and s["superbubbles_kernel_ms"] > 0 and s["superbubbles"] == want.count() and s["superbubble_members"] == len(want.member_sides)
    assert s["superbubbles_unmirrored"] == want.unmirrored and s["links"] == want.links
    out = str(tmp_path / "superbubbles.tsv")
    r = R.run_graphdump(args + ["--superbubbles", by, "--gpu", "--superbubbles-out", out, "--prefix"], cwd=cwd)
    assert r.returncode == 0 and r.stdout == b"" and open(out, "rb").read() == want.tsv()


def test_graphdump_gpu_the_bound_beside_the_other_tables_and_a_failing_walk(tmp_path, made):
    case, fasta, _, want, args, cwd = program_inputs("s81", made, "sequence")
    for max_inside in (8, 2):
        small = oracle_of(made, "s81", "sequence", max_inside)
        r = R.run_graphdump(args + ["--superbubbles", "sequence", "--superbubbles-max", str(max_inside), "--gpu"], cwd=cwd)
        assert r.returncode == 0 and r.stderr == b"" and r.stdout == small.tsv()
    alone = {flag: R.run_graphdump(args + [flag, "sequence"], cwd=cwd).stdout for flag in ("--colors", "--bubbles", "--distances", "--components")}
    for flag in alone:
        r = R.run_graphdump(args + [flag, "sequence", "--superbubbles", "sequence", "--gpu"], cwd=cwd)
        assert r.returncode == 0 and r.stderr == b"" and r.stdout == alone[flag] + want.tsv(), flag
    v = R.vector_of("edge_k5")
    out, members = str(tmp_path / "superbubbles.tsv"), str(tmp_path / "members.tsv")
    r = R.run_graphdump(R.superbubbles_args(v) + ["--superbubbles", "file", "--gpu", "--superbubbles-out", out, "--superbubbles-members", members])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode() == v["stderr"] and not os.path.exists(out) and not os.path.exists(members)


def cli_input(name, fasta):
    """(fasta as twopaco is given it, its directory): a golden file by its name inside tests/golden, as the reference's vectors
    name it -- the colours' labels are the file names as given."""
    return (None, GOLDEN) if name in CASES else (fasta, os.path.dirname(fasta))


def cli(case, extra, fasta=None, cwd=GOLDEN, timeout=300, env=None):
    args = [R.TWOPACO, "-k", str(case["k"]), "-f", str(case["L"]), "-q", str(case["q"]), "-r", str(case["n_rounds"]), "--seed", str(case["seed"])]
    if case["abundance"] is not None:
        args += ["-a", str(case["abundance"])]
    return subprocess.run(args + extra + [case["fasta"] if fasta is None else fasta], cwd=cwd, capture_output=True, timeout=timeout, env=env)


@pytest.mark.parametrize("by", ["file", "sequence"])
@pytest.mark.parametrize("name", NAMES)
def test_twopaco_writes_the_oracle_bytes(tmp_path, made, name, by):
    case, fasta, data, want = inputs(name, made, by)
    d = str(tmp_path)
    table, members, junctions = os.path.join(d, "superbubbles.tsv"), os.path.join(d, "members.tsv"), os.path.join(d, "j.bin")
    given, cwd = cli_input(name, fasta)
    r = cli(case, ["--tmpdir", d, "--superbubbles", by, "--superbubbles-out", table, "--superbubbles-members", members, "-o", junctions], given, cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert open(junctions, "rb").read() == data
    assert open(table, "rb").read() == want.tsv() and open(members, "rb").read() == want.members_tsv()
    assert sorted(os.listdir(d)) == ["j.bin", "members.tsv", "superbubbles.tsv"]


@pytest.mark.parametrize("name", ["s81", "c2_k29"])
def test_twopaco_superbubbles_beside_everything_else(tmp_path, made, name):
    """--superbubbles with --graph gfa1 --graph-compact --links --colors --bubbles --distances --components: one segment, colour and link
    build serve all, and every other file has the bytes it has without --superbubbles."""
    case, fasta, _, want = inputs(name, made, "sequence")
    given, cwd = cli_input(name, fasta)
    with_dir, without_dir = str(tmp_path / "with"), str(tmp_path / "without")
    files = ("graph.gfa", "links.tsv", "colors.tsv", "bubbles.tsv", "distances.tsv", "components.tsv")
    for d, extra in ((without_dir, []), (with_dir, ["--superbubbles", "sequence", "--superbubbles-out", os.path.join(with_dir, "superbubbles.tsv")])):
        os.mkdir(d)
        r = cli(case, ["--tmpdir", d, "--graph", "gfa1", "--graph-compact", "--graph-out", os.path.join(d, "graph.gfa"), "--links", "--links-out", os.path.join(d, "links.tsv"),
                       "--colors", "sequence", "--colors-out", os.path.join(d, "colors.tsv"), "--bubbles", "sequence", "--bubbles-out", os.path.join(d, "bubbles.tsv"),
                       "--distances", "sequence", "--distances-out", os.path.join(d, "distances.tsv"), "--components", "sequence", "--components-out",
                       os.path.join(d, "components.tsv")] + extra, given, cwd=cwd)
        assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert sorted(os.listdir(without_dir)) == sorted(files) and sorted(os.listdir(with_dir)) == sorted(files + ("superbubbles.tsv",))
    for f in files:
        assert open(os.path.join(with_dir, f), "rb").read() == open(os.path.join(without_dir, f), "rb").read(), f
    assert open(os.path.join(with_dir, "superbubbles.tsv"), "rb").read() == want.tsv()
    # beside the plain graph rendered on the device, where no event table is fetched for the graph, and with a bound
    d = str(tmp_path / "device")
    os.mkdir(d)
    small = oracle_of(made, name, "sequence", 8)
    r = cli(case, ["--tmpdir", d, "--graph", "gfa1", "--graph-text", "device", "--graph-out", os.path.join(d, "graph.gfa"), "--superbubbles", "sequence", "--superbubbles-max", "8",
                   "--superbubbles-out", os.path.join(d, "superbubbles.tsv"), "--superbubbles-members", os.path.join(d, "members.tsv")], given, cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert open(os.path.join(d, "superbubbles.tsv"), "rb").read() == small.tsv() and open(os.path.join(d, "members.tsv"), "rb").read() == small.members_tsv()
    assert sorted(os.listdir(d)) == ["graph.gfa", "members.tsv", "superbubbles.tsv"]


def test_twopaco_default_file_timing_lines_and_refusals(tmp_path, made):
    case, fasta, _, want = inputs("s81", made)
    d = str(tmp_path)
    r = cli(case, ["--tmpdir", d, "--superbubbles", "file"], fasta, cwd=d, env=dict(os.environ, TWOPACO_TIMING="1"))
    assert r.returncode == 0, r.stderr[-400:]
    assert sorted(os.listdir(d)) == ["de_bruijn.bin", "de_bruijn.superbubbles.tsv"]
    err = r.stderr.decode()
    assert "segment superbubbles:" in err and "segment superbubbles fetch:" in err and "superbubbles_kernel_ms" in err and "superbubble table writing:" in err
    assert open(os.path.join(d, "de_bruijn.superbubbles.tsv"), "rb").read() == want.tsv()
    os.unlink(os.path.join(d, "de_bruijn.bin"))
    os.unlink(os.path.join(d, "de_bruijn.superbubbles.tsv"))
    r = cli(case, ["--tmpdir", d, "--superbubbles", "file", "--gpus", "2"], fasta, cwd=d)
    assert r.returncode == 1 and r.stderr.decode().endswith("not with --gpus above 1 for arg (--superbubbles)\n") and os.listdir(d) == []
    # an input the walk refuses: the walk's message, no file
    bad = CASES["edge_k5"]
    r = cli(bad, ["--tmpdir", d, "--superbubbles", "file", "--superbubbles-out", os.path.join(d, "superbubbles.tsv"), "--superbubbles-members", os.path.join(d, "members.tsv"),
                  "--graph", "gfa1", "--graph-out", os.path.join(d, "graph.gfa")])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: The input is corrupted\n"
    assert os.listdir(d) == []


# ------------------------------------------------------------------------------------------------ 6. at size
def test_m2r2_superbubbles_equal_the_serial_graphdump(tmp_path):
    """synth m2r2 at scale 0.05, synth seed 12345, k = 25, f = 32 (62 files, tracts and minisatellites): sha256 and size of
    `twopaco --superbubbles file --bubbles file -o` == those of the serial `graphdump --superbubbles file` over the junction stream of the
    same command, table and members; the numbers of superbubbles and of simple bubbles are printed -- their ratio is why the table
    exists.  The serial program over the CPU restatement's stream of the same input: 82 986 segments, 111 432 links, 1 726 superbubbles
    (1 219 with 14 sides inside, three at the bound of 62), 85 simple bubbles, no entrance without its mirror; the set-definition oracle
    gives the same two files there."""
    d = str(tmp_path)
    case = {"name": "m2r2_superbubbles", "fasta": None, "synth": {"workload": "m2r2", "seed": 12345, "scale": 0.05}}
    files = case_files(case, d)
    assert len(files) == 62
    base = [R.TWOPACO, "-k", "25", "-f", "32", "-t", "16", "--seed", "12345", "--tmpdir", d]
    junctions, table, members, bubbles = (os.path.join(d, f) for f in ("m2r2.bin", "superbubbles.tsv", "members.tsv", "bubbles.tsv"))
    r = subprocess.run(base + ["-o", junctions, "--superbubbles", "file", "--superbubbles-out", table, "--superbubbles-members", members, "--bubbles", "file", "--bubbles-out", bubbles] +
                       files, capture_output=True, timeout=900, env=dict(os.environ, TWOPACO_TIMING="1"))
    assert r.returncode == 0, r.stderr[-800:]
    print("\n".join(line for line in r.stderr.decode().split("\n") if "bubbles" in line or "links" in line))
    seqs = []
    for f in files:
        seqs += ["-s", f]
    serial, serial_members = os.path.join(d, "serial.tsv"), os.path.join(d, "serial_members.tsv")
    r = subprocess.run([R.GRAPHDUMP, junctions, "-k", "25", "--superbubbles", "file", "--superbubbles-out", serial, "--superbubbles-members", serial_members] + seqs,
                       capture_output=True, timeout=900)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    got, ref = open(table, "rb").read(), open(serial, "rb").read()
    head = ref.split(b"\n", 1)[0].decode().split("\t")
    assert head[:4] == ["#twopaco-superbubbles", "1", "by=file", "k=25"] and head[4] == "colors=62" and head[7] == "max_inside=62"
    segments, links, rows = (int(head[i].split("=")[1]) for i in (5, 6, 8))
    simple = int(open(bubbles, "rb").readline().decode().rstrip("\n").split("bubbles=")[1])
    sizes = [line.decode() for line in ref.split(b"\n") if line.startswith(b"#inside")]
    print("segments", segments, "links", links, "superbubbles", rows, "simple bubbles", simple, "inside:", " ".join(s.replace("#inside\t", "").replace("\t", "x") for s in sizes))
    assert rows > 0 and simple > 0
    assert len(got) == len(ref) and hashlib.sha256(got).hexdigest() == hashlib.sha256(ref).hexdigest()
    got, ref = open(members, "rb").read(), open(serial_members, "rb").read()
    assert len(got) == len(ref) and hashlib.sha256(got).hexdigest() == hashlib.sha256(ref).hexdigest()
