"""GPU (-m gpu): the connected components on the device (csrc/tpc_components.hip, the tpc_segments_components_* group of
include/twopaco_hip.h) against their definition, restated in components_reference.py over the serial gfa1 text (pinned to the real
reference's sha256 by tests/golden/graphdump.json): component[], every plane of the rows, presence and info[] through the C-ABI on
a host stream and a resident stream, the colour counts at the word boundaries, the step bound's error return, the stages it leaves
untouched, ranges and refusals, and the bytes of `graphdump --components --gpu` and `twopaco --components`."""
import json
import os
import subprocess
import time

import numpy as np
import pytest

import components_reference as R
from colors_reference import presence_words
from helpers import GOLDEN, case_files, golden_cases
from links_reference import read_fasta

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in golden_cases()}
MAXU = (1 << 64) - 1
GENERATED_CASE = {
    "islands": {"k": R.ISLANDS_K, "L": R.ISLANDS_L, "q": R.ISLANDS_Q, "seed": R.ISLANDS_SEED, "rounds": [{"low": 0, "high": 1 << R.ISLANDS_L}], "n_rounds": 1, "abundance": None},
    "b78": {"k": R.BUBBLE_K, "L": R.BUBBLE_L, "q": R.BUBBLE_Q, "seed": R.BUBBLE_SEED, "rounds": [{"low": 0, "high": 1 << R.BUBBLE_L}], "n_rounds": 1, "abundance": None},
    "short": {"k": 11, "L": 20, "q": 5, "seed": 11, "rounds": [{"low": 0, "high": 1 << 20}], "n_rounds": 1, "abundance": None},
}
NAMES = ["islands", "b78", "short", "rand6_k3", "tr_k25_L28", "c2_k29", "example_k11"]


@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


def ambiguous_positions(fasta, rec_start):
    return [int(rec_start[r]) + i for r, (_, s) in enumerate(read_fasta(fasta)) for i, ch in enumerate(s) if ch not in "ACGTN"]


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
    """components_reference.generated_inputs, made once: FASTA, junction stream (from the CPU restatement of the pipeline, oracle/)
    and the serial gfa1 of islands, b78 and short; the oracles are kept beside them."""
    d = str(tmp_path_factory.mktemp("components"))
    got = {"dir": d}
    for name, (fa, stream, gfa1, k) in R.generated_inputs(d).items():
        got[name] = {"fasta": fa, "stream": stream, "gfa1": gfa1, "k": k, "oracle": {}}
    R.check_islands(R.Components(got["islands"]["gfa1"], "sequence"))
    return got


def inputs(name, made, by="file"):
    """(case, fasta, stream bytes, oracle, graphdump's arguments, its directory)"""
    if name in made:
        m = made[name]
        if by not in m["oracle"]:
            m["oracle"][by] = R.Components(m["gfa1"], by, k=m["k"])
        return dict(GENERATED_CASE[name], name=name), m["fasta"], open(m["stream"], "rb").read(), m["oracle"][by], [m["stream"], "-k", str(m["k"]), "-s", m["fasta"]], made["dir"]
    case = CASES[name]
    v = R.case_vector(case)
    key = (name, by)
    if key not in _GOLDEN_ORACLES:
        _GOLDEN_ORACLES[key] = R.Components(R.golden_gfa1(v), by, k=case["k"])
    return case, os.path.join(GOLDEN, case["fasta"]), open(os.path.join(GOLDEN, case["bin"]), "rb").read(), _GOLDEN_ORACLES[key], R.components_args(v), GOLDEN


_GOLDEN_ORACLES = {}


def color_map_of(want):
    """What tpc_segments_colors_build takes for the oracle's colours."""
    g = want.g
    if want.by == "sequence":
        return list(range(len(g.seq_name))), len(g.seq_name)
    files = list(dict.fromkeys(g.seq_file))
    return [files.index(f) for f in g.seq_file], len(files)


def check_table(ctx, want):
    """Everything the device holds after a component build == the oracle's."""
    info = ctx.segments_components_build()
    assert (info["components"], info["rows"], info["largest"]) == (want.count(), want.rows, want.largest())
    words = (want.colors["colors"] + 31) // 32
    assert info["peak_bytes"] >= 16 * want.rows + want.count() * (44 + 4 * words)
    component = ctx.segments_components_fetch_members()
    assert component.dtype == np.uint32 and component.size == want.rows and (component == want.component).all()
    root, segments, links, length, edges, occurrences = ctx.segments_components_fetch_rows()
    assert root.dtype == np.uint32 and all(a.dtype == np.uint64 for a in (segments, links, length, edges, occurrences))
    for got, ref in ((root, want.root), (segments, want.segments), (links, want.links), (length, want.length), (edges, want.edges), (occurrences, want.occurrences)):
        assert got.size == ref.size and (got.astype(np.int64) == ref).all()
    presence = ctx.segments_components_fetch_presence()
    assert presence.dtype == np.uint32 and presence.shape == (want.count(), words)
    if want.count():
        ref = presence_words(want.presence)
        assert (presence == ref).all()
        assert (np.unpackbits(presence.view(np.uint8), axis=1).sum(axis=1) == want.n_colors).all()
    assert int(segments.sum()) == want.rows and int(links.sum()) == want.n_links
    assert ctx.kernel_ms("components") > 0
    return info


# ------------------------------------------------------------------------------------------------ 1. the arrays by their definition
@pytest.mark.parametrize("source", ["host", "resident"])
@pytest.mark.parametrize("name", NAMES)
def test_component_arrays_by_their_definition(capi, made, name, source):
    case, fasta, data, want, _, _ = inputs(name, made)
    ctx = host_context(capi, fasta, data, case["k"]) if source == "host" else resident_context(capi, case, fasta, data)
    assert ctx.segments_error() is None
    assert ctx.segments_links_build()["rows"] == want.n_links
    ctx.segments_colors_build(*color_map_of(want))
    check_table(ctx, want)
    check_table(ctx, want)   # a second build replaces the first
    if name == "islands":
        assert want.largest() >= 10000 and want.root[int(want.segments.argmax())] != 0
    if name == "short":
        assert want.count() == want.rows > 0 and want.n_links == 0
    ctx.close()


def test_every_sequence_lies_in_one_component(capi, made):
    """by=sequence colours on islands: the bit of every sequence with an event is set in exactly one component."""
    case, fasta, data, want, _, _ = inputs("islands", made, "sequence")
    ctx = host_context(capi, fasta, data, case["k"])
    ctx.segments_links_build()
    ctx.segments_colors_build(*color_map_of(want))
    check_table(ctx, want)
    presence = ctx.segments_components_fetch_presence()
    bits = np.unpackbits(presence.view(np.uint8), axis=1, bitorder="little")[:, :len(want.g.seq_name)]
    held = bits.sum(axis=0)
    has_event = np.array([(want.g.occ_seq == s).any() for s in range(len(want.g.seq_name))])
    assert (held == has_event).all() and int(has_event.sum()) == len(want.g.seq_name) - 7
    ctx.close()


def test_no_event_at_all(capi, made):
    fa = made["short"]["fasta"]
    text = capi.PackedText.from_fasta([fa])
    ctx = capi.Context(0)
    ctx.seq_upload(text)
    ctx.segments_build(b"", 11, text.rec_start, text.rec_length)
    ctx.segments_links_build()
    ctx.segments_colors_build([0] * len(text.rec_start), 1)
    info = ctx.segments_components_build()
    assert (info["components"], info["rows"], info["largest"]) == (0, 0, 0)
    assert ctx.segments_components_fetch_members().size == 0 and all(a.size == 0 for a in ctx.segments_components_fetch_rows())
    assert ctx.segments_components_fetch_presence().shape == (0, 1)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 2. colour counts
@pytest.mark.parametrize("n_colors", [1, 31, 32, 33, 64, 65])
def test_presence_at_every_word_boundary(capi, made, n_colors):
    case, fasta, data, _, _, _ = inputs("islands", made)
    n_seq = len(read_fasta(fasta))
    color_of_seq = [s % n_colors for s in range(n_seq)]
    want = R.Components(made["islands"]["gfa1"], k=case["k"], color_of_seq=color_of_seq)
    # every colour is held somewhere, the last one of the last word included; the chain family's four records follow one another
    assert want.colors["colors"] == n_colors and want.presence.any(axis=0).all() and int(want.n_colors.max()) >= min(n_colors, 4)
    ctx = host_context(capi, fasta, data, case["k"])
    ctx.segments_links_build()
    ctx.segments_colors_build(color_of_seq, n_colors)
    check_table(ctx, want)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 3. the bound
def test_the_step_limit_gives_up_with_an_error_text(capi, made):
    """test_components_step_limit = 1: a find may look at one parent, so the flatten pass gives up at the first row that is not its
    own root.  An ordinary error return from kernels that end normally; the other tables are what they were."""
    case, fasta, data, want, _, _ = inputs("islands", made)
    ctx = host_context(capi, fasta, data, case["k"])
    ctx.segments_links_build()
    ctx.segments_colors_build(*color_map_of(want))

    def others():
        name, first = ctx.segments_fetch()
        return [name, first] + list(ctx.segments_links_fetch_rows()) + list(ctx.segments_colors_fetch_rows()) + [ctx.segments_colors_fetch_presence()]

    before = others()
    check_table(ctx, want)
    ctx.set_option("test_components_step_limit", 1)
    with pytest.raises(RuntimeError, match="segment components: gave up after 1 steps"):
        ctx.segments_components_build()
    with pytest.raises(RuntimeError, match="tpc_segments_components_build first"):   # "build first": the failed build left no table
        ctx.segments_components_info()
    assert all((a == b).all() for a, b in zip(before, others()))
    ctx.set_option("test_components_step_limit", 0)
    check_table(ctx, want)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 4. opt-in
@pytest.mark.parametrize("order", ["colours_last", "colours_first"])
def test_the_other_tables_are_unchanged(capi, made, order):
    case, fasta, data, want, _, _ = inputs("b78", made, "sequence")
    n_seq = len(read_fasta(fasta))
    colours = (list(range(n_seq)), n_seq)

    def build_others(ctx):
        if order == "colours_last":
            ctx.segments_links_build()
            ctx.segments_colors_build(*colours)
        else:
            ctx.segments_colors_build(*colours)
            ctx.segments_links_build()
        ctx.segments_bubbles_build()
        ctx.segments_distances_build()

    def outputs(ctx):
        name, first = ctx.segments_fetch()
        begin, end = ctx.segments_fetch_events()
        got = [name, first, begin, end, ctx.segments_fetch_sequences(0, n_seq + 1)]
        got += list(ctx.segments_colors_fetch_rows()) + [ctx.segments_colors_fetch_presence()] + list(ctx.segments_colors_fetch_hist())
        got += list(ctx.segments_links_fetch_rows()) + [ctx.segments_links_fetch_first()]
        got += list(ctx.segments_bubbles_fetch_rows()) + list(ctx.segments_bubbles_fetch_sides()) + [ctx.segments_bubbles_fetch_hist()]
        got += list(ctx.segments_distances_fetch())
        counts = {key: n for key, n in ctx.segments_counts().items() if key != "peak_device_bytes"}   # that one belongs to one build, not to the input
        return counts, ctx.segments_error(), ctx.segments_colors_info(), ctx.segments_links_info(), got

    alone = host_context(capi, fasta, data, case["k"])
    build_others(alone)
    ref = outputs(alone)
    alone.close()
    ctx = host_context(capi, fasta, data, case["k"])
    build_others(ctx)
    for _ in range(2):
        check_table(ctx, want)
        got = outputs(ctx)
        assert got[:4] == ref[:4]
        assert all(a.shape == b.shape and (a == b).all() for a, b in zip(got[4], ref[4]))
    # a bubble build and a distance build leave the components where they are
    ctx.segments_bubbles_build()
    ctx.segments_distances_build()
    assert (ctx.segments_components_fetch_members() == want.component).all()
    # a new link build drops them, and so does a new colour build
    ctx.segments_links_build()
    with pytest.raises(RuntimeError, match="tpc_segments_components_build first"):
        ctx.segments_components_info()
    check_table(ctx, want)
    ctx.segments_colors_build(*colours)
    with pytest.raises(RuntimeError, match="tpc_segments_components_build first"):
        ctx.segments_components_fetch_members(0, 0)
    check_table(ctx, want)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 5. ranges and refusals
def test_fetch_ranges(capi, made):
    case, fasta, data, want, _, _ = inputs("b78", made, "sequence")
    ctx = host_context(capi, fasta, data, case["k"])
    ctx.segments_links_build()
    ctx.segments_colors_build(*color_map_of(want))
    n, rows = ctx.segments_components_build()["components"], want.rows
    assert n == want.count() == 4
    assert (ctx.segments_components_fetch_members(100, 71) == want.component[100:171]).all()
    assert ctx.segments_components_fetch_members(rows, 0).size == 0
    for r0, m in ((rows, 1), (rows + 1, 0), (0, rows + 1), (MAXU, 2)):
        with pytest.raises(RuntimeError, match="segment components: bad row range"):
            ctx.segments_components_fetch_members(r0, m)
    got = ctx.segments_components_fetch_rows(1, 2)
    for a, ref in zip(got, (want.root, want.segments, want.links, want.length, want.edges, want.occurrences)):
        assert (a.astype(np.int64) == ref[1:3]).all()
    assert (ctx.segments_components_fetch_presence(2, 2) == presence_words(want.presence)[2:4]).all()
    assert all(a.size == 0 for a in ctx.segments_components_fetch_rows(n, 0)) and ctx.segments_components_fetch_presence(n, 0).shape[0] == 0
    for p0, m in ((n, 1), (n + 1, 0), (0, n + 1), (MAXU, 2)):
        with pytest.raises(RuntimeError, match="segment components: bad row range"):
            ctx.segments_components_fetch_rows(p0, m)
        with pytest.raises(RuntimeError, match="segment components: bad row range"):
            ctx.segments_components_fetch_presence(p0, m)
    check_table(ctx, want)   # still usable
    ctx.close()


def test_refusals(capi, made):
    case, fasta, data, want, _, _ = inputs("b78", made)
    text = capi.PackedText.from_fasta([fasta])
    colours = color_map_of(want)
    ctx = capi.Context(0)
    with pytest.raises(RuntimeError, match="segment components: build the segment table first"):   # no table
        ctx.segments_components_build()
    for call in (ctx.segments_components_info, ctx.segments_components_fetch_members, ctx.segments_components_fetch_rows, ctx.segments_components_fetch_presence):
        with pytest.raises(RuntimeError, match="tpc_segments_components_build first"):
            call()
    # the context is usable: a table, then no link table yet, then no colour table yet
    ctx.seq_upload(text)
    ctx.segments_build(data, case["k"], text.rec_start, text.rec_length, ambiguous_positions(fasta, text.rec_start))
    with pytest.raises(RuntimeError, match="segment components: build the link table first"):
        ctx.segments_components_build()
    ctx.segments_colors_build(*colours)
    with pytest.raises(RuntimeError, match="segment components: build the link table first"):
        ctx.segments_components_build()
    ctx.segments_build(data, case["k"], text.rec_start, text.rec_length, ambiguous_positions(fasta, text.rec_start))
    ctx.segments_links_build()
    with pytest.raises(RuntimeError, match="segment components: build the colour table first"):
        ctx.segments_components_build()
    with pytest.raises(RuntimeError, match="tpc_segments_components_build first"):
        ctx.segments_components_info()
    assert ctx.segments_counts()["events"] > 0 and ctx.segments_error() is None
    ctx.segments_colors_build(*colours)
    check_table(ctx, want)
    # a new segment build drops the components of the old one (and its links and colours)
    ctx.segments_build(b"", case["k"], text.rec_start, text.rec_length)
    with pytest.raises(RuntimeError, match="tpc_segments_components_build first"):
        ctx.segments_components_fetch_members(0, 0)
    with pytest.raises(RuntimeError, match="segment components: build the link table first"):
        ctx.segments_components_build()
    ctx.close()
    # a table whose walk failed
    bad = CASES["edge_k5"]
    ctx = host_context(capi, os.path.join(GOLDEN, bad["fasta"]), open(os.path.join(GOLDEN, bad["bin"]), "rb").read(), bad["k"])
    assert ctx.segments_error() is not None
    with pytest.raises(RuntimeError, match="segment components: the segment table holds the walk's error 1 at slot 3"):
        ctx.segments_components_build()
    with pytest.raises(RuntimeError, match="tpc_segments_components_build first"):
        ctx.segments_components_info()
    # and the same context goes on: a new table in it gets its components
    bad_text = capi.PackedText.from_fasta([os.path.join(GOLDEN, bad["fasta"])])
    ctx.segments_build(b"", bad["k"], bad_text.rec_start, bad_text.rec_length)
    ctx.segments_links_build()
    ctx.segments_colors_build([0] * len(bad_text.rec_start), 1)
    assert ctx.segments_components_build()["components"] == 0
    with pytest.raises(RuntimeError, match="unknown option"):
        ctx.set_option("test_components_step_limits", 1)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 6. bytes
@pytest.mark.parametrize("by", ["file", "sequence"])
@pytest.mark.parametrize("name", NAMES)
def test_graphdump_gpu_writes_the_oracle_bytes(tmp_path, made, name, by):
    case, fasta, _, want, args, cwd = inputs(name, made, by)
    stats, members = str(tmp_path / "stats.json"), str(tmp_path / "members.tsv")
    env = dict(os.environ, TWOPACO_GRAPHDUMP_STATS=stats)
    r = subprocess.run([R.GRAPHDUMP] + args + ["--components", by, "--components-members", members, "--gpu", "--threads", "16"], cwd=cwd, capture_output=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert r.stdout == want.tsv(), name
    assert open(members, "rb").read() == want.members()
    s = json.load(open(stats))
    assert s["path"] == "device" and s["components_kernel_ms"] > 0 and s["components"] == want.count() and s["largest_component"] == want.largest() and s["links"] == want.n_links
    out = str(tmp_path / "components.tsv")
    r = R.run_graphdump(args + ["--components", by, "--gpu", "--components-out", out, "--prefix"], cwd=cwd)
    assert r.returncode == 0 and r.stdout == b"" and open(out, "rb").read() == want.tsv()


def test_graphdump_gpu_beside_the_other_tables_and_a_failing_walk(tmp_path, made):
    case, fasta, _, want, args, cwd = inputs("b78", made, "sequence")
    alone = {flag: R.run_graphdump(args + [flag, "sequence"], cwd=cwd).stdout for flag in ("--colors", "--bubbles", "--distances")}
    for flag in alone:
        r = R.run_graphdump(args + [flag, "sequence", "--components", "sequence", "--gpu"], cwd=cwd)
        assert r.returncode == 0 and r.stderr == b"" and r.stdout == alone[flag] + want.tsv(), flag
    v = R.vector_of("edge_k5")
    out, members = str(tmp_path / "components.tsv"), str(tmp_path / "members.tsv")
    r = R.run_graphdump(R.components_args(v) + ["--components", "file", "--gpu", "--components-out", out, "--components-members", members])
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
    case, fasta, data, want, _, _ = inputs(name, made, by)
    d = str(tmp_path)
    table, members, junctions = os.path.join(d, "components.tsv"), os.path.join(d, "members.tsv"), os.path.join(d, "j.bin")
    given, cwd = cli_input(name, fasta)
    r = cli(case, ["--tmpdir", d, "--components", by, "--components-out", table, "--components-members", members, "-o", junctions], given, cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert open(junctions, "rb").read() == data
    assert open(table, "rb").read() == want.tsv() and open(members, "rb").read() == want.members()
    assert sorted(os.listdir(d)) == ["components.tsv", "j.bin", "members.tsv"]


@pytest.mark.parametrize("name", ["b78", "c2_k29"])
def test_twopaco_components_beside_everything_else(tmp_path, made, name):
    """--components with --graph gfa1 --graph-compact --links --colors --bubbles --distances: one segment, colour and link build serve
    all, and every other file has the bytes it has without --components."""
    case, fasta, _, want, _, _ = inputs(name, made, "sequence")
    given, cwd = cli_input(name, fasta)
    with_dir, without_dir = str(tmp_path / "with"), str(tmp_path / "without")
    files = ("graph.gfa", "links.tsv", "colors.tsv", "bubbles.tsv", "distances.tsv")
    for d, extra in ((without_dir, []), (with_dir, ["--components", "sequence", "--components-out", os.path.join(with_dir, "components.tsv")])):
        os.mkdir(d)
        r = cli(case, ["--tmpdir", d, "--graph", "gfa1", "--graph-compact", "--graph-out", os.path.join(d, "graph.gfa"), "--links", "--links-out", os.path.join(d, "links.tsv"),
                       "--colors", "sequence", "--colors-out", os.path.join(d, "colors.tsv"), "--bubbles", "sequence", "--bubbles-out", os.path.join(d, "bubbles.tsv"),
                       "--distances", "sequence", "--distances-out", os.path.join(d, "distances.tsv")] + extra, given, cwd=cwd)
        assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert sorted(os.listdir(without_dir)) == sorted(files) and sorted(os.listdir(with_dir)) == sorted(files + ("components.tsv",))
    for f in files:
        assert open(os.path.join(with_dir, f), "rb").read() == open(os.path.join(without_dir, f), "rb").read(), f
    assert open(os.path.join(with_dir, "components.tsv"), "rb").read() == want.tsv()
    # beside the plain graph rendered on the device, where no event table is fetched for the graph
    d = str(tmp_path / "device")
    os.mkdir(d)
    r = cli(case, ["--tmpdir", d, "--graph", "gfa1", "--graph-text", "device", "--graph-out", os.path.join(d, "graph.gfa"), "--components", "sequence",
                   "--components-out", os.path.join(d, "components.tsv"), "--components-members", os.path.join(d, "members.tsv")], given, cwd=cwd)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    assert open(os.path.join(d, "components.tsv"), "rb").read() == want.tsv() and open(os.path.join(d, "members.tsv"), "rb").read() == want.members()
    assert sorted(os.listdir(d)) == ["components.tsv", "graph.gfa", "members.tsv"]


def test_twopaco_default_file_timing_lines_and_refusals(tmp_path, made):
    case, fasta, _, want, _, _ = inputs("b78", made)
    d = str(tmp_path)
    r = cli(case, ["--tmpdir", d, "--components", "file"], fasta, cwd=d, env=dict(os.environ, TWOPACO_TIMING="1"))
    assert r.returncode == 0, r.stderr[-400:]
    assert sorted(os.listdir(d)) == ["de_bruijn.bin", "de_bruijn.components.tsv"]
    err = r.stderr.decode()
    assert "segment components:" in err and "segment components fetch:" in err and "components_kernel_ms" in err and "component table writing:" in err
    assert open(os.path.join(d, "de_bruijn.components.tsv"), "rb").read() == want.tsv()
    os.unlink(os.path.join(d, "de_bruijn.bin"))
    os.unlink(os.path.join(d, "de_bruijn.components.tsv"))
    r = cli(case, ["--tmpdir", d, "--components", "file", "--gpus", "2"], fasta, cwd=d)
    assert r.returncode == 1 and r.stderr.decode().endswith("not with --gpus above 1 for arg (--components)\n") and os.listdir(d) == []
    # an input the walk refuses: the walk's message, no file
    bad = CASES["edge_k5"]
    r = cli(bad, ["--tmpdir", d, "--components", "file", "--components-out", os.path.join(d, "components.tsv"), "--components-members", os.path.join(d, "members.tsv"),
                  "--graph", "gfa1", "--graph-out", os.path.join(d, "graph.gfa")])
    assert r.returncode == 1 and r.stderr.decode() == "\nError: The input is corrupted\n"
    assert os.listdir(d) == []


# ------------------------------------------------------------------------------------------------ 7. at size
M2R2_SCALE, M2R2_SEED = 0.05, 450


def test_m2r2_components_equal_the_serial_graphdump(tmp_path):
    """synth m2r2 at scale 0.05, synth seed 450, k = 25, f = 32 (the workload of test_gpu_bubbles.py at a smaller scale: 62 files,
    tracts and minisatellites): sha256 and size of `twopaco --components file -o` == those of the serial `graphdump --components file`
    over the junction stream of the same command, and the table has more than one component.
    Why this seed.  m2r2's 62 genomes descend from one root, so nearly every contig shares (k+1)-mers with the same stretch of its
    clade's other members and hangs in the one giant component.  An island needs a contig all of whose (k+1)-mers are private: one of
    k + 1 .. 2k letters with a substitution of the member's own (0.2 % of the letters) where all its windows overlap -- about 0.2 such
    contigs per input at this scale.  Seed 12345 (test_gpu_bubbles.py) has none, at scale 0.05 and at 0.18 alike: components=1.  Seeds
    were read off the generator's records alone (a contig whose 26-mers occur nowhere else in the input, no record shorter than k, which
    the serial walk refuses): seed 450 has three such contigs of 33 letters.  The serial table then holds 78 034 segments, 104 733 links
    and 4 components: the giant one and three of one segment.
    Measured on an MI355X: the test takes 0.56 s (twopaco 0.2 s, serial graphdump 0.2 s)."""
    import hashlib
    d = str(tmp_path)
    case = {"name": "m2r2_components", "fasta": None, "synth": {"workload": "m2r2", "seed": M2R2_SEED, "scale": M2R2_SCALE}}
    files = case_files(case, d)
    assert len(files) == 62
    base = [R.TWOPACO, "-k", "25", "-f", "32", "-t", "16", "--seed", "12345", "--tmpdir", d]
    junctions, table = os.path.join(d, "m2r2.bin"), os.path.join(d, "components.tsv")
    t0 = time.time()
    r = subprocess.run(base + ["-o", junctions, "--components", "file", "--components-out", table] + files, capture_output=True, timeout=900)
    device_s = time.time() - t0
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-800:]
    seqs = []
    for f in files:
        seqs += ["-s", f]
    serial = os.path.join(d, "serial.tsv")
    t0 = time.time()
    r = subprocess.run([R.GRAPHDUMP, junctions, "-k", "25", "--components", "file", "--components-out", serial] + seqs, capture_output=True, timeout=900)
    serial_s = time.time() - t0
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    got, ref = open(table, "rb").read(), open(serial, "rb").read()
    head = ref.split(b"\n", 1)[0].decode().split("\t")
    assert head[:4] == ["#twopaco-components", "1", "by=file", "k=25"] and head[4] == "colors=62"
    segments, links, components = (int(head[i].split("=")[1]) for i in (5, 6, 7))
    print("segments", segments, "links", links, "components", components, "twopaco %.1f s" % device_s, "serial graphdump %.1f s" % serial_s)
    assert len(got) == len(ref) and hashlib.sha256(got).hexdigest() == hashlib.sha256(ref).hexdigest()
    assert components > 1 and components == 4
