"""GPU (-m gpu): tpc_distinct_sketch (csrc/tpc_sketch.hip) bit for bit against its definition (tests/sketch_reference.py, which
evaluates every window directly), the properties a strand or a reset bug breaks, and `twopaco -f auto` end to end: the log, the
estimate against the exact count, and the junction file against the run with the chosen size typed by hand."""
import os
import re
import subprocess

import numpy as np
import pytest

import sketch_reference as SR
from helpers import GOLDEN, golden_cases, parse_log, text_codes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWOPACO = os.path.join(ROOT, "twopaco_amd", "bin", "twopaco")
BOUND = 3 * 1.04 / np.sqrt(16384)   # three standard errors of HyperLogLog at p = 14: 2.44 %
TILE = 8192
MAIN_POSITIONS = 3 * TILE + 777     # three tiles and a partial one


@pytest.fixture(scope="module")
def capi():
    from twopaco_amd import capi as m
    m.hip()
    m.host()
    return m


def codes_of(text):
    return text_codes(text.bases, text.nmask, text.length)


def sketch_of(capi, text, k):
    ctx = capi.Context(0)
    ctx.seq_upload(text)
    got = ctx.distinct_sketch(k)
    ctx.close()
    return got


def check_equal(got, want, what):
    (reg, windows), (want_reg, want_windows) = got, want
    assert reg.dtype == np.uint8 and reg.shape == (16384,)
    assert windows == want_windows, what
    diff = np.nonzero(reg != want_reg)[0]
    assert diff.size == 0, (what, diff[:8], reg[diff[:8]], want_reg[diff[:8]])


# ------------------------------------------------------------------------------------------------ 1. registers by their definition
def main_fasta(k, path):
    """Records separated by 'N' (the record boundaries) that fill MAIN_POSITIONS text positions: one of exactly k + 1 letters, one
    of k letters (no window), and a long one that holds an 'N', a run of k + 2 'N', an IUPAC letter and lower-case letters, each
    followed by a little more than one window of letters; the rest is random and covers the tile borders."""
    n = k + 1
    rng = np.random.default_rng(1000 + k)

    def letters(count):
        return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, count)]).decode()

    a, b = letters(k + 1), letters(k)
    c = letters(n + 5) + "N" + letters(n + 7) + "N" * (k + 2) + letters(n + 3) + "R" + letters(n + 9).lower() + "y" + letters(n + 2)
    c += letters(MAIN_POSITIONS - 4 - len(a) - len(b) - len(c))
    with open(path, "w") as f:
        for name, rec in (("exact", a), ("short", b), ("long", c)):
            f.write(">%s\n" % name)
            for i in range(0, len(rec), 70):
                f.write(rec[i:i + 70] + "\n")


@pytest.mark.parametrize("k", [3, 25, 31, 63, 65, 129, 603])
def test_registers_equal_the_definition_on_the_main_text(capi, tmp_path, k):
    path = str(tmp_path / "main.fa")
    main_fasta(k, path)
    text = capi.PackedText.from_fasta([path])
    codes = codes_of(text)
    assert text.length == MAIN_POSITIONS == codes.size
    assert text.rec_length.tolist()[:2] == [k + 1, k]
    # what the text is there for: a window starts at the last offset of a tile and at the first of the next
    for g in (TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, 3 * TILE - 1, 3 * TILE):
        assert (codes[g:g + k + 1] < 4).all(), g
    assert (codes == 4).sum() >= 4 + 1 + (k + 2) + 2   # separators, the runs, the IUPAC letters
    want = SR.sketch_reference(codes, k)
    assert 0 < want[1] < MAIN_POSITIONS
    check_equal(sketch_of(capi, text, k), want, "main text, k = %d" % k)


@pytest.mark.parametrize("fasta,k", [("lk.fa", 603), ("tracts.fa", 25), ("tracts.fa", 11), ("c2.fa", 25), ("c2.fa", 65)])
def test_registers_equal_the_definition_on_golden_inputs(capi, fasta, k):
    text = capi.PackedText.from_fasta([os.path.join(GOLDEN, fasta)])
    want = SR.sketch_reference(codes_of(text), k)
    assert want[1] > 0
    check_equal(sketch_of(capi, text, k), want, "%s, k = %d" % (fasta, k))


_MILLION = {}


def million(capi):
    """A text of 2^20 positions (128 tiles) with a few 'N' inside, and its reference, made once."""
    if not _MILLION:
        rng = np.random.default_rng(77)
        lens = [400000, 300000]
        lens.append((1 << 20) - 1 - sum(x + 1 for x in lens) - 1)
        recs = []
        for x in lens:
            r = rng.integers(0, 4, x).astype(np.uint8)
            r[rng.integers(0, x, 40)] = 4
            recs.append(r)
        text = capi.PackedText.from_codes(recs)
        assert text.length == 1 << 20
        _MILLION.update(text=text, want=SR.sketch_reference(codes_of(text), 25))
    return _MILLION["text"], _MILLION["want"]


def test_a_million_positions_one_workgroup_per_tile(capi):
    """128 workgroups merge into the global registers."""
    text, want = million(capi)
    check_equal(sketch_of(capi, text, 25), want, "2^20 positions")


def test_a_million_positions_five_striding_workgroups(capi):
    """Option test_sketch_grid: five long-lived workgroups take 25 or 26 tiles each (registers kept across tiles, one merge each)."""
    text, want = million(capi)
    ctx = capi.Context(0)
    try:
        ctx.set_option("test_sketch_grid", 5)
        ctx.seq_upload(text)
        check_equal(ctx.distinct_sketch(25), want, "2^20 positions, 5 workgroups")
    finally:
        ctx.set_option("test_sketch_grid", 0)
        ctx.close()


def test_k_beyond_the_halo_is_refused_with_a_text(capi):
    text = capi.PackedText.from_fasta([os.path.join(GOLDEN, "lk.fa")])
    ctx = capi.Context(0)
    ctx.seq_upload(text)
    check_equal(ctx.distinct_sketch(669), SR.sketch_reference(codes_of(text), 669), "k = 669")
    with pytest.raises(RuntimeError, match="too large for the sketch"):
        ctx.distinct_sketch(671)
    fresh = capi.Context(0)
    with pytest.raises(RuntimeError, match="seq_upload first"):
        fresh.distinct_sketch(25)
    fresh.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------ 2. properties
def test_text_followed_by_its_reverse_complement_gives_the_same_registers(capi):
    codes = SR.fasta_codes(os.path.join(GOLDEN, "tracts.fa"))
    for k in (25, 64):   # window 65: the rotation wraps
        alone = capi.PackedText.from_codes([codes[1:-1]])
        both = capi.PackedText.from_codes([codes[1:-1], SR.revcomp_codes(codes[1:-1])])
        assert both.length == 2 * alone.length - 1
        a, b = sketch_of(capi, alone, k), sketch_of(capi, both, k)
        assert a[1] > 0 and b[1] == 2 * a[1] and (a[0] == b[0]).all()
        check_equal(a, SR.sketch_reference(codes, k), "tracts alone")


def test_repeated_calls_and_calls_around_a_run_give_the_same_registers(capi, tmp_path):
    case = [c for c in golden_cases() if c["name"] == "c2_k29"][0]
    text = capi.PackedText.from_fasta([os.path.join(GOLDEN, case["fasta"])])
    k = case["k"]
    want = SR.sketch_reference(codes_of(text), k)
    ctx = capi.Context(0)
    ctx.seq_upload(text)                       # upload -> sketch -> set_params -> the rest of the run
    check_equal(ctx.distinct_sketch(k), want, "first call")
    check_equal(ctx.distinct_sketch(k), want, "second call")
    other = ctx.distinct_sketch(35)
    assert (other[0] != want[0]).any()         # (another k in between: every call starts from zero)
    check_equal(ctx.distinct_sketch(k), want, "after another k")
    assert ctx.kernel_ms("sketch") > 0
    ctx.set_params(k, case["L"], case["q"], capi.seed_table(case["q"], case["L"], seed=case["seed"]))
    check_equal(ctx.distinct_sketch(k), want, "after set_params")
    ctx.run_begin()
    for st in case["rounds"]:
        ctx.filter_reset()
        ctx.pass1_insert(st["low"], st["high"])
        ctx.pass1_query(st["low"], st["high"])
        ctx.pass2_filter()
    assert ctx.junctions_finalize() == case["distinct"]
    ctx.emit()
    stream, _ = ctx.emit_stream(text.rec_start, text.rec_length)
    assert stream == open(os.path.join(GOLDEN, case["bin"]), "rb").read()   # the sketch before the run disturbed nothing
    check_equal(ctx.distinct_sketch(k), want, "after a full run")
    ctx.close()


def test_text_shorter_than_a_window_gives_zeros(capi):
    text = capi.PackedText.from_codes([np.array([0, 1, 2, 3, 0, 1], dtype=np.uint8)])
    ctx = capi.Context(0)
    ctx.seq_upload(text)
    for k in (7, 25, 603):   # the text has 8 positions; k = 7 has a window's length but its separators are 'N'
        reg, windows = ctx.distinct_sketch(k)
        assert windows == 0 and not reg.any()
    reg, windows = ctx.distinct_sketch(5)
    assert windows == 1 and (reg != 0).sum() == 1
    ctx.close()


# ------------------------------------------------------------------------------------------------ 3. twopaco -f auto
CASES = {c["name"]: c for c in golden_cases()}
_EXACT = {}


def exact_and_junctions(fasta):
    """(exact distinct edges at k = 25, distinct junctions at k = 25).  The junction count does not depend on the filter: it is the
    golden's (rand6_k25_q3, tr_k25_L28); c2.fa has no golden at k = 25, so the oracle counts there."""
    if fasta not in _EXACT:
        exact = SR.exact_distinct(SR.fasta_codes(os.path.join(GOLDEN, fasta)), 25)
        if fasta == "c2.fa":
            from oracle import oracle as O
            o = O.Oracle(25, 20, 5, O.seed_table(7, 5, 20))
            o.add_fasta(os.path.join(GOLDEN, fasta))
            o.enumerate()
            junctions = len(o.keys)
            o.close()
        else:
            junctions = CASES[{"rand6.fa": "rand6_k25_q3", "tracts.fa": "tr_k25_L28"}[fasta]]["distinct"]
        _EXACT[fasta] = (exact, junctions)
    return _EXACT[fasta]


def twopaco(args, cwd, env=None, timeout=300):
    full = dict(os.environ)
    full.update(env or {})
    return subprocess.run([TWOPACO] + args, cwd=cwd, capture_output=True, timeout=timeout, env=full)


def auto_lines(log):
    """The lines -f auto adds, which must come before "Threads = "."""
    head = log[:log.index("Threads = ")]
    out = {}
    for key, pat in (("estimate", r"^Distinct edges \(estimate\) = (\d+)$"), ("L", r"^Filter size \(auto\) = (\d+)$"), ("rounds", r"^Rounds \(auto\) = (\d+)$"),
                     ("false_marks", r"^Predicted false marks per position = (\S+)$")):
        m = re.search(pat, head, re.M)
        if m:
            out[key] = float(m.group(1)) if key == "false_marks" else int(m.group(1))
    return out


def after_threads(log):
    """What a run prints from "Threads = " on, without its clock: the parameters, every round's range and counters, the totals
    (the phase times are whole seconds and may differ between two runs)."""
    tail = log[log.index("Threads = "):]
    head = [ln for ln in tail.split("\n") if re.match(r"(Threads|Vertex length|Hash functions|Filter size|Capacity|Distinct junctions) ", ln)]
    return head, parse_log(tail)


@pytest.mark.parametrize("fasta", ["rand6.fa", "c2.fa", "tracts.fa"])
@pytest.mark.parametrize("q", [5, 3])
def test_auto_run_equals_the_run_with_the_chosen_size_typed(capi, tmp_path, fasta, q):
    d = str(tmp_path)
    path = os.path.join(GOLDEN, fasta)
    exact, junctions = exact_and_junctions(fasta)
    base = ["-k", "25", "--seed", "7", "-q", str(q), "--tmpdir", d]
    r = twopaco(base + ["-f", "auto", "-o", "auto.bin", path], d)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    log = r.stdout.decode()
    auto = auto_lines(log)
    print(fasta, q, auto, "exact", exact)
    assert set(auto) == {"estimate", "L", "rounds", "false_marks"}
    assert abs(auto["estimate"] - exact) <= BOUND * exact
    plan = capi.filter_plan(auto["estimate"], q, 1 << 40, 1 << 40)
    assert auto["L"] == plan["L"] == 32 and auto["rounds"] == plan["rounds"] == 1      # the floor: these inputs need far less
    assert abs(auto["false_marks"] - plan["false_marks"]) <= 1e-4 * plan["false_marks"] + 1e-300   # (six digits are printed)
    assert "Filter size = %d\n" % (1 << auto["L"]) in log and "Distinct junctions = %d\n" % junctions in log
    r2 = twopaco(base + ["-f", str(auto["L"]), "-r", str(auto["rounds"]), "-o", "typed.bin", path], d)
    assert r2.returncode == 0 and r2.stderr == b"", r2.stderr[-400:]
    typed = r2.stdout.decode()
    assert "(auto)" not in typed and after_threads(typed) == after_threads(log)
    want = open(os.path.join(d, "typed.bin"), "rb").read()
    assert len(want) > 0 and open(os.path.join(d, "auto.bin"), "rb").read() == want
    # the same through CreateEnumerator with autoFilterSize
    e = capi.Enumerator([path], 25, "auto", q=q, rounds=0, tmpdir=d, out=os.path.join(d, "host.bin"), seed=7)
    assert e.vertices_count() == junctions
    assert auto_lines(e.log) == auto and after_threads(e.log)[1] == after_threads(log)[1] and after_threads(e.log)[0] == after_threads(log)[0][:-1]
    e.close()
    assert open(os.path.join(d, "host.bin"), "rb").read() == want
    if q == 5:
        # --graph under auto: the text of the run with the size typed
        for name, size in (("auto.gfa", ["-f", "auto"]), ("typed.gfa", ["-f", str(auto["L"]), "-r", str(auto["rounds"])])):
            rg = twopaco(base + size + ["--graph", "gfa1", "--graph-out", name, path], d)
            assert rg.returncode == 0 and rg.stderr == b"", rg.stderr[-400:]
        text = open(os.path.join(d, "typed.gfa"), "rb").read()
        assert text.startswith(b"H\tVN:Z:1.0\n") and open(os.path.join(d, "auto.gfa"), "rb").read() == text
        e = capi.Enumerator([path], 25, "auto", q=q, rounds=0, tmpdir=d, seed=7, graph="gfa1", graph_out=os.path.join(d, "host.gfa"))
        e.close()
        assert open(os.path.join(d, "host.gfa"), "rb").read() == text


def test_given_rounds_enter_the_plan_and_are_not_announced(capi, tmp_path):
    d = str(tmp_path)
    path = os.path.join(GOLDEN, "rand6.fa")
    r = twopaco(["-k", "25", "--seed", "7", "-f", "auto", "-r", "2", "-o", "auto.bin", "--tmpdir", d, path], d)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    log = r.stdout.decode()
    auto = auto_lines(log)
    assert set(auto) == {"estimate", "L", "false_marks"} and auto["L"] == 32 and log.count("Round ") == 2
    r2 = twopaco(["-k", "25", "--seed", "7", "-f", "32", "-r", "2", "-o", "typed.bin", "--tmpdir", d, path], d)
    assert r2.returncode == 0 and after_threads(r2.stdout.decode()) == after_threads(log)
    assert open(os.path.join(d, "auto.bin"), "rb").read() == open(os.path.join(d, "typed.bin"), "rb").read()


def test_a_low_cap_turns_into_rounds(capi, tmp_path):
    """TWOPACO_FILTER_CAP_BYTES = 8192: L_mem = 16 where tracts.fa needs 20 bits, so the plan cuts the edges over rounds; the
    run gives the counters and the file of `-f 16 -r <that r>`."""
    d = str(tmp_path)
    path = os.path.join(GOLDEN, "tracts.fa")
    exact, junctions = exact_and_junctions("tracts.fa")
    r = twopaco(["-k", "25", "--seed", "7", "-f", "auto", "-o", "auto.bin", "--tmpdir", d, path], d, env={"TWOPACO_FILTER_CAP_BYTES": "8192"})
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-400:]
    log = r.stdout.decode()
    auto = auto_lines(log)
    plan = capi.filter_plan(auto["estimate"], 5, 1 << 40, 8192)
    print(auto, plan)
    assert plan["L_fp"] == 20 and plan["L_mem"] == 16 and not plan["clipped"]
    assert auto["L"] == 16 == plan["L"] and auto["rounds"] == plan["rounds"] > 1 and auto["false_marks"] <= 1e-3
    assert "Warning" not in log and log.count("Round ") == auto["rounds"] and "Distinct junctions = %d\n" % junctions in log
    r2 = twopaco(["-k", "25", "--seed", "7", "-f", "16", "-r", str(auto["rounds"]), "-o", "typed.bin", "--tmpdir", d, path], d)
    assert r2.returncode == 0 and r2.stderr == b"", r2.stderr[-400:]
    # The rounds' ranges come from the split pass's first-seen histogram, and at 2^16 bits the scratch filter holds collisions: which
    # occurrence still finds an unset bit is the hardware's arrival order, so two runs of the SAME command may cut a few bins apart
    # (tests/test_gpu_parity.py says the same of the multi-round goldens).  What does not depend on the cuts must be equal: the
    # parameters, the number of rounds, the junctions the rounds add up to, the occurrences, and every byte of the junction file.
    (head_a, run_a), (head_t, run_t) = after_threads(log), after_threads(r2.stdout.decode())
    assert head_a == head_t and len(run_a["rounds"]) == len(run_t["rounds"]) == auto["rounds"]
    assert run_a["rounds"][0]["low"] == run_t["rounds"][0]["low"] == 0 and run_a["rounds"][-1]["high"] == run_t["rounds"][-1]["high"] >= 1 << 16
    assert sum(x["true"] for x in run_a["rounds"]) == sum(x["true"] for x in run_t["rounds"]) == junctions
    assert run_a["true_marks"] == run_t["true_marks"] > 0
    assert open(os.path.join(d, "auto.bin"), "rb").read() == open(os.path.join(d, "typed.bin"), "rb").read()
    # rounds given by hand that do not make up for the cap: the run says so and still finds the junctions
    r3 = twopaco(["-k", "25", "--seed", "7", "-f", "auto", "-r", "2", "-o", "clipped.bin", "--tmpdir", d, path], d, env={"TWOPACO_FILTER_CAP_BYTES": "8192"})
    assert r3.returncode == 0, r3.stderr[-400:]
    clipped = r3.stdout.decode()
    assert auto_lines(clipped)["L"] == 16 and auto_lines(clipped)["false_marks"] > 1e-3 and "Rounds (auto)" not in clipped
    assert "Warning: the filter is clipped by memory" in clipped and clipped.count("Round ") == 2
    assert "Distinct junctions = %d\n" % junctions in clipped


def test_timing_names_the_edge_sketch(tmp_path):
    d = str(tmp_path)
    r = twopaco(["-k", "25", "--seed", "7", "-f", "auto", "-o", "auto.bin", "--tmpdir", d, os.path.join(GOLDEN, "c2.fa")], d, env={"TWOPACO_TIMING": "1"})
    assert r.returncode == 0
    m = re.search(r"^\[timing\] edge sketch: (\S+) ms$", r.stderr.decode(), re.M)
    assert m and 0 < float(m.group(1)) < 1000
