"""CPU: the host half of `twopaco -f auto` -- the HyperLogLog estimate and the filter plan of twopaco_amd/host/filterplan.h
through libtwopaco_host.so, the sketch's definition (tests/sketch_reference.py) against exact distinct counts, and the flags of
the command line as far as they go without a device."""
import os
import subprocess

import numpy as np
import pytest

import sketch_reference as SR

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
BOUND = 3 * 1.04 / np.sqrt(16384)   # three standard errors of HyperLogLog at p = 14: 2.44 %
POSITIONS_M2 = 309532583            # text positions of the 62-genome workload (profiles/r04s_f_sweep.json)
REAL_MARKS_M2 = 43996758


@pytest.fixture(scope="module")
def capi(built):
    from twopaco_amd import capi as m
    return m


@pytest.fixture(scope="module")
def twopaco(built):
    path = os.path.join(os.path.dirname(HERE), "twopaco_amd", "bin", "twopaco")
    assert os.path.exists(path)
    return path


# ------------------------------------------------------------------------------------------------ inputs
def synthetic_codes(seed, base_len):
    """Position codes of N base N copy N revcomp-copy N: a random genome with a 400-bp poly-A tract, a copy of it with 1 % of
    its letters substituted and a reverse-complemented copy with 2 %."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 4, base_len).astype(np.uint8)
    at = int(rng.integers(0, base_len - 400))
    base[at:at + 400] = 0

    def mutated(x, rate):
        y = x.copy()
        hit = rng.random(y.size) < rate
        y[hit] = (y[hit] + rng.integers(1, 4, int(hit.sum())).astype(np.uint8)) & 3
        return y

    n = np.array([4], dtype=np.uint8)
    return np.concatenate([n, base, n, mutated(base, 0.01), n, SR.revcomp_codes(mutated(base, 0.02)), n])


# (name, k, seed, letters of the base genome): 2 * 10^4 to 1.5 * 10^6 distinct edges; window 66 = k 65: the rotation wraps
INPUTS = [("k11_small", 11, 101, 18000), ("k11_large", 11, 102, 1100000), ("k25_small", 25, 103, 20000), ("k25_large", 25, 104, 300000),
          ("k65_small", 65, 105, 40000), ("k65_large", 65, 106, 150000), ("k129_small", 129, 107, 30000), ("k129_large", 129, 108, 100000)]
_SKETCHED = {}


def sketched(name):
    """(registers, windows, exact distinct count) of an input, computed once per session."""
    if name not in _SKETCHED:
        if name == "linear":
            k, codes = 25, synthetic_codes(109, 3600)
        else:
            _, k, seed, base_len = [i for i in INPUTS if i[0] == name][0]
            codes = synthetic_codes(seed, base_len)
        reg, windows = SR.sketch_reference(codes, k)
        _SKETCHED[name] = (reg, windows, SR.exact_distinct(codes, k))
    return _SKETCHED[name]


# ------------------------------------------------------------------------------------------------ the sketch's accuracy
@pytest.mark.parametrize("name", [i[0] for i in INPUTS])
def test_reference_estimate_is_within_three_standard_errors(name):
    reg, windows, exact = sketched(name)
    estimate = SR.hll_estimate(reg)
    print(name, "windows", windows, "exact", exact, "estimate", estimate, "error %.3f %%" % (100 * (estimate - exact) / exact))
    assert 2e4 <= exact <= 1.5e6 and windows > exact
    assert abs(estimate - exact) <= BOUND * exact


def test_linear_counting_branch_and_the_empty_text():
    reg, windows, exact = sketched("linear")
    estimate = SR.hll_estimate(reg)
    print("linear", "exact", exact, "estimate", estimate)
    assert 4000 <= exact <= 6000
    zeros = int((reg == 0).sum())
    assert zeros > 0 and estimate == 16384 * np.log(16384 / zeros)   # the small-range branch
    assert abs(estimate - exact) <= BOUND * exact
    for codes in ([4], [4, 4], [4, 0, 1, 2, 4], []):
        reg, windows = SR.sketch_reference(np.array(codes, dtype=np.uint8), 5)
        assert windows == 0 and not reg.any() and SR.hll_estimate(reg) == 0.0


def test_golden_inputs_of_the_end_to_end_test_are_within_the_bound():
    """rand6.fa, c2.fa and tracts.fa at k = 25 (tests/test_gpu_distinct_sketch.py runs -f auto on them), lk.fa at 603."""
    for fasta, k in (("rand6.fa", 25), ("c2.fa", 25), ("tracts.fa", 25), ("lk.fa", 603)):
        codes = SR.fasta_codes(os.path.join(GOLDEN, fasta))
        reg, _ = SR.sketch_reference(codes, k)
        exact = SR.exact_distinct(codes, k)
        assert abs(SR.hll_estimate(reg) - exact) <= BOUND * exact, fasta


def test_reference_parser_agrees_with_the_packer(capi):
    from helpers import text_codes
    for fasta in ("rand6.fa", "c2.fa", "tracts.fa", "lk.fa", "edge.fa"):
        path = os.path.join(GOLDEN, fasta)
        text = capi.PackedText.from_fasta([path])
        assert (text_codes(text.bases, text.nmask, text.length) == SR.fasta_codes(path)).all(), fasta


def test_host_estimate_equals_the_numpy_estimate(capi):
    arrays = [sketched(name)[0] for name in [i[0] for i in INPUTS] + ["linear"]]
    rng = np.random.default_rng(5)
    arrays += [np.zeros(16384, dtype=np.uint8), np.full(16384, 51, dtype=np.uint8), rng.integers(0, 52, 16384).astype(np.uint8),
               (rng.random(16384) < 0.01).astype(np.uint8)]
    for reg in arrays:
        want, got = SR.hll_estimate(reg), capi.hll_estimate(reg)
        assert abs(got - want) <= 1e-9 * max(want, 1e-300), (want, got)
    assert capi.hll_estimate(np.zeros(16384, dtype=np.uint8)) == 0.0


# ------------------------------------------------------------------------------------------------ the plan
BIG_CAP = 1 << 40


def fill_power(n, q, L, r):
    return 6 * (-np.expm1(-q * (n / r) / 2.0 ** L)) ** q   # 1 - exp(-x), without the cancellation at small x


def test_plan_of_the_62_genome_workload(capi):
    p = capi.filter_plan(30_800_000, 5, POSITIONS_M2, BIG_CAP)
    assert p["L_fp"] == 30 and p["L"] == 32 and p["rounds"] == 1 and not p["clipped"]
    assert p["L_mem"] == 40


def test_model_against_the_recorded_false_marks(capi):
    """Predicted false marks x positions at L = 28 and L = 30 against the round-4 sweep's marks minus the real ones."""
    for L, recorded in ((28, 28559823), (30, 85598)):
        p = capi.filter_plan(30_800_000, 5, POSITIONS_M2, (1 << L) // 8, rounds=1)
        assert p["L"] == L and p["L_mem"] == L
        predicted = p["false_marks"] * POSITIONS_M2
        print("L", L, "predicted", predicted, "recorded", recorded)
        assert recorded / 1.25 <= predicted <= recorded * 1.25
        assert abs(p["false_marks"] - fill_power(30.8e6, 5, L, 1)) <= 1e-9 * p["false_marks"]


def test_plan_is_monotone(capi):
    """L never falls when the edges grow and never rises when the cap shrinks."""
    counts = [0, 1, 1000, 10 ** 5, 10 ** 6, 10 ** 7, 3 * 10 ** 7, 10 ** 8, 10 ** 9, 3 * 10 ** 9, 10 ** 10, 10 ** 11]
    caps = [1 << b for b in range(10, 41, 3)]
    for q in (1, 3, 5, 8):
        for cap in caps:
            Ls = [capi.filter_plan(n, q, 1 << 62, cap, rounds=1)["L"] for n in counts]
            assert Ls == sorted(Ls), (q, cap, Ls)
        for n in counts:
            Ls = [capi.filter_plan(n, q, 1 << 62, cap, rounds=1)["L"] for cap in caps]
            assert Ls == sorted(Ls), (q, n, Ls)   # non-increasing as the cap shrinks


def test_target_holds_whenever_the_plan_is_not_clipped(capi):
    seen_clipped = seen_rounds = 0
    for q in (1, 2, 3, 5, 8, 16):
        for n in (0, 10, 10 ** 4, 10 ** 6, 3 * 10 ** 7, 10 ** 9, 10 ** 10, 10 ** 12):
            for cap_bits in (13, 20, 28, 31, 34, 37, 40, 43):
                for rounds in (0, 1, 3):
                    p = capi.filter_plan(n, q, 1 << 62, (1 << cap_bits) // 8, rounds=rounds)
                    assert 1 <= p["rounds"] <= 64 and p["L"] <= min(cap_bits, 40)
                    if rounds:
                        assert p["rounds"] == rounds
                    value = fill_power(n, q, p["L"], p["rounds"])
                    assert abs(p["false_marks"] - value) <= 1e-9 * max(value, 1e-300)
                    assert p["clipped"] == (p["false_marks"] > 1e-3)
                    if not p["clipped"]:
                        assert value <= 1e-3
                    seen_clipped += p["clipped"]
                    seen_rounds += p["rounds"] > 1 and not rounds
    assert seen_clipped and seen_rounds


def test_memory_clip_turns_into_rounds(capi):
    p = capi.filter_plan(3_500_000_000, 5, 1 << 40, 2 << 30)
    assert p["L"] == p["L_mem"] == 34 and p["L_fp"] > 34 and 1 < p["rounds"] <= 64 and not p["clipped"]
    # the smallest such r
    assert fill_power(3.5e9, 5, 34, p["rounds"]) <= 1e-3 < fill_power(3.5e9, 5, 34, p["rounds"] - 1)
    # 64 rounds are not enough: clipped
    p = capi.filter_plan(10 ** 12, 5, 1 << 62, 2 << 30)
    assert p["rounds"] == 64 and p["clipped"]


def test_given_rounds_are_respected(capi):
    for r in (1, 2, 7, 64, 100):
        p = capi.filter_plan(3_500_000_000, 5, 1 << 40, 2 << 30, rounds=r)
        assert p["rounds"] == r and p["L"] == min(34, max(32, p["L_fp"])) and p["L_mem"] == 34
    # ... and enter the model: the same edges over four rounds need two bits less
    one, four = capi.filter_plan(30_800_000, 5, POSITIONS_M2, BIG_CAP, rounds=1), capi.filter_plan(30_800_000, 5, POSITIONS_M2, BIG_CAP, rounds=4)
    assert four["L_fp"] == one["L_fp"] - 2


def test_no_edges_give_the_floor_or_the_cap(capi):
    assert capi.filter_plan(0, 5, 1000, BIG_CAP)["L"] == 32
    assert capi.filter_plan(0, 5, 1000, 1 << 20)["L"] == 23
    assert capi.filter_plan(0, 5, 0, 0)["L"] == 3
    # an estimate beyond the text's length is clamped to it
    assert capi.filter_plan(10 ** 12, 5, 1000, BIG_CAP) == capi.filter_plan(1000, 5, 1000, BIG_CAP)


# ------------------------------------------------------------------------------------------------ the command line
def run(exe, args, cwd):
    return subprocess.run([exe] + args, cwd=cwd, capture_output=True, timeout=300)


@pytest.mark.parametrize("args,what", [
    (["-f", "auto", "--filtermemory", "4"], "Mutually exclusive argument already set! for arg (--filtersize|--filtermemory)"),
    (["--filtersize", "auto", "--filtermemory", "4"], "Mutually exclusive argument already set! for arg (--filtersize|--filtermemory)"),
    (["-f", "auto", "--gpus", "2"], "--gpus"),
    (["-f", "auto", "--load-filter", "x"], "--load-filter"),
    (["-f", "auto", "--test"], "--test"),
    (["-f", "autox"], "Couldn't read argument value from string 'autox' for arg (--filtersize)"),
    (["-f", "Auto"], "Couldn't read argument value from string 'Auto' for arg (--filtersize)"),
    (["-f", "auto", "-f"], "Missing a value for this argument! for arg (--filtersize)"),
])
def test_auto_flag_errors_need_no_device(twopaco, tmp_path, args, what):
    r = run(twopaco, ["-k", "11", os.path.join(GOLDEN, "example.fa")] + args, str(tmp_path))
    assert r.returncode == 1 and r.stdout == b""
    err = r.stderr.decode()
    assert err.startswith("\nError: ") and err.count("\n") == 2 and what in err
    if what.startswith("--"):
        assert err.endswith("for arg (--filtersize)\n")
    assert os.listdir(str(tmp_path)) == []


def test_help_names_auto(twopaco, tmp_path):
    r = run(twopaco, ["--help"], str(tmp_path))
    assert r.returncode == 0 and "-f <integer|auto>" in r.stdout.decode() and "-f auto:" in r.stdout.decode()


def test_auto_without_a_device_is_an_error_and_leaves_no_file(twopaco, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    r = run(twopaco, ["-k", "11", "-f", "auto", os.path.join(GOLDEN, "example.fa")], str(tmp_path))
    assert r.returncode == 1 and "Error: " in r.stderr.decode() and "GPU" in r.stderr.decode()
    assert os.listdir(str(tmp_path)) == []
