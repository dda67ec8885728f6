"""CPU: the host half of `twopaco --graph` (twopaco_amd/host/graphformat.h) on a machine without a device.

The formatter's only input is the EVENT TABLE (include/twopaco_hip.h, the tpc_segments_* group) and the letters of the FASTA
files.  Here the table is computed in Python from the golden junction streams by its definition, handed to
libtwopaco_host.so:tpch_graph_format, and the file it writes is compared with what the REAL reference graphdump printed
(tests/golden/graphdump.json).  The flags of the command line are checked as far as they go without a GPU."""
import hashlib
import json
import os
import subprocess

import pytest

from graph_table import event_table, read_fasta, vector_parts

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
FORMATS = ("gfa1", "gfa2", "fasta")
VECTORS = [v for v in json.load(open(os.path.join(GOLDEN, "graphdump.json"))) if v["case"] != "cli" and v["args"][2] in FORMATS and v["rc"] == 0]
CASES = sorted({v["case"] for v in VECTORS})


@pytest.fixture(scope="module")
def capi(built):
    from twopaco_amd import capi as m
    return m


@pytest.fixture(scope="module")
def twopaco(built):
    path = os.path.join(os.path.dirname(HERE), "twopaco_amd", "bin", "twopaco")
    assert os.path.exists(path)
    return path


@pytest.fixture()
def in_golden():
    """cwd = tests/golden with relative file names: UR:Z: carries the name as it was given."""
    before = os.getcwd()
    os.chdir(GOLDEN)
    yield
    os.chdir(before)


def test_the_vectors_are_all_there():
    assert len(VECTORS) == 95 and len(CASES) == 19
    assert {(v["case"], v["args"][2], "--prefix" in v["args"]) for v in VECTORS} >= {(c, f, False) for c in CASES for f in FORMATS}


@pytest.mark.parametrize("case", CASES)
def test_formatter_writes_the_reference_bytes_from_the_table(capi, tmp_path, in_golden, case):
    """Every gfa1 / gfa2 / fasta vector of the real reference that exits 0 (95 over the 19 cases, with and without
    --prefix), at 1, 3 and 16 threads: size and sha256 of the file tpch_graph_format writes."""
    mine = [v for v in VECTORS if v["case"] == case]
    assert mine
    tables = {}
    for v in mine:
        bin_name, fmt, k, files, prefix = vector_parts(v)
        key = (bin_name, k, tuple(files))
        if key not in tables:
            seqs = [s for f in files for s in read_fasta(f)]
            tables[key] = event_table(open(bin_name, "rb").read(), seqs, k)
        name, first, begin, end, seq_event_begin = tables[key]
        for threads in (1, 3, 16):
            out = str(tmp_path / "graph.txt")
            capi.graph_format(files, k, fmt, out, name, first, begin, end, seq_event_begin, prefix=prefix, threads=threads)
            got = open(out, "rb").read()
            assert len(got) == v["stdout_bytes"], (v["args"], threads)
            assert hashlib.sha256(got).hexdigest() == v["stdout_sha256"], (v["args"], threads)
            os.unlink(out)


def test_formatter_refuses_a_table_that_does_not_fit_the_sequences(capi, tmp_path, in_golden):
    """What the formatter indexes with is checked first: an error text and no file, never a fault."""
    v = [v for v in VECTORS if v["case"] == "example_k11" and v["args"][2] == "gfa1" and "--prefix" not in v["args"]][0]
    bin_name, fmt, k, files, prefix = vector_parts(v)
    name, first, begin, end, seq_event_begin = event_table(open(bin_name, "rb").read(), [s for f in files for s in read_fasta(f)], k)
    out = str(tmp_path / "graph.txt")
    past = end.copy()
    past[-1] = 0xFFFFFFF0
    back = begin.copy()
    back[0] = end[0]
    short = seq_event_begin.copy()
    short[-1] -= 1
    down = seq_event_begin.copy()
    down[1] = len(name) + 1
    for args, what in [((name, first, begin, past, seq_event_begin), "inside its sequence"), ((name, first, back, end, seq_event_begin), "inside its sequence"),
                       ((name, first, begin, end, short), "cover"), ((name, first, begin, end, down), "ascend|cover"),
                       ((name, first, begin, end, seq_event_begin[:-1]), "sequences")]:
        with pytest.raises(RuntimeError, match=what):
            capi.graph_format(files, k, fmt, out, *args)
        assert not os.path.exists(out)
    with pytest.raises(RuntimeError, match="gfa1, gfa2, fasta"):
        capi.graph_format(files, k, "dot", out, name, first, begin, end, seq_event_begin)
    with pytest.raises(RuntimeError):
        capi.graph_format(["no_such_file.fa"], k, fmt, out, name, first, begin, end, seq_event_begin)
    assert not os.path.exists(out)


# ------------------------------------------------------------------------------------------------ the command line
def run(exe, args, cwd):
    return subprocess.run([exe] + args, cwd=cwd, capture_output=True, timeout=300)


def test_help_lists_the_graph_flags(twopaco, tmp_path):
    r = run(twopaco, ["--help"], str(tmp_path))
    assert r.returncode == 0
    for flag in ("--graph <gfa1|gfa2|fasta>", "--graph-out", "--graph-prefix", "--graph-threads"):
        assert flag in r.stdout.decode(), flag


def test_graphdump_help_names_the_one_process_way(built, tmp_path):
    exe = os.path.join(os.path.dirname(HERE), "twopaco_amd", "bin", "graphdump")
    r = run(exe, ["--help"], str(tmp_path))
    assert r.returncode == 0 and "twopaco --graph" in r.stdout.decode()


@pytest.mark.parametrize("args,arg,what", [
    (["--graph", "xml"], "(--graph)", "Value 'xml' does not meet constraint: gfa1|gfa2|fasta"),
    (["--graph"], "(--graph)", "Missing a value for this argument!"),
    (["--graph", "gfa1", "--graph-threads", "0"], "(--graph-threads)", "Couldn't read argument value from string '0'"),
    (["--graph", "gfa1", "--graph-threads", "x"], "(--graph-threads)", "Couldn't read argument value from string 'x'"),
    (["--graph", "gfa1", "--graph-threads", "-2"], "(--graph-threads)", "Couldn't read argument value from string '-2'"),
    (["--graph", "gfa1", "--graph-threads", "3x"], "(--graph-threads)", "Couldn't read argument value from string '3x'"),
    (["--graph", "gfa1", "--graph-threads", ""], "(--graph-threads)", "Couldn't read argument value from string ''"),
    (["--graph", "gfa1", "--graph-threads"], "(--graph-threads)", "Missing a value for this argument!"),
])
def test_bad_graph_flags_are_parse_errors(twopaco, tmp_path, args, arg, what):
    r = run(twopaco, ["-k", "11", "-f", "20", os.path.join(GOLDEN, "example.fa")] + args, str(tmp_path))
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode() == "\nError: %s for arg %s\n" % (what, arg)
    assert os.listdir(str(tmp_path)) == []


def test_graph_over_several_gpus_is_refused_at_parsing(twopaco, tmp_path):
    r = run(twopaco, ["-k", "11", "-f", "20", "--graph", "gfa1", "--gpus", "2", os.path.join(GOLDEN, "example.fa")], str(tmp_path))
    assert r.returncode == 1 and r.stdout == b""
    err = r.stderr.decode()
    assert err.startswith("\nError: ") and err.count("\n") == 2 and "one GPU" in err and err.endswith("for arg (--graph)\n")
    assert os.listdir(str(tmp_path)) == []


def test_graph_without_a_device_is_an_error_and_leaves_no_file(twopaco, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    for extra in ([], ["-o", "junctions.bin"]):
        r = run(twopaco, ["-k", "11", "-f", "20", "--graph", "gfa1", os.path.join(GOLDEN, "example.fa")] + extra, str(tmp_path))
        assert r.returncode == 1
        assert "Error: " in r.stderr.decode() and "GPU" in r.stderr.decode()
        assert os.listdir(str(tmp_path)) == []
