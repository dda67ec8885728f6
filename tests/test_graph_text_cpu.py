"""CPU: what `twopaco --graph-text` and `graphdump --text` must keep true on a machine without a device
(twopaco_amd/host/constructor.cpp, junctiondump.cpp): the flags parse, their bad values are parse errors in the wording of the
other flags, the device formatter without a device is an error and never a fallback, the default is the host formatter, and
graphdump still links no device library (the two new calls are resolved with dlsym like the rest)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
GFA1 = ["example_k11.bin", "-f", "gfa1", "-k", "11", "-s", "example.fa"]
TWOPACO = ["-k", "11", "-f", "20", os.path.join(GOLDEN, "example.fa")]


@pytest.fixture(scope="module")
def graphdump(built):
    path = os.path.join(ROOT, "twopaco_amd", "bin", "graphdump")
    assert os.path.exists(path)
    return path


@pytest.fixture(scope="module")
def twopaco(built):
    path = os.path.join(ROOT, "twopaco_amd", "bin", "twopaco")
    assert os.path.exists(path)
    return path


def run(exe, args, cwd=GOLDEN):
    return subprocess.run([exe] + args, cwd=str(cwd), capture_output=True, timeout=300)


# ------------------------------------------------------------------------------------------------ graphdump --text
def test_graphdump_help_lists_the_text_flag(graphdump):
    r = run(graphdump, ["--help"])
    assert r.returncode == 0
    assert "--text <host|device>" in r.stdout.decode()


def test_graphdump_text_host_is_the_default_and_changes_nothing(graphdump):
    """`--text host` is accepted with and without --gpu (without it the serial walk runs, as ever)."""
    a, b = run(graphdump, GFA1), run(graphdump, GFA1 + ["--text", "host"])
    assert a.returncode == b.returncode == 0 and a.stdout == b.stdout and b.stderr == b""


def test_graphdump_text_device_without_gpu_is_a_parse_error(graphdump):
    for args in (GFA1 + ["--text", "device"], ["--text", "device"] + GFA1):
        r = run(graphdump, args)
        assert r.returncode == 1 and r.stdout == b""
        lines = r.stderr.decode().split("\n")
        assert lines[0] == "PARSE ERROR: Argument: (--text)", lines[:2]
        assert lines[1].strip().startswith("Value 'device' does not meet constraint:") and "--gpu" in lines[1]
        assert "Brief USAGE" in r.stderr.decode()


@pytest.mark.parametrize("value", ["xml", "", "Device", "gpu"])
def test_graphdump_bad_text_values_are_parse_errors(graphdump, value):
    for extra in ([], ["--gpu"]):
        r = run(graphdump, GFA1 + extra + ["--text", value])
        assert r.returncode == 1 and r.stdout == b""
        lines = r.stderr.decode().split("\n")
        assert lines[0] == "PARSE ERROR: Argument: (--text)"
        assert lines[1].strip() == "Value '%s' does not meet constraint: host|device" % value


def test_graphdump_text_without_a_value_is_a_parse_error(graphdump):
    r = run(graphdump, GFA1 + ["--gpu", "--text"])
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode().split("\n")[:2] == ["PARSE ERROR: (--text)", "             Missing a value for this argument!"]


def test_graphdump_text_device_without_a_device_is_an_error(graphdump):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    for fmt in ("gfa1", "gfa2", "fasta"):
        r = run(graphdump, ["example_k11.bin", "-f", fmt, "-k", "11", "-s", "example.fa", "--gpu", "--text", "device"])
        assert r.returncode == 1 and r.stdout == b"", (fmt, r.stdout[:80])
        err = r.stderr.decode()
        assert err.startswith("error: ") and err.count("\n") == 1, err


def test_graphdump_text_device_is_ignored_by_the_formats_without_segments(graphdump):
    for fmt in ("seq", "group", "dot"):
        a = run(graphdump, ["example_k11.bin", "-f", fmt, "-k", "11", "-s", "example.fa"])
        b = run(graphdump, ["example_k11.bin", "-f", fmt, "-k", "11", "-s", "example.fa", "--gpu", "--text", "device"])
        assert a.returncode == b.returncode == 0 and a.stdout == b.stdout and b.stderr == b""


def test_graphdump_still_links_no_device_library(graphdump):
    needed = subprocess.run(["readelf", "-d", graphdump], capture_output=True, timeout=60, check=True).stdout.decode()
    libs = [line for line in needed.splitlines() if "NEEDED" in line]
    assert libs, needed
    for line in libs:
        assert "twopaco" not in line and "amdhip" not in line and "hsa" not in line, line
    # ... and does not import the new entry points either: they are names in its data, looked up at run time
    undefined = subprocess.run(["nm", "-D", "--undefined-only", graphdump], capture_output=True, timeout=60, check=True).stdout.decode()
    assert "tpc_" not in undefined, undefined
    assert b"tpc_segments_text_plan" in open(graphdump, "rb").read() and b"tpc_segments_text_write" in open(graphdump, "rb").read()


def test_the_device_library_exports_the_text_calls(built):
    lib = os.path.join(ROOT, "twopaco_amd", "lib", "libtwopaco_hip.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, timeout=60, check=True).stdout.decode()
    for name in ("tpc_segments_text_plan", "tpc_segments_text_fetch", "tpc_segments_text_write"):
        assert " T " + name + "\n" in exported, name


def test_capi_has_the_text_wrappers(built):
    from twopaco_amd import capi
    for name in ("segments_text_plan", "segments_text_fetch", "segments_text_write"):
        assert callable(getattr(capi.Context, name))
    assert capi.KERNELS["segtext"] == 16 and capi.TEXT_FORMATS == {"gfa1": 1, "gfa2": 2, "fasta": 3}


# ------------------------------------------------------------------------------------------------ twopaco --graph-text
def test_twopaco_help_lists_the_graph_text_flag(twopaco, tmp_path):
    r = run(twopaco, ["--help"], tmp_path)
    assert r.returncode == 0 and "--graph-text <host|device>" in r.stdout.decode()


@pytest.mark.parametrize("args,arg,what", [
    (["--graph", "gfa1", "--graph-text", "xml"], "(--graph-text)", "Value 'xml' does not meet constraint: host|device"),
    (["--graph", "gfa1", "--graph-text", ""], "(--graph-text)", "Value '' does not meet constraint: host|device"),
    (["--graph", "gfa1", "--graph-text"], "(--graph-text)", "Missing a value for this argument!"),
    (["--graph-text", "device"], "(--graph-text)", "This argument needs --graph <gfa1|gfa2|fasta>"),
    (["--graph-text", "host"], "(--graph-text)", "This argument needs --graph <gfa1|gfa2|fasta>"),
])
def test_twopaco_bad_graph_text_flags_are_parse_errors(twopaco, tmp_path, args, arg, what):
    r = run(twopaco, TWOPACO + args, tmp_path)
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode() == "\nError: %s for arg %s\n" % (what, arg)
    assert os.listdir(str(tmp_path)) == []


def test_twopaco_graph_text_over_several_gpus_is_refused_at_parsing(twopaco, tmp_path):
    r = run(twopaco, TWOPACO + ["--graph", "gfa1", "--graph-text", "device", "--gpus", "2"], tmp_path)
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().endswith("for arg (--graph)\n")
    assert os.listdir(str(tmp_path)) == []


def test_twopaco_graph_text_without_a_device_is_one_error_line_and_no_file(twopaco, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    for text in ("device", "host"):
        for extra in ([], ["--graph-threads", "3"], ["-o", "junctions.bin"]):   # --graph-threads is unused by `device`, and accepted
            r = run(twopaco, TWOPACO + ["--graph", "gfa1", "--graph-text", text] + extra, tmp_path)
            assert r.returncode == 1
            err = r.stderr.decode()
            assert len([line for line in err.split("\n") if line]) == 1, err
            assert err.lower().count("error:") == 1 and err.startswith("\nError: ") and "GPU" in err, err
            assert os.listdir(str(tmp_path)) == []
