"""CPU: what `graphdump --gpu` must keep true on a machine without a device (twopaco_amd/host/junctiondump.cpp): the binary
links no device library (libtwopaco_hip.so is loaded with dlopen only when the flag is given), the flag without a device is
an error and never a fallback, and the new flags parse like the old ones."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
GFA1 = ["example_k11.bin", "-f", "gfa1", "-k", "11", "-s", "example.fa"]


@pytest.fixture(scope="module")
def exe(built):
    path = os.path.join(os.path.dirname(HERE), "twopaco_amd", "bin", "graphdump")
    assert os.path.exists(path)
    return path


def run(exe, args):
    return subprocess.run([exe] + args, cwd=GOLDEN, capture_output=True, timeout=300)


def test_no_link_time_dependency_on_the_device_library(exe):
    needed = subprocess.run(["readelf", "-d", exe], capture_output=True, timeout=60, check=True).stdout.decode()
    libs = [line for line in needed.splitlines() if "NEEDED" in line]
    assert libs, needed
    for line in libs:
        assert "twopaco" not in line and "amdhip" not in line and "hsa" not in line, line


def test_help_lists_the_new_flags(exe):
    r = run(exe, ["--help"])
    assert r.returncode == 0
    text = r.stdout.decode()
    assert "--gpu" in text and "--threads" in text


def test_gpu_flag_without_a_device_is_an_error(exe):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    for fmt in ("gfa1", "gfa2", "fasta"):
        r = run(exe, ["example_k11.bin", "-f", fmt, "-k", "11", "-s", "example.fa", "--gpu"])
        assert r.returncode == 1 and r.stdout == b"", (fmt, r.stdout[:80])
        err = r.stderr.decode()
        assert err.startswith("error: ") and err.count("\n") == 1, err


def test_gpu_flag_is_ignored_by_the_formats_without_segments(exe):
    """seq / group / dot have nothing for the device to do: --gpu is accepted and the host path runs, with or without a device."""
    for fmt in ("seq", "group", "dot"):
        a = run(exe, ["example_k11.bin", "-f", fmt, "-k", "11", "-s", "example.fa"])
        b = run(exe, ["example_k11.bin", "-f", fmt, "-k", "11", "-s", "example.fa", "--gpu", "--threads", "3"])
        assert a.returncode == b.returncode == 0 and a.stdout == b.stdout and b.stderr == b""


@pytest.mark.parametrize("value", ["0", "x", "-2", "3x", ""])
def test_bad_thread_counts_are_parse_errors(exe, value):
    r = run(exe, GFA1 + ["--threads", value])
    assert r.returncode == 1 and r.stdout == b""
    lines = r.stderr.decode().split("\n")
    assert lines[0] == "PARSE ERROR: (--threads)"
    assert lines[1].strip() == "Couldn't read argument value from string '%s'" % value


def test_threads_without_a_value_is_a_parse_error(exe):
    r = run(exe, GFA1 + ["--threads"])
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode().split("\n")[:2] == ["PARSE ERROR: (--threads)", "             Missing a value for this argument!"]


def test_threads_alone_changes_nothing(exe):
    """Without --gpu the serial walk runs whatever --threads says."""
    a, b = run(exe, GFA1), run(exe, GFA1 + ["--threads", "7"])
    assert a.returncode == b.returncode == 0 and a.stdout == b.stdout
