"""CPU: every command line about graph tables that `graphdump` and `twopaco` refuse while parsing, replayed against
tests/golden/cli_refusals.json (recorded by tools/record_cli_refusals.py, the command lines grouped by what they were told): the
exit status and every byte of stderr, which pins the wording of each complaint and which one comes first when several apply.  graphdump runs without --gpu and twopaco's parse
errors precede any use of a device."""
import json
import os
import shlex
import subprocess

import pytest

from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAMS = {name: os.path.join(ROOT, "twopaco_amd", "bin", name) for name in ("graphdump", "twopaco")}
FA = os.path.join(GOLDEN, "rand6.fa")
RECORDING = json.load(open(os.path.join(GOLDEN, "cli_refusals.json")))


def test_the_recording_covers_both_programs():
    for program in PROGRAMS:
        lines = [a for e in RECORDING[program]["refusals"] for a in e["argv"]]
        assert len(lines) > 600 and len(set(lines)) == len(lines)
        assert all(e["status"] != 0 and e["stderr"] and e["argv"] for e in RECORDING[program]["refusals"])


@pytest.mark.parametrize("program", sorted(PROGRAMS))
def test_every_refusal_is_replayed_exactly(program, tmp_path):
    exe, rec = PROGRAMS[program], RECORDING[program]
    assert os.path.exists(exe), "run build() first"
    cwd = GOLDEN if program == "graphdump" else str(tmp_path)
    before = sorted(os.listdir(cwd))
    wrong = []
    for e in rec["refusals"]:
        want = e["stderr"].replace("{usage}", rec["usage"]).replace("{argv0}", exe).replace("{fa}", FA)
        for line in e["argv"]:
            argv = rec["base"] + [a.replace("{fa}", FA) for a in shlex.split(line)] + ([FA] if program == "twopaco" else [])
            r = subprocess.run([exe] + argv, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
            if (r.returncode, r.stderr.decode(), r.stdout) != (e["status"], want, b""):
                wrong.append((line, r.returncode, r.stderr.decode(), want))
    assert not wrong, "%d of them, the first: %r" % (len(wrong), wrong[0])
    assert sorted(os.listdir(cwd)) == before
