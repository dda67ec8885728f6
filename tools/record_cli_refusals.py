#!/usr/bin/env python3
"""Record what `graphdump` and `twopaco` say to the command lines about graph tables that they refuse while parsing.

    python tools/record_cli_refusals.py [--out tests/golden/cli_refusals.json]

Writes, per program, its base arguments, the text that ends every one of its parse errors ("usage"), and the refusals grouped by
what was said: {"status", "stderr", "argv": [the options of every command line that was told so, as one shell-quoted string each]}.
tests/test_cli_refusals_cpu.py replays every command line against the built programs and compares status and stderr exactly.
Only lines that are refused before anything is read or any device is opened are generated: every one must end nonzero with the
program's parse-error text, or nothing is written.  Placeholders: {argv0} for the program's own path where it prints it, {fa} for
the one FASTA file `twopaco` is given (tests/golden/rand6.fa), {usage} for the program's constant last lines.  graphdump runs in
tests/golden with relative names, twopaco in an empty directory that must stay empty.
"""
import argparse
import itertools
import json
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PROGRAMS = {name: os.path.join(ROOT, "twopaco_amd", "bin", name) for name in ("graphdump", "twopaco")}
FA = os.path.join(GOLDEN, "rand6.fa")

# the tables that take file|sequence, in the order both programs write them; --links takes no value
BY = ["colors", "bubbles", "distances", "components", "superbubbles", "anchors", "locate"]
SECOND = {"distances": "--distances-phylip", "components": "--components-members", "superbubbles": "--superbubbles-members",
          "anchors": "--anchors-paf", "locate": "--locate-walks"}
# every option that is nothing without its table, with a value that is fine in itself
ORPHANS = {"colors": [["--colors-out", "x.tsv"]], "links": [["--links-out", "x.tsv"]], "bubbles": [["--bubbles-out", "x.tsv"]],
           "distances": [["--distances-out", "x.tsv"], ["--distances-phylip", "x.phy"]],
           "components": [["--components-out", "x.tsv"], ["--components-members", "m.tsv"]],
           "superbubbles": [["--superbubbles-out", "x.tsv"], ["--superbubbles-members", "m.tsv"], ["--superbubbles-max", "5"]],
           "anchors": [["--anchors-out", "x.tsv"], ["--anchors-paf", "x.paf"], ["--anchors-ref", "0"]],
           "locate": [["--locate-out", "x.tsv"], ["--locate-walks", "w.tsv"], ["--locate-in", "rand6.fa"]]}
BASE = {"graphdump": ["rand6_k3.bin", "-k", "3", "-s", "rand6.fa"], "twopaco": ["-f", "20"]}


def table(name, by):
    """The options that turn one table on."""
    if name == "links":
        return ["--links"]
    return ["--" + name, by] + (["--locate-in", "{fa}"] if name == "locate" else [])


def both_orders(groups):
    yield [a for g in groups for a in g]
    if len(groups) > 1:
        yield [a for g in reversed(groups) for a in g]


def table_lines(program):
    """The option part of every command line, without the program's base arguments."""
    graphdump = program == "graphdump"
    # 1. pairs and triples of the file|sequence tables whose modes are not all equal, in both argument orders
    for n in (2, 3):
        for names in itertools.combinations(BY, n):
            for modes in itertools.product(("file", "sequence"), repeat=n):
                if len(set(modes)) > 1:
                    yield from both_orders([table(t, by) for t, by in zip(names, modes)])
    # 2. graphdump: every table with what it is not written beside (twopaco writes all of these together)
    if graphdump:
        for name in ["links"] + BY:
            for other in (["--links"], ["--compact"], ["--text", "host"], ["--text", "device"], ["-f", "gfa1"], ["-f", "gfa1", "--compact"]):
                if name == "links" and other == ["--links"]:
                    continue
                yield from both_orders([table(name, "file"), other])
        yield from both_orders([table("colors", "file"), table("bubbles", "file")])
        yield ["--compact"]
        yield ["-f", "gfa2", "--compact"]
        yield ["-f", "gfa1", "--compact", "--gpu", "--text", "device"]
        yield ["-f", "gfa1", "--text", "device"]
    # 3. every option of a table without its table: alone, the table's together, beside another table, and all of them at once
    for name, options in ORPHANS.items():
        for o in options:
            yield list(o)
            yield table("colors" if name != "colors" else "distances", "file") + list(o)
        yield from both_orders([list(o) for o in options])
    yield [a for options in ORPHANS.values() for o in options for a in o]
    yield [a for options in reversed(list(ORPHANS.values())) for o in reversed(options) for a in o]
    # 4. empty file names
    for name, option in SECOND.items():
        yield table(name, "sequence") + [option, ""]
        yield [option, ""] + table(name, "file")
        yield [option, ""]
    if not graphdump:   # (graphdump's tables go to the standard output without a name, and so does twopaco's colour table)
        for name in ["links"] + BY[1:]:
            yield table(name, "file") + ["--%s-out" % name, ""]
            if name in SECOND:
                yield table(name, "file") + ["--%s-out" % name, "", SECOND[name], ""]
    # 5. values that do not meet their constraint, and missing ones
    for name in BY:
        for bad in ("both", "", "File"):
            yield ["--" + name, bad]
            yield table("links", "") + ["--" + name, bad]
        yield ["--" + name]
    for bad in ("1", "63", "0", "-2", "x", "", "62x"):
        yield table("superbubbles", "file") + ["--superbubbles-max", bad]
        yield ["--superbubbles-max", bad]
    for bad in ("-1", "x", "", "2147483648", "1x"):
        yield table("anchors", "file") + ["--anchors-ref", bad]
        yield ["--anchors-ref", bad]
    yield table("anchors", "file") + ["--anchors-ref", "1"]            # one input file: colour 1 does not exist
    if graphdump:   # (twopaco knows the sequences only after it read them, on the device's side of the parse)
        yield table("anchors", "sequence") + ["--anchors-ref", "1000"]
    for option in [o[0] for options in ORPHANS.values() for o in options]:
        yield [option]
    yield ["--locate", "file"]
    yield ["--locate", "file", "--locate-out", "x.tsv", "--locate-walks", ""]
    yield ["--colors", "sequence", "--locate", "file"]
    # 6. twopaco: every table on more than one GPU
    if not graphdump:
        for name in ["links"] + BY:
            yield from both_orders([table(name, "file"), ["--gpus", "2"]])
        yield [a for name in ["links"] + BY for a in table(name, "file")] + ["--gpus", "2"]
        yield ["--gpus", "2"] + [a for name in reversed(["links"] + BY) for a in table(name, "sequence")]
        yield ["--gpus", "2", "--colors", "file", "--bubbles", "sequence"]
        yield ["--gpus", "2", "--bubbles-out", "x.tsv"]
    # 7. several complaints at once: which one comes first
    yield table("colors", "file") + table("bubbles", "sequence") + ["--distances-out", "x", "--components-members", ""]
    yield table("locate", "file") + table("anchors", "sequence") + ["--superbubbles-max", "5", "--colors-out", "x"]
    yield table("distances", "file") + ["--distances-phylip", "", "--components-out", "x", "--links-out", "y"]
    yield table("superbubbles", "file") + table("components", "sequence") + ["--superbubbles-members", "", "--anchors-paf", ""]
    if graphdump:
        yield table("locate", "file") + table("colors", "sequence") + ["--links", "--compact", "--text", "host", "-f", "gfa1"]
        yield table("anchors", "file") + ["--links", "--compact", "--text", "host", "-f", "gfa1", "--bubbles-out", "x"]
        yield table("bubbles", "file") + table("colors", "file") + ["--links", "--text", "host"]
        yield table("components", "file") + ["--text", "host", "--components-members", "", "--locate-in", "q.fa"]
        yield ["--links", "--colors", "file", "--text", "device", "--colors-out", "x"]


def command_lines(program):
    """The options of every command line, each once."""
    seen = set()
    for options in table_lines(program):
        if program == "graphdump":
            options = [a.replace("{fa}", "rand6.fa") for a in options]
        if tuple(options) not in seen:
            seen.add(tuple(options))
            yield options


def full_argv(program, options):
    return BASE[program] + [a.replace("{fa}", FA) for a in options] + ([FA] if program == "twopaco" else [])


USAGE = {"graphdump": "\n\nBrief USAGE: \n   {argv0}  [-k <integer>] [-s <string>] ... -f <seq|group|dot|gfa1|gfa2|fasta> [--prefix] [--] [--version] [-h] <file name>\n\n"
                      "For complete USAGE and HELP type: \n   {argv0} --help\n\n", "twopaco": ""}
REFUSED = {"graphdump": re.compile(r"\A(PARSE ERROR: |error: )"), "twopaco": re.compile(r"\A\nError: .* for arg \(.*\)\n\Z", re.S)}


def run(program, options, cwd):
    """(status, stderr with the placeholders) of one command line; stdout must stay empty."""
    exe = PROGRAMS[program]
    r = subprocess.run([exe] + full_argv(program, options), cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    stderr = r.stderr.decode().replace(exe, "{argv0}").replace(FA, "{fa}")
    if USAGE[program] and stderr.endswith(USAGE[program]):
        stderr = stderr[:-len(USAGE[program])] + "{usage}"
    if r.returncode == 0 or not REFUSED[program].search(stderr) or r.stdout:
        raise SystemExit("not refused at parsing: %s %r -> %d %r" % (program, options, r.returncode, stderr[:300]))
    return r.returncode, stderr


def record():
    recording = {}
    with tempfile.TemporaryDirectory() as empty:
        for program in ("graphdump", "twopaco"):
            cwd = GOLDEN if program == "graphdump" else empty
            before = sorted(os.listdir(cwd))
            said = {}   # (status, stderr) -> the command lines, in the order they were generated
            for options in command_lines(program):
                said.setdefault(run(program, options, cwd), []).append(shlex.join(options))
            if sorted(os.listdir(cwd)) != before:
                raise SystemExit("%s left files behind in %s" % (program, cwd))
            recording[program] = {"base": BASE[program], "usage": USAGE[program],
                                  "refusals": [{"status": k[0], "stderr": k[1], "argv": v} for k, v in said.items()]}
    return recording


def dump(recording):
    out = ["{"]
    for program, r in recording.items():
        out.append('%s: {"base": %s, "usage": %s, "refusals": [' % (json.dumps(program), json.dumps(r["base"]), json.dumps(r["usage"])))
        out.append(",\n".join(json.dumps(e, sort_keys=True) for e in r["refusals"]))
        out.append("]}" + ("," if program != list(recording)[-1] else ""))
    return "\n".join(out + ["}"]) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(GOLDEN, "cli_refusals.json"))
    args = ap.parse_args()
    recording = record()
    with open(args.out, "w") as f:
        f.write(dump(recording))
    print(", ".join("%s: %d command lines, %d texts" % (p, sum(len(e["argv"]) for e in r["refusals"]), len(r["refusals"])) for p, r in recording.items()), "->", args.out)


if __name__ == "__main__":
    sys.exit(main())
