#!/usr/bin/env python3
"""
Capture golden vectors of `zot hgvs-gen` from the reference's hgvs-gen (drtconway/zotmer at /root/reference).

Runs ONLY in the development container, by the recipe of tests/golden/make_golden_spikein.py: the reference's own
commands/hgvs-gen.py, with the library modules it imports, is copied to a throw-away directory under /tmp and passed through
the stdlib's lib2to3; docopt is stubbed (the options the reference's docopt would give are made from the case's option words
and the defaults of the usage text), and so is tqdm; openFile becomes a text-mode (gzip) open.  The reference finds a
chromosome's file through its table of the 24 hg19 accessions; the table is replaced by one that names the toy chromosomes of
tests/_spikein_cases.py, which the command reads as chr*.fa.gz from its working directory (-g .).  Nothing of the logic is
touched.

What is committed is data only: tests/golden/g1_hgvsgen.json holds, per case, the option words, the BED text and the lines the
reference printed with -T -V -- or, for the two cases with a mean of exactly 1, the error its geomvar raises there (log1p(-1);
the cases next to them, with means of 1.001, are the nearest it runs).  The reference's random numbers are Python's: the lines
are data for the renderer -- every line, parsed back into a row, must be spelled again exactly so --, not something this
project reproduces.

Usage:  python3 tests/golden/make_golden_hgvsgen.py        (rewrites tests/golden/g1_hgvsgen.json)
"""
import contextlib
import importlib
import io
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
WORK = "/tmp/zot3_hgvsgen"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests._hgvsgen_cases import GOLDEN_CASES  # noqa: E402
from tests._spikein_cases import GENOME, write_genome  # noqa: E402

DEFAULTS = {"-D": "1.5", "-I": "1.5", "-U": "3.0", "-g": None, "-N": "1", "-S": None, "-t": "sub,del,ins,delins,dup", "-T": False,
            "-v": False, "-V": False}


def build_derived():
    shutil.rmtree(WORK, ignore_errors=True)
    os.makedirs(WORK + "/stubs")
    shutil.copytree(REF + "/zotmer", WORK + "/zotmer")
    subprocess.check_call(["chmod", "-R", "u+w", WORK])
    mods = ("file", "misc", "hgvs", "rope", "align", "basics", "bits")
    files = [WORK + "/zotmer/library/%s.py" % m for m in mods] + [WORK + "/zotmer/commands/hgvs-gen.py"]
    subprocess.check_call([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n"] + files,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    shutil.copy(WORK + "/zotmer/commands/hgvs-gen.py", WORK + "/zotmer/commands/hgvs_gen.py")      # a name import can spell
    with open(WORK + "/stubs/docopt.py", "w") as f:
        f.write("_next = {}\n\ndef docopt(doc, argv=None, **kw):\n    return dict(_next)\n")
    with open(WORK + "/stubs/tqdm.py", "w") as f:
        f.write("def tqdm(*a, **kw):\n    raise RuntimeError('not used without -v')\n")
    sys.path.insert(0, WORK + "/stubs")
    sys.path.insert(0, WORK)


def open_text(fn, mode="r"):
    import gzip
    if fn.endswith(".gz"):
        return gzip.open(fn, mode + "t", encoding="latin-1")
    return open(fn, mode)


def run_case(case, d):
    import docopt
    hgvs = importlib.import_module("zotmer.library.hgvs")
    hgvs.refSeq2Hg19 = {name: name for name in GENOME}
    hgvs.hg19ToRefSeq = {}
    mod = importlib.import_module("zotmer.commands.hgvs_gen")
    mod.openFile = open_text
    opts = dict(DEFAULTS)
    words = list(case["opts"]) + ["-T", "-V"]
    while words:
        o = words.pop(0)
        opts[o] = words.pop(0) if not isinstance(DEFAULTS[o], bool) else True
    with open(d + "/zones.bed", "w") as f:
        f.write(case["bed"])
    opts["<regions>"] = "zones.bed"
    docopt._next = opts
    cwd = os.getcwd()
    os.chdir(d)
    out = io.StringIO()
    error = None
    try:
        with contextlib.redirect_stdout(out):
            mod.main([])
    except ValueError as e:                         # a mean of exactly 1: math.log1p(-1.0) in the reference's geomvar
        error = "%s: %s" % (type(e).__name__, e)
    finally:
        os.chdir(cwd)
    lines = out.getvalue().split("\n")
    assert lines[-1] == ""
    return {"name": case["name"], "opts": case["opts"], "bed": case["bed"], "lines": [] if error else lines[:-1], "error": error}


def main():
    build_derived()
    d = WORK + "/genome"
    write_genome(d)
    res = []
    for case in GOLDEN_CASES:
        r = run_case(case, d)
        res.append(r)
        print(case["name"], case["opts"], len(r["lines"]), "lines")
    with open(os.path.join(HERE, "g1_hgvsgen.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in res) + "\n]\n")


if __name__ == "__main__":
    main()
