#!/usr/bin/env python3
"""
Capture golden vectors of `zot hgvs-index` from the indexing mode of the reference's hgvs-find (drtconway/zotmer at
/root/reference): `hgvs-find -X` and `hgvs-find -X -T`.

Runs ONLY in the development container, by the recipe of tests/golden/make_golden_hgvsfind.py: the reference's own
commands/hgvs-find.py, with the library modules it imports, is copied to a throw-away directory under /tmp and passed
through the stdlib's lib2to3; docopt is stubbed (the options the reference's docopt would give are made from the case's
option words and the defaults of the usage text).  In addition the derived module's openFile is replaced by a text-mode
gzip open: under Python 3 the reference's `gunzip -c` pipe yields bytes, which its readFasta cannot strip and compare.  The
command is driven in-process from a directory that holds the toy genome of tests/_hgvsindex_cases.py as chr*.fa.gz (-g .),
with the case's -f file as 'variants.txt'.  The reference needs no -n: it maps NC_000007.13 to chr7 by its own table.

What is committed is data only: tests/golden/x1_hgvsindex.json holds, per case, the option words, the text of the index
file -X wrote and the stdout of -X -T.  The chromosomes are not committed.

Usage:  python3 tests/golden/make_golden_hgvsindex.py        (rewrites tests/golden/x1_hgvsindex.json)
"""
import contextlib
import gzip
import importlib
import io
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
WORK = "/tmp/zot3_hgvsindex"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests._hgvsindex_cases import make_cases, write_genome  # noqa: E402

DEFAULTS = {"-X": False, "-T": False, "-A": "0.001", "-B": "none", "-C": "10", "-c": None, "-D": "2", "-f": None, "-F": "rds,vaf",
            "-k": "25", "-g": None, "-o": None, "-s": False, "-v": False, "-V": "0.05", "-w": "75", "-W": "1024", "<input>": []}


def build_derived():
    shutil.rmtree(WORK, ignore_errors=True)
    os.makedirs(WORK + "/stubs")
    shutil.copytree(REF + "/zotmer", WORK + "/zotmer")
    subprocess.check_call(["chmod", "-R", "u+w", WORK])
    mods = ("basics", "bits", "file", "misc", "stats", "capture", "debruijn", "hgvs", "rope", "align", "reads")
    files = [WORK + "/zotmer/library/%s.py" % m for m in mods] + [WORK + "/zotmer/commands/hgvs-find.py"]
    subprocess.check_call([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n"] + files,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(WORK + "/stubs/docopt.py", "w") as f:
        f.write("_next = {}\n\ndef docopt(doc, argv=None, **kw):\n    return dict(_next)\n")
    sys.path.insert(0, WORK + "/stubs")
    sys.path.insert(0, WORK)


def open_text(fn, mode="r"):
    return gzip.open(fn, "rt", encoding="latin-1") if fn.endswith(".gz") else open(fn, mode)


def run_indexing(case, d, test):
    """the reference's hgvs-find.main with -X (and -T) -> (the index file's text or None, stdout)"""
    import docopt
    opts = dict(DEFAULTS)
    words = list(case["opts"])
    while words:
        o = words.pop(0)
        opts[o] = words.pop(0) if not isinstance(DEFAULTS[o], bool) else True
    opts.update({"-X": True, "-T": test, "-g": ".", "<index>": "index.yaml", "<variant>": list(case["variants"])})
    if case["file"] is not None:
        with open(d + "/variants.txt", "w") as f:
            f.write(case["file"])
        opts["-f"] = "variants.txt"
    docopt._next = opts
    mod = importlib.import_module("zotmer.commands.hgvs-find")
    mod.openFile = open_text
    out = io.StringIO()
    cwd = os.getcwd()
    os.chdir(d)
    try:
        if os.path.exists("index.yaml"):
            os.remove("index.yaml")
        with contextlib.redirect_stdout(out):
            mod.main(["hgvs-find"])
        index = open("index.yaml").read() if os.path.exists("index.yaml") else None
    finally:
        os.chdir(cwd)
    return index, out.getvalue()


def main():
    build_derived()
    d = WORK + "/genome"
    write_genome(d)
    res = []
    for case in make_cases():
        index, quiet = run_indexing(case, d, False)
        none, stdout = run_indexing(case, d, True)
        assert index is not None and quiet == "" and none is None
        res.append({"name": case["name"], "opts": case["opts"], "index": index, "test": stdout})
        print(case["name"], case["opts"])
        print(index + stdout, end="")
    with open(os.path.join(HERE, "x1_hgvsindex.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in res) + "\n]\n")


if __name__ == "__main__":
    main()
