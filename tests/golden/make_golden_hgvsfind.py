#!/usr/bin/env python3
"""
Capture golden vectors of `zot hgvs-find` (scanning mode) from the reference (drtconway/zotmer at /root/reference).

Runs ONLY in the development container, as tests/golden/make_golden_pulldown.py does: the reference's own
commands/hgvs-find.py, with the library modules it imports, is copied to a throw-away directory under /tmp and passed
through the stdlib's lib2to3; docopt is stubbed (the options the reference's docopt would give are made from the case's
option words and the defaults of the usage text).  The command is driven in-process from the case's directory, with the index
written by yaml.safe_dump as 'index.yaml' (what the reference's -X writes) and the inputs under the relative names
'in<i>.fastq', and its stdout captured.  What is committed is data only: tests/golden/h1_hgvsfind.json holds, per case of
tests/_hgvsfind_cases.py (the seeded generator of the inputs), the option words and the stdout text.

Usage:  python3 tests/golden/make_golden_hgvsfind.py        (rewrites tests/golden/h1_hgvsfind.json)
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
WORK = "/tmp/zot3_hgvsfind"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests._hgvsfind_cases import make_cases  # noqa: E402

DEFAULTS = {"-X": False, "-T": False, "-A": "0.001", "-B": "none", "-C": "10", "-c": None, "-D": "2", "-f": None, "-F": "rds,vaf",
            "-k": "25", "-g": None, "-o": None, "-s": False, "-v": False, "-V": "0.05", "-w": "75", "-W": "1024", "<variant>": []}


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


class KeptText(io.StringIO):
    """the reference leaves `with sys.stdout as out:` (hgvs-find.py:982): the text must outlive that close"""

    def close(self):
        pass


def run_hgvs_find(case, tmp):
    """the reference's hgvs-find.main on the case's index and inputs -> stdout text"""
    import docopt
    import yaml
    d = os.path.join(tmp, case["name"])
    shutil.rmtree(d, ignore_errors=True)
    os.makedirs(d)
    with open(d + "/index.yaml", "w") as f:
        yaml.safe_dump(case["index"], f, default_flow_style=False)
    inputs = []
    for i, text in enumerate(case["inputs"]):
        with open(d + "/in%d.fastq" % i, "w", newline="") as f:
            f.write(text)
        inputs.append("in%d.fastq" % i)
    opts = dict(DEFAULTS)
    words = list(case["opts"])
    while words:
        o = words.pop(0)
        opts[o] = words.pop(0) if not isinstance(DEFAULTS[o], bool) else True
    opts.update({"<index>": "index.yaml", "<input>": inputs})
    docopt._next = opts
    mod = importlib.import_module("zotmer.commands.hgvs-find")
    out = KeptText()
    cwd = os.getcwd()
    os.chdir(d)
    try:
        with contextlib.redirect_stdout(out):
            mod.main(["hgvs-find"])
    finally:
        os.chdir(cwd)
    return out.getvalue()


def main():
    build_derived()
    tmp = WORK + "/runs"
    res = []
    for case in make_cases():
        stdout = run_hgvs_find(case, tmp)
        res.append({"name": case["name"], "opts": case["opts"], "stdout": stdout})
        print(case["name"], case["opts"])
        print(stdout, end="")
    with open(os.path.join(HERE, "h1_hgvsfind.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in res) + "\n]\n")


if __name__ == "__main__":
    main()
