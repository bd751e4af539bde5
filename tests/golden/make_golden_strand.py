#!/usr/bin/env python3
"""
Capture golden vectors of `zot strand` from the reference (drtconway/zotmer at /root/reference).

Runs ONLY in the development container: the reference's own commands/strand.py (with library/{basics,bits,file}.py) is
copied to a throw-away directory under /tmp, passed through the stdlib's lib2to3, docopt is stubbed, and the command is
driven in-process, as tests/golden/make_golden_capture.py does for `zot capture`.  What is committed is data only:
tests/golden/s1_strand.json holds, per case of tests/_strand_cases.py (the seeded generator of the inputs), the options,
the number of lines the reference printed and the SHA-256 of those lines sorted as text (the reference prints in dict
order).  The run also checks that the cases together exercise what the fixture is for: a line with both counts non-zero,
a line with a zero, a palindrome and an orphan (by the restatement, once it has reproduced the reference's lines).

Usage:  python3 tests/golden/make_golden_strand.py        (rewrites tests/golden/s1_strand.json)
"""
import contextlib
import hashlib
import importlib
import io
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
WORK = "/tmp/zot3_strand"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import _strand_restatement as R  # noqa: E402
from tests._strand_cases import make_cases  # noqa: E402


def build_derived():
    shutil.rmtree(WORK, ignore_errors=True)
    os.makedirs(WORK + "/stubs")
    shutil.copytree(REF + "/zotmer", WORK + "/zotmer")
    subprocess.check_call(["chmod", "-R", "u+w", WORK])
    files = [WORK + "/zotmer/library/%s.py" % m for m in ("basics", "bits", "file")]
    files += [WORK + "/zotmer/commands/strand.py"]
    subprocess.check_call([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n"] + files,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(WORK + "/stubs/docopt.py", "w") as f:
        f.write("_next = {}\n\ndef docopt(doc, argv=None, **kw):\n    return dict(_next)\n")
    sys.path.insert(0, WORK + "/stubs")
    sys.path.insert(0, WORK)


def run_strand(case, tmp):
    """the reference's strand.main on the case's inputs -> its stdout lines"""
    import docopt
    d = os.path.join(tmp, case["name"])
    shutil.rmtree(d, ignore_errors=True)
    os.makedirs(d)
    inputs = []
    for i, text in enumerate(case["inputs"]):
        p = d + "/in%d.fastq" % i
        with open(p, "w", newline="") as f:
            f.write(text)
        inputs.append(p)
    docopt._next = {"-k": str(case["k"]), "-p": repr(case["p"]), "-r": None, "-s": False, "-v": False, "<fastq>": inputs}
    mod = importlib.import_module("zotmer.commands.strand")
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        mod.main(["strand"])
    return out.getvalue().splitlines(keepends=True)


def digest(lines):
    return hashlib.sha256("".join(sorted(lines)).encode()).hexdigest()


def main():
    build_derived()
    tmp = WORK + "/runs"
    out = []
    seen = dict(both=0, zero=0, palindromes=0, orphans=0)
    for case in make_cases():
        lines = run_strand(case, tmp)
        rec = {k: v for k, v in case.items() if k != "inputs"}
        rec["lines"] = len(lines)
        rec["sha256_sorted"] = digest(lines)
        out.append(rec)
        mine, _, st = R.strand(case["k"], case["p"], case["inputs"])
        assert sorted(mine) == sorted(lines), case["name"]
        pairs = [tuple(int(v) for v in l.split("\t")) for l in lines]
        seen["both"] += sum(1 for a, b in pairs if a and b)
        seen["zero"] += sum(1 for a, b in pairs if not (a and b))
        seen["palindromes"] += st["palindromes"]
        seen["orphans"] += st["orphans"]
        print(case["name"], len(lines), st, sum(1 for a, b in pairs if not (a and b)))
    assert all(seen.values()), seen
    with open(os.path.join(HERE, "s1_strand.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
