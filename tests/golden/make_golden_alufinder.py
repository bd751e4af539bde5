#!/usr/bin/env python3
"""
Capture golden vectors of `zot alu-finder` from the reference (drtconway/zotmer at /root/reference).

Runs ONLY in the development container: the reference's own commands/alu-finder.py (with library/{basics,bits,file,hgvs,
reads,misc}.py) is copied to a throw-away directory under /tmp, passed through the stdlib's lib2to3, docopt, tqdm and yaml are
stubbed, and the command is driven in-process, as tests/golden/make_golden_strand.py does for `zot strand`.  What is committed
is data only: tests/golden/a1_alufinder.json holds, per case of tests/_alufinder_cases.py (the seeded generator of the
inputs), the options, the number of lines the reference printed and the lines themselves -- or their SHA-256 where they are
long.  The run asserts that
  * the restatement (tests/_alufinder_restatement.py) reproduces the reference's lines exactly, in order;
  * the cases together hold a joined insertion line, an `after` and a `before` raw spur, and a case that prints only the header;
  * the cases hold a read with two diagonals in one zone (by the restatement, once it has reproduced the reference's lines).

Usage:  python3 tests/golden/make_golden_alufinder.py        (rewrites tests/golden/a1_alufinder.json)
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
WORK = "/tmp/zot3_alufinder"
LONG = 4000          # characters of output above which a case stores a digest instead of its lines
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import _alufinder_restatement as R  # noqa: E402
from tests._alufinder_cases import make_cases, write_case  # noqa: E402


def build_derived():
    shutil.rmtree(WORK, ignore_errors=True)
    os.makedirs(WORK + "/stubs")
    shutil.copytree(REF + "/zotmer", WORK + "/zotmer")
    subprocess.check_call(["chmod", "-R", "u+w", WORK])
    files = [WORK + "/zotmer/library/%s.py" % m for m in ("basics", "bits", "file", "hgvs", "reads", "misc")]
    files += [WORK + "/zotmer/commands/alu-finder.py"]
    subprocess.check_call([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n"] + files,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(WORK + "/stubs/docopt.py", "w") as f:
        f.write("_next = {}\n\ndef docopt(doc, argv=None, **kw):\n    return dict(_next)\n")
    with open(WORK + "/stubs/tqdm.py", "w") as f:
        f.write("def tqdm(*a, **k):\n    raise RuntimeError('not verbose')\n")
    with open(WORK + "/stubs/yaml.py", "w") as f:
        f.write("")
    sys.path.insert(0, WORK + "/stubs")
    sys.path.insert(0, WORK)


def run_reference(case, tmp):
    """the reference's alu-finder.main on the case's files -> its stdout lines, without their newlines"""
    import docopt
    d = os.path.join(tmp, case["name"])
    shutil.rmtree(d, ignore_errors=True)
    args = write_case(case, d)
    n_in = len(case["inputs"])
    docopt._next = {"-k": str(case["k"]), "-g": d, "-C": str(case["C"]), "-L": str(case["L"]), "-r": case["raw"], "-S": str(case["S"]),
                    "-V": repr(case["V"]), "-v": False, "<regions>": args[-n_in - 1], "<input>": args[-n_in:]}
    mod = importlib.import_module("zotmer.commands.alu-finder")
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        mod.main(["alu-finder"])
    text = out.getvalue()
    assert text.endswith("\n")
    return text[:-1].split("\n")


def digest(lines):
    return hashlib.sha256("".join(l + "\n" for l in lines).encode()).hexdigest()


def main():
    build_derived()
    tmp = WORK + "/runs"
    out = []
    seen = dict(joined=0, after=0, before=0, header_only=0, two_diagonals=0)
    for case in make_cases():
        lines = run_reference(case, tmp)
        diags = []
        mine = R.alu_finder(case, diag_log=diags)
        assert mine == lines, (case["name"], len(mine), len(lines))
        rec = {k: case[k] for k in ("name", "k", "C", "L", "S", "V", "raw")}
        rec["n_lines"] = len(lines)
        if sum(len(l) + 1 for l in lines) > LONG:
            rec["sha256"] = digest(lines)
        else:
            rec["lines"] = lines
        out.append(rec)
        body = lines[1:]
        seen["header_only"] += not body
        if case["raw"]:
            seen["after"] += sum(1 for l in body if l.split("\t")[2] == "after")
            seen["before"] += sum(1 for l in body if l.split("\t")[2] == "before")
        else:
            seen["joined"] += len(body)
        two = sum(1 for d in diags if len(d) != len({z for z, _ in d}))
        seen["two_diagonals"] += two
        print(case["name"], "lines", len(lines), "lists with two diagonals in a zone", two, "most diagonals", max(map(len, diags), default=0))
    assert all(seen.values()), seen
    print(seen)
    with open(os.path.join(HERE, "a1_alufinder.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
