#!/usr/bin/env python3
"""
Capture golden vectors of `zot disass` from the reference (drtconway/zotmer).

Runs ONLY where a checkout of the reference is at hand: its commands/disass.py and library/{basics,bits,file}.py are copied to
a throw-away directory outside the repository and passed through the stdlib's lib2to3, with one further edit that Python 3
needs: file.openFile reads compressed files through a pipe, which hands out bytes under Python 3, so the two Popen calls get
universal_newlines=True.  docopt is stubbed; yaml is the real PyYAML.  disass.main is the reference's own, driven in-process
with the working directory at the case's files, so that the `file` entries are the bare file names.

What is committed is data only: tests/golden/d1_disass.json holds, per case of tests/_disass_cases.py, yaml.safe_load of the
reference's stdout (JSON keeps the int or float type of `median`).

The run also checks
  * that the restatement (tests/_disass_restatement.py) reproduces every case, types included;
  * that no contig and no file of a case keeps exactly one distinct k-mer (the reference dies there: disass.py:43; those inputs
    belong to the deviation tests), and that the reference does die on such an input;
  * that the cases hold what the fixture is for (see `check_classes`).

Usage:  python3 tests/golden/make_golden_disass.py <reference checkout>      (rewrites tests/golden/d1_disass.json)
"""
import contextlib
import importlib
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import _disass_restatement as R  # noqa: E402
from tests._disass_cases import argv, make_cases, write_files  # noqa: E402


def edit(path, pairs):
    s = open(path).read()
    for a, b in pairs:
        assert a in s, (path, a)
        s = s.replace(a, b)
    with open(path, "w") as f:
        f.write(s)


def build_derived(ref, work):
    os.makedirs(work + "/stubs")
    shutil.copytree(ref + "/zotmer", work + "/zotmer")
    subprocess.check_call(["chmod", "-R", "u+w", work])
    files = [work + "/zotmer/library/%s.py" % m for m in ("basics", "bits", "file")] + [work + "/zotmer/commands/disass.py"]
    subprocess.check_call([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n"] + files,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    edit(work + "/zotmer/library/file.py", [("stdout=subprocess.PIPE)", "stdout=subprocess.PIPE, universal_newlines=True)")])
    with open(work + "/stubs/docopt.py", "w") as f:
        f.write("_next = {}\n\ndef docopt(doc, argv=None, **kw):\n    return dict(_next)\n")
    sys.path.insert(0, work + "/stubs")
    sys.path.insert(0, work)


def run_main(opts, names, where):
    """the reference's disass.main in `where` -> its stdout"""
    import docopt
    docopt._next = {"-k": str(opts["K"]), "-c": str(opts["C"]), "-p": repr(opts["P"]), "-q": str(opts["Q"]), "-S": str(opts["S"]),
                    "-s": not opts["both"], "-v": False, "<input>": list(names)}
    mod = importlib.import_module("zotmer.commands.disass")
    out = io.StringIO()
    cwd = os.getcwd()
    os.chdir(where)
    try:
        with contextlib.redirect_stdout(out):
            mod.main(["disass"])
    finally:
        os.chdir(cwd)
    return out.getvalue()


def same(a, b):
    """equal, the types of the numbers included"""
    return json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)


def check_classes(case, dicts):
    """dicts: per file ([(name, dict)], the file's dict).  What each case is in the fixture for; AssertionError if it is not"""
    o, name = case["opts"], case["name"]
    K = o["K"]
    every = [d for contigs, _ in dicts for _, d in contigs]
    if name in ("k4", "k6"):
        pal = [d[x] for d in every for x in d if x == _rc(K, x)]
        assert pal and all(c % 2 == 0 for c in pal), name    # palindromes: one dict entry for both strands, counted twice a window
    if name == "sampled":
        assert any(_rc(K, x) not in d for d in every for x in d), name      # x kept while rc x is dropped
        assert any(_rc(K, x) in d for d in every for x in d), name
    if name == "edges":
        by = {nm: d for contigs, _ in dicts for nm, d in contigs}
        assert by["shorter than K"] == {} and by["all_N"] == {} and len(by["poly_A"]) == 2
        assert len(by["n_inside"]) < 2 * (199 - K + 1) and len(by["lower case and u"]) > 0
    if name == "two_files":
        contigs, glob = dicts[0]
        assert contigs[0][1] == dict(contigs)["again"] and contigs[0][1]
        assert all(glob[x] >= 2 * c for x, c in contigs[0][1].items())              # global differs from per-contig
    if name == "c2_q4":
        assert any(c >= 2 for d in every for c in d.values()) and any(c < 2 for d in every for c in d.values())


def _rc(K, x):
    y = 0
    for _ in range(K):
        y = (y << 2) | (3 - (x & 3))
        x >>= 2
    return y


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    import yaml
    work = tempfile.mkdtemp(prefix="zot3_disass_")
    try:
        build_derived(sys.argv[1], work)
        out = {}
        for case in make_cases():
            o, name = case["opts"], case["name"]
            where = os.path.join(work, "case_" + name)
            os.makedirs(where)
            write_files(case, where)
            names = [fn for fn, _ in case["files"]]
            text = run_main(o, names, where)
            got = yaml.safe_load(text)
            rs = R.disass(case["files"], o["K"], o["C"], o["P"], o["Q"], o["S"], o["both"])
            assert same(got, rs), name
            dicts = [R.contig_dicts(t, o["K"], o["both"], o["S"], o["P"]) for _, t in case["files"]]
            for contigs, glob in dicts:
                assert len(glob) != 1 and all(len(d) != 1 for _, d in contigs), name
            check_classes(case, dicts)
            out[name] = got
            print(name, " ".join(argv(case)), "contigs", [len(f["contigs"]) for f in got],
                  "distinct", [len(g) for _, g in dicts], "medians", [c["median"] for f in got for c in f["contigs"]])
        # exactly one distinct k-mer: the reference dies (disass.py:43)
        where = os.path.join(work, "case_single")
        os.makedirs(where)
        with open(os.path.join(where, "one.fa"), "w") as f:
            f.write(">one\n" + "A" * 30 + "\n")
        try:
            run_main(dict(K=25, C=5, P=8.0, Q=10, S=17, both=False), ["one.fa"], where)
            raise AssertionError("the reference summarised a dict of one k-mer")
        except IndexError:
            pass
        with open(os.path.join(HERE, "d1_disass.json"), "w") as f:
            json.dump(out, f, indent=None, sort_keys=True, separators=(",", ":"))
            f.write("\n")
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
