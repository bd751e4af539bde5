#!/usr/bin/env python3
"""
Capture golden vectors of `zot spoligo` from the reference (drtconway/zotmer).

Runs ONLY where a checkout of the reference is at hand: its commands/spoligo.py (with library/{basics,bits,misc,sparse}.py)
is copied to a throw-away directory outside the repository and passed through the stdlib's lib2to3; docopt and the two
modules that read k-mer files (library/kmers.py, library/files.py) are stubbed, so that the command sees the k-mers of
tests/_spoligo_cases.py (the seeded generator of the inputs) without a container file.  The command is driven in-process, in
its default and its -l form, and findProbe(probe, K, sparse(2 * K, array('Q', set))) is called per probe as well: both give
the same answers.  What is committed is data only: tests/golden/sp1_spoligo.json holds per case the name, K, the options and
the reference's 0/1 string, and for the probe file with badly formatted lines what the reference wrote to stderr ("{path}"
standing for the file's name) and its exit status.

The run also checks that the cases hold what the fixture is for (see the list in `main`) and that the restatement
(tests/_spoligo_restatement.py) reproduces every string.

Usage:  python3 tests/golden/make_golden_spoligo.py <reference checkout>      (rewrites tests/golden/sp1_spoligo.json)
"""
import array
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

from tests import _spoligo_restatement as R  # noqa: E402
from tests._spoligo_cases import encode, ham, make_cases, nearest  # noqa: E402

# a probe file the reference refuses: a blank line, three tokens; the numbers it prints count probe lines, not lines
BAD_FILE = "#c\nACGTACGT\n\nn1 ACGTTTGA\n# another\na b c\nACGTAAAA\n"

KMERS_STUB = '''_sets = {}


class kmers:
    def __init__(self, path, mode):
        self.path, self.meta = path, {"K": _sets[path][0]}

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
'''
FILES_STUB = '''def readKmers(z):
    from zotmer.library.kmers import _sets
    return _sets[z.path][1]
'''


def build_derived(ref, work):
    os.makedirs(work + "/stubs")
    shutil.copytree(ref + "/zotmer", work + "/zotmer")
    subprocess.check_call(["chmod", "-R", "u+w", work])
    files = [work + "/zotmer/library/%s.py" % m for m in ("basics", "bits", "misc", "sparse")]
    files += [work + "/zotmer/commands/spoligo.py"]
    subprocess.check_call([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n"] + files,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(work + "/stubs/docopt.py", "w") as f:
        f.write("_next = {}\n\ndef docopt(doc, argv=None, **kw):\n    return dict(_next)\n")
    with open(work + "/zotmer/library/kmers.py", "w") as f:
        f.write(KMERS_STUB)
    with open(work + "/zotmer/library/files.py", "w") as f:
        f.write(FILES_STUB)
    sys.path.insert(0, work + "/stubs")
    sys.path.insert(0, work)


def run_main(probe_path, inputs, long_format):
    """the reference's spoligo.main -> (stdout, stderr, exit status)"""
    import docopt
    docopt._next = {"-p": probe_path, "-l": long_format, "<input>": inputs}
    mod = importlib.import_module("zotmer.commands.spoligo")
    out, err, code = io.StringIO(), io.StringIO(), 0
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            mod.main(["spoligo"])
        except SystemExit as e:
            code = e.code
    return out.getvalue(), err.getvalue(), code


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    work = tempfile.mkdtemp(prefix="zot3_spoligo_")
    try:
        build_derived(sys.argv[1], work)
        from zotmer.library import kmers as kmers_stub
        from zotmer.library.sparse import sparse
        ref = importlib.import_module("zotmer.commands.spoligo")
        out = []
        seen = set()
        for case in make_cases():
            K, xs = case["K"], case["kmers"]
            pf = os.path.join(work, case["name"] + ".probes")
            with open(pf, "w") as f:
                f.write(case["probe_text"])
            kmers_stub._sets["set_" + case["name"]] = (K, xs)
            text, err, code = run_main(pf, ["set_" + case["name"]], False)
            assert code == 0 and err == "" and text.startswith("set_%s\t" % case["name"]) and text.endswith("\n"), (text, err, code)
            bits = text[:-1].split("\t")[1]
            long_text, _, _ = run_main(pf, ["set_" + case["name"]], True)
            assert long_text == "".join("set_%s\t%s\t%s\n" % (case["name"], p["name"], b) for p, b in zip(case["probes"], bits))
            sp = sparse(2 * K, array.array("Q", xs))
            direct = "".join("1" if ref.findProbe(ref.probe(p["seq"]), K, sp) else "0" for p in case["probes"])
            assert direct == bits, (case["name"], direct, bits)
            assert R.spoligo(K, xs, [p["seq"] for p in case["probes"]]) == bits, case["name"]
            out.append(dict(name=case["name"], K=K, options=[], present=bits))
            print(case["name"], K, len(xs), bits)
            for p, b in zip(case["probes"], bits):
                near = nearest(p["seq"], K, xs)
                assert (b == "1") == all(d <= 2 for d in near), (case["name"], p["name"])
                kind = "short" if len(p["seq"]) < K else ("K" if len(p["seq"]) == K else "long")
                seen.add((kind, b))
                if p["design"] is not None and case["name"] in ("k25", "k32"):
                    assert near == p["design"], (case["name"], p["name"], near, p["design"])
                    seen.update(p["tags"])
                    if K == 32 and len(p["seq"]) == 32:
                        seen.add("K32")
                    if "below_window" in p["tags"]:          # k-mers that differ from each other only below the window
                        s, v = 2 * (K - len(p["seq"])), encode(p["seq"])
                        assert sum(1 for x in xs if ham(x >> s, v) == 1) >= 2
            assert "#" in case["probe_text"] and any(p["name"].isdigit() for p in case["probes"]) and \
                any(not p["name"].isdigit() for p in case["probes"])
        need = {"d0", "d1", "d2", "d3", "first", "last", "both_bits", "below_window", "all_present", "one_absent", "K32"}
        need |= {(kind, b) for kind in ("short", "K", "long") for b in "01"}
        assert need <= seen, need - seen
        # the badly formatted file
        pf = os.path.join(work, "bad.probes")
        with open(pf, "w") as f:
            f.write(BAD_FILE)
        text, err, code = run_main(pf, ["set_k25"], False)
        assert text == "" and code == 1, (text, code)
        out.append(dict(name="bad_file", probe_text=BAD_FILE, stderr=err.replace(pf, "{path}"), exit=code))
        print(repr(err))
        with open(os.path.join(HERE, "sp1_spoligo.json"), "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
