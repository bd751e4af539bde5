#!/usr/bin/env python3
"""
Capture golden vectors of `zot vars -r` from the reference (drtconway/zotmer).

Runs ONLY where a checkout of the reference is at hand: its commands/vars.py and library/{basics,bits,misc,stats,file,
exceptions}.py are copied to a throw-away directory outside the repository and passed through the stdlib's lib2to3; nothing
else is edited.  docopt and the two modules that read k-mer sets (library/kmers.py, library/files.py) are stubbed, so that the
command sees the (k-mer, count) pairs of tests/_vars_cases.py (the seeded generator of the inputs) without a set file.
vars.main, group, logBinGe and everything under them are the reference's own, driven in-process.

What is committed is data only: tests/golden/v1_vars.json holds per case K, the reference's stdout lines per input, and
`noise`: the largest |v| that the reference's logBinGe returned for a base whose sample count is 0 (the tail probability is
then 1 and its log 0, so whatever else comes back is rounding noise; the tests derive their tolerance for such columns from
it).

The run also checks
  * that the restatement (tests/_vars_restatement.py) reproduces every line as text, and the noise;
  * that no case has a sample context that the reference set lacks, and that the reference dies with AssertionError on
    tests/_vars_cases.missing_case(), after printing the lines before the first such context;
  * that the reference dies without -r (AttributeError or NameError);
  * that no computed v lies within 1e-6 of -10 (the letter column does not depend on the machine), that every case prints at
    least 5 lines, that some line's letter stands for more than one base and that some printed line has a v within 3 of -10.

Usage:  python3 tests/golden/make_golden_vars.py <reference checkout>      (rewrites tests/golden/v1_vars.json)
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

from tests import _vars_restatement as R  # noqa: E402
from tests._vars_cases import make_cases, missing_case  # noqa: E402

KMERS_STUB = '''_sets = {}


class kmers:
    def __init__(self, path, mode):
        self.path, self.meta = path, {"K": _sets[path][0]}

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
'''
FILES_STUB = '''def readKmersAndCounts(z):
    from zotmer.library.kmers import _sets
    for xc in _sets[z.path][1]:
        yield xc
'''


def build_derived(ref, work):
    os.makedirs(work + "/stubs")
    shutil.copytree(ref + "/zotmer", work + "/zotmer")
    subprocess.check_call(["chmod", "-R", "u+w", work])
    files = [work + "/zotmer/library/%s.py" % m for m in ("basics", "bits", "misc", "stats", "file", "exceptions")]
    files += [work + "/zotmer/commands/vars.py"]
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


def run_main(opts):
    """the reference's vars.main -> (stdout, the exception it died with or None)"""
    import docopt
    docopt._next = opts
    mod = importlib.import_module("zotmer.commands.vars")
    out, died = io.StringIO(), None
    with contextlib.redirect_stdout(out):
        try:
            mod.main(["vars"])
        except (AssertionError, AttributeError, NameError) as e:
            died = e
    return out.getvalue(), died


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    work = tempfile.mkdtemp(prefix="zot3_vars_")
    try:
        build_derived(sys.argv[1], work)
        from zotmer.library import kmers as kmers_stub
        mod = importlib.import_module("zotmer.commands.vars")
        calls = []                                   # every logBinGe of the reference: (p, n, k, v)
        real = mod.logBinGe

        def spy(p, n, k):
            v = real(p, n, k)
            calls.append((p, n, k, v))
            return v
        mod.logBinGe = spy

        out, Ks, multi, near = [], set(), False, False
        for case in make_cases():
            K, name = case["K"], case["name"]
            Ks.add(K)
            kmers_stub._sets[name + "_ref"] = (K, case["ref"])
            for nm, pairs in case["samples"]:
                kmers_stub._sets[nm] = (K, pairs)
            del calls[:]
            text, died = run_main({"-r": name + "_ref", "<input>": [nm for nm, _ in case["samples"]]})
            assert died is None, (name, died)
            lines = text.splitlines()
            want = [l for _, pairs in case["samples"] for l in R.stdout_lines(K, case["ref"], pairs)]
            assert lines == want, name
            assert len(lines) >= 5, (name, len(lines))
            assert all(abs(v + 10) >= 1e-6 for _, _, _, v in calls), name
            noise = max([0.0] + [abs(v) for _, _, k, v in calls if k == 0])
            assert noise == R.noise(K, case["ref"], case["samples"]), name
            for l in lines:
                f = l.split("\t")
                multi = multi or f[1] not in "ACGT"
                near = near or any(abs(float(x) + 10) < 3 for x in f[2:])
            per_input, at = {}, 0
            for nm, pairs in case["samples"]:
                n = len(R.stdout_lines(K, case["ref"], pairs))
                per_input[nm] = lines[at:at + n]
                at += n
            out.append(dict(name=name, K=K, inputs=[nm for nm, _ in case["samples"]], stdout=per_input, noise=noise))
            print(name, K, "inputs", len(case["samples"]), "lines", len(lines), "calls", len(calls), "noise", noise)
        assert Ks == {1, 2, 7, 25, 31, 32} and multi and near

        # a context that the reference set lacks: AssertionError, after the lines of the contexts before it
        m = missing_case()
        kmers_stub._sets["m_ref"], kmers_stub._sets["m_sam"] = (m["K"], m["ref"]), (m["K"], m["sample"])
        text, died = run_main({"-r": "m_ref", "<input>": ["m_sam"]})
        assert isinstance(died, AssertionError) and text == "", (text, died)      # the first context is already missing
        kmers_stub._sets["m_shared"] = (m["K"], m["shared"])
        text, died = run_main({"-r": "m_ref", "<input>": ["m_shared"]})
        assert died is None and text.splitlines() == R.stdout_lines(m["K"], m["ref"], m["sample"], skip_missing=True)
        assert len(text.splitlines()) == 3
        # without -r
        text, died = run_main({"-r": None, "<input>": ["m_shared"]})
        assert isinstance(died, (AttributeError, NameError)), died
        print("missing context: AssertionError; no -r:", type(died).__name__)

        with open(os.path.join(HERE, "v1_vars.json"), "w") as f:
            json.dump(out, f, indent=None, sort_keys=True, separators=(",", ":"))
            f.write("\n")
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
