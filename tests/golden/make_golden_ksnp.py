#!/usr/bin/env python3
"""
Capture golden vectors of `zot ksnp` from the reference (drtconway/zotmer).

Runs ONLY where a checkout of the reference is at hand: its commands/ksnp.py and library/{basics,bits,misc}.py are copied to a
throw-away directory outside the repository and passed through the stdlib's lib2to3; nothing else is edited.  docopt and the
three modules the generators never touch (library/sparse.py, library/kmers.py, library/files.py) are stubbed.  The reference's
main cannot finish (it calls writeKmers, which it does not import), so the three generators ksnp, hamming and levenshtein --
the reference's own, with its ham, lev, popcnt and unionfind under them -- are driven in-process on the k-mer lists of
tests/_ksnp_cases.py, and what they yield is flattened and sorted, as main does before it dies.

What is committed is data only: tests/golden/k1_ksnp.json holds per case K, the mode, d, the generator's parameters (with the
number of k-mers and a digest of them) and the sorted k-mers the reference's generator yielded.

The run also checks
  * that the restatement (tests/_ksnp_restatement.py) and the brute force (tests/_ksnp_brute.py) reproduce every case;
  * that the reference's main dies with NameError;
  * that every K has a case that keeps something and one that keeps less than everything, that -H 0 keeps nothing, and that
    some -L 2 case keeps k-mers that -H 2 does not.

Usage:  python3 tests/golden/make_golden_ksnp.py <reference checkout>      (rewrites tests/golden/k1_ksnp.json)
"""
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import _ksnp_brute as B  # noqa: E402
from tests import _ksnp_restatement as R  # noqa: E402
from tests._ksnp_cases import DEFAULT, FIXTURE_SEED, HAMMING, LEVENSHTEIN, digest, fixture_cases  # noqa: E402

KMERS_STUB = '''class kmers:
    def __init__(self, path, mode):
        self.path, self.meta = path, {"K": 5}

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
'''


def build_derived(ref, work):
    os.makedirs(work + "/stubs")
    shutil.copytree(ref + "/zotmer", work + "/zotmer")
    subprocess.check_call(["chmod", "-R", "u+w", work])
    files = [work + "/zotmer/library/%s.py" % m for m in ("basics", "bits", "misc")] + [work + "/zotmer/commands/ksnp.py"]
    subprocess.check_call([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n"] + files,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(work + "/stubs/docopt.py", "w") as f:
        f.write("_next = {}\n\ndef docopt(doc, argv=None, **kw):\n    return dict(_next)\n")
    with open(work + "/zotmer/library/sparse.py", "w") as f:
        f.write("sparse = None\n")
    with open(work + "/zotmer/library/kmers.py", "w") as f:
        f.write(KMERS_STUB)
    with open(work + "/zotmer/library/files.py", "w") as f:
        f.write("def readKmers(z):\n    return iter([1, 2, 3])\n")
    sys.path.insert(0, work + "/stubs")
    sys.path.insert(0, work)


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    work = tempfile.mkdtemp(prefix="zot3_ksnp_")
    try:
        build_derived(sys.argv[1], work)
        mod = importlib.import_module("zotmer.commands.ksnp")
        import docopt
        docopt._next = {"-H": None, "-L": None, "<output>": work + "/out.k", "<ref>": "x"}
        try:
            mod.main(["ksnp"])
            raise AssertionError("the reference's main finished")
        except NameError as e:
            print("main:", type(e).__name__, e)

        out, kept_by = [], {}
        for case in fixture_cases():
            K, mode, d, xs = case["K"], case["mode"], case["d"], list(case["kmers"])
            gen = {DEFAULT: lambda: mod.ksnp(K, iter(xs)), HAMMING: lambda: mod.hamming(K, d, iter(xs)),
                   LEVENSHTEIN: lambda: mod.levenshtein(K, d, iter(xs))}[mode]
            want = sorted(x for ys in gen() for x in ys)
            assert len(set(want)) == len(want) and set(want) <= set(xs), case["name"]
            assert R.run(K, mode, d, xs) == want, case["name"]
            assert B.run(K, mode, d, xs).tolist() == want, case["name"]
            kept_by[(K, mode, d)] = set(want)
            out.append(dict(name=case["name"], K=K, mode=mode, d=d, params=dict(seed=FIXTURE_SEED, n=len(xs), digest=digest(xs)),
                            kept=want))
            print(case["name"], "n", len(xs), "kept", len(want))
        for K in sorted({k for k, _, _ in kept_by}):
            sizes = [len(v) for (k, _, _), v in kept_by.items() if k == K]
            assert max(sizes) > 0 and kept_by[(K, HAMMING, 0)] == set(), K
            assert kept_by[(K, DEFAULT, 0)] <= kept_by[(K, HAMMING, 1)] <= kept_by[(K, HAMMING, 2)], K
            assert kept_by[(K, HAMMING, 1)] <= kept_by[(K, LEVENSHTEIN, 1)] and kept_by[(K, HAMMING, 2)] <= kept_by[(K, LEVENSHTEIN, 2)], K
        assert any(kept_by[(K, LEVENSHTEIN, 2)] - kept_by[(K, HAMMING, 2)] for K, _, _ in kept_by)
        assert any(len(c["kept"]) < c["params"]["n"] for c in out if c["mode"] == DEFAULT)

        with open(os.path.join(HERE, "k1_ksnp.json"), "w") as f:
            json.dump(out, f, indent=None, sort_keys=True, separators=(",", ":"))
            f.write("\n")
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
