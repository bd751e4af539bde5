#!/usr/bin/env python3
"""
Capture golden values of the spectrum measures of `zot dist` (the *.quant, *.ab and jensen.shannon rows) from the reference
(a checkout of drtconway/zotmer, given on the command line).

Runs ONLY where the reference is at hand: its zotmer/library/dist.py is copied to a throw-away directory, passed through the
stdlib's lib2to3 (xrange), imported, and every `vec=True` branch is called as written: dist.<measure>(lhs, rhs, True).  What is
committed is data only: tests/golden/g11_dist_spectrum.json.

The ONE departure from the reference: the two vectors.  The reference's Measure.prep (commands/dist.py:29-41) reads the set with
readKmers and then unpacks (x, c) pairs, so its vector branch cannot run; here the vector is built the way that code intends,
v[x >> S] += c over the (k-mer, count) pairs of the set, S = 2 * (fK - K), as an array('I') of 4**K counters.

Inputs are the golden sets already in this directory (the reference's own `kmerize` output): g4_part0 .. g4_part4 (K = 25) and
g3_kmerize_genome_k12 / _k24, whose pairing gives the two sides different shifts; <k> in {1, 4, 6, 8} (a pure-Python loop over
4**8 counters takes seconds).  One more pair has no prefix in common (the even 8-mer prefixes of g4_part0 against the odd ones
of g4_part1): the reference runs every measure on it but jaccard.ab and sorensen.ab, which divide by zero.

A value enters the file only if its text is safe from the last bits: with n = the prefixes present in either set and
delta = (n + 8) * 2**-52 (more than the rounding a sum of n terms can gather, in either implementation),
'%g' % (v * (1 - delta)), '%g' % v and '%g' % (v * (1 + delta)) must be the same text.  The script fails on a value that is not.

Usage:  python3 tests/golden/make_golden_dist_spectrum.py <reference checkout>      (rewrites tests/golden/g11_dist_spectrum.json)
"""
import array
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

# golden name -> the reference's name of the measure function in library/dist.py (commands/dist.py:59-92)
FUNCS = {"bray.curtis.quant": "brayCurtis", "chord.quant": "chord", "hellinger.quant": "hellinger", "jaccard.ab": "jaccard",
         "jensen.shannon": "jensenShannon", "kulczynski.quant": "kulczynski", "ochiai.ab": "ochiai", "sorensen.ab": "sorensen",
         "whittaker.quant": "whittaker"}
PAIRS = [("g4_part0", "g4_part1"), ("g4_part0", "g4_part2"), ("g4_part3", "g4_part4"),
         ("g3_kmerize_genome_k12", "g3_kmerize_genome_k24"), ("g3_kmerize_genome_k24", "g4_part1")]
KS = [1, 4, 6, 8]


def derived_dist(ref):
    work = tempfile.mkdtemp(prefix="zot_dist_spectrum_")
    shutil.copy(os.path.join(ref, "zotmer", "library", "dist.py"), os.path.join(work, "refdist.py"))
    subprocess.check_call(["chmod", "u+w", os.path.join(work, "refdist.py")])
    subprocess.check_call([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n", os.path.join(work, "refdist.py")],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    sys.path.insert(0, work)
    mod = importlib.import_module("refdist")
    sys.path.pop(0)
    return mod, work


def load_set(name):
    with open(os.path.join(HERE, name + ".json")) as f:
        fK = json.load(f)["K"]
    z = np.load(os.path.join(HERE, name + ".npz"))
    return fK, [int(x) for x in z["kmers"]], [int(c) for c in z["counts"]]


def vector(K, fK, kmers, counts, parity=None):
    """Measure.prep as it is meant (see the header); parity: keep only the prefixes with that lowest bit"""
    assert fK >= K
    S = 2 * (fK - K)
    v = array.array("I", [0 for i in range(1 << (2 * K))])
    for x, c in zip(kmers, counts):
        y = x >> S
        if parity is None or (y & 1) == parity:
            v[y] += c
    return v


def safe_text(v, n):
    delta = (n + 8) * 2.0 ** -52
    texts = {"%g" % (v * (1 - delta)), "%g" % v, "%g" % (v * (1 + delta))}
    assert len(texts) == 1, "value %r is within %g (relative) of a change of its %%g text: %r" % (v, delta, sorted(texts))
    return "%g" % v


def case(dist, sets, lhs, rhs, K, parity=None):
    lv = vector(K, *sets[lhs], parity=None if parity is None else parity[0])
    rv = vector(K, *sets[rhs], parity=None if parity is None else parity[1])
    shared = sum(1 for a, b in zip(lv, rv) if a and b)
    union = sum(1 for a, b in zip(lv, rv) if a or b)
    rec = {"lhs": lhs, "rhs": rhs, "k": K, "n_shared": shared, "n_union": union, "values": {}}
    if parity is not None:
        rec["prefix_parity"] = list(parity)
    for name in sorted(FUNCS):
        try:
            v = getattr(dist, FUNCS[name])(lv, rv, True)
        except ZeroDivisionError:
            assert shared == 0 and name in ("jaccard.ab", "sorensen.ab"), name
            continue
        rec["values"][name] = {"hex": float(v).hex(), "g": safe_text(v, union)}
    return rec


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "zotmer", "library", "dist.py")):
        sys.exit(__doc__)
    dist, work = derived_dist(sys.argv[1])
    try:
        sets = {n: load_set(n) for n in sorted({n for p in PAIRS for n in p})}
        out = []
        for lhs, rhs in PAIRS:
            for K in KS:
                out.append(case(dist, sets, lhs, rhs, K))
                print(lhs, rhs, K, out[-1]["n_shared"], out[-1]["n_union"])
        out.append(case(dist, sets, "g4_part0", "g4_part1", 8, parity=(0, 1)))
        assert out[-1]["n_shared"] == 0 and len(out[-1]["values"]) == 7
        with open(os.path.join(HERE, "g11_dist_spectrum.json"), "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
