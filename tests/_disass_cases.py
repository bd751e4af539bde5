"""The inputs of the `zot disass` fixtures (tests/golden/d1_disass.json): FASTA texts built by a seeded generator, so that the
fixture holds only what the reference made of them.  Read by tests/golden/make_golden_disass.py and by the tests.

A case is dict(name, opts, files): opts = dict(K, C, P, Q, S, both) (the values of -k -c -p -q -S and `not -s`), files =
[(file name, FASTA text)]; a name ending in .gz is written gzip-compressed.  `argv(case)` is the command line."""
import gzip
import os
import random

BASES = "ACGT"
DEFAULTS = dict(K=25, C=5, P=1.0, Q=10, S=17, both=True)


def _wrap(seq, width):
    return "\n".join(seq[i:i + width] for i in range(0, len(seq), width))


def _fasta(recs, width=70):
    return "".join(">%s\n%s\n" % (nm, _wrap(s, width)) for nm, s in recs)


def _contigs(rng, n, lo=40, hi=400, repeat=0.3):
    """n contigs of lo .. hi bases from one random genome, so that k-mers are shared between contigs; a contig may carry a
    stretch of itself twice"""
    g = "".join(rng.choice(BASES) for _ in range(1500))
    out = []
    for i in range(n):
        L = rng.randrange(lo, hi + 1)
        p = rng.randrange(0, len(g) - L)
        s = g[p:p + L]
        if rng.random() < repeat and L >= 80:
            s = s[:L - 30] + s[10:40]
        out.append(("contig_%d" % (i + 1), s))
    return out


def make_cases():
    rng = random.Random(20261018)
    cases = []

    def add(name, files, **opts):
        cases.append(dict(name=name, opts=dict(DEFAULTS, **opts), files=files))

    add("defaults", [("defaults.fa", _fasta(_contigs(rng, 5)))])
    add("k4", [("k4.fa", _fasta(_contigs(rng, 4)))], K=4)
    add("k6", [("k6.fa", _fasta(_contigs(rng, 4)))], K=6, P=8.0)         # murmer / (2^61 - 1) is below 8: every k-mer is kept
    add("k5_single", [("k5s.fa", _fasta(_contigs(rng, 4)))], K=5, both=False)
    sampled = _fasta(_contigs(rng, 5, lo=200))
    add("sampled", [("sampled.fa", sampled)], K=11, P=0.3, S=5)
    add("sampled_single", [("sampled.fa", sampled)], K=11, P=0.3, S=5, both=False)
    add("c2_q4", [("c2q4.fa", _fasta(_contigs(rng, 4, repeat=1.0)))], K=9, C=2, Q=4)

    a, b, c = (s for _, s in _contigs(rng, 3, lo=120, hi=200, repeat=0.0))
    edge = [("shorter than K", a[:20]),
            ("all_N", "N" * 60),
            ("lower case and u", b.lower().replace("t", "u")),
            ("n_inside", c[:70] + "N" + c[71:]),
            ("poly_A", "A" * 60),
            ("mixed", a[:50] + "nn" + b[:50].lower() + "R" + c[:10])]          # the last stretch is shorter than K
    add("edges", [("edges.fa", _fasta(edge, width=33))], P=8.0)

    one, two, three = _contigs(rng, 3, lo=100, hi=250)
    add("two_files", [("first.fa", _fasta([one, two, ("again", one[1])])), ("second.fa", _fasta([("again_elsewhere", one[1]), three]))], K=15)
    add("gzip", [("packed.fa.gz", _fasta(_contigs(rng, 3)))], K=21, C=3)
    return cases


def argv(case, names=None):
    """the arguments after `zot disass`"""
    o, d = case["opts"], DEFAULTS
    out = []
    for flag, key in (("-k", "K"), ("-c", "C"), ("-p", "P"), ("-q", "Q"), ("-S", "S")):
        if o[key] != d[key]:
            out += [flag, str(o[key])]
    if not o["both"]:
        out.append("-s")
    return out + list(names if names is not None else [fn for fn, _ in case["files"]])


def write_files(case, where):
    """the case's files under `where` -> their paths"""
    paths = []
    for fn, text in case["files"]:
        paths.append(os.path.join(where, fn))
        if fn.endswith(".gz"):
            with gzip.open(paths[-1], "wb") as f:
                f.write(text.encode())
        else:
            with open(paths[-1], "w") as f:
                f.write(text)
    return paths
