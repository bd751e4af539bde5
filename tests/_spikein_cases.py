"""
Toy inputs of `zot spikein`: a genome of two chromosomes made with zotmer_amd.synth, with lower-case stretches and runs of N;
BED files with several zones, one at a chromosome's start (the u = fl clamp), one at its end (the u = G - fl clamp), an
unnamed zone and a `track` line; and variants of every kind but insALU, spelled from the genome so that they are true.
"""
import gzip
import os

import numpy as np

from zotmer_amd import synth

SEED = 20261020
SIZES = {"chrA": 8192, "chrB": 4096}
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def genome():
    out = {}
    for n, (name, size) in enumerate(sorted(SIZES.items())):
        b = synth.rnd(SEED + n, 1, np.arange(size, dtype=np.uint64)) & np.uint64(3)
        s = np.frombuffer(b"ACGT", dtype=np.uint8)[b.astype(np.intp)].tobytes().decode()
        s = s[:600] + s[600:760].lower() + s[760:]                    # a soft-masked stretch inside the first zones
        s = s[:2500] + "N" * 40 + s[2540:]                            # a run of N
        s = s[:size - 150] + s[size - 150:size - 90].lower() + s[size - 90:]
        out[name] = s
    return out


GENOME = genome()


def golden_allele(rec):
    """an allele of tests/golden/s1_spikein.json: the chromosome's first `keep` bases, `middle`, its last `tail` bases"""
    seq = GENOME[rec["ch"]]
    return seq[:rec["keep"]] + rec["middle"] + seq[len(seq) - rec["tail"]:]


def write_genome(d, gz=True):
    os.makedirs(d, exist_ok=True)
    for name, s in GENOME.items():
        text = ">%s toy\n" % name + "".join(s[i:i + 70] + "\n" for i in range(0, len(s), 70))
        if gz:
            with gzip.open(os.path.join(d, name + ".fa.gz"), "wt") as f:
                f.write(text)
        else:
            with open(os.path.join(d, name + ".fa"), "w") as f:
                f.write(text)


BED = ("track name=toy\n"
       "chrA\t1000\t1400\tmid1\n"
       "chrA\t5\t300\tstart\n"
       "chrA\t2400\t2700\n"
       "chrA\t3000\t3600\tmid2\n"
       "chrA\t7900\t8192\tend\n"
       "chrB\t1500\t2100\tother\n"
       "chrB\t3000\t3300\tlate\n")
BED_SMALL = "chrA\t1000\t1400\tmid1\nchrB\t1500\t2100\tother\n"


def _ref(ch, a, b):
    """bases a .. b (1-based, inclusive), upper-cased"""
    return GENOME[ch][a - 1:b].upper()


def _sub(ch, p):
    c = _ref(ch, p, p)
    return "%s:g.%d%s>%s" % (ch, p, c, _COMP[c])


def variants_all_kinds():
    return [_sub("chrA", 1100),
            "chrA:g.1200_1211del",
            "chrA:g.1300_1304dup",
            "chrA:g.150_151insACGTTGCA",
            "chrA:g.3100_3101ins9",
            "chrA:g.3200_3207inv",
            "chrA:g.3300_3303delinsTT",
            "chrA:g.3400_3405delins4",
            "chrA:g.8000_8002%s[3]" % _ref("chrA", 8000, 8002),
            "chrA:g.2450del%s" % _ref("chrA", 2450, 2450),
            _sub("chrB", 1800),
            "chrB:g.3100_3149del"]


# the round trip hgvs-index -> spikein -> hgvs-find: one zone, about 200-fold coverage of a variant in its middle
ROUND_ZONE = "chrA\t1000\t1400\tmid1\n"
ROUND_N = 600
ROUND_VARIANTS = {"sub": _sub("chrA", 1250), "del": "chrA:g.1250_1261del"}


def make_cases():
    """name, opts (option words without -b -g -f -m, which the runner adds), bed, variants, file, pop"""
    kinds = variants_all_kinds()
    return [
        dict(name="sub", opts=["-S", "1", "-N", "100", "-e", "0.02", "-V", "0.5"], bed=BED, variants=[_sub("chrA", 1100)], file=None, pop=None),
        dict(name="kinds", opts=["-S", "2", "-N", "100", "-e", "0.02", "-V", "0.7"], bed=BED, variants=kinds[:6], file="\n".join(kinds[6:]) + "\n",
             pop=None),
        dict(name="short", opts=["-S", "3", "-N", "100", "-e", "0.02", "-L", "30", "-I", "80", "-d", "0.2"], bed=BED,
             variants=["chrA:g.1200_1211del", _sub("chrB", 1800)], file=None, pop=None),
        dict(name="pop", opts=["-S", "4", "-N", "100", "-e", "0.02", "-V", "0.5"], bed=BED_SMALL, variants=[_sub("chrA", 1100)], file=None,
             pop="1.0 %s\n0.0 %s\n0.5 %s\n1.0 %s\n0.5 chrB:g.1700_1703del\n" % (_sub("chrA", 1050), _sub("chrA", 1060), _sub("chrA", 1250),
                                                                               _sub("chrA", 1100))),
    ]


def case_numbers(case):
    """the numeric options of a case as keywords of the restatement's command()"""
    kw, words = {}, list(case["opts"])
    names = {"-S": ("seed", int), "-N": ("N", int), "-e": ("E", float), "-V": ("V", float), "-L": ("L", int), "-I": ("I", int), "-d": ("D", float)}
    while words:
        o = words.pop(0)
        k, f = names[o]
        kw[k] = f(words.pop(0))
    return kw


def all_variants(case):
    return list(case["variants"]) + (case["file"].split() if case["file"] else [])


def write_case(case, d):
    """the case's files under d -> the option words that name them"""
    words = []
    with open(os.path.join(d, "zones.bed"), "w") as f:
        f.write(case["bed"])
    words += ["-b", os.path.join(d, "zones.bed")]
    if case["file"] is not None:
        with open(os.path.join(d, "variants.txt"), "w") as f:
            f.write(case["file"])
        words += ["-f", os.path.join(d, "variants.txt")]
    if case["pop"] is not None:
        with open(os.path.join(d, "pop.txt"), "w") as f:
            f.write(case["pop"])
        words += ["-m", os.path.join(d, "pop.txt")]
    return words


# ---- builders of the device tests ----------------------------------------------------------------------------------------------
ALPHABET = np.frombuffer(b"ACGTACGTACGTacgtNn*-RyU.", dtype=np.uint8)      # upper and lower case, N, and bytes that are no base


def allele_text(seed, n):
    """n bytes of ALPHABET as a str (latin-1)"""
    return ALPHABET[(synth.rnd(seed, 1, np.arange(n, dtype=np.uint64)) % np.uint64(len(ALPHABET))).astype(np.intp)].tobytes().decode("latin-1")


def tables(zones, windows=None):
    """the restatement's zones [(head, pairs, [(text, s0, e0)] * 2)] as the arrays of zk_spike_pairs; windows: {(zone, allele):
    (lo, hi)} where the window is not the whole allele"""
    texts, rows, at = [], [], 0
    for zi, (head, n, als) in enumerate(zones):
        for ai, (text, s0, e0) in enumerate(als):
            lo, hi = (windows or {}).get((zi, ai), (0, len(text)))
            t = text[lo:hi].encode("latin-1")
            rows += [at, lo, len(t), len(text), s0, e0]
            texts.append(t)
            at += len(t)
    first = np.zeros(len(zones) + 1, dtype=np.uint64)
    first[1:] = np.cumsum([z[1] for z in zones])
    heads = [z[0].encode("latin-1") for z in zones]
    offs = np.zeros(len(zones) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(h) for h in heads])
    return (np.frombuffer(b"".join(texts), dtype=np.uint8), np.asarray(rows, dtype=np.int64).view(np.uint64), first,
            np.frombuffer(b"".join(heads), dtype=np.uint8), offs)
