#!/usr/bin/env python3
"""
Capture golden vectors of `zot spikein` from the reference's spikein (drtconway/zotmer at /root/reference).

Runs ONLY in the development container, by the recipe of tests/golden/make_golden_hgvsindex.py: the reference's own
commands/spikein.py, with the library modules it imports, is copied to a throw-away directory under /tmp and passed through
the stdlib's lib2to3; docopt is stubbed (the options the reference's docopt would give are made from the case's option words
and the defaults of the usage text), and so is tqdm.  What Python 3 no longer has is put back without touching the logic:
a `cmp` for library/hgvs.py and an ordering of its variants from their __cmp__; openFile becomes a text-mode (gzip) open.
The command is driven in-process from a directory that holds the toy genome of tests/_spikein_cases.py as chr*.fa.gz (-g .).
ReadMaker.prepareAllele is wrapped so that every allele the reference prepares is recorded.

What is committed is data only: tests/golden/s1_spikein.json holds, per case, the option words, the sequences the reference
drew for the anonymous variants, per zone and variant list the variants in the list, the reference's sourceRange and its
flattened allele, and the first 25 record pairs the reference wrote (-e 0.02 so that errors occur).  An allele is the toy
chromosome but for a stretch around the zone's variants, and is stored so: "keep" bases of the chromosome's start, then
"middle", then its last "tail" bases (tests/_spikein_cases.py::golden_allele puts it together again); the chromosomes
themselves are made at test time and not committed.  The reference's random
numbers are Python's: the records are data for the checker, not something this project reproduces.

Usage:  python3 tests/golden/make_golden_spikein.py        (rewrites tests/golden/s1_spikein.json)
"""
import importlib
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
WORK = "/tmp/zot3_spikein"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests._spikein_cases import GENOME, golden_allele, make_cases, write_genome  # noqa: E402

DEFAULTS = {"-b": None, "-d": "0.1", "-e": "0.005", "-f": None, "-g": ".", "-I": "300", "-l": None, "-L": "100", "-m": None, "-M": None,
            "-N": "1000000", "-S": None, "-z": False, "-v": False, "-V": "1.0"}


def build_derived():
    shutil.rmtree(WORK, ignore_errors=True)
    os.makedirs(WORK + "/stubs")
    shutil.copytree(REF + "/zotmer", WORK + "/zotmer")
    subprocess.check_call(["chmod", "-R", "u+w", WORK])
    mods = ("file", "misc", "hgvs", "rope", "align", "basics", "bits")
    files = [WORK + "/zotmer/library/%s.py" % m for m in mods] + [WORK + "/zotmer/commands/spikein.py"]
    subprocess.check_call([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n"] + files,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(WORK + "/stubs/docopt.py", "w") as f:
        f.write("_next = {}\n\ndef docopt(doc, argv=None, **kw):\n    return dict(_next)\n")
    with open(WORK + "/stubs/tqdm.py", "w") as f:
        f.write("def tqdm(*a, **kw):\n    raise RuntimeError('not used without -v')\n")
    sys.path.insert(0, WORK + "/stubs")
    sys.path.insert(0, WORK)


def open_text(fn, mode="r"):
    import gzip
    if fn.endswith(".gz"):
        return gzip.open(fn, mode + "t", encoding="latin-1")
    return open(fn, mode)


def cmp(a, b):
    """Python 2's cmp for the objects of library/hgvs.py"""
    if hasattr(a, "__cmp__"):
        return a.__cmp__(b)
    return (a > b) - (a < b)


PAIRS = 25


def pack_allele(ch, allele):
    """the flattened allele against its chromosome: the common start, what lies between, the common end"""
    seq = GENOME[ch]
    keep = 0
    while keep < min(len(seq), len(allele)) and seq[keep] == allele[keep]:
        keep += 1
    tail = 0
    while tail < min(len(seq), len(allele)) - keep and seq[len(seq) - 1 - tail] == allele[len(allele) - 1 - tail]:
        tail += 1
    rec = {"ch": ch, "keep": keep, "middle": allele[keep:len(allele) - tail], "tail": tail}
    assert golden_allele(rec) == allele
    return rec


def run_case(case, d):
    import docopt
    hgvs = importlib.import_module("zotmer.library.hgvs")
    hgvs.cmp = cmp
    hgvs.HGVS.__lt__ = lambda a, b: a.__cmp__(b) < 0
    mod = importlib.import_module("zotmer.commands.spikein")
    mod.openFile = open_text
    opts = dict(DEFAULTS)
    words = list(case["opts"])
    while words:
        o = words.pop(0)
        opts[o] = words.pop(0) if not isinstance(DEFAULTS[o], bool) else True
    with open(d + "/zones.bed", "w") as f:
        f.write(case["bed"])
    opts["-b"] = "zones.bed"
    if case["file"] is not None:
        with open(d + "/variants.txt", "w") as f:
            f.write(case["file"])
        opts["-f"] = "variants.txt"
    if case["pop"] is not None:
        with open(d + "/pop.txt", "w") as f:
            f.write(case["pop"])
        opts["-m"] = "pop.txt"
    opts.update({"<output-prefix>": "out", "<variant>": list(case["variants"])})
    docopt._next = opts

    alleles, anon = [], []
    prepare = mod.ReadMaker.prepareAllele

    def recording(self):
        prepare(self)
        seq = self.seq
        alleles.append(dict(pack_allele(self.chrom, str(seq[0:len(seq)])), zone=list(self.zone), variants=[str(v) for v in self.variants],
                            sourceRange=list(self.sourceRange)))
    mod.ReadMaker.prepareAllele = recording
    sets = {}
    for name in dir(hgvs):
        cls = getattr(hgvs, name)
        if isinstance(cls, type) and "setSequence" in cls.__dict__:
            sets[cls] = cls.setSequence

            def recording_set(self, seq, _orig=cls.setSequence):
                _orig(self, seq)
                anon.append([str(self), seq])
            cls.setSequence = recording_set
    cwd = os.getcwd()
    os.chdir(d)
    try:
        mod.main(["spikein"])
        r1, r2 = open("out_1.fastq").read(), open("out_2.fastq").read()
    finally:
        os.chdir(cwd)
        mod.ReadMaker.prepareAllele = prepare
        for cls, f in sets.items():
            cls.setSequence = f
    l1, l2 = r1.split("\n"), r2.split("\n")
    pairs = [[l1[i:i + 4], l2[i:i + 4]] for i in range(0, len(l1) - 1, 4)][:PAIRS]
    return {"name": case["name"], "opts": case["opts"], "anonymous": anon, "alleles": alleles, "pairs": pairs}


def main():
    build_derived()
    d = WORK + "/genome"
    write_genome(d)
    res = []
    for case in make_cases():
        r = run_case(case, d)
        res.append(r)
        print(case["name"], case["opts"], len(r["alleles"]), "alleles", len(r["pairs"]), "pairs")
    with open(os.path.join(HERE, "s1_spikein.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in res) + "\n]\n")


if __name__ == "__main__":
    main()
