"""The inputs of the `zot hgvs-index` tests and of tests/golden/make_golden_hgvsindex.py: a seeded toy genome of 24
chromosomes and variant lists over it.  Nothing here is read from a file; the chromosomes are written at test time
(write_genome) and only the reference's outputs on them are committed (tests/golden/x1_hgvsindex.json).

The genome: chr1 .. chr22, chrX, chrY, 300 to 520 bases each, 60 columns a line unless said otherwise, some lines in lower
case.  chr2 holds a copy of 70 bases of chr1 (k-mers seen twice), chr3 a run of N, chr5 the 16-base palindrome
ACGTACGTACGTACGT, chr6 a Y; chr9 has CRLF line ends, chr10 a second record (never read), chr11 lines before its first header,
chr12 lines of 7 columns, chr13 no final line break, chrX is all lower case."""
import gzip
import os
import random

CHROMS = ["chr%d" % i for i in range(1, 23)] + ["chrX", "chrY"]
PALINDROME = "ACGTACGTACGTACGT"


def rnd(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def make_genome(seed=20):
    """-> ({name: sequence as the reference joins it}, {name: the text of <name>.fa})"""
    rng = random.Random(seed)
    seqs = {c: rnd(rng, 300 + 10 * i - (i % 3)) for i, c in enumerate(CHROMS)}
    s = seqs["chr2"]
    seqs["chr2"] = s[:100] + seqs["chr1"][200:270] + s[170:]
    s = seqs["chr3"]
    seqs["chr3"] = s[:120] + "N" * 40 + s[160:]
    s = seqs["chr5"]
    seqs["chr5"] = s[:150] + PALINDROME + s[166:]
    s = seqs["chr6"]
    seqs["chr6"] = s[:90] + "Y" + s[91:]
    seqs["chrX"] = seqs["chrX"].lower()
    texts = {}
    for c in CHROMS:
        width = 7 if c == "chr12" else 60
        eol = "\r\n" if c == "chr9" else "\n"
        lines = [seqs[c][i:i + width] for i in range(0, len(seqs[c]), width)]
        lines = [ln.lower() if rng.random() < 0.3 else ln for ln in lines]
        if c == "chr8":          # mixed case inside a line
            lines = ["".join(ch.lower() if rng.random() < 0.5 else ch for ch in ln) for ln in lines]
        seqs[c] = "".join(lines)
        t = ">%s toy chromosome%s" % (c, eol) + eol.join(lines) + eol
        if c == "chr10":
            t += ">%s_second%s%s%s" % (c, eol, rnd(rng, 90), eol)
        if c == "chr11":
            t = "; a line before the header%sACGTACGTACGTACGTACGTACGTACGTACGT%s" % (eol, eol) + t
        if c == "chr13":
            t = t[:-1]
        texts[c] = t
    return seqs, texts


def write_genome(directory, texts=None):
    """<directory>/<name>.fa.gz for every chromosome"""
    texts = texts if texts is not None else make_genome()[1]
    os.makedirs(directory, exist_ok=True)
    for c, t in texts.items():
        with gzip.GzipFile(os.path.join(directory, c + ".fa.gz"), "wb", mtime=0) as f:
            f.write(t.encode("latin-1"))


def names_text():
    """an -n file: one RefSeq accession for chr7, and a made-up accession per other chromosome so that -T scans all 24"""
    return "# accession  file stem\nNC_000007.13\tchr7\n" + "".join("toy_%s  %s\n" % (c[3:], c) for c in CHROMS if c != "chr7")


def make_cases(seed=20):
    """[{name, opts: the option words but -g / -n / -f, variants: the words on the command line, file: the text of an -f file or
    None, names: the text of an -n file or None}]"""
    seqs, _ = make_genome(seed)
    n4 = len(seqs["chr4"])
    kinds = [
        "chr1:g.230A>T",                 # inside the stretch chr2 repeats
        "chr1:g.40_44del", "chr1:g.50delA", "chr1:g.60_62delACG",       # a del prints without its bases
        "chr2:g.30dup", "chr2:g.40_45dup", "chr2:g.50_52dupACG",
        "chr3:g.200_201insACGTT", "chr3:g.198_205insGG",                # only the second position counts
        "chr3:g.210_211ins12", "chr3:g.220_221insALU",
        "chr4:g.100_130inv", "chr4:g.140_141invAC",
        "chr5:g.152delinsTT", "chr5:g.140_170delinsACGTACGT", "chr5:g.155_160delins7", "chr5:g.158delins3",
        "chr6:g.91A>G",                  # the reference holds a Y there
        "chr6:g.200_202[4]", "chr6:g.210[3]", "chr6:g.220ACG[2]", "chr6:g.230_232ACG[5]",
        "chr3:g.130A>C", "chr3:g.119_121del",                           # on and beside the N run
        "chr4:g.1A>C", "chr4:g.1_2insT", "chr4:g.%dC>A" % n4, "chr4:g.%d_%ddel" % (n4 - 3, n4),      # the ends: an empty flank
        "chr4:g.20_30del", "chr4:g.20_30del",                           # said twice
        "chr1:g.230A>T",                 # ... and twice with other variants in between
        "chr1:g.12_15A>T", "chr1:g.5ins7", "chr1:c.5A>T", "nonsense",   # unparsable
        "chrX:g.100_110inv", "chr9:g.150_155dup", "chr12:g.77_80del", "chr13:g.%dA>T" % len(seqs["chr13"]),
    ]
    cases = [dict(name="kinds_k25", opts=[], variants=kinds, file=None, names=None)]
    cases.append(dict(name="names_k16", opts=["-k", "16", "-w", "20"],
                      variants=["NC_000007.13:g.100A>G", "chr7:g.100A>G", "chr5:g.149_150insGATTACA", "chr5:g.151_166del"],
                      file="chr5:g.158T>A\n  chr5:g.158_159insAC chr2:g.120_140inv\n\nNC_000007.13:g.50_60del oops:g.1\n", names=names_text()))
    cases.append(dict(name="k1_w3", opts=["-k", "1", "-w", "3", "-W", "9"],
                      variants=["chr1:g.10A>C", "chr1:g.11_12insNN", "chr1:g.11_12insGG", "chr2:g.1del", "chr3:g.130_131dup"], file=None, names=None))
    cases.append(dict(name="k32_w5", opts=["-k", "32", "-w", "5"],
                      variants=["chr1:g.230_262inv", "chr2:g.130_131insA", "chr5:g.151_166[3]", "chr5:g.120_200delins40"], file=None, names=None))
    cases.append(dict(name="nothing_parses", opts=["-k", "8"], variants=["chr1:5A>T", "chr1:g.A>T"], file=None, names=None))
    return cases
