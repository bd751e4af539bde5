"""The inputs of the `zot hgvs-find` fixtures (tests/golden/h1_hgvsfind.json): index entries cut from a random "chromosome" of
about 2 kb and read pairs of 100 bases drawn from its wild-type and mutated haplotypes, by a seeded generator, so that the
fixture holds only the reference's outputs.  Read by tests/golden/make_golden_hgvsfind.py and by the tests.  A case: name,
opts (the command's options, a list of words), index (the list of dicts the reference's -X writes: hgvs, lhsFlank, rhsFlank,
wtSeq, mutSeq), inputs (FASTQ texts, mate 1 and mate 2 of each file pair in turn; file i is written as 'in<i>.fastq')."""
import random

_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N", "a": "t", "c": "g", "g": "c", "t": "a", "n": "n"}


def rc(s):
    return "".join(_COMP[c] for c in reversed(s))


def entry(chrom, hgvs, s, e, mut, W=75):
    """the index entry of a variant that replaces chrom[s:e] by mut (None: not spelled out), with flanks of W bases"""
    return {"hgvs": hgvs, "lhsFlank": chrom[max(0, s - W):s], "rhsFlank": chrom[e:e + W], "wtSeq": chrom[s:e], "mutSeq": mut}


def apply(chrom, edits):
    """the haplotype with every (s, e, seq) of edits applied (they do not overlap)"""
    for s, e, seq in sorted(edits, reverse=True):
        chrom = chrom[:s] + seq + chrom[e:]
    return chrom


def fastq(rng, seqs, name):
    out = []
    for i, s in enumerate(seqs):
        q = "".join(rng.choice("#5?FIJ") for _ in s)
        out.append("@%s\n%s\n+\n%s\n" % (name(i), s, q))
    return "".join(out)


def pairs(rng, haps, n, lo, hi, L=100, err=0.0):
    """n read pairs of L bases from fragments of 180-320 bases that start in [lo, hi) of a haplotype of haps, drawn in turn;
    every other pair comes from the reverse strand; err: the rate of substituted bases"""
    m1, m2 = [], []
    for i in range(n):
        h = haps[i % len(haps)]
        st = rng.randrange(lo, hi)
        frag = h[st:st + rng.randrange(180, 321)]
        if (i // len(haps)) % 2:
            frag = rc(frag)
        a, b = frag[:L], rc(frag[-L:])
        if err:
            a, b = ("".join(rng.choice([x for x in "ACGT" if x != c]) if rng.random() < err else c for c in s) for s in (a, b))
        m1.append(a)
        m2.append(b)
    return m1, m2


def files(rng, m1, m2, tag="p"):
    return [fastq(rng, m1, lambda i: "%s%d/1" % (tag, i)), fastq(rng, m2, lambda i: "%s%d/2" % (tag, i))]


def make_cases():
    rng = random.Random(20261020)

    def rnd(n):
        return "".join(rng.choice("ACGT") for _ in range(n))

    def other(c):
        return rng.choice([x for x in "ACGT" if x != c])

    cases = []

    def add(name, opts, index, inputs):
        cases.append(dict(name=name, opts=opts, index=index, inputs=inputs))

    # ---- one chromosome, one variant per case -----------------------------------------------------------------------------
    C = rnd(2000)
    p = 1000
    alt = other(C[p])
    sub = entry(C, "chr1:g.%d%s>%s" % (p + 1, C[p], alt), p, p + 1, alt)
    hap_sub = apply(C, [(p, p + 1, alt)])
    add("het_sub", [], [sub], files(rng, *pairs(rng, [C, hap_sub], 240, 650, 1100)))
    add("wt_only", [], [sub], files(rng, *pairs(rng, [C], 160, 650, 1100)))
    add("uncovered", [], [sub], files(rng, *pairs(rng, [C], 100, 0, 300)))

    dl = entry(C, "chr1:g.%d_%ddel" % (p + 1, p + 7), p, p + 7, "")
    add("hom_del7", [], [dl], files(rng, *pairs(rng, [apply(C, [(p, p + 7, "")])], 200, 650, 1100)))

    ins = rnd(12)
    i12 = entry(C, "chr1:g.%d_%dins%s" % (p, p + 1, ins), p, p, ins)
    hap_ins = apply(C, [(p, p, ins)])
    add("het_ins12", [], [i12], files(rng, *pairs(rng, [C, hap_ins], 260, 650, 1100)))

    dseq = rnd(5)
    di = entry(C, "chr1:g.%d_%ddelins%s" % (p + 1, p + 9, dseq), p, p + 9, dseq)
    add("het_delins", [], [di], files(rng, *pairs(rng, [C, apply(C, [(p, p + 9, dseq)])], 260, 650, 1100)))

    # dup and inv are only index entries for scanning: mutSeq is spelled out
    dup = entry(C, "chr1:g.%d_%ddup" % (p + 1, p + 6), p, p + 6, C[p:p + 6] * 2)
    inv = entry(C, "chr1:g.%d_%dinv" % (p + 301, p + 310), p + 300, p + 310, rc(C[p + 300:p + 310]))
    rpt = entry(C, "chr1:g.%d_%d[3]" % (p + 501, p + 502), p + 500, p + 502, C[p + 500:p + 502] * 3)
    haps = [C, apply(C, [(p, p + 6, C[p:p + 6] * 2), (p + 300, p + 310, rc(C[p + 300:p + 310]))])]
    add("dup_inv_repeat", [], [dup, inv, rpt], files(rng, *pairs(rng, haps, 300, 600, 1450)))

    alu = entry(C, "chr1:g.%d_%dinsALU" % (p, p + 1), p, p, None)
    add("ins_alu", [], [alu], files(rng, *pairs(rng, [C], 160, 650, 1100)))

    # anonymous variants: the alleles are bridged between anchors in the flanks
    an_i = entry(C, "chr1:g.%d_%dins12" % (p, p + 1), p, p, None)
    add("anon_ins12", [], [an_i], files(rng, *pairs(rng, [C, hap_ins], 260, 650, 1100)))
    d8 = rnd(8)
    an_d = entry(C, "chr1:g.%d_%ddelins8" % (p + 1, p + 5), p, p + 5, None)
    add("anon_delins8", [], [an_d], files(rng, *pairs(rng, [C, apply(C, [(p, p + 5, d8)])], 260, 650, 1100)))

    # two variants 40 bases apart: pairs hit two baits
    q = p + 40
    alt2 = other(C[q])
    sub2 = entry(C, "chr1:g.%d%s>%s" % (q + 1, C[q], alt2), q, q + 1, alt2)
    two = [C, apply(C, [(p, p + 1, alt), (q, q + 1, alt2)])]
    m_two = pairs(rng, two, 260, 650, 1150)
    add("two_close", [], [sub, sub2], files(rng, *m_two))

    # substitution errors put Hamming neighbours into the candidate sets
    m_err = pairs(rng, [C, hap_sub], 300, 650, 1100, err=0.02)
    f_err = files(rng, *m_err)
    for D in (1, 2, 3):
        add("errors_D%d" % D, ["-D", str(D)], [sub, i12], f_err)

    # flanks shorter than K - 1
    short = entry(C, sub["hgvs"], p, p + 1, alt, W=20)
    add("flanks20", [], [short], files(rng, *pairs(rng, [C, hap_sub], 240, 650, 1100)))

    # mates with N, lower case and lines shorter than K
    m1, m2 = pairs(rng, [C, hap_sub], 240, 650, 1100)
    for i in range(len(m1)):
        if i % 5 == 0:
            j = rng.randrange(len(m1[i]))
            m1[i] = m1[i][:j] + "N" + m1[i][j + 1:]
        if i % 7 == 0:
            m2[i] = m2[i].lower()
        if i % 11 == 0:
            m1[i] = m1[i][:rng.randrange(0, 25)]
        if i % 13 == 0:
            m2[i] = "N".join(m2[i][k:k + 24] for k in range(0, len(m2[i]), 25))
    add("ragged_mates", [], [sub], files(rng, m1, m2))

    # other K, thresholds and formats
    f_het = files(rng, *pairs(rng, [C, hap_sub, C], 300, 650, 1100))
    add("k21", ["-k", "21"], [sub, dl], f_het)
    add("k31", ["-k", "31"], [sub, dl], f_het)
    add("C5_V03", ["-C", "5", "-V", "0.3"], [sub, dl], f_het)
    add("F_all", ["-F", "ks,binom,rds,vaf"], [sub, dl, i12, an_i], f_het)
    add("F_none", ["-F", "none"], [sub, dl], f_het)

    # two file pairs
    add("two_file_pairs", [], [sub, sub2], files(rng, *pairs(rng, two, 130, 650, 1150)) + files(rng, *pairs(rng, two, 140, 650, 1150), tag="s"))
    return cases
