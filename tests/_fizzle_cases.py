"""The inputs of the `zot fizzle` tests: small seeded genomes with genes on both strands, the refGene table and gene lists that
-P reads, and read pairs of every kind (tests/golden/z1_fizzle.json holds what the reference's own functions make of them), and
builders for the device tests.  Everything is a pure function of its arguments."""
import gzip
import hashlib
import os
import random

from zotmer_amd import synth

FIXTURE_SEED = 25
SEG = 44                       # length of a segment shared between exons (at least K + 3 for every K)


def rc(s):
    return s[::-1].translate(str.maketrans("ACGTUacgtu", "TGCAAtgcaa"))


def digest(texts):
    h = hashlib.sha256()
    for t in texts:
        h.update(t.encode("latin-1"))
        h.update(b"\0")
    return h.hexdigest()[:16]


def fastq_text(seqs, name="r%d", eol="\n"):
    return "".join("@%s%s%s%s+%s%s%s" % (name % i, eol, s, eol, eol, "I" * len(s.strip()), eol) for i, s in enumerate(seqs))


class _Bases:
    """random bases from the project's counter-based generator (synth.read_strings), a fresh stretch at every call"""

    def __init__(self, seed):
        self.seed, self.at = seed, 0

    def __call__(self, n):
        reads = synth.read_strings(self.seed, self.at, (n + 99) // 100, 100)
        self.at += len(reads)
        return "".join(r if isinstance(r, str) else r.decode("latin-1") for r in reads)[:n]


def make_case(name, K, gen, n_pairs=120, L=60):
    """Three chromosomes of a few kilobases.  Genes GA (+), GB (-) on c1, GC (+), GD (-) on c2, and the one-exon genes TA, TB,
    TC (+) on c3, which share segments pairwise (S_ab, S_bc, S_ac) and no segment all three.  A duplicated segment D lies in
    GA/02, GC/01 and GD/02 (tuples of 2 and 3 exons come from it and from D2 in GA/03, GB/01); a copy of GB/02 lies in an
    intergenic stretch of c2 (-T reports it).  Parts of the chromosomes are lower case; an intron and GC/02 hold an N."""
    rng = random.Random(gen)
    bases = _Bases(gen)
    D, D2 = bases(SEG), bases(SEG)
    S_ab, S_bc, S_ac = bases(SEG), bases(SEG), bases(SEG)
    ex = lambda lo=90, hi=170: bases(rng.randrange(lo, hi))
    genes = {
        "GA": ("c1", "+", [ex(), ex(40, 60) + D + ex(40, 60), ex(40, 60) + D2 + ex(30, 50), ex()]),
        "GB": ("c1", "-", [ex(40, 60) + D2 + ex(40, 60), ex(), ex()]),
        "GC": ("c2", "+", [ex(30, 50) + D + ex(40, 60), ex(50, 70) + "N" + ex(50, 70)]),
        "GD": ("c2", "-", [ex(), ex(40, 60) + D + ex(40, 60), ex(100, 120)]),
        "TA": ("c3", "+", [bases(50) + S_ab + bases(31) + S_ac + bases(50)]),
        "TB": ("c3", "+", [bases(50) + S_ab + bases(31) + S_bc + bases(50)]),
        "TC": ("c3", "+", [bases(50) + S_bc + bases(31) + S_ac + bases(50)]),
    }
    chroms, where = {"c1": "", "c2": "", "c3": ""}, {}
    for g, (ch, st, exons) in genes.items():
        seq = chroms[ch] + bases(rng.randrange(150, 300)).lower()
        spots = []
        for e in (exons if st == "+" else [rc(e) for e in exons[::-1]]):
            spots.append((len(seq), len(seq) + len(e)))
            seq += e + bases(rng.randrange(40, 90))
        chroms[ch] = seq
        where[g] = spots
    chroms["c2"] += bases(120) + rc(genes["GB"][2][1]) + bases(200)          # GB/02 once more, outside every exon
    chroms["c1"] = chroms["c1"][:where["GA"][0][0] + 20] + chroms["c1"][where["GA"][0][0] + 20:where["GA"][0][0] + 50].lower() + \
        chroms["c1"][where["GA"][0][0] + 50:]
    gap = where["GB"][0][1] + 10
    chroms["c1"] = chroms["c1"][:gap] + "N" + chroms["c1"][gap + 1:]
    chroms["c3"] += bases(300)
    # the refGene table: bin name chrom strand txStart txEnd cdsStart cdsEnd exonCount exonStarts exonEnds score name2 ...
    lines = []

    def tx_line(tx, ch, st, spots, g):
        return "\t".join(["0", tx, ch, st, str(spots[0][0]), str(spots[-1][1]), str(spots[0][0]), str(spots[-1][1]), str(len(spots)),
                          "".join("%d," % s for s, _ in spots), "".join("%d," % e for _, e in spots), "0", g, "cmpl", "cmpl", "0,"])

    for n, (g, (ch, st, _)) in enumerate(genes.items()):
        lines.append(tx_line("NM_%04d" % (10 * n), ch, st, where[g], g))
    sp = where["GA"]
    lines.append(tx_line("NM_9001", "c1", "+", [sp[0], (sp[1][0] + 10, sp[1][1]), (sp[2][0], sp[2][1] - 7)], "GA"))     # merged away
    lines.append(tx_line("NM_9002", "c1", "+", [(sp[3][1], sp[3][1] + 25)], "GA"))                                      # touches GA/04
    lines.append(tx_line("NM_9003", "c2_hap1", "+", [(10, 90)], "GC"))                                                  # ignored
    lines.append(tx_line("NM_9004", "c3", "+", [(5, 60)], "GB"))                                                        # another chromosome
    lines.append(tx_line("NM_9005", "c3", "+", [(700, 760)], "GX"))                                                     # not listed
    ref_gene = "".join(l + "\n" for l in lines)
    gene_list = "".join("%s\n" % g for g in list(genes) + ["GNONE"])
    tx_list = "GA\tNM_0000\nGA\tNM_9001\nGB\tNM_0010\nGD\tNM_0030\nTA\tNM_0040 extra\nGQ\tNM_7777\n"
    # the read pairs
    tx = {g: "".join(e for e in exons).upper() for g, (_, _, exons) in genes.items()}
    exon_at = {g: [sum(len(e) for e in exons[:i]) for i in range(len(exons) + 1)] for g, (_, _, exons) in genes.items()}

    def mates(frag, flip):
        a, b = frag[:L], rc(frag[-L:])
        return (b, a) if flip else (a, b)

    def noisy(s, p=0.01):
        return "".join(rng.choice([c for c in "ACGT" if c != ch]) if rng.random() < p and ch in "ACGT" else ch for ch in s)

    pairs = []
    names = [g for g in genes if len(genes[g][2]) > 1]
    for i in range(n_pairs):
        kind, g = i % 6, names[rng.randrange(len(names))]
        flip = rng.random() < 0.5
        if kind in (0, 5):                               # inside one exon
            e = rng.randrange(len(genes[g][2]))
            lo, hi = exon_at[g][e], exon_at[g][e + 1]
            n = min(rng.randrange(L + 5, 2 * L + 30), hi - lo)
            p = rng.randrange(lo, hi - n + 1)
            m1, m2 = mates(noisy(tx[g][p:p + n]), flip)
        elif kind in (1, 2):                             # across a junction of one gene
            e = rng.randrange(1, len(genes[g][2]))
            j = exon_at[g][e]
            p = max(0, j - rng.randrange(15, L + 30))
            m1, m2 = mates(noisy(tx[g][p:p + 2 * L + 20]), flip)
        elif kind == 3:                                  # a fusion: the end of one transcript's exon, the start of another's
            h = names[rng.randrange(len(names))]
            j, j2 = exon_at[g][rng.randrange(1, len(genes[g][2]) + 1)], exon_at[h][rng.randrange(len(genes[h][2]))]
            m1, m2 = mates(noisy(tx[g][max(0, j - L - 10):j] + tx[h][j2:j2 + L + 10]), flip)
        else:                                            # dressed: N, lower case, U
            p = rng.randrange(0, max(1, len(tx[g]) - 2 * L))
            m1, m2 = mates(tx[g][p:p + 2 * L + 10], flip)
            m1 = (m1[:20] + "N" + m1[21:], m1.lower(), m1.replace("T", "U"), m1.replace("T", "u"))[(i // 6) % 4]
            m2 = (m2.lower(), m2[:33] + "n" + m2[34:], m2, "  " + m2 + "\t")[(i // 6) % 4]
        pairs.append((m1, m2))
    pairs.append((tx["GA"][:K - 1], tx["GA"][60:60 + L]))                   # a mate shorter than K
    pairs.append((tx["GB"][10:10 + L], ""))                                 # an empty sequence line
    pairs.append(("", ""))
    pairs.append((bases(L), bases(L)))                                      # hits nothing
    piece = lambda s, n: s[:K + n - 1]
    a_only = genes["TA"][2][0][:50]
    pairs.append((piece(S_ab, 3) + "N" + piece(S_ac, 2) + "N" + piece(S_bc, 1), bases(L)))                       # one round of step 4
    pairs.append((piece(S_ab, 4) + "N" + piece(S_bc, 3), rc(piece(S_ac, 3) + "N" + piece(a_only, 1))))           # two rounds
    pairs.append((rc(piece(S_ab, 2) + "N" + piece(S_bc, 2)), piece(S_ac, 2)))                                    # stays empty
    pairs.append((piece(S_ab, 2) + "N" + piece(S_bc, 2) + "N" + piece(S_ac, 2) + "N" + piece(D, 3), bases(L)))   # ... beside a component that answers
    return dict(name=name, K=K, chroms=chroms, gene_list=gene_list, tx_list=tx_list, ref_gene=ref_gene,
                reads=[fastq_text([p[0] for p in pairs], "p%d/1"), fastq_text([p[1] for p in pairs], "p%d/2")])


def fixture_cases():
    """[{name, K, chroms, gene_list, tx_list, ref_gene, reads}] in the fixture's order"""
    return [make_case("k25", 25, FIXTURE_SEED * 1000 + 1), make_case("k5", 5, FIXTURE_SEED * 1000 + 2, n_pairs=60),
            make_case("k32", 32, FIXTURE_SEED * 1000 + 3), make_case("k25_second", 25, FIXTURE_SEED * 1000 + 4),
            make_case("k12", 12, FIXTURE_SEED * 1000 + 5, n_pairs=90)]


def case_digests(case):
    return dict(chroms=digest([n + "\n" + s for n, s in sorted(case["chroms"].items())]), ref_gene=digest([case["ref_gene"]]),
                lists=digest([case["gene_list"], case["tx_list"]]), reads=digest(case["reads"]))


def write_case(case, d, bed=None):
    """the case's files under directory d (the chromosomes as <d>/home/<name>.fa.gz) -> their paths by name"""
    home = os.path.join(d, "home")
    os.makedirs(home, exist_ok=True)
    for nm, seq in case["chroms"].items():
        with gzip.open(os.path.join(home, nm + ".fa.gz"), "wt", newline="") as f:
            f.write(">%s a chromosome\n" % nm + "".join(seq[i:i + 70] + "\n" for i in range(0, len(seq), 70)) + ">other\nACGTACGT\n")
    paths = dict(home=home)
    texts = dict(gene_list=case["gene_list"], tx_list=case["tx_list"], ref_gene=case["ref_gene"], reads_1=case["reads"][0], reads_2=case["reads"][1])
    if bed is not None:
        texts["bed"] = bed
    for nm, text in texts.items():
        paths[nm] = os.path.join(d, nm + (".fastq" if nm.startswith("reads") else ".txt"))
        with open(paths[nm], "w", newline="") as f:
            f.write(text)
    return paths
