"""The inputs of the `zot alu-finder` fixtures (tests/golden/a1_alufinder.json): chromosomes, BED regions and FASTQ texts built
by a seeded generator, so that the fixture holds only the reference's outputs.  Read by tests/golden/make_golden_alufinder.py
and by the tests.  Chromosome names (chrT, chrU) are ones the reference's hg19 <-> RefSeq table does not hold, so the
reference and the port agree on them by construction."""
import os
import random


def rc(s):
    return s[::-1].translate(str.maketrans("ACGTUacgtu", "TGCAAtgcaa"))


def make_cases():
    rng = random.Random(20261019)
    rand_seq = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    chrT, chrU = rand_seq(2000), rand_seq(900)
    ins = rand_seq(300)
    sample = chrT[:1000] + ins + chrT[1000:]               # the sequenced genome: chrT with 300 bases inserted after base 1000

    def pairs(genome, n, L=100, frag=(180, 320), err=0.0):
        m1, m2 = [], []
        for _ in range(n):
            f = rng.randrange(*frag)
            p = rng.randrange(0, len(genome) - f)
            fr = genome[p:p + f]
            if rng.random() < 0.5:
                fr = rc(fr)
            out = []
            for s in (fr[:L], rc(fr)[:L]):
                if err and rng.random() < err:
                    j = rng.randrange(len(s))
                    s = s[:j] + rng.choice("ACGTN") + s[j + 1:]
                out.append(s)
            m1.append(out[0])
            m2.append(out[1])
        return m1, m2

    def fastq(seqs, name="r%d", eol="\n", fill=0):
        out = []
        for i, s in enumerate(seqs):
            q = "".join(rng.choice("!#5?ACGTIJ") for _ in s)
            out.append("@%s%s%s%s%s+%s%s%s" % (name % i, " " + "x" * fill if fill else "", eol, s, eol, eol, q, eol))
        return "".join(out)

    def pair(genome, n, eol="\n", fill=0, **kw):
        m1, m2 = pairs(genome, n, **kw)
        return [fastq(m1, "frag%d/1", eol, fill), fastq(m2, "frag%d/2", eol, fill)]

    one_zone = "chrT\t301\t1700\tzoneA\n"
    two_zones = "track name=zones\nchrT\t301\t1700\tzoneA\nchrU\t101\t800\tzoneB\n"
    genomes = {"chrT": chrT, "chrU": chrU}
    base = dict(k=25, C=5, L=29, S=5, V=0.05, raw=False, bed=one_zone, genomes=genomes)
    cases = []
    reads = pair(sample, 1500, err=0.1)
    cases.append(dict(base, name="insertion", inputs=reads))
    cases.append(dict(base, name="insertion_raw", raw=True, inputs=reads))
    cases.append(dict(base, name="insertion_L60_S2", L=60, S=2, inputs=reads))
    cases.append(dict(base, name="insertion_two_zones_raw", raw=True, bed=two_zones, inputs=reads + pair(chrU, 200)))
    cases.append(dict(base, name="no_insertion", inputs=pair(chrT, 400)))                      # only the header
    cases.append(dict(base, name="too_thin", C=50, inputs=pair(sample, 200)))                  # only the header
    cases.append(dict(base, name="k15_raw", k=15, L=20, raw=True, inputs=pair(sample, 800)))
    # reads that carry one base more than the reference: the windows before it and after it lie on two diagonals of the zone
    extra = chrT[:900] + "G" + chrT[900:]
    cases.append(dict(base, name="one_base_more_raw", k=11, L=1, C=3, raw=True, inputs=pair(extra, 500, L=80, frag=(100, 200))))
    m1, m2 = pairs(sample, 600)
    m1 = [s.lower() if i % 3 == 0 else (s.replace("T", "U") if i % 3 == 1 else s.replace("T", "u")) for i, s in enumerate(m1)]
    m2 = [s + "  " if i % 2 else "\t" + s for i, s in enumerate(m2)]
    cases.append(dict(base, name="lower_U_blanks_crlf_raw", raw=True, C=3, inputs=[fastq(m1, eol="\r\n"), fastq(m2, eol="\r\n")]))
    m1, m2 = pairs(sample, 700)
    cases.append(dict(base, name="mate1_fewer_and_a_third_file", raw=True, C=3,
                      inputs=[fastq(m1[:450]), fastq(m2) + "@tail/2\nACGT", fastq(m1)]))
    # every mate file over two batches of 1 MiB: the read names are long
    cases.append(dict(base, name="batches", inputs=pair(sample, 1500, fill=1400)))
    # the six bases before the insertion come again after it: the two spurs meet only once they are shifted along the reference
    twice = chrT[:1000] + ins + chrT[994:]
    cases.append(dict(base, name="site_duplication", inputs=pair(twice, 1500)))
    cases.append(dict(base, name="site_duplication_S3", S=3, inputs=cases[-1]["inputs"]))
    return cases


def write_case(case, d):
    """the case's files under directory d -> the command's arguments (without its name)"""
    os.makedirs(d, exist_ok=True)
    for nm, seq in case["genomes"].items():
        with open(os.path.join(d, nm + ".fa"), "w") as f:
            f.write(">%s test chromosome\n" % nm)
            for i in range(0, len(seq), 70):
                f.write(seq[i:i + 70] + "\n")
    bed = os.path.join(d, "zones.bed")
    with open(bed, "w") as f:
        f.write(case["bed"])
    inputs = []
    for i, text in enumerate(case["inputs"]):
        p = os.path.join(d, "in%d.fastq" % i)
        with open(p, "w", newline="") as f:
            f.write(text)
        inputs.append(p)
    args = ["-k", str(case["k"]), "-g", d, "-C", str(case["C"]), "-L", str(case["L"]), "-S", str(case["S"]), "-V", repr(case["V"])]
    return args + (["-r"] if case["raw"] else []) + [bed] + inputs
