"""The inputs of the `zot strand` fixtures (tests/golden/s1_strand.json): FASTQ texts built by a seeded generator, so that
the fixture holds only the reference's outputs.  Read by tests/golden/make_golden_strand.py and by the tests."""
import random


def rc(s):
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def make_cases():
    rng = random.Random(20261017)
    g = "".join(rng.choice("ACGT") for _ in range(2000))

    def pair_seqs(n, L=100, frag=(150, 300), n_rate=0.1):
        """n read pairs from fragments of the genome in both orientations: mate 1 reads into the fragment from its start,
        mate 2 from its end on the other strand; a tenth of the reads carry an N"""
        m1, m2 = [], []
        for _ in range(n):
            f = rng.randrange(*frag)
            p = rng.randrange(0, len(g) - f)
            fr = g[p:p + f]
            if rng.random() < 0.5:
                fr = rc(fr)
            a, b = fr[:L], rc(fr)[:L]
            out = []
            for s in (a, b):
                if rng.random() < n_rate:
                    j = rng.randrange(len(s))
                    s = s[:j] + "N" + s[j + 1:]
                out.append(s)
            m1.append(out[0])
            m2.append(out[1])
        return m1, m2

    def fastq(seqs, name="r%d", eol="\n"):
        out = []
        for i, s in enumerate(seqs):
            q = "".join(rng.choice("!#5?ACGTIJ") for _ in s)
            out.append("@%s%s%s%s+%s%s%s" % (name % i, eol, s, eol, eol, q, eol))
        return "".join(out)

    def pair(n, eol="\n", **kw):
        m1, m2 = pair_seqs(n, **kw)
        return [fastq(m1, "frag%d/1", eol), fastq(m2, "frag%d/2", eol)]

    cases = [dict(name="k25_p0.1", k=25, p=0.1, inputs=pair(300)),
             dict(name="k25_p1", k=25, p=1.0, inputs=pair(60)),
             dict(name="k31_p0.3", k=31, p=0.3, inputs=pair(80)),
             dict(name="k6_p1", k=6, p=1.0, inputs=pair(40, L=60)),
             dict(name="k4_p0.5", k=4, p=0.5, inputs=pair(30, L=40))]
    m1, m2 = pair_seqs(60)
    m1 = [s.lower() if i % 3 == 0 else (s.replace("T", "U") if i % 3 == 1 else s.replace("T", "u")) for i, s in enumerate(m1)]
    m2 = [s.replace("t", "u").lower() if i % 2 else s.replace("T", "U") for i, s in enumerate(m2)]
    cases.append(dict(name="lower_and_U", k=12, p=1.0, inputs=[fastq(m1), fastq(m2)]))
    m1, m2 = pair_seqs(60)
    m1 = [s[:rng.randrange(0, 24)] if i % 4 == 0 else s for i, s in enumerate(m1)]
    m2 = [s[:rng.randrange(0, 24)] if i % 5 == 0 else s[:rng.randrange(24, 100)] for i, s in enumerate(m2)]
    cases.append(dict(name="short_reads", k=24, p=1.0, inputs=[fastq(m1), fastq(m2)]))
    m1, m2 = pair_seqs(80)
    cases.append(dict(name="mate2_fewer", k=25, p=0.5, inputs=[fastq(m1), fastq(m2[:55])]))
    m1, m2 = pair_seqs(50)
    cases.append(dict(name="mate1_fewer", k=25, p=0.5, inputs=[fastq(m1[:31]), fastq(m2)]))
    m1, m2 = pair_seqs(50)
    cases.append(dict(name="incomplete_record", k=25, p=1.0,
                      inputs=[fastq(m1) + "@tail/1\nACGTACGTACGTACGTACGTACGTACGTACGT\n+\n", fastq(m2) + "@tail/2\nACGTTGCA"]))
    cases.append(dict(name="crlf", k=25, p=1.0, inputs=pair(40, eol="\r\n")))
    cases.append(dict(name="two_pairs", k=25, p=0.3, inputs=pair(70) + pair(50)))
    return cases
