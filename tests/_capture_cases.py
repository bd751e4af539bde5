"""The inputs of the `zot capture` fixtures (tests/golden/c1_capture.json): bait FASTA and FASTQ texts built by a seeded
generator, so that the fixture holds only the reference's outputs.  Read by tests/golden/make_golden_capture.py and
by the tests."""
import random


def rc(s):
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def make_cases():
    rng = random.Random(20261015)
    g = "".join(rng.choice("ACGT") for _ in range(3000))
    baits = [("b0", g[0:400]), ("b1", g[300:700]), ("b2", g[1000:1300]),
             ("nohit", "".join(rng.choice("ACGT") for _ in range(300))),
             ("geneB desc", g[2000:2400]),
             ("polyA", "A" * 12 + g[2500:2600])]

    def fasta(bs, width=60):
        out = []
        for nm, s in bs:
            out.append(">%s\n" % nm)
            out.extend(s[i:i + width] + "\n" for i in range(0, len(s), width))
        return "".join(out)

    def read_seq(i):
        kind = i % 10
        if kind == 7:        # short
            return g[rng.randrange(0, 2900):][:rng.randrange(5, 25)]
        p = rng.randrange(0, 2900)
        s = g[p:p + 100]
        if kind in (1, 4):   # the other strand: hits only through the bait's reverse complement
            s = rc(s)
        if kind == 2:        # an N somewhere
            j = rng.randrange(len(s))
            s = s[:j] + "N" + s[j + 1:]
        if kind == 3:
            s = s.lower()
        if kind == 5:        # unrelated
            s = "".join(rng.choice("ACGT") for _ in range(100))
        if kind == 6:        # 13 A's then a bait 12-mer (hits with -k 12), or a bait 25-mer after the polyA run (-k 31)
            s = "A" * 13 + g[1000 + rng.randrange(0, 280):][:12] + g[2500 + rng.randrange(0, 60):][:40]
        return s

    def fastq(n, name=lambda i: "r%d" % i, eol="\n", seqs=None):
        out = []
        for i in range(n):
            s = seqs[i] if seqs else read_seq(i)
            q = "".join(rng.choice("!#5?ACGTIJ") for _ in s)
            out.append("@%s%s%s%s+%s%s%s" % (name(i), eol, s, eol, eol, q, eol))
        return "".join(out)

    bfa = fasta(baits)
    single = fastq(300, name=lambda i: "read%d extra words" % i)
    cases = [dict(name="k24", k=24, baits=bfa, inputs=[single]),
             dict(name="k25", k=25, baits=bfa, inputs=[single]),
             dict(name="k12", k=12, baits=bfa, inputs=[single]),
             dict(name="k31", k=31, baits=bfa, inputs=[single]),
             dict(name="crlf", k=25, baits=bfa.replace("\n", "\r\n"), inputs=[fastq(120, eol="\r\n")]),
             dict(name="two_files", k=24, baits=bfa, inputs=[fastq(150), fastq(150, name=lambda i: "second.%d" % i)])]
    m1 = [read_seq(i) for i in range(200)]
    m2 = [rc(g[(j * 13) % 2800:][:90]) if j % 3 else read_seq(j) for j in range(200)]
    cases.append(dict(name="paired", k=25, paired=True, baits=bfa,
                      inputs=[fastq(200, name=lambda i: "frag%d/1" % i, seqs=m1),
                              fastq(200, name=lambda i: "fragment_%d_with_a_longer_name/2" % i, seqs=m2)]))
    return cases
