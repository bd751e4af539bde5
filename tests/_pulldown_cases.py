"""The inputs of the `zot pulldown` fixtures (tests/golden/p1_pulldown.json): bait FASTA, -U FASTA and FASTQ texts built by a
seeded generator, so that the fixture holds only the reference's outputs.  Read by tests/golden/make_golden_pulldown.py and
by the tests.  A case: name, baits (FASTA text), up (FASTA text of -U, or None), inputs (FASTQ texts, mate 1 and mate 2 of
each file pair in turn; file i is written as 'in<i>.fastq' and given to the command under that relative name)."""
import random

from tests._capture_cases import make_cases as capture_cases, rc


def fastq(rng, seqs, name, eol="\n"):
    out = []
    for i, s in enumerate(seqs):
        q = "".join(rng.choice("!#5?ACGTIJ") for _ in s)
        out.append("@%s%s%s%s+%s%s%s" % (name(i), eol, s, eol, eol, q, eol))
    return "".join(out)


def edge_pairs(rng, e, V, V2):
    """[(what, mate 1, mate 2)]: each pair is the smallest input on which one rule of the walk can go wrong.  e: four
    unrelated 200-base baits; V, V2: the two -U sequences (V2 is given in the FASTA as its reverse complement only)."""
    def rnd(n):
        return "".join(rng.choice("ACGT") for _ in range(n))

    def ends_with(n, tail):          # n bases whose only window of a bait is the last one
        return rnd(n - len(tail)) + tail

    P = []
    # mate lengths: no window; one window; the last window is lane 63 of the first chunk of 64 window starts, lane 0 of the
    # second, lane 63 of the second, lane 0 of the third
    P.append(("len24", e[0][40:64], rnd(30)))
    P.append(("len25", e[0][40:65], rnd(30)))
    for n in (88, 89, 152, 153):
        P.append(("len%d" % n, ends_with(n, e[0][100:125]), rnd(30)))
        P.append(("len%d_mate2" % n, rnd(30), ends_with(n, e[1][100:125])))
    P.append(("both_short", rnd(24), rnd(10)))
    # window content
    P.append(("mate2_only", rnd(60), rnd(20) + e[2][30:70]))
    P.append(("reverse_strand", rc(e[3][50:90]), rnd(40)))
    s = e[0][10:35]
    P.append(("n_in_the_window", rnd(20) + s[:12] + "N" + s[13:] + rnd(20), rnd(40)))
    P.append(("lower_case", (rnd(10) + e[1][20:60]).lower(), rnd(40)))
    P.append(("three_baits", e[0][10:50] + e[1][10:50] + e[2][10:50], rnd(40)))
    P.append(("two_baits_over_both_mates", e[0][60:100], e[3][60:100]))
    # the veto (only the cases with -U see it)
    P.append(("veto_last_window_of_mate2", e[0][120:170], ends_with(70, V[5:30])))
    P.append(("veto_and_three_baits", e[0][10:50] + e[1][10:50] + e[2][10:50], rnd(10) + V[20:50] + rnd(10)))
    P.append(("veto_first_window_of_mate1", V[0:25] + rnd(30), e[2][100:140]))
    P.append(("veto_given_as_reverse_complement", rnd(15) + V2[3:33], e[1][140:180]))
    P.append(("veto_reverse_strand_of_the_read", rc(V[10:40]), e[3][100:140]))
    P.append(("no_hit", rnd(100), rnd(100)))
    return P


def make_cases():
    cap = {c["name"]: c for c in capture_cases()}["paired"]
    rng = random.Random(20261019)

    def rnd(n):
        return "".join(rng.choice("ACGT") for _ in range(n))

    def fasta(bs, eol="\n"):
        return "".join(">%s%s%s%s" % (nm, eol, s, eol) for nm, s in bs)

    cases = []
    bfa = cap["baits"]
    # `paired`: the capture fixture's 200 pairs and 6 baits, without and with -U (the first 60 bases of bait b2)
    b2 = "".join(bfa.split(">b2\n")[1].split(">")[0].split())
    cases.append(dict(name="paired", baits=bfa, up=None, inputs=cap["inputs"]))
    cases.append(dict(name="paired_U", baits=bfa, up=">up one\n%s\n" % b2[:60], inputs=cap["inputs"]))

    # `edges`: one pair per rule
    e = [rnd(200) for _ in range(4)]
    V, V2 = rnd(60), rnd(40)
    ebaits = fasta([("e0", e[0]), ("e1 with words", e[1]), ("e2", e[2]), ("e3", e[3])])
    eup = fasta([("v", V), ("v2 as its reverse complement", rc(V2))])
    P = edge_pairs(rng, e, V, V2)
    em = [fastq(rng, [p[1 + m] for p in P], lambda i, m=m: "%s/%d" % (P[i][0], m + 1)) for m in range(2)]
    cases.append(dict(name="edges", baits=ebaits, up=None, inputs=em))
    cases.append(dict(name="edges_U", baits=ebaits, up=eup, inputs=em))

    # `many`: 1500 baits of 28 bases that share one 25-mer, one pair that holds it and one that holds nothing
    S = rnd(25)
    many = []
    for i in range(1500):
        a = i % 4
        many.append(("m%d" % i, rnd(a) + S + rnd(3 - a)))
    mm = [fastq(rng, [rnd(30) + S + rnd(30), rnd(80)], lambda i: "p%d/1" % i), fastq(rng, [rnd(70), rnd(80)], lambda i: "p%d/2" % i)]
    cases.append(dict(name="many", baits=fasta(many), up=None, inputs=mm))

    # `unequal`: 5 records against 3, in both orders: three pairs
    u1 = [e[0][i * 20:i * 20 + 50] for i in range(5)]
    u2 = [e[1][i * 20:i * 20 + 50] for i in range(3)]
    f1, f2 = fastq(rng, u1, lambda i: "u%d/1" % i), fastq(rng, u2, lambda i: "u%d/2" % i)
    cases.append(dict(name="unequal_5_3", baits=ebaits, up=None, inputs=[f1, f2]))
    cases.append(dict(name="unequal_3_5", baits=ebaits, up=None, inputs=[f2, f1]))

    # `crlf`: CRLF line ends in every file
    cm = [fastq(rng, [p[1 + m] for p in P], lambda i, m=m: "c%d/%d" % (i, m + 1), eol="\r\n") for m in range(2)]
    cases.append(dict(name="crlf", baits=ebaits.replace("\n", "\r\n"), up=eup.replace("\n", "\r\n"), inputs=cm))

    # no baits at all: every pair that is not pushed up goes to row 0
    cases.append(dict(name="emptybaits_U", baits="", up=eup, inputs=em))
    cases.append(dict(name="emptyreads", baits=ebaits, up=None, inputs=["", ""]))

    # two file pairs, each also a case of its own
    second = []
    for m in range(2):
        seqs = [e[(i + m) % 4][(i * 7) % 150:][:rng.randrange(20, 50)] if i % 3 else rnd(60) for i in range(40)]
        second.append(fastq(rng, seqs, lambda i, m=m: "s%d/%d" % (i, m + 1)))
    cases.append(dict(name="second", baits=ebaits, up=eup, inputs=second))
    cases.append(dict(name="two_pairs", baits=ebaits, up=eup, inputs=em + second))
    return cases
