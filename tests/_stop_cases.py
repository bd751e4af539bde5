"""The inputs of the `zot stop` tests: the seeded transcripts and reads of the fixture (tests/golden/s1_stop.json holds the lines the
reference's main prints on them) and small builders for the device tests.  Everything is a pure function of its arguments."""
import hashlib
import os
import random

FIXTURE_SEED = 24


def rc(s):
    return s[::-1].translate(str.maketrans("ACGTUacgtu", "TGCAAtgcaa"))


def digest(texts):
    h = hashlib.sha256()
    for t in texts:
        h.update(t.encode("latin-1"))
        h.update(b"\0")
    return h.hexdigest()[:16]


def fasta_text(records, width=60):
    out = []
    for nm, seq in records:
        out.append(">" + nm + "\n")
        out.extend(seq[i:i + width] + "\n" for i in range(0, len(seq), width))
    return "".join(out)


def fastq_text(seqs, name="r%d", eol="\n"):
    return "".join("@%s%s%s%s+%s%s%s" % (name % i, eol, s, eol, eol, "I" * len(s.strip()), eol) for i, s in enumerate(seqs))


def make_case(name, K, gen, n_tx=3, tx_len=400, n_reads=200, read_len=80, sub=0.01, S=17, isoform=False, repeat=0, tail=0, files=1,
              dress=False):
    """Transcripts of random bases cut from a `genome` with flanks, so that reads overhang their ends; reads cut from the
    genome in either orientation with substitutions.  isoform: the last transcript is the first one with a piece left out (a read
    across the first one's piece has two frames).  repeat: a tandem repeat of that many copies of a 7-mer inside transcript 0.
    tail: that many A at the end of every transcript (and 4 on the second: not cut).  dress: lower case, U, N, blanks and \\r."""
    rng = random.Random(gen)
    rand_seq = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    flank = 10
    genomes, records = [], []
    for t in range(n_tx):
        body = rand_seq(tx_len + 17 * t)
        if t == 0 and repeat:
            unit = rand_seq(7)
            body = body[:100] + unit * repeat + body[100:]
        if body.endswith("A"):
            body = body[:-1] + "C"
        genomes.append(rand_seq(flank) + body + rand_seq(flank))
        records.append(["tx%02d some text" % ((7 * t + 3) % 31) if dress else "T%d" % ((7 * t + 3) % 31), body])
    if isoform:
        body = records[0][1]
        records.append(["T_iso", body[:150] + body[210:]])
        genomes.append(rand_seq(flank) + records[-1][1] + rand_seq(flank))
    if tail:
        for i, r in enumerate(records):
            r[1] += "A" * (4 if i == 1 else tail)
    reads = []
    for i in range(n_reads):
        g = genomes[rng.randrange(len(genomes))]
        p = rng.randrange(0, len(g) - read_len + 1)
        s = list(g[p:p + read_len])
        for j in range(len(s)):
            if rng.random() < sub:
                s[j] = rng.choice([c for c in "ACGT" if c != s[j]])
        s = "".join(s)
        if rng.random() < 0.5:
            s = rc(s)
        if i % 11 == 10:
            s = rand_seq(read_len)                      # a read that hits nothing
        if dress:
            k = i % 6
            s = (s.lower(), s.replace("T", "U"), s[:30] + "N" + s[31:], "  " + s + "\t", s, s.replace("T", "u"))[k]
        reads.append(s)
    if dress:
        records[0][1] = records[0][1][:50].lower() + records[0][1][50:]
        records[-1][1] = records[-1][1][:200] + "N" + records[-1][1][201:]
    eol = "\r\n" if dress else "\n"
    cut = [len(reads) * f // files for f in range(files + 1)]
    inputs = [fastq_text(reads[a:b], "q%d", eol) for a, b in zip(cut, cut[1:])]
    return dict(name=name, K=K, S=S, fasta=fasta_text([tuple(r) for r in records]), inputs=inputs)


def fixture_cases():
    """[{name, K, S, fasta, inputs}] in the fixture's order"""
    cases = []
    n = 0
    for K in (15, 21, 24, 25, 27, 30, 31, 32):
        for kind in range(4):
            n += 1
            kw = [dict(), dict(isoform=True, S=5 + n), dict(repeat=12, tail=8, files=2), dict(dress=True, isoform=True, tail=6, sub=0.015)][kind]
            cases.append(make_case("k%d_%s" % (K, ("plain", "isoform", "repeat_tail_two_files", "dressed")[kind]), K,
                                   FIXTURE_SEED * 1000 + n, **kw))
    return cases


def write_case(case, d):
    """the case's files under directory d -> the command's arguments (without its name)"""
    os.makedirs(d, exist_ok=True)
    fa = os.path.join(d, "tx.fa")
    with open(fa, "w", newline="") as f:
        f.write(case["fasta"])
    inputs = []
    for i, text in enumerate(case["inputs"]):
        p = os.path.join(d, "in%d.fastq" % i)
        with open(p, "w", newline="") as f:
            f.write(text)
        inputs.append(p)
    return ["-k", str(case["K"]), "-S", str(case["S"]), "-r", fa] + inputs
