"""The inputs of the `zot vardyger` tests: the seeded sequences and reads of the fixture (tests/golden/v1_vardyger.json holds what
the reference's main prints on them) and small builders for the device tests.  Everything is a pure function of its arguments."""
import hashlib
import os
import random

FIXTURE_SEED = 27


def rc(s):
    return s[::-1].translate(str.maketrans("ACGTUacgtu", "TGCAAtgcaa"))


def digest(texts):
    h = hashlib.sha256()
    for t in texts:
        h.update(t.encode("latin-1"))
        h.update(b"\0")
    return h.hexdigest()[:16]


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def fasta_text(records, width=60):
    out = []
    for nm, seq in records:
        out.append(">" + nm + "\n")
        out.extend(seq[i:i + width] + "\n" for i in range(0, len(seq), width))
    return "".join(out)


def fastq_text(seqs, name="r%d", eol="\n"):
    return "".join("@%s%s%s%s+%s%s%s" % (name % i, eol, s, eol, eol, "I" * len(s), eol) for i, s in enumerate(seqs))


def duplicated(seq, at, unit, snp=None):
    """seq with the `unit` bases from 1-based position `at` written twice; snp: the second copy differs at that offset"""
    u = seq[at - 1:at - 1 + unit]
    if snp is not None:
        u = u[:snp] + {"A": "C", "C": "G", "G": "T", "T": "A"}[u[snp]] + u[snp + 1:]
    return seq[:at - 1 + unit] + u + seq[at - 1 + unit:]


def sample_reads(rng, genome, fold, read_len=100, avoid=()):
    """reads of read_len bases from uniformly drawn places of the genome, either strand, `fold` deep; a read that touches one of the
    0-based intervals of `avoid` is left out"""
    out = []
    for _ in range(fold * len(genome) // read_len):
        p = rng.randrange(0, len(genome) - read_len + 1)
        if any(p < hi and lo < p + read_len for lo, hi in avoid):
            continue
        s = genome[p:p + read_len]
        out.append(rc(s) if rng.random() < 0.5 else s)
    return out


def make_case(name, K, gen, units=(30,), opts=(), seq_len=600, at=201, folds=None, snp=None, phantom=0, shared=False, dress=False, files=1,
              wild=0, gap=None):
    """One record per entry of `units`: random bases, and a sample genome that holds the unit at `at` twice (unit 0: no
    duplication); reads from the sample genomes at folds[i] (60).  phantom: record 0 itself holds that many bases twice, at 401.
    shared: a last record is random bases around the bases 150..260 of record 0.  wild: reads from the records themselves, that
    deep, too.  gap: no read touches the offsets [gap[0], gap[1]) of either copy of record 0's unit.  dress: an N and lower case in record 0 away from the duplication, \\r\\n line ends in the reads."""
    rng = random.Random(gen)
    records, genomes = [], []
    for i, unit in enumerate(units):
        seq = rand_seq(rng, seq_len + 23 * i)
        if i == 0 and phantom:
            seq = duplicated(seq, 401, phantom)
        genomes.append(duplicated(seq, at, unit, snp) if unit else seq)
        records.append(["GENE%d" % (i + 1), seq])
    if shared:
        seq = rand_seq(rng, 200) + records[0][1][149:260] + rand_seq(rng, 200)
        records.append(["SHARED", seq])
        genomes.append(seq)
    folds = folds or [60] * len(genomes)
    reads = []
    for i, (g, fold) in enumerate(zip(genomes, folds)):
        avoid = [(at - 1 + c * units[0] + gap[0], at - 1 + c * units[0] + gap[1]) for c in (0, 1)] if gap and i == 0 else ()
        reads += sample_reads(rng, g, fold, avoid=avoid)
    if wild:
        for _, seq in records:
            reads += sample_reads(rng, seq, wild)
    rng.shuffle(reads)
    if dress:
        s = records[0][1]
        records[0][1] = s[:40] + "N" + s[41:100] + s[100:130].lower() + s[130:]
    cut = [len(reads) * f // files for f in range(files + 1)]
    inputs = [fastq_text(reads[a:b], "q%d", "\r\n" if dress else "\n") for a, b in zip(cut, cut[1:])]
    return dict(name=name, K=K, opts=list(opts), fasta=fasta_text([tuple(r) for r in records]), inputs=inputs)


def fixture_cases():
    """[{name, K, opts, fasta, inputs}] in the fixture's order"""
    S = FIXTURE_SEED * 1000
    return [
        # (the generators are chosen so that the bases around the unit allow the number of rolled placements the names say: a
        # duplication can be moved by one base for every base by which the unit's start repeats behind it or its end before it)
        make_case("u30", 24, S + 3, (30,)),                                     # one row, c.201_230dup
        make_case("u31", 24, S + 6, (31,)),                                     # not in frame: nothing
        make_case("u31_all", 24, S + 6, (31,), opts=["-a"]),                    # ... but with -a
        make_case("u13_all_rolled3", 24, S + 12, (13,), opts=["-a"]),           # J + 1 bases, three placements
        make_case("u12_all", 24, S + 4, (12,), opts=["-a"]),                    # J bases: pc == pb, nothing
        make_case("u48_k32_rolled2", 32, S + 11, (48,)),
        make_case("u30_strict", 24, S + 3, (30,), opts=["-s"]),
        make_case("phantom", 24, S + 6, (0,), phantom=27, opts=["-a"]),         # the record itself holds 27 bases twice
        make_case("shared", 24, S + 7, (30, 0), shared=True, wild=20),          # a second record holds the bases around the unit
        make_case("snp_copy", 24, S + 8, (60,), snp=30),
        make_case("snp_copy_strict", 24, S + 8, (60,), snp=30, opts=["-s"]),    # (the graph holds both copies' paths: -s keeps it)
        make_case("gap", 24, S + 1, (150,), folds=[150], gap=(60, 90)),         # no read crosses the middle of the unit ...
        make_case("gap_strict", 24, S + 1, (150,), folds=[150], gap=(60, 90), opts=["-s"]),      # ... so -s finds no path
        make_case("two_depths", 24, S + 9, (30, 42), folds=[60, 25]),
        make_case("two_depths_m30", 24, S + 9, (30, 42), folds=[60, 25], opts=["-m", "30"]),
        make_case("dressed_two_files", 24, S + 5, (33,), dress=True, files=2, wild=30),
        make_case("u45_k30_strict", 30, S + 13, (45,), opts=["-s"]),
    ]


def write_case(case, d):
    """the case's files under directory d -> the command's arguments (without its name)"""
    os.makedirs(d, exist_ok=True)
    fa = os.path.join(d, "genes.fa")
    with open(fa, "w", newline="") as f:
        f.write(case["fasta"])
    inputs = []
    for i, text in enumerate(case["inputs"]):
        p = os.path.join(d, "in%d.fastq" % i)
        with open(p, "w", newline="") as f:
            f.write(text)
        inputs.append(p)
    return ["-k", str(case["K"])] + case["opts"] + [fa] + inputs


# ---- builders of the device tests ----------------------------------------------------------------------------------------------
def join_by_its_contract(baits, kmers, counts, rseq, rkmer, rpos, by_second, K, min_count):
    """zk_dup_join as include/zotk.h words it, in plain Python -> (cover, rows): rows = [(e, i, j)] ascending by e, then by the
    place of i in by_second, then by j.  For the host layer's tests without a device, and a second opinion beside the
    restatement on one."""
    low = (1 << K) - 1
    at = {(b, x): c for b, x, c in zip(baits, kmers, counts)}
    cover = [at.get((s, x), 0) for s, x in zip(rseq, rkmer)]
    by_b, by_c = {}, {}
    for k, i in enumerate(by_second):
        by_b.setdefault((rseq[i], rkmer[i] & low), []).append(i)
    for j in range(len(rseq)):
        by_c.setdefault((rseq[j], rkmer[j] >> K), []).append(j)
    rows = []
    for e, (s, x, n) in enumerate(zip(baits, kmers, counts)):
        if n < min_count:
            continue
        for i in by_b.get((s, x & low), ()):
            if rkmer[i] >> K == x >> K:
                continue
            for j in by_c.get((s, x >> K), ()):
                if rkmer[j] != x and cover[j] >= min_count and rpos[j] > rpos[i] + K // 2:
                    rows.append((e, i, j))
    return cover, rows



def counted_from(xs_per_seq):
    """[{k-mer: count}] per sequence -> the counted list as three lists ascending by (sequence, k-mer)"""
    baits, kmers, counts = [], [], []
    for n, xs in enumerate(xs_per_seq):
        for x in sorted(xs):
            baits.append(n)
            kmers.append(x)
            counts.append(xs[x])
    return baits, kmers, counts
