"""The seeded inputs of the `zot contigs` tests and of tests/golden/make_golden_contigs.py: small genomes with a repeat, so that
the de Bruijn graph of their k-mers branches, as ascending k-mer lists."""
import hashlib
import random

from tests._contigs_restatement import kmers_of, rc


def genome(seed, insert=""):
    """400 random bases + `insert` + a copy of bases 100..160 + 200 random bases"""
    rng = random.Random(seed)
    g = "".join(rng.choice("ACGT") for _ in range(400))
    tail = "".join(rng.choice("ACGT") for _ in range(200))
    return g + insert + g[100:160] + tail


def digest(xs):
    return hashlib.sha256(b"".join(int(x).to_bytes(8, "little") for x in xs)).hexdigest()[:16]


def _case(name, K, xs, l=None, **params):
    return dict(name=name, K=K, l=l, kmers=xs, params=dict(params, n=len(xs), digest=digest(xs)))


def make_cases():
    cases = []
    for K in (11, 16, 25, 31, 32):
        cases.append(_case("genome_k%d" % K, K, kmers_of(K, genome(K)), seed=K))
    cases.append(_case("l_1", 13, kmers_of(13, genome(101)), l=1, seed=101))
    cases.append(_case("l_above_all", 13, kmers_of(13, genome(102)), l=100000, seed=102))
    xs = kmers_of(15, genome(103))
    xs = [x for i, x in enumerate(xs) if i % 3 != 2][:-40]
    if len(xs) % 64 == 0:
        xs = xs[:-1]
    cases.append(_case("not_closed", 15, xs, l=17, seed=103, dropped="every third, then the 40 largest; one more where n % 64 == 0"))
    cases.append(_case("poly_a", 11, kmers_of(11, genome(104, insert="A" * 20)), seed=104, insert="A" * 20))
    pal = "ACGTACGTACGT"
    cases.append(_case("palindromes_k12", 12, kmers_of(12, genome(105, insert=pal + "GG" + "AATTCCGGAATT")), seed=105,
                       insert=pal + "GG" + "AATTCCGGAATT"))
    return cases


def closed(K, xs):
    s = set(xs)
    return all(rc(K, x) in s for x in xs)
