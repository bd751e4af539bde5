"""The inputs of the `zot spoligo` fixtures (tests/golden/sp1_spoligo.json): k-mer sets and probe files built by a seeded
generator, so that the fixture holds only the reference's outputs.  Read by tests/golden/make_golden_spoligo.py and by the
tests.

A case is dict(name, K, kmers (ascending ints), probe_text (the -p file), probes).  `probes` is what the generator knows of
every probe line: name (as the file's reader must name it), seq, and `design`: per window of the probe (first window first)
the Hamming distance of the nearest k-mer as planted, 3 standing for "absent" -- `nearest` recomputes it by brute force and
the fixture writer asserts that the two agree.  `tags` name what a probe is there for."""
import random

BASES = "ACGT"


def encode(seq):
    r = 0
    for ch in seq:
        r = (r << 2) | BASES.index(ch.upper().replace("U", "T"))
    return r


def mutate(seq, places, both_bits=()):
    """substitute the bases at `places`; at the places in both_bits by the base that differs in both bits (A<->T, C<->G)"""
    s = list(seq)
    for p in places:
        b = BASES.index(s[p])
        s[p] = BASES[b ^ 3] if p in both_bits else BASES[b ^ (1 + (p % 2))]
    return "".join(s)


def ham(x, y):
    z = x ^ y
    return bin((z | (z >> 1)) & 0x5555555555555555555555).count("1")


def windows(seq, K):
    return [seq] if len(seq) <= K else [seq[i:i + K] for i in range(1 + len(seq) - K)]


def nearest(seq, K, kmers):
    """per window of the probe the distance of the nearest k-mer's leading bases, capped at 4 (brute force)"""
    out = []
    for w in windows(seq, K):
        s, v = 2 * (K - len(w)), encode(w)
        out.append(min([4] + [min(4, ham(x >> s, v)) for x in kmers]))
    return out


def _case(name, K, rng, n_random, short, long_):
    """K-base probes at every distance and place, probes of `short` bases, probes of `long_` bases"""
    rand_seq = lambda n: "".join(rng.choice(BASES) for _ in range(n))
    kmers = set(rng.getrandbits(2 * K) for _ in range(n_random))
    probes = []

    def plant(window, places, both_bits=()):
        """a k-mer whose leading bases are the window with substitutions; random bases below it"""
        kmers.add(encode(mutate(window, places, both_bits) + rand_seq(K - len(window))))

    def add(seq, design, tags, name=None):
        probes.append(dict(seq=seq, design=design, tags=tags, name=name))
        return seq

    # Kp = K: distance 0, 1 (first / last base), 2 (one of them a both-bits change), 3 and nothing at all
    plant(add(rand_seq(K), [0], ["K", "d0"], "exact"), [])
    plant(add(rand_seq(K), [1], ["K", "d1", "first"]), [0])
    plant(add(rand_seq(K), [1], ["K", "d1", "last"], "last_base"), [K - 1])
    plant(add(rand_seq(K), [1], ["K", "d1", "both_bits"]), [K // 2], [K // 2])
    plant(add(rand_seq(K), [2], ["K", "d2", "first", "last"], "two"), [0, K - 1])
    plant(add(rand_seq(K), [2], ["K", "d2", "both_bits"]), [1, K - 2], [K - 2])
    if K >= 3:
        plant(add(rand_seq(K), [3], ["K", "d3"], "three"), [0, K // 2, K - 1])
    # Kp < K: 16 k-mers that differ from each other only below the window, one substitution in it; one at distance 3
    if short:
        p = add(rand_seq(short), [1], ["short", "d1", "below_window"], "short_near")
        for _ in range(16):
            plant(p, [short - 1])
        plant(add(rand_seq(short), [0], ["short", "d0"]), [])
        plant(add(rand_seq(short), [3], ["short", "d3"], "short_far"), [0, 1, short - 1])
    # Kp > K: every window present, at different distances; exactly one window absent
    if long_:
        nw = 1 + long_ - K
        p = add(rand_seq(long_), [i % 3 for i in range(nw)], ["long", "all_present"], "long_all")
        for i in range(nw):
            plant(p[i:i + K], [0, K - 1][:i % 3])
        gone = nw // 2
        p = add(rand_seq(long_), [3 if i == gone else (i + 1) % 3 for i in range(nw)], ["long", "one_absent"])
        for i in range(nw):
            plant(p[i:i + K], [0, K // 2, K - 1] if i == gone else [1, K - 2][:(i + 1) % 3])
    return dict(name=name, K=K, kmers=sorted(kmers), probes=probes)


def _probe_text(case, rng):
    """the -p file: comments, named and unnamed lines, lower case and U; fills in the names the reader must give"""
    out = ["# %s: probes for K = %d\n" % (case["name"], case["K"])]
    for i, p in enumerate(case["probes"]):
        seq = p["seq"]
        if i % 4 == 1:
            seq = seq.lower()
        elif i % 4 == 2:
            seq = seq.replace("T", "U")
        if i % 3 == 2:
            out.append("#a comment before probe %d\n" % (i + 1))
        if p["name"] is None:
            p["name"] = str(i + 1)
            out.append(seq + "\n")
        else:
            out.append("%s%s%s\n" % (p["name"], rng.choice(["\t", " ", "  \t"]), seq))
    case["probe_text"] = "".join(out)


def make_cases():
    rng = random.Random(20261018)
    cases = [_case("k25", 25, rng, 3000, 16, 30),
             _case("k32", 32, rng, 3000, 20, 40),         # Kp = K = 32; a probe longer than a word
             _case("k12", 12, rng, 3000, 8, 15),          # a dense set: random k-mers come near the probes by themselves
             _case("k5", 5, rng, 12, 3, 7)]               # the smallest K the reference's index can hold (2K - 10 >= 0)
    # the dense cases also get probes nobody planted anything for
    for c in cases[2:]:
        for n in (c["K"], c["K"], c["K"] - 2, c["K"] + 2):
            seq = "".join(rng.choice(BASES) for _ in range(n))
            c["probes"].append(dict(seq=seq, design=None, tags=["unplanted"], name=None))
    for c in cases:
        _probe_text(c, rng)
        # the set must be storable: codec64 holds differences below 2**60 (the first one is taken from 0)
        assert all(b - a < 1 << 60 for a, b in zip([0] + c["kmers"], c["kmers"]))
    return cases
