"""The inputs of the `zot ksnp` tests: the seeded k-mer sets of the fixture (tests/golden/k1_ksnp.json holds what the reference's
generators yield on them) and the shapes the device tests are built from.  Everything is a pure function of its arguments."""
import functools
import hashlib

import numpy as np

from zotmer_amd import synth

DEFAULT, HAMMING, LEVENSHTEIN = "default", "hamming", "levenshtein"
FIXTURE_KS = (3, 4, 5, 12, 25, 31, 32)
FIXTURE_MODES = ((DEFAULT, 0), (HAMMING, 0), (HAMMING, 1), (HAMMING, 2), (LEVENSHTEIN, 1), (LEVENSHTEIN, 2))
FIXTURE_SEED = 23


def geometry(K):
    J = (K - 1) // 2
    return J, 2 * (J + 1), 2 * J


def digest(xs):
    return hashlib.sha256(np.asarray(xs, dtype="<u8").tobytes()).hexdigest()[:16]


def _draws(seed, tag, n):
    return [int(v) for v in synth.rnd(seed, tag, np.arange(n, dtype=np.uint64))]


@functools.lru_cache(maxsize=None)
def fixture_kmers(K, seed=FIXTURE_SEED, n_base=70):
    """A set with SNP groups in it: random k-mers, and beside some of them a middle-base variant, a tail with one or two
    substituted bases, and the low bases shifted by one (an insertion and a deletion: edit distance 2, Hamming distance
    anything).  At K <= 5 that is most of the 4^K k-mers.  -> ascending tuple of ints"""
    J, S, T = geometry(K)
    full, low = (1 << (2 * K)) - 1, (1 << S) - 1
    out = set()
    for i, (x, r) in enumerate(zip(_draws(seed + K, 40, n_base), _draws(seed + K, 41, n_base))):
        x &= full
        out.add(x)
        if r & 1:
            out.add(x ^ (((r >> 1) % 3 + 1) << T))
        if J and r & 2:
            y = x ^ (((r >> 8) % 3 + 1) << (2 * ((r >> 16) % J)))
            out.add(y)
            if r & 4:
                out.add(y ^ (((r >> 24) % 3 + 1) << (2 * ((r >> 32) % (J + 1)))))
        if r & 8:
            out.add((x & ~low) | (((x & low) << 2) & low) | ((r >> 40) & 3))
        if r & 16:
            out.add((x & ~low) | ((x & low) >> 2) | (((r >> 44) & 3) << (S - 2)))
    # The container stores k-mers as codec64 words of their deltas, and a delta of 2^60 or more has no code (the reference's
    # writer dies on it too).  Above 59 key bits a pair that every mode but -H 0 keeps stands every 2^59, so that the outputs
    # can be written as well as the input.
    for c in range(1 << max(2 * K - 59, 0) if 2 * K > 59 else 0):
        out.add((c << 59) | 0x155)
        out.add(((c << 59) | 0x155) ^ (1 << T))
    return tuple(sorted(out))


def fixture_cases():
    """[{name, K, mode, d, kmers}] in the fixture's order"""
    return [dict(name="k%d_%s_%d" % (K, mode, d), K=K, mode=mode, d=d, kmers=fixture_kmers(K))
            for K in FIXTURE_KS for mode, d in FIXTURE_MODES]


# ---- shapes -------------------------------------------------------------------------------------------------------------------

def group(K, prefix, lows):
    """the k-mers of one prefix with the given low J + 1 bases"""
    _, S, _ = geometry(K)
    return [(int(prefix) << S) | int(v) for v in lows]


def random_lows(K, n, seed):
    """n distinct values of the low J + 1 bases"""
    _, S, _ = geometry(K)
    return np.random.default_rng(seed).choice(1 << S, size=n, replace=False).tolist()


def planted_lows(K, n, seed):
    """n distinct values of the low J + 1 bases (n >= 2), two of which differ in the middle base only"""
    T = geometry(K)[2]
    r = random_lows(K, n, seed)
    out = [r[0], r[0] ^ (1 << T)]
    for v in r[1:]:
        if len(out) < n and v not in out:
            out.append(v)
    return out


def around(K, t, seed, tile=4096):
    """Three groups of t - 1, t and t + 1 members behind as many groups of one as it takes for the first of them to straddle
    a tile edge of the flat passes.  Every one of the three holds a pair that differs in the middle base only.
    -> ascending uint64 array"""
    _, S, _ = geometry(K)
    n_prefix = 1 << (2 * K - S)
    ones = (-(t // 2)) % tile or tile
    ones = min(ones, n_prefix - 3)
    xs = []
    for p in range(ones):
        xs += group(K, p, random_lows(K, 1, seed + p))
    for q, s in enumerate((t - 1, t, t + 1)):
        xs += group(K, ones + q, planted_lows(K, s, seed + 7919 * (q + 1)))
    return np.array(sorted(xs), dtype=np.uint64)


def chain_lows(K, d):
    """Low-base values v_0, v_1, ... in which consecutive ones differ in exactly d bases and all other pairs in more: step t
    adds 1 (mod 4) to the d base positions after the ones step t - 1 took, cyclically over the J + 1 positions."""
    m = geometry(K)[0] + 1
    digits, out, at = [0] * m, [], 0
    while True:
        v = sum(b << (2 * i) for i, b in enumerate(digits))
        if v in out:
            return out
        out.append(v)
        for _ in range(d):
            digits[at] = (digits[at] + 1) & 3
            at = (at + 1) % m


def random_set(K, n, seed):
    """n distinct random k-mers, ascending"""
    return np.sort(np.random.default_rng(seed).choice(1 << (2 * K), size=n, replace=False).astype(np.uint64))
