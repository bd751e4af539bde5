"""Inputs that put a k-mer count at the edge of a packed count field ("count fields"), and their expected results.  Nothing
here touches a device: tests/test_count_edges_host.py checks the builders on any machine, tests/test_gpu_count_fields.py runs them.

zk_kmerize and zk_mirror_expand move a k-mer and its count as one word, (k-mer << s) | count, wherever the count fits the s spare bits
above the 2K key bits.  edge_reads() builds a read stream in which a few target k-mers occur exactly c times each, c at 2^s - 2 ..
2^s + 1, beside background reads whose own counts stay far below; mirror_lists() builds a counted canonical list with one entry at the
bound; block_reads() fills one block of the forced 18-bit plan with a chosen number of keys.  Every builder is seeded and asserts what
it promises, so a case cannot silently stop reaching its edge."""
import functools

import numpy as np

from oracle import zkoracle as zo
from tests._core_cases import mirror_case, revcomp, stream_of          # noqa: F401  (stream_of: for the GPU tests)
from zotmer_amd import synth

U64 = np.uint64
BASES = "ACGT"
COMP = str.maketrans("ACGT", "TGCA")
BLOCK_BITS = 18                      # the forced plan (ZK_TUNE_DEDUPE_BITS = 18): a block = the keys that share their first nine bases
BLOCK_PREFIX = "A" * 9
SPREADS = ("together", "strided")
BACKGROUNDS = ("deep", "flat", "wide")


def pack_bits(K):
    """the width s of the count field beside a K-mer (pipeline.hip: pack_bits_for), restated"""
    spare = 64 - 2 * K
    return min(spare, 31) if spare >= 10 else 0


def encode(s):
    v = 0
    for ch in s:
        v = (v << 2) | BASES.index(ch)
    return v


def rc_str(s):
    return s[::-1].translate(COMP)


def canonical(s):
    return min(encode(s), encode(rc_str(s)))


def is_palindrome(s):
    return s == rc_str(s)


def _rnd(rng, n):
    return "".join(BASES[i] for i in rng.integers(0, 4, size=n))


# ---- the cases the GPU tests run (tests/test_gpu_count_fields.py) and the host tests check (tests/test_count_edges_host.py) ----------------
EDGE = {"2^s-2": -2, "2^s-1": -1, "2^s": 0, "2^s+1": 1}          # the count, relative to 2^s
LAYOUTS = [("together", "deep"), ("strided", "deep"), ("together", "flat"), ("strided", "wide")]
PACKED_K = (27, 26, 25, 24, 23)                                    # s = 10, 12, 14, 16, 18
CUT_K, CUT_C = (27, 26), (511, 512, 513, 1023, 1024, 1025)         # collapse_kernel cuts a run every 512 slots where 2^s <= 8192
# the forced block plan: (K, count, two targets in one block).  K = 20 (s = 24) is out of reach: 2^15 - 1 and 2^15 there
FORCED = [(K, (1 << (64 - 2 * K)) + e, sb) for K in (25, 27, 24) for e in (-1, 0) for sb in (False, True)] + \
         [(20, (1 << 15) + e, sb) for e in (-1, 0) for sb in (False, True)]
LDS_K, LDS_BLOCKS = (21, 20), [(65535,), (65534, 1), (65536,), (65536, 1)]          # the keys of one block, per k-mer


def packed_cases():
    return [(K, (1 << pack_bits(K)) + e, spread, bg) for K in PACKED_K for e in EDGE.values() for spread, bg in LAYOUTS]


def edge_cases():
    """every (K, c, spread, background, same_block) the GPU tests hand to edge_reads"""
    return [x + (False,) for x in packed_cases()] + [(K, c, "together", "deep", False) for K in CUT_K for c in CUT_C] + \
           [(K, c, "together", "deep", sb) for K, c, sb in FORCED]


# ---- the background reads ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def background_reads(name):
    if name == "deep":          # ~25x over 12 000 bases: it repeats its k-mers
        return tuple(synth.read_strings(31, 0, 2000, 150, genome=12000, sub_thr=synth.frac32(0.004), n_thr=synth.frac32(0.001)))
    if name == "flat":          # random reads: no k-mer twice
        return tuple(synth.read_strings(32, 0, 3000, 150, genome=0))
    if name == "wide":          # random reads, just enough of them for 2^16 distinct canonical k-mers
        return tuple(synth.read_strings(33, 0, 700, 150, genome=0))
    raise ValueError("background must be one of %r (got %r)" % (BACKGROUNDS, name))


@functools.lru_cache(maxsize=None)
def background_table(name, K):
    """(both-strand k-mers of the background, its windows, its distinct canonical k-mers, its largest count)"""
    t = zo.kmerize(K, list(background_reads(name)))
    k, c = t["kmers"], t["counts"]
    pal = int(np.count_nonzero(revcomp(k, K) == k)) if K % 2 == 0 else 0
    return k, int(c.astype(U64).sum()) // 2, (len(k) + pal) // 2, int(c.max())


def check_background(name, K, bound, reads=None):
    """what each background promises, and that its counts leave the maximum to the targets (at most half the bound under test).
    reads: check these reads against the promise of `name` instead (the host tests hand in a wrong one on purpose)."""
    if reads is None:
        k, windows, distinct, largest = background_table(name, K)
    else:
        t = zo.kmerize(K, list(reads))
        k = t["kmers"]
        pal = int(np.count_nonzero(revcomp(k, K) == k)) if K % 2 == 0 else 0
        windows, distinct, largest = int(t["counts"].astype(U64).sum()) // 2, (len(k) + pal) // 2, int(t["counts"].max())
    if name == "deep":
        assert distinct <= 0.5 * windows, "deep: the background must repeat its k-mers (%d distinct of %d windows)" % (distinct, windows)
    else:
        assert distinct >= 0.999 * windows, "%s: the background must not repeat its k-mers (%d distinct of %d windows)" % (name, distinct, windows)
    if name == "wide":
        assert distinct >= 1 << 16, "wide: at least 2^16 distinct canonical k-mers (%d)" % distinct
    assert 2 * largest <= bound, "the largest background count (%d) must be at most half the bound (%d)" % (largest, bound)
    return k


# ---- reads with target k-mers of an exact count --------------------------------------------------------------------------------------

def target_kmers(K, same_block=False):
    """the one-window target reads: the lowest key, one in the middle, one whose canonical form is high, at even K a palindrome.
    same_block: the middle one shares its first nine bases with the lowest (one block of the forced 18-bit plan); the others never do."""
    rng = np.random.default_rng(7000 + K)
    low = "A" * (K - 1) + "C"
    while True:
        mid = BLOCK_PREFIX + _rnd(rng, K - 9) if same_block else "C" + _rnd(rng, K - 2) + "A"
        high = "TT" + _rnd(rng, K - 4) + "AA"
        h = _rnd(rng, K // 2)
        pal = h + rc_str(h)
        ts = [low, mid, high] + ([pal] if K % 2 == 0 else [])
        cs = [canonical(t) for t in ts]
        blocks = [x >> (2 * K - BLOCK_BITS) for x in cs]
        if len(set(cs)) == len(cs) and not any(is_palindrome(t) for t in ts[:3]) and (blocks[1] == blocks[0]) == same_block and \
                len(set(blocks)) == len(blocks) - (1 if same_block else 0) and cs[0] == 1 and cs[2] >> (2 * K - 2) == 3:
            return ts


def edge_reads(K, c, spread, background, same_block=False):
    """-> (reads, targets): every target read (exactly K bases: one window) c times beside the background reads.
    together: the copies in one stretch of the stream; strided: dealt evenly among the background reads, so that the partial counts
    come from different tiles and the sum first crosses a field where partial counts are added."""
    assert spread in SPREADS, "spread must be one of %r (got %r)" % (SPREADS, spread)
    bg = list(background_reads(background))
    bk = check_background(background, K, c)
    targets = target_kmers(K, same_block)
    for t in targets:
        assert len(t) == K and not np.any(bk == U64(encode(t))), "a target k-mer occurs in the background"
    if spread == "together":
        half = len(bg) // 2
        copies = [t for t in targets for _ in range(c)]          # a stretch per target, the stretches adjacent
        return bg[:half] + copies + bg[half:], targets
    reads = []
    for i, r in enumerate(bg):
        reads.append(r)
        n = c * (i + 1) // len(bg) - c * i // len(bg)           # sums to c over the background
        reads += targets * n
    return reads, targets


def expected_counts(K, c, targets):
    """{k-mer of the table: count} the targets alone account for: c on both strands, c + c for a palindrome"""
    out = {}
    for t in targets:
        for x in (encode(t), encode(rc_str(t))):
            out[x] = out.get(x, 0) + c
    return out


@functools.lru_cache(maxsize=4)
def edge_want(K, c, spread, background, same_block=False):
    """the oracle's table of edge_reads(...), its histogram and the number of canonical k-mers; computed once per input"""
    reads, targets = edge_reads(K, c, spread, background, same_block)
    return want_of(K, reads)


def want_of(K, reads):
    w = zo.kmerize(K, reads)
    hv, hf = zo.hist(w["counts"])
    k = w["kmers"]
    n_can = int(np.count_nonzero(k <= revcomp(k, K)))
    return dict(kmers=k, counts=w["counts"], acgt=w["acgt"], hist={int(a): int(b) for a, b in zip(hv, hf)}, n_canonical=n_can,
                max_canonical=canonical_max(K, k, w["counts"]))


def canonical_max(K, k, counts):
    """the largest count of the CANONICAL list (a palindrome's is half its table count): what the packed maximum is taken of"""
    if not len(k):
        return 0
    c = counts.astype(U64).copy()
    if K % 2 == 0:
        c[revcomp(k, K) == k] //= U64(2)
    return int(c.max())


DENSE = 14000          # distinct k-mers under one nine-base prefix: more than any LDS table of the block dedupe holds


def dense_block_reads(K, c):
    """-> (reads, targets): edge_reads(K, c, "together", "deep", same_block=True) and, in the block its two lowest targets share, DENSE
    more distinct k-mers, once each: the block fills every LDS table and is counted by sorting (dedupe_bad_blocks), the targets' counts
    by a run-length pass with the field"""
    reads, targets = edge_reads(K, c, "together", "deep", True)
    rng = np.random.default_rng(9000 + K)
    seen = set()
    while len(seen) < DENSE:
        t = BLOCK_PREFIX + _rnd(rng, K - 9)
        if canonical(t) == encode(t) and t not in targets:
            seen.add(t)
    return reads + sorted(seen), targets


@functools.lru_cache(maxsize=4)
def dense_block_want(K, c):
    return want_of(K, dense_block_reads(K, c)[0])


DENSE_CASES = [(K, (1 << (64 - 2 * K)) + e) for K in (25, 27) for e in (-1, 0)]


# ---- one block of the forced plan with a chosen number of keys ---------------------------------------------------------------------

def block_reads(K, copies, background="deep"):
    """-> (reads, k-mers): distinct k-mers that share their first nine bases (one block of the forced 18-bit plan), the i-th copies[i]
    times, in one stretch between the background reads, none of whose k-mers falls into that block (the first block the background
    leaves empty is taken): the block holds sum(copies) keys exactly."""
    bg = list(background_reads(background))
    bk = check_background(background, K, max(copies))
    can = np.minimum(bk, revcomp(bk, K))
    taken = np.unique(can >> U64(2 * K - BLOCK_BITS))
    v = next(i for i in range(1 << BLOCK_BITS) if i >= len(taken) or int(taken[i]) != i)
    prefix = "".join(BASES[(v >> (2 * (8 - i))) & 3] for i in range(9))
    assert not np.any(can >> U64(2 * K - BLOCK_BITS) == U64(v)), "a background k-mer falls into the block under test"
    rng = np.random.default_rng(8000 + K)
    kmers = []
    while len(kmers) < len(copies):
        t = prefix + _rnd(rng, K - 9)
        if canonical(t) == encode(t) and not is_palindrome(t) and t not in kmers:
            kmers.append(t)
    half = len(bg) // 2
    block = [t for t, n in zip(kmers, copies) for _ in range(n)]
    return bg[:half] + block + bg[half:], kmers


@functools.lru_cache(maxsize=4)
def block_want(K, copies, background="deep"):
    return want_of(K, block_reads(K, list(copies), background)[0])


# ---- counted canonical lists for zk_mirror_expand -------------------------------------------------------------------------------------

WHERES = ("first", "middle", "last")


@functools.lru_cache(maxsize=4)
def mirror_lists(K, bound, where, palindrome=False):
    """-> (canonical k-mers, counts, table k-mers, table counts as u64, index of the edge entry): about 70 000 entries with counts in
    [1, bound - 1] (some of them bound - 1) but for one equal to `bound`: the first, middle or last entry that is no palindrome -- or,
    at even K, the first, middle or last PALINDROME, whose table count is bound + bound.  The table is built in numpy; its counts are u64, so a count beyond
    32 bits shows as such (the call must then refuse)."""
    assert where in WHERES and bound >= 2
    c, n, _, _, _ = mirror_case(K, size=70000)
    assert len(c) >= 1 << 16, "the list must be long enough for the grouped mirror (2^16 entries)"
    n = n.astype(U64)
    if bound > 2:
        n = U64(1) + (n - U64(1)) % U64(bound - 1)          # [1, bound - 1]
    else:
        n[:] = 1
    rc = revcomp(c, K)
    pick = np.flatnonzero((rc == c) == palindrome)
    assert len(pick) >= 3, "no palindromes at this K"
    at = int(pick[{"first": 0, "middle": len(pick) // 2, "last": len(pick) - 1}[where]])
    # the neighbours of the field's edge elsewhere in the list: ordinary entries, and a palindrome if there is one
    for j in (1, len(c) // 3, len(c) - 2):
        n[j] = bound - 1
    other = np.flatnonzero(rc == c)
    if len(other):
        n[int(other[len(other) // 3])] = bound - 1
    n[at] = bound
    assert int(n.max()) == bound and int(np.count_nonzero(n == U64(bound))) == 1 and int(n.min()) >= 1
    keys, inv = np.unique(np.concatenate([c, rc]), return_inverse=True)
    cnt = np.zeros(len(keys), dtype=U64)
    np.add.at(cnt, inv, np.concatenate([n, n]))
    assert len(keys) == 2 * len(c) - int(np.count_nonzero(rc == c))
    return c, n.astype(np.uint32), keys, cnt, at
