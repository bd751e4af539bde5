"""The inputs of the core entry points and their oracle results, built once and shared by the tests that run the entries on the
GPU (tests/test_gpu_capacity.py: the output-capacity contract; tests/test_gpu_views.py: offset views of larger arrays).  Nothing here
touches a device: every builder runs on a machine without one.  The lengths are about three of the largest tile of the entry's
kernels plus a few (N)."""
import functools
import random

import numpy as np

from oracle import zkoracle as zo
from tests import _capture_restatement as R
from zotmer_amd import synth

GUARD = 0xABCDABCDABCDABCD
PAD = 64
U64 = np.uint64

SEL_TILE = 2048         # select.hip: SEL_BLOCK * SEL_ITEMS (the selections, zk_encode: input elements / stream bytes a tile)
RLE_TILE = 8192         # select.hip: RLE_BLOCK * RLE_ITEMS
MRG_TILE = 4096         # setops.hip: MRG_BLOCK * MRG_ITEMS (merged elements a tile)
KW_CAP = 2048           # kway.hip: KW_BLOCK * KW_ITEMS (the most elements a tile of the k-way pass holds)
PS_TILE = 4096          # spectrum.hip: PS_BLOCK * PS_ROUNDS
DEC_TILE = 2048         # codec.hip: CD_BLOCK * DEC_ITEMS (words a tile of the decoder)
ENC_TILE = 8192         # codec.hip: CD_BLOCK * ENC_CH (values a tile of the encoder)
CP_TILE = 4096          # compact.hpp: CP_BLOCK * CP_ITEMS (zk_line_ends: text bytes a tile)
N = 3 * RLE_TILE + 5    # the length needed, where the case can choose it


def stream_of(reads):
    return ("".join(r + "\n" for r in reads)).encode()


def guard(n, dtype):
    dt = np.dtype(dtype)
    return np.full(n, GUARD & ((1 << (8 * dt.itemsize)) - 1), dtype=dt)


def revcomp(k, K):
    k = np.asarray(k, dtype=U64)
    r = np.zeros_like(k)
    for i in range(K):
        r = (r << U64(2)) | (U64(3) - ((k >> U64(2 * i)) & U64(3)))
    return r


# ---- the inputs, built once ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def encode_case():
    """reads with N windows of 25 bases: 195 reads of 150 bases (126 windows each) and one of 35 (11)"""
    reads = synth.read_strings(7, 0, 195, 150, genome=0) + synth.read_strings(8, 0, 1, 35, genome=0)
    one = np.concatenate([zo.kmers_list(25, r, False) for r in reads])
    both = np.concatenate([zo.kmers_list(25, r, True) for r in reads])
    return stream_of(reads), one, both


@functools.lru_cache(maxsize=None)
def subsample_case():
    """basics.sub divides a 64-bit hash by 2^61 - 1: p = 4.2 keeps about 0.52 of the k-mers"""
    _, _, both = encode_case()
    keep = np.array([zo.sub(5, 4.2, int(x)) for x in both], dtype=bool)
    return both, both[keep]


@functools.lru_cache(maxsize=None)
def rle_case():
    """N distinct values in runs of 1 or 2, but for run 5000, which starts in the first tile and ends in the third (it crosses two
    tile edges), and the last run, which crosses at least one: rle_fixup_kernel adds their leading pieces to an output entry that a
    short capacity has cut off"""
    rng = np.random.default_rng(41)
    vals = np.sort(rng.choice(1 << 40, size=N, replace=False)).astype(U64)
    cnt = rng.integers(1, 3, size=N).astype(np.uint32)
    cnt[5000] = 9000
    cnt[N - 1] = RLE_TILE + 10
    first = int(cnt[:5000].sum())
    assert first < RLE_TILE and first + 9000 > 2 * RLE_TILE
    return np.repeat(vals, cnt), vals, cnt


@functools.lru_cache(maxsize=None)
def union_case():
    """two lists that share half their keys: 8193 shared, 8194 in each alone -> a union of N"""
    rng = np.random.default_rng(42)
    pool = rng.permutation(np.sort(rng.choice(1 << 50, size=N, replace=False)).astype(U64))
    x = np.sort(pool[:8193 + 8194])
    y = np.sort(np.concatenate([pool[:8193], pool[8193 + 8194:]]))
    xc = rng.integers(1, 1000, size=len(x), dtype=U64)
    yc = rng.integers(1, 1000, size=len(y), dtype=U64)
    zs, zc = zo.union_sum(x, xc, y, yc)
    assert len(zs) == N
    return x, xc, y, yc, zs, zc


@functools.lru_cache(maxsize=None)
def counted_case():
    """a counted set of 51 000 ascending k-mers (counts 1 .. 10) for the selections that keep about half of it"""
    rng = np.random.default_rng(43)
    k = np.sort(rng.choice(1 << 50, size=51000, replace=False)).astype(U64)
    c = rng.integers(1, 11, size=len(k), dtype=U64)
    return k, c


@functools.lru_cache(maxsize=None)
def project_case():
    """N of the set's 40 000 k-mers are in the reference, which holds 10 000 others as well"""
    rng = np.random.default_rng(44)
    pool = rng.permutation(np.sort(rng.choice(1 << 50, size=50000, replace=False)).astype(U64))
    k = np.sort(pool[:40000])
    ref = np.sort(np.concatenate([pool[:N], pool[40000:]]))
    c = rng.integers(1, 1 << 40, size=len(k), dtype=U64)
    ek, ec = zo.project(ref, k, c)
    assert len(ek) == N
    return ref, k, c, ek, ec


@functools.lru_cache(maxsize=None)
def prefix_case():
    """ascending k-mers under N distinct prefixes (the bits above 20), one to three k-mers under each"""
    rng = np.random.default_rng(45)
    pre = np.sort(rng.choice(1 << 30, size=N, replace=False)).astype(U64)
    reps = rng.integers(1, 4, size=N)
    low = np.concatenate([np.sort(rng.choice(1 << 20, size=int(r), replace=False)) for r in reps]).astype(U64)
    k = (np.repeat(pre, reps) << U64(20)) | low
    assert np.all(k[1:] > k[:-1])
    c = rng.integers(1, 1 << 31, size=len(k), dtype=U64)
    return k, c


@functools.lru_cache(maxsize=None)
def merge_case(k):
    """k lists whose union has N keys; a key is in about 2.5 of them (in all of them when k <= 2)"""
    rng = np.random.default_rng(500 + k)
    pool = np.sort(rng.choice(1 << 50, size=N, replace=False)).astype(U64)
    member = rng.random((k, N)) < min(1.0, 2.5 / k)
    orphan = ~member.any(axis=0)
    member[np.arange(N)[orphan] % k, np.arange(N)[orphan]] = True
    sets = [(pool[m], rng.integers(1, 50, size=int(m.sum()), dtype=U64)) for m in member]
    zs, zc, acgt = zo.merge_n(25, sets)
    assert len(zs) == N
    return sets, zs, zc, acgt


@functools.lru_cache(maxsize=None)
def mirror_case(K, size=None):
    """a counted canonical list and its both-strand table.  K = 25: 2 n entries.  K = 24: 200 of the 12 400 k-mers are palindromes
    (a 12-mer followed by its reverse complement), which the table holds once, with twice the count.  size: draw that many
    k-mers instead (at even K a sixtieth of them palindromes, one at least)"""
    rng = np.random.default_rng(600 + K)
    x = rng.integers(0, 1 << (2 * K), size=size or (12400 if K % 2 == 0 else 12291), dtype=U64)
    if K % 2 == 0:
        h = rng.integers(0, 1 << K, size=200 if size is None else size // 60 + 1, dtype=U64)
        x[:len(h)] = (h << U64(K)) | revcomp(h, K // 2)
    c = np.unique(np.minimum(x, revcomp(x, K)))
    n = rng.integers(1, 5000, size=len(c)).astype(np.uint32)
    rc = revcomp(c, K)
    pal = int(np.count_nonzero(rc == c))
    keys, inv = np.unique(np.concatenate([c, rc]), return_inverse=True)
    cnt = np.zeros(len(keys), dtype=U64)
    np.add.at(cnt, inv, np.concatenate([n, n]).astype(U64))
    assert len(keys) == 2 * len(c) - pal and (size is not None or len(keys) >= 3 * RLE_TILE)
    return c, n, keys, cnt.astype(np.uint32), pal


@functools.lru_cache(maxsize=None)
def codec_case():
    """70 000 values of mixed widths (one to six to a word) and N + 119 ascending k-mers for the delta form"""
    rng = np.random.default_rng(46)
    widths = rng.choice([1, 3, 9, 10, 12, 15, 16, 20, 21, 30, 31, 59, 60], size=70000)
    v = rng.integers(0, 1 << 62, size=len(widths), dtype=U64) >> (U64(62) - widths.astype(U64))
    v32 = (v & U64(0xFFFFFFFF)).astype(np.uint32)
    k = np.sort(rng.choice(1 << 50, size=N + 119, replace=False)).astype(U64)          # (most differences take a word each)
    return v, zo.codec64_encode(v), v32, zo.codec64_encode(v32.astype(U64)), k, zo.codec64_encode(zo.delta(k))


@functools.lru_cache(maxsize=None)
def hist_case():
    """30 000 counts of 300 distinct values, four of them beyond the dense range of the kernel (4096 bins in LDS)"""
    rng = np.random.default_rng(47)
    small = rng.choice(np.arange(1, 4096), size=296, replace=False)
    values = np.concatenate([small, [4096, 70000, (1 << 31) + 5, (1 << 32) - 1]]).astype(U64)
    counts = np.concatenate([values, rng.choice(values, size=30000 - len(values))])
    rng.shuffle(counts)
    return counts


@functools.lru_cache(maxsize=None)
def capture_case():
    """FASTQ text of 400 reads against a panel of six baits cut from a 4000-base genome (300 bases out of every 600): 300 reads
    come from the genome, either strand, so that about half of all reads share a 25-mer with a bait; 100 are random, and their
    quality strings are pieces of the baits -- a kernel that looked at the wrong line would capture them.  Reads of 100 and 150
    bases hold their windows in two chunks of 64."""
    rng = random.Random(77)
    genome = "".join(rng.choice("ACGT") for _ in range(4000))
    baits = [genome[600 * b:600 * b + 300] for b in range(6)]
    comp = str.maketrans("ACGT", "TGCA")
    seqs, quals = [], []
    for i in range(400):
        n = rng.choice((60, 100, 150))
        if i % 4 == 3:
            seqs.append("".join(rng.choice("ACGT") for _ in range(n)))
            p = rng.randrange(0, 300 - 150)
            quals.append(baits[i % 6][p:p + n])
        else:
            p = rng.randrange(0, len(genome) - n)
            s = genome[p:p + n]
            if rng.random() < 0.5:
                s = s[::-1].translate(comp)
            if rng.random() < 0.1:
                q = rng.randrange(n)
                s = s[:q] + "N" + s[q + 1:]
            seqs.append(s)
            quals.append("".join(rng.choice("ACGTIF#") for _ in range(n)))
    text = "".join("@r%d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(zip(seqs, quals)))
    table = {}
    for b, seq in enumerate(baits):
        for x in R.kmers(R.READ_K, seq, True):
            table.setdefault(x, set()).add(b)
    pairs, raw = [], 0
    for r, s in enumerate(seqs):
        hits = set()
        # the pairs BEFORE deduplication, which is what the capacity of zk_capture_hits has to hold: one per bait and chunk of 64
        # window starts (include/zotk.h)
        chunks = {}
        run = 0
        for p, ch in enumerate(s):
            run = run + 1 if ch in "ACGTUacgtu" else 0
            if run >= R.READ_K:
                w = p - R.READ_K + 1
                ids = table.get(R.kmers(R.READ_K, s[w:w + R.READ_K], False)[0], ())
                chunks.setdefault(w // 64, set()).update(ids)
                hits.update(ids)
        raw += sum(len(v) for v in chunks.values())
        pairs += [(b << 32) | r for b in hits]
    pairs = np.array(sorted(pairs), dtype=U64)
    recs = R.fastq_records(text)
    gathered = "".join("%s\n%s\n%s\n%s\n" % recs[int(w) & 0xFFFFFFFF] for w in pairs).encode()
    n_hit = len({int(w) & 0xFFFFFFFF for w in pairs})
    return text.encode(), baits, pairs, raw, gathered, n_hit


DENSE_PREFIX = "AAAAAAAAA"


def dense_block(rnd, K, n=14000):
    """n reads of K bases that share their first nine, each given twice (rnd(m): m random bases): n distinct canonical k-mers in ONE
    block of the 18-bit plan of zk_kmerize, 1.7 times a tile of the block dedupe at 14 000 (their mirror images are spread over
    random blocks).  Shared by tests/test_gpu_strand_blocks.py (`dense_block`) and the `dense` input below."""
    return [DENSE_PREFIX + rnd(K - len(DENSE_PREFIX)) for _ in range(n)] * 2


def kmerize_reads(name, K=None):
    """deep: ~60x over a genome of 12 000 bases, it repeats its k-mers; flat: random reads, no repeats.  Both end with 64 reads that
    hold a palindromic 24-mer each (a 12-mer and its reverse complement between random flanks; twenty copies of them in `deep`):
    random reads have none, and at even K the table is shorter than twice the canonical list only where there are some.
    dense (needs K): the first 3000 reads of `deep` and a dense_block of K-base reads -- a declined block on the forced block plans"""
    return _kmerize_reads(name, K if name == "dense" else None)


@functools.lru_cache(maxsize=None)
def _kmerize_reads(name, K):
    if name == "dense":
        assert K is not None and K > len(DENSE_PREFIX), "the dense input is built for one K"
        drng = random.Random(79 + K)
        return _kmerize_reads("deep", None)[:3000] + dense_block(lambda m: "".join(drng.choice("ACGT") for _ in range(m)), K)
    rng = random.Random(78)
    comp = str.maketrans("ACGT", "TGCA")

    def rnd(n):
        return "".join(rng.choice("ACGT") for _ in range(n))
    pal = []
    for _ in range(64):
        h = rnd(12)
        pal.append(rnd(30) + h + h[::-1].translate(comp) + rnd(30))
    if name == "deep":
        return synth.read_strings(31, 0, 6000, 150, genome=12000, sub_thr=synth.frac32(0.004), n_thr=synth.frac32(0.001)) + pal * 20
    return synth.read_strings(32, 0, 3000, 150, genome=0) + pal


@functools.lru_cache(maxsize=None)
def kmerize_want(name, K, flags):
    """(k-mers, counts, the capacity the call needs).  With ZK_KMERIZE_SUBSAMPLE the capacity is that of the table BEFORE the
    subsample, which is applied to the counted table in the caller's arrays.  name: deep, flat or dense; flags: canonical, both (the
    same table), canonical_only, subsample (p 0.5, seed 3)"""
    assert flags in ("canonical", "both", "canonical_only", "subsample"), flags
    reads = kmerize_reads(name, K)
    full = _kmerize_full(name, K)
    wk, wc = full["kmers"], full["counts"]
    if flags == "subsample":
        sub = zo.kmerize(K, reads, 1, 0.5, 3)
        return sub["kmers"], sub["counts"], len(wk)
    if flags == "canonical_only":
        rc = revcomp(wk, K)
        keep = wk <= rc
        ck, cc = wk[keep], wc[keep].copy()
        cc[ck == rc[keep]] //= 2
        return ck, cc, len(ck)
    return wk, wc, len(wk)


@functools.lru_cache(maxsize=None)
def _kmerize_full(name, K):
    """the oracle's table of both strands, computed once per input and K"""
    return zo.kmerize(K, kmerize_reads(name, K))


@functools.lru_cache(maxsize=None)
def kmerize_facts(name, K):
    """what zk_kmerize_stats must say of the input on every plan: dict(n_windows, n_instances, n_canonical, acgt).  n_canonical: the
    entries of the table that are not above their reverse complement (a palindrome is one entry, and canonical)"""
    full = _kmerize_full(name, K)
    wk = np.asarray(full["kmers"], dtype=U64)
    inst = int(np.asarray(full["counts"], dtype=U64).sum())          # two emissions per valid window
    assert inst % 2 == 0 and sum(full["acgt"]) == inst
    return dict(n_windows=inst // 2, n_instances=inst, n_canonical=int(np.count_nonzero(wk <= revcomp(wk, K))), acgt=list(full["acgt"]))
