"""
The block dedupe's unsorted write-out (dedupe2.hip, UNSORTED): every wave compacts the entries of its own table rows in LDS, in place,
and writes them in dense rounds of 64 -- the words and, on the fused strand route, their mirror images.  The sizes here are the ones
at which those loops can go wrong: one block of n distinct k-mers (a shared nine-base prefix) with n at and around a wave's 64 lanes,
a row of 512 slots, a whole number of rounds for every wave (4096), and a table at 0.98 load (11 000 of 11 264 slots) where compaction
moves almost nothing; the largest count that fits the packed field inside a dense round; the degenerate inputs.

As tests/test_strand_fused_mirror.py does it: the plan of a 50 M-read batch is forced (ZK_TUNE_DEDUPE_BITS = 18) on inputs the C
oracle can count; keys, counts, histogram, acgt and n_unique are compared bit for bit with oracle/zkoracle.py (kmerize, hist).  Every
case runs by ZK_TUNE_STRAND_BLOCKS = 1 (the fused kernel: ZK_TUNE_DEDUPE_VARIANT 0 and 2 are its two-swap instantiation, 1 the
one-swap one) and = 4 (the plain unsorted dedupe + strand_mirror_kernel), and the routes must agree with each other.
"""
import numpy as np
import pytest

from oracle import zkoracle as zo
from zotmer_amd import native

pytestmark = pytest.mark.gpu

FUSED, MIRROR_KERNEL = 1, 4          # ZK_TUNE_STRAND_BLOCKS
ROUTES = [(FUSED, 0), (FUSED, 1), (FUSED, 2), (MIRROR_KERNEL, 0)]          # (strand_blocks, dedupe_variant)
BASES = np.array(list("ACGT"))


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def stream_of(reads):
    return ("".join(r + "\n" for r in reads)).encode()


def random_reads(seed, n=2000, length=60, genome=20000, sub=0.01, n_rate=0.002):
    """n reads of `length` bases from a random genome, sub substitutions and n_rate N per base"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, size=genome)
    starts = rng.integers(0, genome - length + 1, size=n)
    codes = g[starts[:, None] + np.arange(length)[None, :]]
    hit = rng.random(codes.shape) < sub
    codes = np.where(hit, (codes + rng.integers(1, 4, size=codes.shape)) % 4, codes)
    text = BASES[codes]
    text[rng.random(codes.shape) < n_rate] = "N"
    return ["".join(row) for row in text]


def prefixed(seed, K, n):
    """n distinct K-long reads that share their first nine bases: one block of the 18-bit plan"""
    rng = np.random.default_rng(seed)
    seen = set()
    while len(seen) < n:
        seen.add("AAAAAAAAA" + "".join(BASES[rng.integers(0, 4, size=K - 9)]))
    return sorted(seen)


@pytest.fixture(scope="module")
def beside():
    """the 2000 random reads every one-block case stands beside"""
    return random_reads(2900)


def run(ctx, d, K, route, variant):
    """-> (k-mers, counts, histogram, bytes booked by the mirror step, stats) by the given route"""
    ctx.tune(dedupe_bits=18, strand_blocks=route, dedupe_variant=variant)
    ctx.profile(True)
    try:
        k, c, st = ctx.kmerize(d, K, cap=max(2 * d.n, 64))
        sel = ctx.profile_read().get("select", dict(launches=0, bytes=0))
        return k.to_host(), c.to_host(), ctx.hist(c) if c.n else {}, sel["bytes"], st
    finally:
        ctx.profile(False)
        ctx.tune(dedupe_bits=0, strand_blocks=FUSED, dedupe_variant=0)


def check(ctx, reads, K, taken=True):
    """every route against the oracle and against the first one; taken: the strand route must have been taken by all of them (None:
    either way)"""
    want = zo.kmerize(K, reads)
    hv, hf = zo.hist(want["counts"])
    want_hist = {int(a): int(b) for a, b in zip(hv, hf)} if len(want["counts"]) else {}
    d = ctx.upload_stream(stream_of(reads))
    first = None
    for route, variant in ROUTES:
        what = (route, variant)
        k, c, h, nbytes, st = run(ctx, d, K, route, variant)
        assert np.array_equal(k, want["kmers"]) and np.array_equal(c, want["counts"]), what
        assert h == want_hist and list(st.acgt) == want["acgt"] and st.n_unique == len(want["kmers"]), what
        if taken is not None:          # 16 bytes per canonical k-mer: every k-mer has its mirror image in the table (odd K)
            assert (nbytes == 8 * len(k)) == taken, what
        if first is None:
            first = (k, c, h)
        else:
            assert np.array_equal(first[0], k) and np.array_equal(first[1], c) and first[2] == h, what
    return want


# a wave with no entry, a last dense round of one lane, whole rounds exactly, a full table; 12 000: declined (more than a table holds)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 4095, 4096, 4097, 11000, 12000])
def test_one_block_of_n_entries(ctx, beside, n):
    K = 25
    block = prefixed(3000 + n, K, n)
    want = check(ctx, beside + block, K)
    assert len(want["kmers"]) >= n


@pytest.mark.parametrize("n", [1, 64, 65, 200])
def test_one_block_tags_of_eight_bits(ctx, beside, n):
    """K = 13: the smallest odd K the forced route takes, 8-bit tags (a block has at most 256 distinct ones)"""
    K = 13
    check(ctx, beside + prefixed(3100 + n, K, n), K)


def test_every_entry_three_times(ctx, beside):
    K = 25
    check(ctx, beside + prefixed(3200, K, 600) * 3, K)


@pytest.mark.parametrize("copies,taken", [(16383, True), (16384, False)], ids=["16383_fits", "16384_beyond"])
def test_largest_count_inside_a_dense_round(ctx, beside, copies, taken):
    """counts of 14 bits at K = 25: one entry of 600 occurs 16 383 times (the largest count a word holds), the others 3 times; once
    more and the count goes to the side list, the strand route is not taken"""
    K = 25
    block = prefixed(3300, K, 600)
    reads = beside + block * 3 + [block[300]] * (copies - 3)
    want = check(ctx, reads, K, taken=taken)
    assert int(want["counts"].max()) == copies


@pytest.mark.parametrize("reads", [[], ["ACGTTGCATGCAGGATTACAGATTACACCATGGTACCAGT"], ["", "", "", ""]], ids=["empty", "one_read", "separators"])
def test_degenerate_inputs(ctx, reads):
    check(ctx, reads, 25, taken=None)
