"""
The strand route at odd K with the mirror words written by the block dedupe itself (dedupe2.hip, MIRROR; strand_blocks.hip): the plan
of a 50 M-read batch forced (ZK_TUNE_DEDUPE_BITS = 18) on inputs small enough for the oracle, as test_kmerize_forced_block_dedupe does.

Every case is compared, keys and counts, bit for bit with the C oracle (oracle/zkoracle.py: kmerize_packed through kmerize, and hist),
and is run a second time with the mirror words written by strand_mirror_kernel (ZK_TUNE_STRAND_BLOCKS = 4, the route before), which
must give the same arrays.  The step books the same record either way ("select": 16 bytes per canonical k-mer whenever the strand
route is taken), so the records tell that the route was taken, not which form wrote the mirror words: the two forms are told apart by
the knob alone.
"""
import numpy as np
import pytest

from oracle import zkoracle as zo
from zotmer_amd import native

pytestmark = pytest.mark.gpu

FUSED, MIRROR_KERNEL, TIGHT = 1, 4, 5          # ZK_TUNE_STRAND_BLOCKS
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


def run(ctx, d, K, route, **knobs):
    """-> (k-mers, counts, histogram, bytes booked by the mirror step, stats) by the given route"""
    ctx.tune(dedupe_bits=18, strand_blocks=route, **knobs)
    ctx.profile(True)
    try:
        k, c, st = ctx.kmerize(d, K, cap=max(2 * d.n, 64))
        sel = ctx.profile_read().get("select", dict(launches=0, bytes=0))
        return k.to_host(), c.to_host(), ctx.hist(c) if c.n else {}, sel["bytes"], st
    finally:
        ctx.profile(False)
        ctx.tune(dedupe_bits=0, strand_blocks=FUSED, dedupe_variant=0, dedupe_limit=65536)


def check(ctx, reads, K, route=FUSED, taken=True, **knobs):
    """the route against the oracle and against strand_mirror_kernel's; taken: the strand route must have been taken by both"""
    want = zo.kmerize(K, reads)
    hv, hf = zo.hist(want["counts"])
    want_hist = {int(a): int(b) for a, b in zip(hv, hf)}
    d = ctx.upload_stream(stream_of(reads))
    k, c, h, nbytes, st = run(ctx, d, K, route, **knobs)
    assert np.array_equal(k, want["kmers"]) and np.array_equal(c, want["counts"])
    assert h == want_hist and list(st.acgt) == want["acgt"] and st.n_unique == len(want["kmers"])
    k0, c0, h0, nbytes0, _ = run(ctx, d, K, MIRROR_KERNEL, **knobs)
    assert np.array_equal(k0, k) and np.array_equal(c0, c) and h0 == h
    # 16 bytes per canonical k-mer: every k-mer has its mirror image in the table (odd K)
    assert (nbytes == 8 * len(k)) == taken and (nbytes0 == 8 * len(k)) == taken


@pytest.mark.parametrize("K", [25, 13])          # 32-bit tags beside a 14-bit count; 13: the smallest odd K the forced route takes
def test_random_reads(ctx, K):
    check(ctx, random_reads(100 + K), K)


def test_two_and_one_swaps_in_flight(ctx):
    """the fused kernel's two instantiations (ZK_TUNE_DEDUPE_VARIANT 2 and 1)"""
    reads = random_reads(7)
    for variant in (2, 1):
        check(ctx, reads, 25, dedupe_variant=variant)


def test_declined_block_table_full(ctx):
    """a block with more distinct entries than a dedupe2_kernel table holds (11 264) beside ordinary reads: dedupe_kernel counts it,
    strand_mirror_kernel writes its mirror words behind the dedupe's"""
    K = 25
    check(ctx, random_reads(11) + prefixed(12, K, 12000), K)


def test_declined_block_too_many_keys(ctx):
    """a block of 70 000 keys (16-bit counts: declined up front), no count above 16 383"""
    K = 25
    ten = prefixed(13, K, 10)
    check(ctx, random_reads(14) + [ten[i % 10] for i in range(70000)], K)


def test_every_block_declined(ctx):
    """dedupe_limit 6: the ordinary blocks count as too large, the dedupe writes few mirror words and the list has the rest"""
    check(ctx, random_reads(15), 25, dedupe_limit=6)


def test_count_beyond_the_packed_field(ctx):
    """17 000 copies of a read at K = 25 (counts of 14 bits): the strand route is not taken"""
    one = random_reads(16, n=1)
    check(ctx, random_reads(17) + one * 17000, 25, taken=False)


def test_tight_room_for_the_mirror_words(ctx):
    """room for 1024 mirror words: the cursor passes it, the dedupe's list is dropped and strand_mirror_kernel writes all of it"""
    check(ctx, random_reads(18), 25, route=TIGHT)


@pytest.mark.parametrize("reads", [[], ["ACGTTGCATGCAGGATTACAGATTACACCATGGTACCAGT"], ["", "", "", ""]], ids=["empty", "one_read", "separators"])
def test_degenerate_inputs(ctx, reads):
    K = 25
    want = zo.kmerize(K, reads)
    d = ctx.upload_stream(stream_of(reads))
    for route in (FUSED, MIRROR_KERNEL):
        k, c, h, _, st = run(ctx, d, K, route)
        assert np.array_equal(k, want["kmers"]) and np.array_equal(c, want["counts"]) and st.n_unique == len(want["kmers"])
