"""zk_kmerize over the (read length, K) plane, and over every K.

Both first-pass implementations lay their tiles along the records when the stream is uniform (make_tiling, stream_pass.hip;
record_tiles, radix_sort.hip).  Which geometry a stream gets depends on L and K through ceil(W / 8) or ceil(W / 16) threads per
record, records per tile rounded down to 16, a fit into the tile image, a pay-off test, rec >= 16, W >= 1 and a division by
multiplication: evaluated on the host that is 26 to 47 changes of geometry per K along L, with islands where tiling by record
switches back on (L = 261..264 at K = 9, L = 522..536 at K = 25; the last one ends at L = 543 for K = 32).  The other suites visit
L in {40, 100, 150, 255}.  Here every L from K - 1 to 560 is run on every first-pass route, and every K from 1 to 32 on one mixed
input through the plans the K decides (digit widths, packed pairs, the block dedupe, palindromes at even K).  Exact, against the
oracle."""
import functools

import numpy as np
import pytest

from oracle import zkoracle as zo
from tests import _window_streams as W
from zotmer_amd import native

pytestmark = pytest.mark.gpu

L_MAX = 560                       # past the last island of tiling by record
BLOCK = 64                        # lengths per case
U64 = np.uint64
# the first-pass routes: the ranged pass with its default ranges, its 512-thread form on three ranges (ranges of many tiles), the
# two-burst form, the look-back pipeline
ROUTES = (dict(stream_pass=1, stream_ranges=0), dict(stream_pass=2, stream_ranges=3), dict(stream_pass=3, stream_ranges=0),
          dict(stream_pass=0, stream_ranges=0))


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def differs(ctx, d, K, want, flags=native.KMERIZE_CANONICAL):
    """None, or what of a kmerize differs from the oracle's result (an error the library returns is such a difference: the route
    refused an input it should take; a HIP error is not caught)"""
    try:
        k, c, st = ctx.kmerize(d, K, flags)
    except native.ZotkError as e:
        if e.code == native.ZK_EHIP:
            raise
        return str(e)
    if not np.array_equal(k.to_host(), want["kmers"]):
        return "k-mers (%d for %d)" % (k.n, len(want["kmers"]))
    if not np.array_equal(c.to_host(), want["counts"]):
        return "counts"
    if list(st.acgt) != want["acgt"]:
        return "acgt"
    n_windows = int(want["counts"].sum(dtype=U64)) // 2
    if (st.n_windows, st.n_unique) != (n_windows, len(want["kmers"])):
        return "n_windows, n_unique = %d, %d for %d, %d" % (st.n_windows, st.n_unique, n_windows, len(want["kmers"]))
    return None


def blocks(K):
    lo = max(K - 1, 1)
    return [(a, min(a + BLOCK, L_MAX + 1)) for a in range(lo, L_MAX + 1, BLOCK)]


CASES = [(K, a, b) for K in (1, 9, 25, 32) for a, b in blocks(K)]


@pytest.mark.parametrize("K,lo,hi", CASES, ids=["K%d-L%d-%d" % (K, a, b - 1) for K, a, b in CASES])
def test_uniform_records_every_length(ctx, K, lo, hi):
    """reads of exactly L bases, every L of the block, through every first-pass route; every 7th L also one base short in the
    last read, and with a separator and a base swapped for 'N' and '\\n' (the stream still looks uniform by its first newline
    and its length: only the check of every separator on the device can tell).

    What this found: reads with so few windows that one thread takes a whole record (W <= 8 in the ranged pass, W <= 16 in the
    pipeline, where the tile still fits and pays: L = 15, 16 and 16..24 at K = 9, L = 25..32 and 25..30 at K = 25, L = 32..39 at
    K = 32).  The division thread / cpr by a multiply had ceil(2^32 / 1) cut to 32 bits, 0, as its inverse: every thread took
    itself for a chunk of record 0.  The ranged pass then disagreed with its histogram (ZK_EINTERNAL); the pipeline returned a wrong table."""
    bad = None
    try:
        for L in range(lo, hi):
            reads = W.uniform_reads(L, K, seed=L)
            streams = [("uniform", W.stream_of(reads), ROUTES)]
            if L % 7 == 0:
                a, b = W.near_uniform(reads)
                streams += [("last read short", a, (ROUTES[0], ROUTES[3])), ("N and newline swapped", b, (ROUTES[0], ROUTES[3]))]
            for name, stream, routes in streams:
                want = zo.kmerize(K, [stream])
                if L == K - 1 and name == "uniform":
                    assert len(want["kmers"]) == 0
                d = ctx.upload_stream(stream)
                for knobs in routes:
                    ctx.tune(**knobs)
                    what = differs(ctx, d, K, want)
                    if what:
                        bad = (K, L, name, knobs, what)
                        break
                if bad:
                    break
            if bad:
                break
    finally:
        ctx.tune(stream_pass=1, stream_ranges=0)
    assert bad is None, "zk_kmerize differs from the oracle at (K, L, stream, knobs, what) = %r" % (bad,)


@functools.lru_cache(maxsize=None)
def mixed_input():
    """about 300 KB: reads of 20 to 200 bases from a genome of 5 000, homopolymers, short periods (palindromes at even K), N at 0.5 %"""
    rng = np.random.default_rng(32)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=5000)]
    reads = []
    total = 0
    while total < 290_000:
        n = int(rng.integers(20, 201))
        p = int(rng.integers(0, len(genome) - n + 1))
        r = genome[p:p + n].copy()
        r[rng.random(n) < 0.005] = ord("N")
        reads.append(r.tobytes())
        total += n + 1
    reads += [b"A" * 150] * 8 + [b"ACGT" * 30] * 8 + [b"AT" * 40] * 8 + [b"GC" * 40] * 8
    return tuple(reads)


@pytest.mark.parametrize("K", range(1, 33))
def test_every_K(ctx, K):
    reads = list(mixed_input())
    stream = W.stream_of(reads)
    want = zo.kmerize(K, reads)
    both = np.concatenate([zo.kmers_list(K, r, True) for r in reads])
    k, c = W.counted(both)
    assert np.array_equal(k, want["kmers"]) and np.array_equal(c, want["counts"])
    if K % 2 == 0:
        assert np.any(want["kmers"] == W.revcomp(want["kmers"], K)), "no palindrome in the input"
    d = ctx.upload_stream(stream)
    # zk_encode and the independent encoder
    out, acgt = ctx.encode(d, K, True)
    assert np.array_equal(out.to_host(), both) and acgt == want["acgt"]
    out, acgt = ctx.encode(d, K, False)
    assert np.array_equal(out.to_host(), both[0::2]) and acgt == W.acgt_of(both[0::2])
    M = (1 << 64) - 1
    sums = [len(both), int(both.sum(dtype=U64)), int(sum(zo.murmer(int(x), 0) * int(n) for x, n in zip(k, c)) & M)]
    assert [int(v) for v in ctx.stream_checksum(d, K)] + ctx.stream_acgt(d, K) == sums + want["acgt"]
    # zk_kmerize: its defaults, and the knobs the plan may or may not heed at this K
    rc = W.revcomp(want["kmers"], K)
    keep = want["kmers"] <= rc
    ck_want, cc_want = want["kmers"][keep], want["counts"][keep].copy()
    cc_want[ck_want == rc[keep]] //= 2
    try:
        assert differs(ctx, d, K, want) is None
        ctx.tune(early_collapse=0)
        assert differs(ctx, d, K, want) is None, "early_collapse=0"
        ctx.tune(early_collapse=1)
        assert differs(ctx, d, K, want, native.KMERIZE_BOTH) is None, "both"
        ck, cc, st = ctx.kmerize(d, K, native.KMERIZE_CANONICAL_ONLY)
        assert np.array_equal(ck.to_host(), ck_want) and np.array_equal(cc.to_host(), cc_want)
        assert st.n_canonical == len(ck_want) and list(st.acgt) == want["acgt"]
        ek, ec = ctx.mirror_expand(ck, cc, K)
        assert np.array_equal(ek.to_host(), want["kmers"]) and np.array_equal(ec.to_host(), want["counts"])
        for bits in (9, 18):
            ctx.tune(dedupe_bits=bits)
            assert differs(ctx, d, K, want) is None, ("dedupe_bits", bits)
    finally:
        ctx.tune(early_collapse=1, dedupe_bits=0)
