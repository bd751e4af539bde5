"""
The wide form of the first sort pass (stream_pass.hip, ZK_TUNE_STREAM_PASS 1: one 1024-thread workgroup per CU, tiles of 8192
windows, whole 128-byte units, a digit's left-over keys waiting in a carry area of their own) against the 512-thread form (variant 2)
and the oracle: the same k-mers, counts, acgt and number of distinct k-mers, for the stream shapes that stress the carry logic,
the tiling and the cut into ranges.
"""
import numpy as np
import pytest

from oracle import zkoracle as zo
from zotmer_amd import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def stream_of(reads):
    return ("".join(r + "\n" for r in reads)).encode()


def reads_of(shape, rng):
    def rnd(n, p_n=0.0, alphabet="ACGT"):
        a = rng.choice(list(alphabet), size=n)
        a[rng.random(n) < p_n] = "N"
        return "".join(a)
    genome = rnd(30000)

    def sampled(L):
        p = int(rng.integers(0, len(genome) - L))
        return genome[p:p + L]
    if shape == "poly_a":                # one digit fills whole tiles: its runs of 16 and its carry across many tiles
        return ["A" * 150] * 8000 + [sampled(150) for _ in range(4000)] + ["T" * 150] * 4000 + ["A" * 150] * 500
    if shape == "u150":                  # uniform records: tiles follow them (64 records of 151 bytes a tile)
        return [sampled(150) for _ in range(20000)]
    if shape == "u150_odd":              # uniform, the stream's length not a multiple of 16
        return [sampled(150) for _ in range(7777)]
    if shape == "u100":
        return [sampled(100) for _ in range(12000)]
    if shape == "var_80_150":            # never uniform: tiles of positions
        return [sampled(int(rng.integers(80, 151))) for _ in range(15000)]
    if shape == "long_records":          # records longer than a tile
        return [rnd(int(rng.integers(9000, 40000)), 0.0005) for _ in range(40)]
    if shape == "small":                 # a few keys per (range, digit): pieces shorter than a unit, off the 128-byte grid
        return [rnd(int(rng.integers(30, 151)), 0.002) for _ in range(600)]
    raise ValueError(shape)


CASES = [("poly_a", 25), ("u150", 25), ("u150", 9), ("u150", 31), ("u150", 32), ("u150_odd", 25), ("u100", 31),
         ("var_80_150", 25), ("var_80_150", 32), ("long_records", 25), ("long_records", 9), ("small", 25), ("small", 32)]


def run(ctx, d, K, flags, variant, ranges):
    ctx.tune(stream_pass=variant, stream_ranges=ranges)
    k, c, st = ctx.kmerize(d, K, flags)
    return k.to_host(), c.to_host(), list(st.acgt), int(st.n_unique)


@pytest.mark.parametrize("shape,K", CASES)
@pytest.mark.parametrize("flags", [native.KMERIZE_CANONICAL, native.KMERIZE_BOTH], ids=["canonical", "both"])
def test_wide_pass0_matches_512_thread_pass_and_oracle(ctx, shape, K, flags):
    rng = np.random.default_rng(sum(map(ord, shape)) + K)
    reads = reads_of(shape, rng)
    s = stream_of(reads)
    if shape == "u150_odd":
        assert len(s) % 16
    want = zo.kmerize(K, reads)
    d = ctx.upload_stream(s)
    # 1 range (every tile in one workgroup), 3 and 7 (not dividing the tile count), 61 (tiny pieces), the default (one per CU)
    all_ranges = (1, 3, 7, 61, 0) if shape == "small" else (1, 3, 0)
    try:
        for ranges in all_ranges:
            got = {v: run(ctx, d, K, flags, v, ranges) for v in (1, 2)}
            for v, (kh, ch, acgt, nu) in got.items():
                where = (shape, K, flags, ranges, v)
                assert np.array_equal(kh, want["kmers"]), where
                assert np.array_equal(ch, want["counts"]), where
                assert acgt == want["acgt"] and nu == len(want["kmers"]), where
            assert got[1][2:] == got[2][2:]
    finally:
        ctx.tune(stream_pass=1, stream_ranges=0)


def test_stream_pass_variants_are_checked(ctx):
    for v in (0, 1, 2, 3):
        ctx.tune(stream_pass=v)
    ctx.tune(stream_pass=1)
    with pytest.raises(Exception):
        ctx.tune(stream_pass=4)
    ctx.tune(stream_pass=1)
