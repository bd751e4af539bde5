"""The strand route with the block dedupe's unsorted output (ZK_TUNE_STRAND_BLOCKS 1: dedupe2_kernel writes each block's words in
table order, the persistent union sorts C_b with M_b in LDS) against the route before it (2: sorted blocks, one union workgroup per
block) and the oracle, at odd K with 18 block bits forced on small inputs (ZK_TUNE_DEDUPE_BITS): the plain route, blocks declined by
the union (C_b alone several tiles), the route not taken after an unsorted dedupe (counts beyond the packed field: the blocks are
sorted by dedupe_sort_blocks before the dense copy), blocks that dedupe2_kernel declines to dedupe_kernel mixed with unsorted ones,
the last-resort merge-path union (3: declined blocks go there directly), several calls on one context and one on a fresh context."""
import numpy as np
import pytest

from oracle import zkoracle as zo
from zotmer_amd import native, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def stream_of(reads):
    return ("".join(r + "\n" for r in reads)).encode()


def _revcomp(k, K):
    k = np.asarray(k, dtype=np.uint64)
    r = np.zeros_like(k)
    for i in range(K):
        r = (r << np.uint64(2)) | (np.uint64(3) - ((k >> np.uint64(2 * i)) & np.uint64(3)))
    return r


def _inputs(K):
    rng = np.random.default_rng(900 + K)
    deep = synth.read_strings(37, 0, 6000, 150, genome=12000, sub_thr=synth.frac32(0.004), n_thr=synth.frac32(0.001))

    def rnd(n):
        return "".join(rng.choice(list("ACGT"), size=n))
    # 40 000 distinct canonical k-mers under one 9-base prefix: C_b alone five times a union tile (and above a dedupe2 table: dedupe_kernel's)
    big_c = deep + ["AAAAAAAAA" + rnd(K - 9) for _ in range(40000)] * 2
    # 9 000 under one prefix: more than a union tile, within a dedupe2 table (counted unsorted, declined by the union)
    mid_c = deep + ["AAAAAAAAC" + rnd(K - 9) for _ in range(9000)] * 2
    # poly-A and a dinucleotide repeat: counts beyond the packed field at K = 25 and 27 (the route is not taken; at K = 27 the tags are
    # wider than dedupe2_kernel's and every block is counted sorted by dedupe_kernel)
    heavy = deep[:1500] + ["A" * 150] * 400 + ["AC" * 75] * 300
    return {"deep": deep, "big_c_block": big_c, "mid_c_block": mid_c, "heavy_counts": heavy}


def _want(K, reads):
    want = zo.kmerize(K, reads)
    wk = np.asarray(want["kmers"], dtype=np.uint64)
    hv, hf = zo.hist(want["counts"])
    return want, int(np.count_nonzero(wk <= _revcomp(wk, K))), {int(a): int(b) for a, b in zip(hv, hf)}


def _check(c, d, K, want, n_can, want_hist, what):
    k, cn, st = c.kmerize(d, K)
    assert np.array_equal(k.to_host(), want["kmers"]), what
    assert np.array_equal(cn.to_host(), want["counts"]), what
    assert st.n_unique == len(want["kmers"]) and st.n_canonical == n_can, (what, st.n_canonical, n_can)
    assert c.hist(cn) == want_hist, what


def _run(c, d, K, sb, **tune):
    c.tune(dedupe_bits=18, strand_blocks=sb, **tune)
    c.profile(True)
    k, cn, st = c.kmerize(d, K)
    prof = c.profile_read()
    c.profile(False)
    return k, cn, st, prof


@pytest.mark.parametrize("K", [21, 25, 27])
def test_unsorted_dedupe_route_vs_sorted_and_oracle(ctx, K):
    try:
        for name, reads in _inputs(K).items():
            want, n_can, want_hist = _want(K, reads)
            d = ctx.upload_stream(stream_of(reads))
            for limit in (65536, 6):          # 6: every block of six keys or more goes to dedupe_kernel (sorted), the rest stay unsorted
                prof = {}
                for sb in (1, 2, 3, 0):
                    k, cn, st, prof[sb] = _run(ctx, d, K, sb, dedupe_limit=limit)
                    what = (name, K, limit, sb)
                    assert np.array_equal(k.to_host(), want["kmers"]), what
                    assert np.array_equal(cn.to_host(), want["counts"]), what
                    assert st.n_unique == len(want["kmers"]) and st.n_canonical == n_can, (what, st.n_canonical, n_can)
                    assert ctx.hist(cn) == want_hist, what
                sel = {sb: prof[sb].get("select", {}).get("bytes", 0) for sb in prof}
                rle = {sb: prof[sb].get("rle", {}).get("launches", 0) for sb in prof}
                uni = {sb: prof[sb].get("union_sum", {}).get("launches", 0) for sb in prof}
                du = 1 if 2 * K - 18 <= 32 else 0          # dedupe2_kernel (and its unsorted output) takes tags of up to 32 bits: K <= 25
                route = sel[0] - sel[1] == 8 * n_can          # the copy of the strand route books 8 B less a canonical k-mer
                assert route == (sel[0] - sel[2] == 8 * n_can), (name, K, limit, prof)
                assert route == (name != "heavy_counts" or K == 21), (name, K, limit, prof)
                if not route:
                    # the route not taken after the unsorted dedupe: one more launch under the dedupe's record -- the blocks sorted
                    assert rle[1] == rle[2] + du and sel[1] == sel[2] and uni[1] == uni[2], (name, K, limit, prof)
                elif name in ("big_c_block", "mid_c_block"):
                    assert uni[1] == uni[2] == uni[0] + 1, (name, K, limit, prof)          # the declined blocks' kernel on both
                    assert rle[3] == rle[1] + du, (name, K, limit, prof)          # the last resort sorted the blocks
                else:
                    assert rle[1] == rle[2] and uni[1] == uni[2] == uni[0], (name, K, limit, prof)
    finally:
        ctx.tune(dedupe_bits=0, strand_blocks=1, dedupe_limit=65536)


def test_unsorted_route_fresh_context_and_repeated_calls():
    K = 25
    reads = _inputs(K)["mid_c_block"]
    want, n_can, want_hist = _want(K, reads)
    with native.Context(0) as c:
        c.tune(dedupe_bits=18)
        d = c.upload_stream(stream_of(reads))
        for i in range(3):
            _check(c, d, K, want, n_can, want_hist, ("call", i))
