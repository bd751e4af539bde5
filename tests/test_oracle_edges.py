"""
The CPU oracle at the ends of its ranges, against plain Python ints: the all-T 32-mer (2^64 - 1) and its mirror 0, keys and counts
at or above 2^63, and the codec64 limit of 2^60.  The GPU edge tests (test_gpu_domain_edges.py) trust the oracle there.
"""
from collections import Counter

import numpy as np
import pytest

from oracle import zkoracle as zo

TOP = (1 << 64) - 1
BASE = {"A": 0, "C": 1, "G": 2, "T": 3}


def _kmer(s):
    x = 0
    for ch in s:
        x = (x << 2) | BASE[ch]
    return x


def _rc(K, x):
    y = 0
    for _ in range(K):
        y = (y << 2) | (3 - (x & 3))
        x >>= 2
    return y


def _table(K, reads):
    """zot kmerize's table in Python ints: every window x and rc(x) counted, acgt[x & 3] over every instance"""
    cnt, acgt = Counter(), [0, 0, 0, 0]
    for r in reads:
        for i in range(len(r) - K + 1):
            x = _kmer(r[i:i + K])
            for y in (x, _rc(K, x)):
                cnt[y] += 1
                acgt[y & 3] += 1
    ks = sorted(cnt)
    return ks, [cnt[k] for k in ks], acgt


@pytest.mark.parametrize("reads", [["T" * 40], ["A" * 33], ["T" * 31 + "G", "C" + "A" * 31], ["T" * 40 + "ACGTTGCA" * 3, "G" * 32]])
def test_kmerize_k32_ends(reads):
    K = 32
    ks, cs, acgt = _table(K, reads)
    for mode, p in ((0, 0.0), (1, 9.0)):          # plain, and -D subsample with a p that keeps every k-mer
        got = zo.kmerize(K, reads, mode=mode, p=p)
        assert [int(v) for v in got["kmers"]] == ks and [int(v) for v in got["counts"]] == cs and got["acgt"] == acgt, mode
    if reads == ["T" * 40]:
        assert ks == [0, TOP] and cs == [9, 9] and acgt == [9, 0, 0, 9]
    for r in reads:
        fwd = [_kmer(r[i:i + K]) for i in range(len(r) - K + 1)]
        assert [int(v) for v in zo.kmers_list(K, r, False)] == fwd
        assert [int(v) for v in zo.kmers_list(K, r, True)] == [y for x in fwd for y in (x, _rc(K, x))]


def test_union_sum_and_hist_beyond_2_63():
    xs = [1, (1 << 63) - 1, 1 << 63, (1 << 63) + 5, TOP - 1]
    xc = [1 << 63, 5, (1 << 62) + 1, 1, 7]
    ys = [0, 1 << 63, (1 << 63) + 4, TOP - 1, TOP]
    yc = [3, (1 << 62) - 1, 1 << 63, TOP - 7, (1 << 63) + 9]
    want = Counter()
    for k, c in list(zip(xs, xc)) + list(zip(ys, yc)):
        want[k] += c
    assert all(v <= TOP for v in want.values())
    zs, zc = zo.union_sum(np.array(xs, np.uint64), np.array(xc, np.uint64), np.array(ys, np.uint64), np.array(yc, np.uint64))
    assert [int(v) for v in zs] == sorted(want) and [int(v) for v in zc] == [want[k] for k in sorted(want)]
    counts = [1 << 63, 1 << 63, TOP, 1 << 32, (1 << 32) - 1, 4095, 4096, 1, 1, 1, (1 << 63) + 1, TOP]
    hv, hf = zo.hist(np.array(counts, np.uint64))
    h = Counter(counts)
    assert [int(v) for v in hv] == sorted(h) and [int(v) for v in hf] == [h[v] for v in sorted(h)]


def test_codec64_at_2_60():
    e60 = 1 << 60
    ok = [0, 1, e60 - 2, e60 - 1, (1 << 30) - 1, 1 << 30, (1 << 59) + 3]
    assert [int(v) for v in zo.codec64_decode(zo.codec64_encode(np.array(ok, np.uint64)))] == ok
    for bad in (e60, e60 + 1, 1 << 63, TOP):
        with pytest.raises(IndexError):
            zo.codec64_encode(np.array(ok[:3] + [bad] + ok[3:], np.uint64))
    # the delta form: steps of up to 2^60 - 1 reach 2^64 - 1 exactly; a step of 2^60 has no code
    keys = [15] + [15 + i * (e60 - 1) for i in range(1, 17)]
    assert keys[-1] == TOP
    d = zo.delta(np.array(keys, np.uint64))
    assert [int(v) for v in d] == [15] + [e60 - 1] * 16
    assert [int(v) for v in zo.undelta(zo.codec64_decode(zo.codec64_encode(d)))] == keys
    with pytest.raises(IndexError):
        zo.codec64_encode(zo.delta(np.array([0, e60], np.uint64)))
