"""The block union of the strands in its block-local form (strand_blocks.hip, strand_block_union_kernel<true>: 32-bit tags below the 18
block bits, K <= 25) and in the generic one (K = 27), on blocks built entry by entry: against the oracle and against the same call
with strand_blocks=0 (the mirror sort and the merge-path union), exactly.

Every read is one k-mer long (and given twice), so the table is the reads' k-mers and their reverse complements and nothing else, and block b of the
table (C_b and M_b together) holds exactly the k-mers that start with the nine bases b.  A k-mer is only taken when its reverse
complement starts none of the prefixes the shapes are built under, so every block below has the size it was built with; the sizes
are counted again in the oracle's table before a route is asserted.  Taken and declined are told apart as in
tests/test_gpu_strand_blocks.py: the declined blocks' kernel is one more `union_sum` record.

Shapes (all under their own 9-base prefix):
  block 0 (AAAAAAAAA: its k-mers are canonical, so M_b is empty) and block 2^18 - 1 (TTTTTTTTT: none is, so C_b is empty);
  a block of one entry; blocks of 513 and 1023 entries (m = 1 and 511 mod 512: the slots beyond the block's entries in the last round
  of 512 are nearly all and nearly none of the lanes); a block of exactly 8192 = CAP entries (taken) and of 8193 (declined);
  a group (the 9 bases and the next 11 bits shared) of exactly 128 entries (taken) and of 129 (declined);
  the tags 0 and 2^below - 1 (suffix all A, suffix all T) in one block;
  at K = 25 one k-mer read 16 383 times: the packed count field's maximum.
K = 13 is the smallest odd K the forced plan takes (plan_kmerize: 18 + 9 / 2 < 2 K, so K >= 12; mirror_groups: 2 K >= 26): 8 bits
below the block, the group is the whole tag (a shift of max(8 - 11, 0) = 0), a block holds 256 k-mers at most -- the shapes that fit
are built, and a block with 80 of its 256."""
import functools
import random

import numpy as np
import pytest

from oracle import zkoracle as zo
from tests import _core_cases as cc
from zotmer_amd import native

pytestmark = pytest.mark.gpu

CAP = 8192                # strand_blocks.hip: TS_BLOCK * SB_ITEMS
GROUP_MAX = 128           # SB_GROUP_MAX
BLOCK_BITS = 18
K_MIN = 13

P_FIRST, P_LAST = "AAAAAAAAA", "TTTTTTTTT"
P_ONE, P_M1, P_M511, P_CAP, P_GROUP, P_ENDS, P_MOST = ("GATTACAGA", "ACCGGTTAC", "CGATCGTAG", "CCGTTGCAA", "GTTGACCAT", "CAGTCAGTC",
                                                       "TGCATCGGA")
SPECIAL = (P_FIRST, P_LAST, P_ONE, P_M1, P_M511, P_CAP, P_GROUP, P_ENDS, P_MOST)
COMP = str.maketrans("ACGT", "TGCA")


def _rc(s):
    return s[::-1].translate(COMP)


def _code(s):
    v = 0
    for ch in s:
        v = (v << 2) | "ACGT".index(ch)
    return v


def _text(v, n):
    return "".join("ACGT"[(v >> (2 * (n - 1 - i))) & 3] for i in range(n))


class _Builder:
    """k-mers under chosen prefixes; none is taken twice, and none whose reverse complement starts a special prefix"""

    def __init__(self, K, seed):
        self.K, self.rng, self.seen, self.reads = K, random.Random(seed), set(), []

    def add(self, kmer, anywhere=False):
        r = _rc(kmer)
        if kmer in self.seen or r in self.seen or (r[:9] in SPECIAL and not anywhere):
            return False
        self.seen.add(kmer)
        self.reads.append(kmer)
        return True

    def fill(self, prefix, n, keep=lambda s: True, head=""):
        """n k-mers prefix + head + random bases (keep(suffix): which suffixes may be drawn)"""
        free = self.K - len(prefix) - len(head)
        assert n <= 4 ** free // 3, (prefix, n, free)
        got = 0
        while got < n:
            s = head + _text(self.rng.getrandbits(2 * free), free)
            if keep(s) and self.add(prefix + s):
                got += 1

    def background(self, n):
        got = 0
        while got < n:
            s = _text(self.rng.getrandbits(2 * self.K), self.K)
            if s[:9] not in SPECIAL and self.add(s):
                got += 1


def _pack_bits(K):
    return min(64 - 2 * K, 31)


@functools.lru_cache(maxsize=None)
def _case(K, name):
    """-> (reads, {prefix: entries of its block}, (the group's key bits, its entries) or None)"""
    b = _Builder(K, 9000 + K)
    sizes, group, heavy = {}, None, []
    b.background(1500)
    if name == "shapes":
        # (not ...T: canonical under AAAAAAAAA; not ...A: not canonical under TTTTTTTTT)
        n_ends = min(40, 4 ** (K - 9) // 4)
        b.fill(P_FIRST, n_ends, keep=lambda s: s[-1] != "T")
        b.fill(P_LAST, n_ends, keep=lambda s: s[-1] != "A")
        b.fill(P_ONE, 1)
        # (from K = 18 on the mirror image of the suffix of T starts with nine A, a canonical k-mer of block 0, and that of the suffix of
        # A with nine T, a k-mer of block 2^18 - 1 that is not canonical: one entry more in each, and block 0 is still C_b alone)
        assert b.add(P_ENDS + "A" * (K - 9), anywhere=True) and b.add(P_ENDS + "T" * (K - 9), anywhere=True)
        far = 1 if K - 9 >= 9 else 0
        b.fill(P_ENDS, 5 if K > K_MIN else 2)
        sizes.update({P_FIRST: n_ends + far, P_LAST: n_ends + far, P_ONE: 1, P_ENDS: 7 if K > K_MIN else 4})
        if K > K_MIN:
            b.fill(P_M1, 513)
            b.fill(P_M511, 1023)
            b.fill(P_CAP, CAP)
            sizes.update({P_M1: 513, P_M511: 1023, P_CAP: CAP})
        else:
            b.fill(P_MOST, 80)          # (a third of the 256 the block can hold: the builder draws, it does not enumerate)
            sizes[P_MOST] = 80
        if K == 25:
            b.background(1)
            heavy = [b.reads.pop()] * ((1 << _pack_bits(K)) - 1)
    elif name == "over_cap":
        b.fill(P_CAP, CAP + 1)
        sizes[P_CAP] = CAP + 1
    else:
        n = GROUP_MAX + (1 if name == "group_129" else 0)
        head = "CGTAC"          # 10 of the group's 11 bits; the 11th: the suffix's first base is A or C
        b.fill(P_GROUP, n, keep=lambda s: s[len(head)] in "AC", head=head)
        b.fill(P_GROUP, 300, keep=lambda s: not s.startswith(head))
        sizes[P_GROUP] = n + 300
        group = (((_code(P_GROUP + head) << 1) | 0), n)          # the key's top 18 + 11 bits
    # every read twice, as tests/_core_cases.py::dense_block gives its own: zk_kmerize takes the block dedupe only for reads that
    # repeat their k-mers (at most 0.6 of a sample distinct)
    return b.reads * 2 + heavy, sizes, group


def _check_sizes(K, want, sizes, group):
    """the blocks (and the group) in the oracle's table have the sizes they were built with"""
    wk = np.asarray(want["kmers"], dtype=np.uint64)
    blocks = (wk >> np.uint64(2 * K - BLOCK_BITS)).astype(np.int64)
    for prefix, n in sizes.items():
        assert int(np.count_nonzero(blocks == _code(prefix))) == n, (K, prefix, n)
    if group is not None:
        gkeys = (wk >> np.uint64(2 * K - BLOCK_BITS - 11)).astype(np.int64)
        assert int(np.count_nonzero(gkeys == group[0])) == group[1], (K, group)
    canon = wk <= cc.revcomp(wk, K)
    if P_FIRST in sizes:
        first, last = blocks == 0, blocks == (1 << BLOCK_BITS) - 1
        assert first.any() and canon[first].all(), "block 0: C_b alone"
        assert last.any() and not canon[last].any(), "block 2^18 - 1: M_b alone"
        ends = wk[blocks == _code(P_ENDS)] & np.uint64((1 << (2 * K - BLOCK_BITS)) - 1)
        assert int(ends.min()) == 0 and int(ends.max()) == (1 << (2 * K - BLOCK_BITS)) - 1, "the tags 0 and 2^below - 1 in one block"
    return int(np.count_nonzero(canon))


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


CASES = [(K, name) for K in (K_MIN, 21, 23, 25, 27) for name in ("shapes", "over_cap", "group_128", "group_129")
         if K > K_MIN or name == "shapes"]


@pytest.mark.parametrize("K,name", CASES)
def test_strand_union_tags(ctx, K, name):
    reads, sizes, group = _case(K, name)
    assert len(reads) <= 40000
    want = zo.kmerize(K, reads)
    n_can = _check_sizes(K, want, sizes, group)
    if K == 25 and name == "shapes":
        assert int(np.max(want["counts"])) == (1 << _pack_bits(K)) - 1 == 16383
    hv, hf = zo.hist(want["counts"])
    want_hist = {int(a): int(b) for a, b in zip(hv, hf)}
    d = ctx.upload_stream(cc.stream_of(reads))
    prof = {}
    try:
        for sb in (1, 0):
            ctx.tune(dedupe_bits=18, strand_blocks=sb)
            ctx.profile(True)
            k, c, st = ctx.kmerize(d, K)
            prof[sb] = ctx.profile_read()
            ctx.profile(False)
            assert np.array_equal(k.to_host(), want["kmers"]), (K, name, sb)
            assert np.array_equal(c.to_host(), want["counts"]), (K, name, sb)
            assert st.n_unique == len(want["kmers"]) and st.n_canonical == n_can, (K, name, sb, st.n_canonical, n_can)
            assert list(st.acgt) == want["acgt"]
            assert ctx.hist(c) == want_hist, (K, name, sb)
    finally:
        ctx.tune(dedupe_bits=0, strand_blocks=1)
    sel = {sb: prof[sb].get("select", {}).get("bytes", 0) for sb in (1, 0)}
    uni = {sb: prof[sb].get("union_sum", {}).get("launches", 0) for sb in (1, 0)}
    if name == "group_129":
        # declined: one more union record at least.  The block fits one sub-tile, whose groups are the block's own, so
        # strand_big_block_kernel finds the same crowded group and the union is made the other way (no 8 bytes a k-mer saved)
        assert uni[1] - uni[0] >= 1, (K, name, prof)
    else:
        assert sel[0] - sel[1] == 8 * n_can, (K, name, prof)          # the route, and the union was not made the other way
        assert uni[1] - uni[0] == (1 if name == "over_cap" else 0), (K, name, prof)
