"""The inputs of tests/test_gpu_count_fields.py (tests/_count_edge_cases.py), checked without a device: every case really holds the
counts it claims, at the places it claims, and the builders' own assertions fire on inputs that break their promises.  A case that
drifted off its edge would leave the GPU tests green and worthless."""
import numpy as np
import pytest

from tests import _count_edge_cases as E
from tests._core_cases import revcomp

U64 = np.uint64


def table_count(want, x):
    i = int(np.searchsorted(want["kmers"], U64(x)))
    assert i < len(want["kmers"]) and int(want["kmers"][i]) == x, "the k-mer is not in the oracle's table"
    return int(want["counts"][i])


@pytest.mark.parametrize("K,c,spread,background,same_block", E.edge_cases(),
                         ids=["K%d-%d-%s-%s%s" % (K, c, s, b, "-one_block" if sb else "") for K, c, s, b, sb in E.edge_cases()])
def test_targets_have_exactly_their_count(K, c, spread, background, same_block):
    """the oracle's table holds every target with exactly c on both strands (the palindrome with c + c), and nothing above them"""
    reads, targets = E.edge_reads(K, c, spread, background, same_block)
    want = E.edge_want(K, c, spread, background, same_block)
    assert len(targets) == (4 if K % 2 == 0 else 3) and all(len(t) == K for t in targets)
    assert (K % 2 == 0) == E.is_palindrome(targets[-1])
    for x, n in E.expected_counts(K, c, targets).items():
        assert table_count(want, x) == n
    assert int(want["counts"].max()) == (2 * c if K % 2 == 0 else c) and want["max_canonical"] == c
    assert len(reads) == len(E.background_reads(background)) + c * len(targets)
    # the ends of the key range, and the block the targets of the forced plan share
    can = [E.canonical(t) for t in targets]
    assert can[0] == 1 and can[2] >> (2 * K - 2) == 3
    blocks = [x >> (2 * K - E.BLOCK_BITS) for x in can]
    assert (blocks[0] == blocks[1]) == same_block and len(set(blocks)) == len(blocks) - int(same_block)
    # the spread: one stretch, or never more copies between two background reads than an even deal gives
    at = [i for i, r in enumerate(reads) if len(r) == K]
    if spread == "together":
        assert at == list(range(at[0], at[0] + c * len(targets)))
        assert all(reads[at[0] + j * c] == t and reads[at[0] + j * c + c - 1] == t for j, t in enumerate(targets))
    else:
        gaps = np.diff(np.array([i for i, r in enumerate(reads) if len(r) != K] + [len(reads)])) - 1
        per = -(-c // len(E.background_reads(background)))
        assert int(gaps.max()) <= per * len(targets) and int(gaps.sum()) == c * len(targets)
        assert c < len(gaps) or int(gaps.min()) >= (per - 1) * len(targets)


@pytest.mark.parametrize("copies", E.LDS_BLOCKS, ids=["+".join(map(str, b)) for b in E.LDS_BLOCKS])
@pytest.mark.parametrize("K", E.LDS_K)
def test_block_holds_exactly_its_keys(K, copies):
    reads, kmers = E.block_reads(K, list(copies))
    want = E.block_want(K, copies)
    assert [table_count(want, E.encode(t)) for t in kmers] == list(copies)
    assert want["max_canonical"] == max(copies)
    k = want["kmers"]
    canon = k <= revcomp(k, K)
    block = E.encode(kmers[0]) >> (2 * K - E.BLOCK_BITS)
    inside = canon & (k >> U64(2 * K - E.BLOCK_BITS) == U64(block))
    assert int(np.count_nonzero(inside)) == len(copies) and int(want["counts"][inside].sum()) == sum(copies)
    assert all(E.encode(t) >> (2 * K - E.BLOCK_BITS) == block and E.canonical(t) == E.encode(t) for t in kmers)


@pytest.mark.parametrize("K,c", E.DENSE_CASES)
def test_dense_block_holds_the_targets(K, c):
    reads, targets = E.dense_block_reads(K, c)
    want = E.dense_block_want(K, c)
    for x, n in E.expected_counts(K, c, targets).items():
        assert table_count(want, x) == n
    assert want["max_canonical"] == c
    k = want["kmers"]
    inside = (k <= revcomp(k, K)) & (k >> U64(2 * K - E.BLOCK_BITS) == U64(0))
    assert int(np.count_nonzero(inside)) >= E.DENSE + 2 and int(want["counts"][inside].sum()) >= E.DENSE + 2 * c
    assert [E.canonical(t) >> (2 * K - E.BLOCK_BITS) for t in targets[:2]] == [0, 0]


def test_builders_are_deterministic():
    a, ta = E.edge_reads(27, 1023, "strided", "deep")
    E.background_reads.cache_clear()
    b, tb = E.edge_reads(27, 1023, "strided", "deep")
    assert a == b and ta == tb == E.target_kmers(27)
    x = E.mirror_lists(24, 1 << 16, "last")
    E.mirror_lists.cache_clear()
    y = E.mirror_lists(24, 1 << 16, "last")
    assert all(np.array_equal(p, q) for p, q in zip(x[:4], y[:4])) and x[4] == y[4]
    assert E.block_reads(21, [65534, 1]) == E.block_reads(21, [65534, 1])


def test_pack_bits_restated():
    assert [E.pack_bits(K) for K in (28, 27, 26, 25, 24, 23, 21, 20, 17, 16, 9)] == [0, 10, 12, 14, 16, 18, 22, 24, 30, 31, 31]


# ---- the builders refuse inputs that break their promises -------------------------------------------------------------------------------

def test_deep_background_must_repeat():
    with pytest.raises(AssertionError, match="must repeat"):
        E.check_background("deep", 25, 16384, reads=E.background_reads("flat"))


@pytest.mark.parametrize("name", ["flat", "wide"])
def test_flat_background_must_not_repeat(name):
    with pytest.raises(AssertionError, match="must not repeat"):
        E.check_background(name, 25, 16384, reads=E.background_reads("deep"))


def test_wide_background_must_have_2p16_kmers():
    with pytest.raises(AssertionError, match="2\\^16"):
        E.check_background("wide", 25, 16384, reads=E.background_reads("wide")[:300])


def test_background_counts_must_stay_below_half_the_bound():
    largest = E.background_table("deep", 27)[3]
    E.check_background("deep", 27, 2 * largest)
    with pytest.raises(AssertionError, match="half the bound"):
        E.check_background("deep", 27, 2 * largest - 1)
    with pytest.raises(AssertionError, match="half the bound"):
        E.edge_reads(27, 2 * largest - 1, "together", "deep")


def test_unknown_spread_and_background():
    with pytest.raises(AssertionError):
        E.edge_reads(27, 1023, "scattered", "deep")
    with pytest.raises(ValueError):
        E.edge_reads(27, 1023, "together", "shallow")


# ---- the counted lists of zk_mirror_expand --------------------------------------------------------------------------------------------

MIRROR = [(K, (1 << E.pack_bits(K)) + e, False) for K in (25, 27, 24, 16) for e in (-1, 0)] + \
         [(24, n, True) for n in ((1 << 15) - 1, 1 << 15, (1 << 16) - 1)] + [(16, (1 << 31) - 1, True), (16, 1 << 31, True)]


@pytest.mark.parametrize("where", E.WHERES)
@pytest.mark.parametrize("K,bound,palindrome", MIRROR, ids=["K%d-%d%s" % (K, b, "-palindrome" if p else "") for K, b, p in MIRROR])
def test_mirror_lists(K, bound, palindrome, where):
    c, n, keys, cnt, at = E.mirror_lists(K, bound, where, palindrome)
    assert len(c) >= 1 << 16 and np.all(c[1:] > c[:-1]) and np.array_equal(c, np.minimum(c, revcomp(c, K)))
    assert n.dtype == np.uint32 and int(n.min()) >= 1 and int(n.max()) == bound == int(n[at])
    assert int(np.count_nonzero(n == bound)) == 1 and int(np.count_nonzero(n == bound - 1)) >= 3
    pals = np.flatnonzero(revcomp(c, K) == c)
    pick = np.flatnonzero((revcomp(c, K) == c) == palindrome)
    assert at == int(pick[{"first": 0, "middle": len(pick) // 2, "last": len(pick) - 1}[where]])
    assert (K % 2 == 0) == (len(pals) > 0)
    # the table: both strands of every entry, a palindrome once with twice its count
    assert len(keys) == 2 * len(c) - len(pals) and np.all(keys[1:] > keys[:-1])
    i = int(np.searchsorted(keys, c[at]))
    assert int(cnt[i]) == (2 * bound if palindrome else bound)
    assert int(cnt.sum()) == 2 * int(n.astype(U64).sum())
    assert (int(cnt.max()) >= 1 << 32) == (palindrome and bound == 1 << 31)
