"""The inputs of tests/test_gpu_merge_seams.py are the edge cases they claim to be: every builder of tests/_seam_cases.py against its
own host model -- the merged order of two lists (A first on ties), the sampled cut of a k-way pass, the cuts of the tile sort.  No
device."""
import numpy as np
import pytest

from oracle import zkoracle as zo
from tests import _seam_cases as S


def ascending(x):
    return x.dtype == np.uint64 and bool(np.all(x[1:] > x[:-1]))


def test_tile_geometry_is_pinned():
    """the values the layouts were worked out for; a change here moves the cases, and this says so"""
    assert (S.MRG_TILE, S.MRG_ITEMS, S.MRG_BLOCK, S.MERGE_TILE) == (4096, 8, 512, 4096)
    assert (S.KW_CAP, S.KW_S, S.KW_MAX) == (2048, 64, 16)
    assert (S.TS_SLACK, S.TS_BLOCK) == (1024, 512)
    assert S.TS_ITEMS == dict(keys=14, pairs=10, count=12)
    assert S.TS_CAP == dict(keys=7168, pairs=5120, count=6144) and S.TS_T == dict(keys=6144, pairs=4096, count=5120)


# ---- two lists ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(S.two_list_layouts()))
def test_two_list_layout_against_the_merged_order(name):
    spec = S.two_list_layouts()[name]
    x, xc, y, yc, role = S.build_two_lists(name)
    assert ascending(x) and ascending(y) and len(x) + len(y) == spec["L"] == len(role)
    assert len(xc) == len(x) and len(yc) == len(y) and xc.min() >= 1 and yc.min() >= 1
    key, src = S.merged_order(x, y)
    # the model's merged sequence is the plan: the same slots are A's, and the pairs stand where the plan put them
    assert np.array_equal(src == 0, (role == S.A) | (role == S.PA))
    pairs = S.pair_slots(x, y)
    assert np.array_equal(pairs, np.flatnonzero(role == S.PA)) and np.array_equal(pairs + 1, np.flatnonzero(role == S.PB))
    assert set(spec["pairs_at"]) <= set(pairs.tolist())
    for lo, hi in spec.get("all_a", ()):
        assert np.all(src[lo:hi] == 0)
    for lo, hi in spec.get("all_b", ()):
        assert np.all(src[lo:hi] == 1)
    # the oracle drops one entry per pair, and keeps a B entry per pair in the projection
    zs, zc = zo.union_sum(x, xc, y, yc)
    assert len(zs) == spec["L"] - len(pairs)
    assert zo.split(x, y) == (len(pairs), len(x) - len(pairs), len(y) - len(pairs))
    assert len(zo.project(x, y, yc)[0]) == len(pairs)


def test_two_list_layouts_reach_the_seams():
    T, I = S.MRG_TILE, S.MRG_ITEMS
    L = S.two_list_layouts()

    def pairs(name):
        x, _, y, _, _ = S.build_two_lists(name)
        return S.pair_slots(x, y), S.merged_order(x, y)[1]
    p, _ = pairs("borders")
    assert {T - 1, 2 * T - 1, 3 * T - 1, 4 * T - 1} <= set(p.tolist())          # A ends tile t - 1, B begins tile t
    p, _ = pairs("borders_one_before")
    assert {t * T - 2 for t in (1, 2, 3, 4)} <= set(p.tolist())                # the pair ends the tile
    p, _ = pairs("borders_one_after")
    assert {t * T for t in (1, 2, 3, 4)} <= set(p.tolist())                    # the pair begins the tile
    p, src = pairs("tile_all_a")
    assert np.all(src[:T] == 0) and T - 1 in p and src[T] == 1                  # 4096 A elements, the last one's partner behind them
    assert int(np.sum(src[:T] == 0)) == T and np.flatnonzero(src == 1)[0] == T  # ... and it is B's first key
    p, src = pairs("tile_all_b")
    assert np.all(src[2 * T:3 * T] == 1) and 2 * T - 1 in p and src[2 * T - 1] == 0
    p, src = pairs("tile_all_a_then_all_b")
    assert np.all(src[T:2 * T] == 0) and np.all(src[2 * T:3 * T] == 1) and 2 * T - 1 in p
    p, _ = pairs("thread_seams")
    assert p.tolist() == [T + I * m + I - 1 for m in range(T // I)]             # every thread seam of tile 1, nothing else
    assert {T + 512 * w - 1 for w in range(1, 9)} <= set(p.tolist())            # the wave seams and the tile's end
    p, _ = pairs("ends_only")
    assert p.tolist() == [0, 5 * T - 2]
    for t in (1, 2):
        for d in (-1, 0, 1):
            name = "length_%dx%d%+d" % (t, T, d)
            p, src = pairs(name)
            assert len(src) == t * T + d and p[-1] == len(src) - 2
    assert len(L) == 14


def test_third_list_is_the_shared_keys():
    x, xc, y, yc, _ = S.build_two_lists("borders")
    z, zc = S.third_list(x, xc, y, 3)
    assert ascending(z) and len(z) == len(S.pair_slots(x, y)) and len(zc) == len(z)
    # x united with z has x's keys: the second level of the tree meets y on the same seams
    assert np.array_equal(zo.union_sum(x, xc, z, zc)[0], x)


# ---- k-way ----------------------------------------------------------------------------------------------------------------------------

def test_kway_model_against_a_plain_cut():
    """the model's tiles partition every list, by value: tile j holds the keys in (splitter j - 1, splitter j]"""
    lists = [x for x, _ in S.kway_solo(5, 1)]
    m = S.kway_model(lists)
    assert m["m"] == sum(-(-len(x) // S.KW_S) for x in lists) and m["tiles"] == m["m"] // m["T"] + 1
    assert np.all(np.diff(m["bounds"], axis=0) >= 0) and m["loads"].sum() == sum(len(x) for x in lists)
    for j in range(1, m["tiles"]):
        if j * m["T"] - 1 < m["m"]:
            s = m["sample"][j * m["T"] - 1]
            for i, x in enumerate(lists):
                b = m["bounds"][j, i]
                assert np.all(x[:b] <= s) and np.all(x[b:] > s)


@pytest.mark.parametrize("k", range(2, 17))
def test_kway_fullest_tile(k):
    """T * S + (k - 1) * (S - 1) = 1985 - k keys in the first tile, and (T + k - 1) * S = 1984 when the sample holds the splitter k
    times; never above KW_CAP"""
    got = {}
    for variant in S.KWAY_FULLEST_VARIANTS:
        lists = S.kway_fullest(k, variant, 1)
        assert all(ascending(x) and len(c) == len(x) for x, c in lists)
        assert all(len(x) <= 4000 for x, _ in lists)
        m = S.kway_model([x for x, _ in lists])
        got[variant] = int(m["loads"].max())
        assert m["loads"][0] == got[variant] == S.kway_fullest_load(k, variant) <= S.KW_CAP, (k, variant, m["loads"])
        V = lists[0][0][m["T"] * S.KW_S - 1]
        assert m["sample"][m["T"] - 1] == V
        keys, mult = np.unique(np.concatenate([x[x <= V] for x, _ in lists]), return_counts=True)
        if variant == "distinct":
            assert mult.max() == 1
        else:
            assert int(np.sum(mult == k)) == (S.KW_S if variant == "splitter_sampled" else S.KW_S - 1)          # runs of k equal keys
            assert (mult[-1] == k) == (variant != "shared")                                                      # ... the splitter among them
    print("k = %2d: fullest tile %s" % (k, got))
    assert got["distinct"] == got["shared"] == got["splitter_run"] == 1985 - k and got["splitter_sampled"] == 1984


@pytest.mark.parametrize("k", range(2, 17))
def test_kway_empty_last_tile_and_solo_tiles(k):
    for mult in (1, 2):
        lists = S.kway_sample_multiple(k, mult, 1)
        assert all(ascending(x) and len(x) >= 1 for x, _ in lists)
        m = S.kway_model([x for x, _ in lists])
        assert m["m"] == mult * m["T"] and m["tiles"] == mult + 1
        assert m["loads"][-1] == 0 and np.all(m["loads"][:-1] > 0) and m["loads"].max() <= S.KW_CAP          # a look-back participant with nothing
    lists = S.kway_solo(k, 1)
    assert all(ascending(x) for x, _ in lists)
    m = S.kway_model([x for x, _ in lists])
    per_list = np.diff(m["bounds"], axis=0)
    solo = [j for j in range(m["tiles"]) if per_list[j, k // 2] > 0 and per_list[j].sum() == per_list[j, k // 2]]
    assert solo and m["loads"].max() <= S.KW_CAP
    assert any(per_list[j, k // 2] == m["T"] * S.KW_S for j in solo)          # T sample points of that list alone: T * S keys
    lists = S.kway_first_and_last(k, 1)
    assert all(ascending(x) for x, _ in lists) and len(np.intersect1d(lists[0][0], lists[-1][0])) > 100
    m = S.kway_model([x for x, _ in lists])
    assert m["loads"].max() <= S.KW_CAP and any(a + b > 500 for _, a, b in S.kway_ends_tiles(lists))


# ---- tile sort ------------------------------------------------------------------------------------------------------------------------

def top_bits(n, key_bits, rbits):
    """tile_sort_top_bits (tilesort.hip) restated"""
    if n < (1 << 16):
        return 0
    passes = 1
    while (n >> (rbits * passes)) > 64 and rbits * passes < key_bits:
        passes += 1
    top = rbits * passes
    if passes + 2 > -(-key_bits // rbits) or top >= key_bits:
        return 0
    return top


@pytest.mark.parametrize("form", ["keys", "pairs", "count"])
def test_tile_sort_layouts_against_the_cut(form):
    CAP, T, SL = S.TS_CAP[form], S.TS_T[form], S.TS_SLACK
    layouts = S.tile_sort_layouts(form)
    assert len(layouts) == 9
    for name, spec in layouts.items():
        keys, spec = S.build_tile_sort(form, name)
        n = spec["n"]
        assert len(keys) == n and S.TS_MIN_N < n < S.TS_MIN_N + 2 * T and keys.dtype == np.uint64
        assert n % T == (1 if name.startswith("whole_tiles_plus_1") else 0)
        # whatever number of top bits the library takes at this size (digits of 8 or 9 bits), the blocks are the same
        assert all(8 <= top_bits(n, 64, rb) <= 32 for rb in (8, 9))
        assert np.all((keys >> np.uint64(32)) << np.uint64(32) == (keys >> np.uint64(56)) << np.uint64(56))
        assert not np.array_equal(keys, np.sort(keys))          # shuffled
        a = np.sort(keys)
        bounds, flag = S.tile_bounds_model(a, 56, T)
        assert np.array_equal(S.tile_bounds_model(a, 32, T)[0], bounds)
        assert flag == spec["flag"], name
        block = a >> np.uint64(56)
        starts = np.flatnonzero(np.concatenate([[True], block[1:] != block[:-1]]))
        lens = np.diff(np.concatenate([starts, [n]]))
        for s, l in spec["fixed"]:
            assert lens[np.searchsorted(starts, s)] == l and s in starts, name          # the blocks are where the plan put them
        long_blocks = [(int(s), int(l)) for s, l in zip(starts, lens) if l > SL]
        sizes = np.diff(bounds)
        if flag:
            # exactly one block is too long, by one key, and it covers [p - S, p] of a cut
            assert len(long_blocks) == 1 and long_blocks[0][1] == SL + 1
            s = long_blocks[0][0]
            assert (s + SL) % T == 0 and bounds[(s + SL) // T] == s
        else:
            assert np.all(sizes > 0) and sizes.max() <= CAP - 1
            assert all(s in starts for s in bounds[:-1])          # every cut is a block border
            for want in spec.get("tile_sizes", ()):
                assert want in sizes, (name, sizes)
            for t, cut in spec.get("cuts", {}).items():
                assert bounds[t] == cut, name
            if name == "block_of_S_ends_on_cut":
                assert int(np.sum(sizes == CAP - 1)) == 2 and bounds[1] == T - SL + 1 and bounds[2] == 2 * T
            if name == "block_of_2S_inside":
                assert [l for _, l in long_blocks] == [2 * SL, 2 * SL]
            if name.startswith("S_identical"):
                v, c = np.unique(a, return_counts=True)
                assert c.max() == SL


def test_count_form_reads_carry_the_layouts():
    """the counting form's layouts as reads of one k-mer each: the reads spell the keys, every key is the smaller of its two strands, and the
    cut of the keys' top bits (16 or 18 of the 62, by the digit width) is the layout's"""
    K, T, CAP = S.COUNT_K, S.TS_T["count"], S.TS_CAP["count"]
    for name in S.tile_sort_layouts("count"):
        stream, keys, spec = S.count_form_reads(name)
        n = spec["n"]
        assert len(keys) == n and len(stream) == n * (K + 1)
        assert {top_bits(len(stream), 2 * K, rb) for rb in (8, 9)} == {16, 18}
        for i in range(0, n, 499):
            read = stream[i * (K + 1):(i + 1) * (K + 1)]
            assert read.endswith(b"\n") and zo.kmers_list(K, read[:-1]).tolist() == [int(keys[i])] and zo.rc(K, int(keys[i])) > int(keys[i])
        assert int(keys.max()) < 1 << (2 * K) and np.all((keys >> np.uint64(32)) << np.uint64(32) == (keys >> np.uint64(2 * K - 8)) << np.uint64(2 * K - 8))
        a = np.sort(keys)
        bounds, flag = S.tile_bounds_model(a, 2 * K - 18, T)
        assert np.array_equal(S.tile_bounds_model(a, 2 * K - 16, T)[0], bounds) and flag == spec["flag"], name
        if not flag:
            sizes = np.diff(bounds)
            assert sizes.max() <= CAP - 1 and all(want in sizes for want in spec.get("tile_sizes", ()))
        if name.startswith("S_identical"):
            assert np.unique(a, return_counts=True)[1].max() == S.TS_SLACK
