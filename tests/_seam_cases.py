"""Inputs that stand exactly on the seams of the merge and tile-sort kernels, and host models that say where the seams are.  No device.

  * setops.hip (union_sum_kernel, intersect_kernel): two ascending lists built from a plan of the MERGED sequence -- which slot is an
    A element, which a B element, which two neighbouring slots are an equal pair (A first) -- so a pair can be put on a tile border,
    a thread seam or a wave seam; merged_order() is the model (A before B on ties).
  * kway.hip: lists whose sampled cut hands one tile the most elements it can, whose sample count makes the last tile empty, or whose
    tile belongs to one list alone; kway_model() restates kway_sample_kernel, the sort of the sample and kway_bounds_kernel.
  * tilesort.hip: keys whose blocks of equal top bits begin and end where the plan says, around the S / S + 1 threshold of
    tile_bounds_kernel; tile_bounds_model() restates that kernel.

The tile geometry is read from the sources, so a changed tile moves the cases with it (tests/test_seam_cases_host.py pins the values).
"""
import os
import re

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zotmer_amd", "csrc")


def _constants(fname, names, known=None):
    """`NAME = expression` out of the constexpr lines of a source; expressions may use names found before"""
    text = open(os.path.join(CSRC, fname)).read()
    env = dict(known or {})
    for name in names:
        m = re.search(r"constexpr (?:int|u32) [^;]*\b%s = ([^,;]+)[,;]" % name, text)
        env[name] = int(eval(m.group(1), {"__builtins__": {}}, env))
    return env


_M = _constants("setops.hip", ["MRG_BLOCK", "MRG_ITEMS", "MRG_TILE"])
MRG_BLOCK, MRG_ITEMS, MRG_TILE = _M["MRG_BLOCK"], _M["MRG_ITEMS"], _M["MRG_TILE"]
MERGE_TILE = _constants("internal.hpp", ["MERGE_TILE"])["MERGE_TILE"]
_K = _constants("kway.hip", ["KW_MAX", "KW_BLOCK", "KW_ITEMS", "KW_CAP", "KW_S"])
KW_MAX, KW_CAP, KW_S = _K["KW_MAX"], _K["KW_CAP"], _K["KW_S"]
_T = _constants("tile_group.hpp", ["TS_BLOCK", "TS_SLACK"])
TS_BLOCK, TS_SLACK = _T["TS_BLOCK"], _T["TS_SLACK"]
_ts = open(os.path.join(CSRC, "tilesort.hip")).read()
TS_ITEMS = {"keys": int(re.search(r"typedef TileSortSmem<(\d+), \d+, false> TileSortKeys;", _ts).group(1)),
            "pairs": int(re.search(r"typedef TileSortSmem<(\d+), \d+, true> TileSortPairs;", _ts).group(1)),
            "count": _constants("tilesort.hip", ["TS_COUNT_ITEMS"])["TS_COUNT_ITEMS"]}
TS_CAP = {form: TS_BLOCK * items for form, items in TS_ITEMS.items()}          # TileSortSmem::CAP
TS_T = {form: cap - TS_SLACK for form, cap in TS_CAP.items()}                  # the cuts stand before every multiple of T
TS_MIN_N = 1 << 16                                                              # tile_sort_top_bits: smaller arrays keep the LSD passes


# ---- two lists from a plan of their merged sequence ------------------------------------------------------------------------------

A, B, PA, PB = 0, 1, 2, 3          # a slot of the merged sequence: an A element, a B element, the A and the B element of an equal pair


def two_lists(L, pairs_at, seed, all_a=(), all_b=(), extra_pairs=0.1):
    """L merged slots; an equal pair at (p, p + 1) for every p of pairs_at (the A element at p); the slot ranges all_a / all_b hold
    A (B) elements only, where a pair does not say otherwise; everywhere else A, B and further pairs at random.
    -> (x, xc, y, yc, role): ascending distinct u64 keys and u64 counts of both lists, role[s] of every merged slot."""
    rng = np.random.default_rng(seed)
    role = np.full(L, -1, np.int8)
    for lo, hi in all_a:
        role[lo:hi] = A
    for lo, hi in all_b:
        role[lo:hi] = B
    for p in pairs_at:
        assert 0 <= p and p + 1 < L and role[p] not in (PA, PB) and role[p + 1] not in (PA, PB), p
        role[p], role[p + 1] = PA, PB
    s, want = 0, rng.random(L) < extra_pairs
    while s + 1 < L:
        if role[s] == -1 and role[s + 1] == -1 and want[s]:
            role[s], role[s + 1] = PA, PB
            s += 2
        else:
            s += 1
    free = role == -1
    role[free] = rng.integers(0, 2, size=int(free.sum()))
    # one key per slot, the B element of a pair takes its A element's: ascending in 39 bits, the low bits (acgt) at random
    rank = np.cumsum(role != PB) - 1
    n_keys = int(rank[-1]) + 1
    key = ((np.arange(n_keys, dtype=np.uint64) << np.uint64(24)) | rng.integers(0, 1 << 24, size=n_keys, dtype=np.uint64))[rank]
    cnt = rng.integers(1, 1000, size=L, dtype=np.uint64)
    in_a = (role == A) | (role == PA)
    return key[in_a], cnt[in_a], key[~in_a], cnt[~in_a], role


def merged_order(x, y):
    """the model: (keys, source) of the merged sequence of two ascending lists, A (source 0) before B (source 1) on ties"""
    key = np.concatenate([x, y])
    src = np.concatenate([np.zeros(len(x), np.int8), np.ones(len(y), np.int8)])
    order = np.lexsort((src, key))
    return key[order], src[order]


def pair_slots(x, y):
    """the slots p of the model's merged sequence at which an equal pair (A at p, B at p + 1) stands"""
    key, src = merged_order(x, y)
    return np.flatnonzero((key[:-1] == key[1:]) & (src[:-1] == 0) & (src[1:] == 1))


def two_list_layouts():
    """{name: dict(L, pairs_at, all_a, all_b)}: what tests/test_seam_cases_host.py checks against the model and
    tests/test_gpu_merge_seams.py runs"""
    T, I = MRG_TILE, MRG_ITEMS
    out = {}
    for name, shift in (("borders", 0), ("borders_one_before", -1), ("borders_one_after", 1)):
        # the A element of a pair is the last of tile t - 1, its B element the first of tile t -- all four borders of five tiles
        out[name] = dict(L=5 * T, pairs_at=[t * T - 1 + shift for t in (1, 2, 3, 4)])
    # tile 0 is all A, its last key is B's first: the partner stands behind the right halo
    out["tile_all_a"] = dict(L=5 * T, pairs_at=[T - 1], all_a=[(0, T)])
    # tile 2 is all B, its first key equals the A element just before it: the partner stands in front of the left halo
    out["tile_all_b"] = dict(L=5 * T, pairs_at=[2 * T - 1], all_b=[(2 * T, 3 * T)])
    # ... both at once: an all-A tile, then an all-B tile
    out["tile_all_a_then_all_b"] = dict(L=5 * T, pairs_at=[2 * T - 1], all_a=[(T, 2 * T)], all_b=[(2 * T, 3 * T)])
    # a pair on every thread seam of tile 1 (A at 8m + 7, B at 8m + 8): the wave seams (multiples of 512) and the tile's end among them
    out["thread_seams"] = dict(L=5 * T, pairs_at=[T + I * m + I - 1 for m in range(T // I)], extra_pairs=0.0)
    # pairs at the very first and the very last merged slots only
    out["ends_only"] = dict(L=5 * T, pairs_at=[0, 5 * T - 2], extra_pairs=0.0)
    for t in (1, 2):
        for d in (-1, 0, 1):
            # the last pair ends the input; with one slot more than t tiles its B element is a tile of its own
            out["length_%dx%d%+d" % (t, T, d)] = dict(L=t * T + d, pairs_at=[t * T + d - 2])
    return out


def build_two_lists(name, seed=0):
    spec = dict(two_list_layouts()[name])
    return two_lists(spec.pop("L"), spec.pop("pairs_at"), seed + sum(map(ord, name)), **spec)


def third_list(x, xc, y, seed):
    """a third list for zk_merge_n: exactly the keys that x and y share (the border keys among them), with counts of its own"""
    z = np.intersect1d(x, y)
    return z, np.random.default_rng(seed).integers(1, 1000, size=len(z), dtype=np.uint64)


# ---- k lists for one k-way pass ---------------------------------------------------------------------------------------------------

def kway_model(lists):
    """kway_sample_kernel, the sort and kway_bounds_kernel restated: dict(T, m, tiles, bounds[tiles + 1][k], loads[tiles])"""
    k = len(lists)
    T = KW_CAP // KW_S - k
    samp = [x[np.minimum((np.arange(-(-len(x) // KW_S)) + 1) * KW_S, len(x)) - 1] for x in lists]
    s = np.sort(np.concatenate(samp))
    m = len(s)
    tiles = m // T + 1
    bounds = np.zeros((tiles + 1, k), np.int64)
    for j in range(1, tiles + 1):
        for i, x in enumerate(lists):
            if j == tiles or j * T - 1 >= m:
                bounds[j, i] = len(x)
            else:
                bounds[j, i] = np.searchsorted(x, s[j * T - 1], side="right")          # the keys <= the splitter
    return dict(T=T, m=m, tiles=tiles, bounds=bounds, loads=np.diff(bounds, axis=0).sum(axis=1), sample=s)


KWAY_FULLEST_VARIANTS = ("distinct", "shared", "splitter_run", "splitter_sampled")


def kway_fullest(k, variant, seed):
    """k lists whose first tile is as full as the cut allows.  List 0 has T * S keys up to V (its T-th sample point, the first
    splitter) and a tail; every other list has S - 1 keys up to V, its S-th key -- its first sample point -- above V, and a tail:
    the tile (.., V] holds T * S + (k - 1) * (S - 1) keys.
      distinct          no key occurs twice
      shared            the S - 1 low keys are the same in the lists 1 .. k - 1 and keys of list 0: runs of k equal keys
      splitter_run      ... and V itself is one of them: the run of k equal keys that ends the tile is the splitter
      splitter_sampled  the S-th key of every list IS V: the sample holds V k times, the T-th sample point is one of them and the
                        tile takes all of them -- (T + k - 1) * S keys, the most any cut can give
    -> [(keys, counts)]"""
    rng = np.random.default_rng(seed * 131 + k)
    S, T = KW_S, KW_CAP // KW_S - k
    step = np.uint64(1000)
    grid = (np.arange(T * S, dtype=np.uint64) + np.uint64(1)) * step          # list 0 up to V; the other lists add 1 .. k - 1 to be distinct
    V = grid[-1]
    # the tails: keys above V from one pool, so that lists share some of them
    pool = V + (np.arange(1, 6000, dtype=np.uint64) * step)
    lists = []
    for i in range(k):
        tail = np.sort(rng.choice(pool, size=int(rng.integers(200, 1500)), replace=False))
        if i == 0:
            low = grid
        else:
            n_low = S if variant == "splitter_sampled" else S - 1
            same = np.random.default_rng(seed)          # the same draw for every list
            if variant in ("splitter_run", "splitter_sampled"):
                low = np.concatenate([grid[np.sort(same.choice(T * S - 1, size=n_low - 1, replace=False))], [V]])
            elif variant == "shared":
                low = grid[np.sort(same.choice(T * S - 1, size=n_low, replace=False))]
            else:
                low = grid[np.sort(rng.choice(T * S - 1, size=n_low, replace=False))] + np.uint64(i)
        x = np.concatenate([low, tail]).astype(np.uint64)
        lists.append((x, rng.integers(1, 50, size=len(x), dtype=np.uint64)))
    return lists


def kway_fullest_load(k, variant):
    S, T = KW_S, KW_CAP // KW_S - k
    return (T + k - 1) * S if variant == "splitter_sampled" else T * S + (k - 1) * (S - 1)


def kway_sample_multiple(k, mult, seed):
    """k lists with mult * T sample points in all: tiles = m / T + 1 makes the last tile empty"""
    rng = np.random.default_rng(seed * 17 + k + mult)
    T = KW_CAP // KW_S - k
    cuts = np.sort(rng.choice(np.arange(1, mult * T), size=k - 1, replace=False))
    per_list = np.diff(np.concatenate([[0], cuts, [mult * T]]))          # >= 1 sample point each
    pool = np.arange(1, 4 * mult * T * KW_S, dtype=np.uint64) * np.uint64(0x3d)
    lists = []
    for c in per_list:
        n = int(c) * KW_S - int(rng.integers(0, KW_S))          # ceil(n / S) == c
        x = np.sort(rng.choice(pool, size=n, replace=False))
        lists.append((x, rng.integers(1, 50, size=n, dtype=np.uint64)))
    return lists


def kway_solo(k, seed):
    """k lists; list k / 2 alone has keys in a stretch wide enough for whole tiles: the other lists' pieces of those tiles are empty"""
    rng = np.random.default_rng(seed * 29 + k)
    T = KW_CAP // KW_S - k
    stretch = 2 * T * KW_S + 100
    below = np.arange(1, 4000, dtype=np.uint64) * np.uint64(7)
    middle = np.uint64(1 << 20) + np.arange(stretch, dtype=np.uint64) * np.uint64(5)
    above = np.uint64(1 << 30) + np.arange(1, 4000, dtype=np.uint64) * np.uint64(11)
    lists = []
    for i in range(k):
        parts = [np.sort(rng.choice(below, size=int(rng.integers(100, 600)), replace=False))]
        if i == k // 2:
            parts.append(middle)
        parts.append(np.sort(rng.choice(above, size=int(rng.integers(100, 600)), replace=False)))
        x = np.concatenate(parts)
        lists.append((x, rng.integers(1, 50, size=len(x), dtype=np.uint64)))
    return lists


def kway_ends_tiles(lists):
    """the tiles (by the model) that hold keys of the first and the last list and of no other, the first list's piece no multiple of a
    thread's four outputs: [(tile, keys of the first list, keys of the last)]"""
    per_list = np.diff(kway_model([x for x, _ in lists])["bounds"], axis=0)
    return [(j, int(r[0]), int(r[-1])) for j, r in enumerate(per_list) if r[0] % 4 and r[-1] and r.sum() == r[0] + r[-1]]


def kway_first_and_last(k, seed):
    """k lists; the first and the last share a stretch of whole tiles with keys in common, and the lists between them have nothing
    there: from five lists on a merge round meets a pair with entries, empty pairs, and a pair with entries again, and the first
    list's piece of a tile is no multiple of a thread's four outputs, so a thread walks across the empty pairs.  (Where the sampled
    cut falls is not in the builder's hand: it draws again until the model finds such a tile.)"""
    T = KW_CAP // KW_S - k
    stretch = 3 * T * KW_S + 50
    below = np.arange(1, 4000, dtype=np.uint64) * np.uint64(7)
    above = np.uint64(1 << 30) + np.arange(1, 4000, dtype=np.uint64) * np.uint64(11)
    for attempt in range(32):
        rng = np.random.default_rng((seed * 31 + k) * 32 + attempt)
        # the last list in steps of 10, the first a random half of the steps of 7 over the same values: every tenth of those is a key
        # of the last list as well
        middle = {k - 1: np.uint64(1 << 20) + np.arange(stretch, dtype=np.uint64) * np.uint64(10)}
        middle[0] = (np.uint64(1 << 20) + np.arange(stretch * 10 // 7, dtype=np.uint64) * np.uint64(7))[rng.random(stretch * 10 // 7) < 0.5]
        lists = []
        for j in range(k):
            parts = [np.sort(rng.choice(below, size=int(rng.integers(100, 600)), replace=False))]
            if j in middle:
                parts.append(middle[j])
            parts.append(np.sort(rng.choice(above, size=int(rng.integers(100, 600)), replace=False)))
            x = np.concatenate(parts)
            lists.append((x, rng.integers(1, 50, size=len(x), dtype=np.uint64)))
        if kway_ends_tiles(lists):
            return lists
    raise AssertionError("no tile of the first and the last list alone")


# ---- keys for the tile sort ---------------------------------------------------------------------------------------------------------

TS_BLOCK_SHIFT = 56          # a key is (block << 56) | 32 random low bits, the bits 32 .. 55 zero: the blocks of equal top bits are the
TS_MAX_BLOCKS = 256          # same for every number of top bits from 8 to 32 that tile_sort_top_bits can choose


def tile_bounds_model(sorted_keys, pshift, T, S=None):
    """tile_bounds_kernel restated on the sorted array: (bounds[tiles + 1], flag)"""
    S = TS_SLACK if S is None else S
    a = sorted_keys >> np.uint64(pshift)
    n = len(a)
    tiles = -(-n // T)
    bounds = np.zeros(tiles + 1, np.int64)
    bounds[tiles] = n
    flag = False
    for t in range(1, tiles):
        p = t * T
        if a[p - S] == a[p]:
            flag = True
            bounds[t] = p - S
        else:
            bounds[t] = p - S + 1 + int(np.searchsorted(a[p - S + 1:p + 1], a[p], side="left"))          # the block's first key
    return bounds, flag


def tile_sort_keys(n, fixed, seed, identical=()):
    """n shuffled keys whose sorted order has a block of equal top bits at every (start, length) of `fixed`, blocks of 300 .. 700 keys
    in between; the blocks whose start is in `identical` hold one key, repeated.  -> (keys, block starts, block lengths)"""
    rng = np.random.default_rng(seed)
    starts, lens, at = [], [], 0
    for s, l in sorted(fixed) + [(n, 0)]:
        assert s >= at, "the fixed blocks overlap"
        while at < s:
            l0 = min(s - at, int(rng.integers(300, 701)))
            if 0 < s - at - l0 < 100:
                l0 = s - at          # (no sliver before a fixed block)
            starts.append(at); lens.append(l0); at += l0
        if l:
            starts.append(s); lens.append(l); at = s + l
    assert at == n and len(starts) <= TS_MAX_BLOCKS and max(l for s, l in zip(starts, lens) if (s, l) not in fixed) <= TS_SLACK
    keys = np.repeat(np.arange(len(starts), dtype=np.uint64) << np.uint64(TS_BLOCK_SHIFT), lens) | rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    for s, l in zip(starts, lens):
        if s in identical:
            keys[s:s + l] = keys[s]
    return rng.permutation(keys), np.array(starts), np.array(lens)


def tile_sort_layouts(form):
    """{name: dict(n, fixed, identical, flag, tile_sizes)} for one form of the tile sort (keys, pairs, count); `flag` and `tile_sizes`
    (sizes that must occur among the tiles) are what the layout claims and the model must confirm"""
    CAP, T, S = TS_CAP[form], TS_T[form], TS_SLACK
    N = -(-(TS_MIN_N + 1) // T)          # the smallest number of whole tiles above the size that takes the route
    n = N * T
    last = (N - 1) * T                   # the last inner cut of N tiles
    out = {}
    # a block of exactly S keys that ends on the key at p = t * T: cut at p - S + 1; the next cut exactly on p + T: a tile of CAP - 1
    out["block_of_S_ends_on_cut"] = dict(n=n, fixed=[(T - S + 1, S), (2 * T, 400), (last - S + 1, S)], flag=False, tile_sizes=[CAP - 1, CAP - 1])
    # one key more, [p - S, p]: declined
    out["block_of_S_plus_1_first_cut"] = dict(n=n, fixed=[(T - S, S + 1)], flag=True)
    out["block_of_S_plus_1_last_cut"] = dict(n=n, fixed=[(last - S, S + 1)], flag=True)
    # a block that starts exactly on p: the cut is p itself
    out["block_starts_on_cut"] = dict(n=n, fixed=[(T, 500), (last, 500)], flag=False, cuts={1: T, N - 1: last})
    # 2 S keys of one block wholly inside a tile: long, but on no cut
    out["block_of_2S_inside"] = dict(n=n, fixed=[(T + 300, 2 * S), (last + 300, 2 * S)], flag=False)
    # S copies of one key inside a tile
    out["S_identical_keys"] = dict(n=n, fixed=[(T + 300, S)], identical=[T + 300], flag=False)
    # ... and as the block that ends on the cut
    out["S_identical_keys_end_on_cut"] = dict(n=n, fixed=[(T - S + 1, S), (2 * T, 400)], identical=[T - S + 1], flag=False, tile_sizes=[CAP - 1])
    # one key more than whole tiles: the last inner cut stands on the last key, whose block of S ends the array
    out["whole_tiles_plus_1"] = dict(n=n + 1, fixed=[(n - S + 1, S)], flag=False, tile_sizes=[S], cuts={N: n - S + 1})
    out["whole_tiles_plus_1_declined"] = dict(n=n + 1, fixed=[(n - S, S + 1)], flag=True)
    return out


def build_tile_sort(form, name, seed=0):
    spec = tile_sort_layouts(form)[name]
    keys, starts, lens = tile_sort_keys(spec["n"], spec["fixed"], seed + sum(map(ord, form + name)), spec.get("identical", ()))
    return keys, spec


# ---- ... and for the counting form, which only zk_kmerize reaches: the keys as reads of one k-mer each -------------------------------

COUNT_K = 31          # K >= 28: no count fits beside the k-mer, so reads that do not repeat their k-mers are counted tile by tile


def count_form_reads(name, seed=0):
    """a layout of the counting form as a stream of reads of COUNT_K bases, one k-mer each: the keys are 62 bits wide, the block in
    their top 8 bits, and every one is the smaller of its k-mer's two strands -- the one the passes of zk_kmerize keep -- (the low bits
    are drawn again until it is), so the keys that zk_kmerize counts are the keys of the layout.  -> (stream bytes, keys in the order of the reads, the layout's spec)"""
    from oracle import zkoracle as zo
    spec = tile_sort_layouts("count")[name]
    keys, starts, lens = tile_sort_keys(spec["n"], spec["fixed"], seed + sum(map(ord, "count" + name)), spec.get("identical", ()))
    rng = np.random.default_rng(seed + 1)
    keys = ((keys >> np.uint64(TS_BLOCK_SHIFT)) << np.uint64(2 * COUNT_K - 8)) | (keys & np.uint64(0xffffffff))
    fixed = {}          # (copies of one key stay copies)
    for i, x in enumerate(keys.tolist()):
        if x not in fixed:
            y = x
            while zo.rc(COUNT_K, y) < y:
                y = (x >> 32 << 32) | int(rng.integers(0, 1 << 32))
            fixed[x] = y
        keys[i] = fixed[x]
    text = np.full((len(keys), COUNT_K + 1), ord("\n"), np.uint8)
    for j in range(COUNT_K):
        text[:, j] = np.frombuffer(b"ACGT", np.uint8)[((keys >> np.uint64(2 * (COUNT_K - 1 - j))) & np.uint64(3)).astype(np.int64)]
    return text.tobytes(), keys, spec
