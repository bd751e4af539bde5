"""
The kernels at the ends of their ranges: 64-bit keys at 0, around 2^63 and at 2^64 - 1 (the all-T 32-mer, and the value several
kernels pad partial tiles with), and counts at the 32-bit limit, at 2^32, 2^63 and beyond the histogram's side list -- against
numpy, the CPU oracle (oracle/zk_oracle.c) and Python-int arithmetic, full arrays or exact error codes throughout.
"""
import numpy as np
import pytest

from oracle import zkoracle as zo
from zotmer_amd import native, synth

pytestmark = pytest.mark.gpu

TOP, HALF = (1 << 64) - 1, 1 << 63
M64 = (1 << 64) - 1
FIXED = [0, 1, 2, 3, HALF - 1, HALF, HALF + 1, TOP - 1, TOP]
TILE_THRESHOLD_PLUS = 65536 + 7168 + 3          # just above the tile sort's threshold (test_gpu_parity.test_sort_finished_in_tiles)
SORT_SIZES = [1, 2, 8191, 8192, 8193, 16383, 16384, 16385, TILE_THRESHOLD_PLUS, 2_500_000]


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def edge_keys(n, seed=0):
    """n sorted distinct u64 keys, the last one 2^64 - 1: 0..3, 2^63 - 1 .. 2^63 + 1, 2^64 - 2, dense runs just below 2^64 and
    on both sides of 2^63, the rest random over the full range with every low 2-bit value (every base at the end of a k-mer)"""
    if n < 16:
        return np.array(sorted(FIXED[:max(n - 1, 0)] + [TOP])[-n:], dtype=np.uint64) if n else np.empty(0, np.uint64)
    rng = np.random.default_rng(seed * 1000003 + n)
    r = max(1, min(n // 8, 4096))
    base = np.unique(np.concatenate([np.array(FIXED, dtype=np.uint64),
                                     np.uint64(TOP) - np.arange(r, dtype=np.uint64),
                                     np.uint64(HALF - r) + np.arange(2 * r, dtype=np.uint64)]))
    while len(base) < n:
        m = n - len(base)
        hi = rng.integers(0, 1 << 62, size=m, dtype=np.uint64)
        base = np.union1d(base, (hi << np.uint64(2)) | (np.arange(m, dtype=np.uint64) & np.uint64(3)))
    assert len(base) == n and int(base[-1]) == TOP
    return base


def _err(fn):
    with pytest.raises(native.ZotkError) as e:
        fn()
    return e.value.code


# ---- sort and count at 64 key bits ---------------------------------------------------------------------------------------

def _sort_inputs(n, rng):
    keys = edge_keys(n, 1)
    # ascending: 2^64 - 1 in the last slot of a full tile (8192, 16384) or inside a cut last tile (8191, 8193, 16383, 16385)
    yield "ascending", keys
    yield "descending", keys[::-1].copy()
    yield "shuffled", rng.permutation(keys)
    dup = np.concatenate([keys, np.full(n // 3 + 1, TOP, np.uint64), np.zeros(n // 5 + 1, np.uint64)])
    yield "copies_of_ends", rng.permutation(dup)
    yield "copies_of_ends_in_runs", dup
    if n >= 65536:
        # a block of equal top bits at the very top of the range (an all-ones prefix), far too long for one tile, 2^64 - 1 in it
        y = rng.permutation(keys)
        m = 3000
        y[n // 2: n // 2 + m] = np.uint64(TOP >> 16 << 16) | rng.integers(0, 1 << 16, size=m, dtype=np.uint64)
        y[n // 2 + m - 40: n // 2 + m] = np.uint64(TOP)
        yield "top_block", y


@pytest.mark.parametrize("n", SORT_SIZES)
def test_sort_and_count_full_range(ctx, n):
    """zk_sort_keys, zk_sort_pairs, zk_rle and zk_sort_count at 64 key bits against numpy, with 2^64 - 1 and 0 as real keys (many
    copies of each), pairs with equal keys in their order of arrival, the tile sort on and off, 16 K-key and 8 K-key tiles"""
    rng = np.random.default_rng(n)
    try:
        for name, x in _sort_inputs(n, rng):
            want = np.sort(x)
            v = np.arange(len(x), dtype=np.uint32)
            order = np.argsort(x, kind="stable")
            uk, uc = np.unique(x, return_counts=True)
            for ts, wide in ((1, 1), (0, 1), (1, 0), (0, 0)):
                ctx.tune(tile_sort=ts, wide_tiles=wide)
                tag = (name, ts, wide)
                assert np.array_equal(ctx.sort_keys(ctx.upload(x), 64).to_host(), want), tag
                dk, dv = ctx.sort_pairs(ctx.upload(x), ctx.upload(v), 64)
                assert np.array_equal(dk.to_host(), want) and np.array_equal(dv.to_host(), v[order]), tag
                k, c = ctx.sort_count(ctx.upload(x), 64)
                assert np.array_equal(k.to_host(), uk) and np.array_equal(c.to_host(), uc.astype(np.uint32)), tag
            k, c = ctx.rle(ctx.upload(want))
            assert np.array_equal(k.to_host(), uk) and np.array_equal(c.to_host(), uc.astype(np.uint32)), name
    finally:
        ctx.tune(tile_sort=1, wide_tiles=1)


# ---- kmerize at K = 28, 31, 32 -------------------------------------------------------------------------------------------

def _edge_reads(K, rng):
    def rnd(m):
        return "".join(rng.choice(list("ACGT"), size=m))
    return (["T" * 150, "A" * 150, "G" * 150, "C" * 150, "T" * 40 + rnd(110), rnd(110) + "T" * 40, "T" * (K - 1) + "G",
             "T" * K + "G" + rnd(50), "G" + "T" * K, "T" * (K - 1) + "G" + "T" * (K - 1), "A" * (K - 1) + "C", "C" + "A" * K]
            + ["T" * 40 + rnd(110) for _ in range(20)])


@pytest.mark.parametrize("K", [28, 31, 32])
def test_kmerize_poly_t_and_the_top_key(ctx, K):
    """zk_kmerize at K >= 28 against the oracle with poly-T / poly-A / poly-G reads, reads that start with 40 Ts and T..TG shapes (at
    K = 32 the all-T k-mer is 2^64 - 1, the padding value of the tile and block sorts): canonical, both strands as they are, and the
    counted canonical list mirrored; on inputs that repeat their k-mers, inputs that do not (the plan that sorts the keys of both
    strands tile by tile meets 2^64 - 1 there), and mixed ones; every early_collapse / packed_pairs / tile_sort setting"""
    rng = np.random.default_rng(500 + K)
    edge = _edge_reads(K, rng)
    deep = synth.read_strings(41, 0, 4000, 150, genome=12000, sub_thr=synth.frac32(0.004), n_thr=synth.frac32(0.001)) + edge * 30
    flat = synth.read_strings(42, 0, 3000, 150, genome=0) + ["T" * 150] * 3 + edge[4:6]
    mixed = deep[:2000] + flat[:2000] + edge * 5
    try:
        for name, reads in (("deep", deep), ("flat", flat), ("mixed", mixed)):
            want = zo.kmerize(K, reads)
            wk, wc = want["kmers"], want["counts"]
            if K == 32:
                assert int(wk[0]) == 0 and int(wk[-1]) == TOP          # the test reaches both ends of the key range
            rc = np.array([zo.rc(K, int(x)) for x in wk], dtype=np.uint64)
            keep = wk <= rc
            ck_want, cc_want = wk[keep], wc[keep].astype(np.uint64)
            cc_want[wk[keep] == rc[keep]] //= 2
            d = ctx.upload_stream(("".join(r + "\n" for r in reads)).encode())
            for ts in (1, 0):
                for collapse in (0, 1, 2, 3):
                    for packed in (0, 1):
                        ctx.tune(early_collapse=collapse, packed_pairs=packed, tile_sort=ts)
                        tag = (name, ts, collapse, packed)
                        for flags in (native.KMERIZE_CANONICAL, native.KMERIZE_BOTH):
                            k, c, st = ctx.kmerize(d, K, flags)
                            assert np.array_equal(k.to_host(), wk), tag + (flags,)
                            assert np.array_equal(c.to_host(), wc), tag + (flags,)
                            assert list(st.acgt) == want["acgt"] and st.n_unique == len(wk), tag + (flags,)
                        ck, cc, st = ctx.kmerize(d, K, native.KMERIZE_CANONICAL_ONLY)
                        assert np.array_equal(ck.to_host(), ck_want), tag
                        assert np.array_equal(cc.to_host().astype(np.uint64), cc_want), tag
                        assert list(st.acgt) == want["acgt"] and st.n_unique == len(ck_want), tag
                        ek, ec = ctx.mirror_expand(ck, cc, K)
                        assert np.array_equal(ek.to_host(), wk) and np.array_equal(ec.to_host(), wc), tag
            if name == "flat" and K == 32:
                # the input that does not repeat its k-mers is counted by the tile sort (the default settings)
                ctx.tune(early_collapse=1, packed_pairs=1, tile_sort=1)
                ctx.profile(True)
                k, c, _ = ctx.kmerize(d, K)
                prof = ctx.profile_read()
                ctx.profile(False)
                assert prof.get("tile_sort", {}).get("launches", 0) >= 1
                assert np.array_equal(k.to_host(), wk) and np.array_equal(c.to_host(), wc)
    finally:
        ctx.profile(False)
        ctx.tune(early_collapse=1, packed_pairs=1, tile_sort=1)


# ---- set operations on edge keys -----------------------------------------------------------------------------------------

SET_SIZES = [(1, 1), (2, 16), (8193, 8191), (16385, 300_001), (2_500_000, 700_000)]


@pytest.mark.parametrize("nx,ny", SET_SIZES)
def test_union_sum_edge_keys(ctx, nx, ny):
    rng = np.random.default_rng(nx + 7 * ny)
    x, y = edge_keys(nx, 2), edge_keys(ny, 3)          # they share 0 .. 3, the keys around 2^63 and the top of the range
    for cdt, hi in ((np.uint64, 1 << 40), (np.uint32, 1 << 31)):
        xc = rng.integers(1, hi, size=nx, dtype=np.uint64)
        yc = rng.integers(1, hi, size=ny, dtype=np.uint64)
        zs, zc = zo.union_sum(x, xc, y, yc)
        k, c, acgt = ctx.union_sum(ctx.upload(x), ctx.upload(xc.astype(cdt)), ctx.upload(y), ctx.upload(yc.astype(cdt)), want_acgt=True)
        assert np.array_equal(k.to_host(), zs) and np.array_equal(c.to_host().astype(np.uint64), zc), cdt
        assert acgt == [int(zc[(zs & np.uint64(3)) == np.uint64(b)].sum()) for b in range(4)]


@pytest.mark.parametrize("nlists", [2, 16, 17])
def test_merge_n_edge_keys(ctx, nlists):
    """zk_merge_n: the tree of 2-way passes (kway 0), the default (1: kway.hip from 4 Mi pairs on) and kway.hip always (2),
    64- and 32-bit counts, lists that all hold 0 and 2^64 - 1"""
    rng = np.random.default_rng(nlists)
    sizes = [int(rng.integers(1, 40000)) for _ in range(nlists)]
    sizes[0] = 1_000_000 if nlists == 2 else 300_000
    sets = [(edge_keys(n, 10 + s), rng.integers(1, 1 << 20, size=n, dtype=np.uint64)) for s, n in enumerate(sizes)]
    zs, zc, acgt = zo.merge_n(32, sets)
    try:
        for cdt in (np.uint64, np.uint32):
            dev = [(ctx.upload(a), ctx.upload(b.astype(cdt))) for a, b in sets]
            for kway in (0, 1, 2):
                ctx.tune(kway=kway)
                gk, gc, gacgt = ctx.merge_n(dev)
                assert np.array_equal(gk.to_host(), zs) and np.array_equal(gc.to_host().astype(np.uint64), zc), (cdt, kway)
                assert gacgt == acgt, (cdt, kway)
    finally:
        ctx.tune(kway=1)


@pytest.mark.parametrize("nx,ny", SET_SIZES)
def test_subsets_and_filters_edge_keys(ctx, nx, ny):
    """zk_split, zk_project_dedupe (shifts 0, 2, 14, 62), zk_project, zk_sample and zk_trim on keys over the full range"""
    rng = np.random.default_rng(3 * nx + ny)
    x, y = edge_keys(nx, 4), edge_keys(ny, 5)
    dx, dy = ctx.upload(x), ctx.upload(y)
    assert ctx.split(dx, dy) == zo.split(x, y)
    assert ctx.split(dy, dx) == zo.split(y, x)
    assert ctx.split(dx, dx) == (nx, 0, 0)
    for sh in (0, 2, 14, 62):
        assert np.array_equal(ctx.project_dedupe(dx, sh).to_host(), zo.project_dedupe(x, sh)), sh
    yc = rng.integers(0, 1 << 63, size=ny, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=ny, dtype=np.uint64)
    yc[-1] = np.uint64(TOP)
    k, c = ctx.project(dx, dy, ctx.upload(yc))
    ek, ec = zo.project(x, y, yc)
    assert np.array_equal(k.to_host(), ek) and np.array_equal(c.to_host(), ec)
    for seed, p in ((0, 0.37), (TOP, 0.5), (HALF + 11, 0.9)):
        k, c = ctx.sample(dy, ctx.upload(yc), seed, p)
        ek, ec = zo.sample_d(p, seed, y, yc)
        assert np.array_equal(k.to_host(), ek) and np.array_equal(c.to_host(), ec), seed
    for lo, hi in ((1, 0), (HALF, 0), (HALF, TOP - 1), (TOP, 0), (1 << 32, HALF - 1), (0, 1 << 32)):
        k, c = ctx.trim(dy, ctx.upload(yc), lo, hi)
        ek, ec = zo.trim(y, yc, lo, hi)
        assert np.array_equal(k.to_host(), ek) and np.array_equal(c.to_host(), ec), (lo, hi)


@pytest.mark.parametrize("n", [1, 2, 8193, 300_001])
def test_lower_bound_and_first_descent_edge_keys(ctx, n):
    keys = edge_keys(n, 6)
    d = ctx.upload(keys)
    q = [0, 1, 3, 4, HALF - 1, HALF, HALF + 1, TOP - 1, TOP]
    want = np.searchsorted(keys, np.array(q, dtype=np.uint64), side="left")
    assert ctx.lower_bound(d, q) == [int(v) for v in want]
    assert ctx.first_descent(d) == n              # strictly ascending across 2^63 (no signed compare)
    if n >= 2:
        bad = keys.copy()
        bad[1] = bad[0]
        assert ctx.first_descent(ctx.upload(bad)) == 1
        bad = keys.copy()
        bad[-1] = np.uint64(0)                    # 2^64 - 1 replaced by 0 at the last index
        assert ctx.first_descent(ctx.upload(bad)) == n - 1
        bad = keys.copy()
        bad[-2] = np.uint64(TOP)                  # equal neighbours at the top of the range
        assert ctx.first_descent(ctx.upload(bad)) == n - 1


@pytest.mark.parametrize("n", [1, 8193, 100_003])
def test_hash_partition_and_checksums_edge_keys(ctx, n):
    """zk_hash_partition: the owner of x is murmer(x, seed) * world >> 64 in Python ints, the split stable; zk_checksum_counts:
    Python sums mod 2^64 over 32- and 64-bit counts"""
    rng = np.random.default_rng(n)
    keys = edge_keys(n, 7)
    c64 = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    c64[-1] = np.uint64(TOP)
    c32 = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    c32[0] = np.uint32((1 << 32) - 1)
    dk = ctx.upload(keys)
    kl = [int(v) for v in keys]
    for seed in (0, HALF + 5):
        h = [zo.murmer(v, seed) for v in kl]
        for world in range(1, 9):
            owner = np.array([(v * world) >> 64 for v in h])
            want_offs = [0] + [int(v) for v in np.cumsum(np.bincount(owner, minlength=world))]
            order = np.argsort(owner, kind="stable")
            for counts in (None, c32, c64):
                ok, oc, offs = ctx.hash_partition(dk, ctx.upload(counts) if counts is not None else None, world, seed)
                assert offs == want_offs, (seed, world)
                assert np.array_equal(ok.to_host(n), keys[order]), (seed, world)
                if counts is not None:
                    assert np.array_equal(oc.to_host(n), counts[order]), (seed, world, counts.dtype)
    m0 = [zo.murmer(v, 0) for v in kl]
    for counts in (None, c32, c64):
        w = [1] * n if counts is None else [int(v) for v in counts]
        want = (sum(w) & M64, sum(a * b for a, b in zip(kl, w)) & M64, sum(a * b for a, b in zip(m0, w)) & M64)
        got = ctx.checksum_counts(dk, ctx.upload(counts) if counts is not None else None)
        assert got == want, None if counts is None else counts.dtype


def test_mirror_expand_k32_edges(ctx):
    """zk_mirror_expand at K = 32: the canonical 0 (its mirror is 2^64 - 1) and even-K palindromes (counted twice)"""
    K = 32
    rng = np.random.default_rng(32)
    pal = [zo.kmer(s) for s in ("ACGT" * 8, "AT" * 16, "TA" * 16, "GC" * 16, "CG" * 16, "A" * 16 + "T" * 16, "T" * 16 + "A" * 16)]
    assert all(zo.rc(K, p) == p for p in pal)
    raw = [int(v) for v in edge_keys(100_000, 30)]
    canon = sorted(set([min(v, zo.rc(K, v)) for v in raw] + pal + [0, 1, zo.kmer("A" * 31 + "C"), zo.kmer("T" * 31 + "G")]))
    canon = sorted(set(min(v, zo.rc(K, v)) for v in canon))
    cnt = rng.integers(1, 1 << 20, size=len(canon), dtype=np.uint64)
    cnt[0] = (1 << 31) - 1                      # the canonical 0 counted 2^31 - 1 times: its mirror 2^64 - 1 the same
    table = {}
    for v, c in zip(canon, (int(x) for x in cnt)):
        table[v] = table.get(v, 0) + c
        r = zo.rc(K, v)
        if r == v:
            table[v] += c
        else:
            table[r] = table.get(r, 0) + c
    wk = np.array(sorted(table), dtype=np.uint64)
    wc = np.array([table[v] for v in sorted(table)], dtype=np.uint32)
    assert int(wk[0]) == 0 and int(wk[-1]) == TOP
    k, c = ctx.mirror_expand(ctx.upload(np.array(canon, dtype=np.uint64)), ctx.upload(cnt.astype(np.uint32)), K)
    assert np.array_equal(k.to_host(), wk) and np.array_equal(c.to_host(), wc)


def test_codec64_full_range(ctx):
    """codec64 words, plain and delta, of full-range values against the oracle: ZK_ERANGE exactly where the oracle has no code
    (a value or delta >= 2^60), an exact round trip everywhere else"""
    rng = np.random.default_rng(60)
    e60 = 1 << 60
    ok_vals = np.concatenate([np.array([0, 1, 3, e60 - 2, e60 - 1], dtype=np.uint64),
                              rng.integers(0, e60, size=100000, dtype=np.uint64) >> rng.integers(0, 60, size=100000).astype(np.uint64)])
    cases = [("ok", ok_vals)]
    for bad in (e60, e60 + 1, HALF - 1, HALF, TOP - 1, TOP):
        for at in (0, 50000, len(ok_vals)):
            cases.append(("bad_%d_at_%d" % (bad, at), np.insert(ok_vals, at, np.uint64(bad))))
    for name, v in cases:
        try:
            want = zo.codec64_encode(v)
        except IndexError:
            want = None
        if want is None:
            assert _err(lambda: ctx.codec_encode(ctx.upload(v), False)) == native.ZK_ERANGE, name
        else:
            got = ctx.codec_encode(ctx.upload(v), False)
            assert np.array_equal(got.to_host(), want), name
            assert np.array_equal(ctx.codec_decode(got, False).to_host(), v), name
    assert cases[0][0] == "ok" and len(cases) > 1
    # delta: ascending keys from 1 that climb to exactly 2^64 - 1, fifteen of the steps 2^60 - 1 (the largest with a code);
    # one step of 2^60, or a first key >= 2^60, has none
    small = [int(v) for v in rng.integers(1, 1 << 20, size=40000)]
    big = [e60 - 1] * 15 + [TOP - 1 - sum(small) - 15 * (e60 - 1)]
    assert 0 < big[-1] < e60
    steps = small + big
    rng.shuffle(steps)
    acc, cur = [], 1
    for st in [0] + steps:
        cur += st
        acc.append(cur)
    keys = np.array(acc, dtype=np.uint64)
    assert int(keys[-1]) == TOP
    for name, k in (("climb", keys), ("step_2^60", np.array([0, e60, e60 + 1, TOP], dtype=np.uint64)),
                    ("first_2^60", np.array([e60, e60 + 1], dtype=np.uint64)), ("first_below", np.array([e60 - 1, TOP - 1], dtype=np.uint64)),
                    ("jump_to_top", np.array([e60 - 1, 2 * e60 - 2, TOP - e60 + 1, TOP], dtype=np.uint64))):
        try:
            want = zo.codec64_encode(zo.delta(k))
        except IndexError:
            want = None
        if want is None:
            assert _err(lambda: ctx.codec_encode(ctx.upload(k), True)) == native.ZK_ERANGE, name
        else:
            got = ctx.codec_encode(ctx.upload(k), True)
            assert np.array_equal(got.to_host(), want), name
            assert np.array_equal(ctx.codec_decode(got, True, len(k)).to_host(), k), name


# ---- counts at their limits ---------------------------------------------------------------------------------------------

LIM32 = (1 << 32) - 1


def _limit_sets(n, rng, nlists, over):
    """nlists lists over the same edge keys whose 32-bit counts add up to exactly 2^32 - 1 at the key 0, at 2^63, at 2^64 - 1 and at a
    key in the middle (over: one more at 2^64 - 1)"""
    keys = edge_keys(n, 20)
    cs = [rng.integers(1, 1000, size=n, dtype=np.uint64) for _ in range(nlists)]
    for at in (0, int(np.searchsorted(keys, np.uint64(HALF))), n // 2, n - 1):
        split = sorted(int(v) for v in rng.integers(1, LIM32, size=nlists - 1))
        parts = [b - a for a, b in zip([0] + split, split + [LIM32])]
        parts = [max(p, 1) for p in parts]
        parts[-1] = LIM32 - sum(parts[:-1])
        for c, p in zip(cs, parts):
            c[at] = p
    if over:
        cs[0][n - 1] += np.uint64(1)
    assert all(int(v) <= LIM32 for c in cs for v in c)
    return [(keys, c) for c in cs]


@pytest.mark.parametrize("n", [1, 8193, 300_001])
def test_union_sum_and_merge_n_32bit_limit(ctx, n):
    """32-bit sums that reach exactly 2^32 - 1 come out exact; one more is ZK_EOVERFLOW (the 2-way union, the tree of 2-way passes
    and kway.hip), and the context gives correct results after the error"""
    rng = np.random.default_rng(n)
    try:
        for nlists in (2, 3, 17):
            for over in (False, True):
                sets = _limit_sets(n, rng, nlists, over)
                dev = [(ctx.upload(k), ctx.upload(c.astype(np.uint32))) for k, c in sets]
                zs, zc, _ = zo.merge_n(32, sets)
                if nlists == 2:
                    if over:
                        assert _err(lambda: ctx.union_sum(dev[0][0], dev[0][1], dev[1][0], dev[1][1])) == native.ZK_EOVERFLOW
                    else:
                        k, c = ctx.union_sum(dev[0][0], dev[0][1], dev[1][0], dev[1][1])
                        assert np.array_equal(k.to_host(), zs) and np.array_equal(c.to_host().astype(np.uint64), zc)
                        assert int(c.to_host()[-1]) == LIM32
                for kway in (0, 2):
                    ctx.tune(kway=kway)
                    if over:
                        assert _err(lambda: ctx.merge_n(dev)) == native.ZK_EOVERFLOW, (nlists, kway)
                    else:
                        gk, gc, _ = ctx.merge_n(dev)
                        assert np.array_equal(gk.to_host(), zs) and np.array_equal(gc.to_host().astype(np.uint64), zc), (nlists, kway)
                        assert int(gc.to_host()[-1]) == LIM32
                # after an error: the same context, a correct result (64-bit counts hold the sums that overflowed)
                dev64 = [(ctx.upload(k), ctx.upload(c)) for k, c in sets]
                gk, gc, _ = ctx.merge_n(dev64)
                assert np.array_equal(gk.to_host(), zs) and np.array_equal(gc.to_host(), zc)
                k, c = ctx.union_sum(dev64[0][0], dev64[0][1], dev64[1][0], dev64[1][1])
                z2k, z2c = zo.union_sum(sets[0][0], sets[0][1], sets[1][0], sets[1][1])
                assert np.array_equal(k.to_host(), z2k) and np.array_equal(c.to_host(), z2c)
    finally:
        ctx.tune(kway=1)


def test_trim_bounds_beyond_32_bits(ctx):
    rng = np.random.default_rng(33)
    n = 200_003
    keys = edge_keys(n, 21)
    c32 = rng.integers(1, 1 << 32, size=n, dtype=np.uint64)
    c32[:4] = [1, LIM32 - 1, LIM32, 4096]
    dk, d32 = ctx.upload(keys), ctx.upload(c32.astype(np.uint32))
    for lo, hi in ((1 << 32, 0), (1 << 32, 1 << 33), (LIM32 + 1, TOP), (TOP, 0), (1, 1 << 32), (LIM32, 1 << 40), (1 << 31, (1 << 32) + 7)):
        k, c = ctx.trim(dk, d32, lo, hi)
        ek, ec = zo.trim(keys, c32, lo, hi)
        assert np.array_equal(k.to_host(), ek) and np.array_equal(c.to_host().astype(np.uint64), ec), (lo, hi)
        if lo > LIM32:
            assert k.n == 0
    c64 = c32 << np.uint64(rng.integers(0, 32))
    c64[:6] = [LIM32, 1 << 32, (1 << 32) + 1, HALF, TOP - 1, TOP]
    d64 = ctx.upload(c64)
    for lo, hi in ((1 << 32, 0), (1 << 32, (1 << 32) + 1), ((1 << 32) + 1, HALF), (HALF, 0), (TOP, 0), (1, LIM32), (1 << 33, TOP - 1)):
        k, c = ctx.trim(dk, d64, lo, hi)
        ek, ec = zo.trim(keys, c64, lo, hi)
        assert np.array_equal(k.to_host(), ek) and np.array_equal(c.to_host(), ec), (lo, hi)


def _want_hist(counts):
    hv, hf = zo.hist(counts)
    return {int(a): int(b) for a, b in zip(hv, hf)}


def test_hist_dense_border_and_wide_counts(ctx):
    """ctx.hist against the oracle across the 4095 / 4096 border of the LDS bins, and u64 counts of 2^32, 2^63 and 2^64 - 1 -- in
    arrays whose length leaves lanes past the end"""
    rng = np.random.default_rng(4096)
    border = rng.choice(np.array([0, 1, 2, 4094, 4095, 4096, 4097, 8191, 8192, LIM32], dtype=np.uint64), size=1_000_003)
    for cdt in (np.uint32, np.uint64):
        assert ctx.hist(ctx.upload(border.astype(cdt))) == _want_hist(border), cdt
    for vals in ([HALF], [1 << 32], [HALF, HALF, 1], [HALF - 1, HALF, HALF + 1, TOP - 1, TOP, 1 << 32, LIM32, 4096, 4095, 1]):
        c = np.array(vals, dtype=np.uint64)
        assert ctx.hist(ctx.upload(c)) == _want_hist(c), vals
    wide = rng.choice(np.array([1, 7, 4096, LIM32, 1 << 32, HALF, TOP], dtype=np.uint64), size=300_001)
    assert ctx.hist(ctx.upload(wide)) == _want_hist(wide)
    assert HALF in _want_hist(wide)


@pytest.mark.parametrize("distinct", ["few", "many"])
def test_hist_more_large_counts_than_the_side_list(ctx, distinct):
    """5 M counts, every one >= 4096: more than the 4 Mi entries the side list of large counts starts with; few distinct values, or
    more than 65 536 (more bins than the first call makes room for)"""
    rng = np.random.default_rng(5 if distinct == "few" else 6)
    n = 5_000_000
    if distinct == "few":
        c = rng.choice(np.array([4096, 5000, 65536, 1 << 20, LIM32], dtype=np.uint64), size=n)
    else:
        c = np.uint64(4096) + rng.integers(0, 200_000, size=n, dtype=np.uint64)
    want = _want_hist(c)
    if distinct == "many":
        assert len(want) > 65536
    for cdt in (np.uint32, np.uint64):
        assert ctx.hist(ctx.upload(c.astype(cdt))) == want, cdt
    # and the context after it: a small histogram as before
    small = np.array([1, 1, 2, 4096, 5000], dtype=np.uint32)
    assert ctx.hist(ctx.upload(small)) == _want_hist(small)
