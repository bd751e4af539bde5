"""
Every entry point on an EMPTY workspace.  A C-ABI call takes its device scratch from the context's bump arena (context.hip:
arena_require / arena_alloc), sized either by the call's own estimate (arena_require, then exactly that size) or by its first
allocation (+ max(64 MiB, 1/16)).  The arena never shrinks, so on a context that earlier calls have grown an estimate that is too
small goes unnoticed; the CLI's process-wide context does not have that cover.  Each case here calls ctx.release_workspace() right
before the call under test (`fresh`), at a size where the proportional terms of the estimate dominate its fixed slack, and checks
the result -- against the oracle or numpy on small inputs, on large ones against arrays known by construction or against the
size-independent properties of test_gpu_fullsize.py (order-free checksums of the stream, strict ascent, a second plan).

Which plan ran is read from the profile records where a case claims one: the number of union passes of zk_merge_n (one per k-way or
2-way pass), the even-K replan of zk_kmerize (the keys of both strands sorted and counted at once: no union of the canonical list
with its mirror image), the block dedupe's copy above 2^29 stream bytes (16 bytes a canonical k-mer on the strand-block route at odd K,
24 with the mirror words at even K, none at K >= 27 where no count packs beside the k-mer), the tile sort, and the mirrored pairs as
words or as pairs.
"""
import numpy as np
import pytest

from oracle import zkoracle as zo
from zotmer_amd import native, synth

pytestmark = pytest.mark.gpu

MiB = 1 << 20


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def fresh(ctx, fn, *a, **kw):
    """fn(*a, **kw) on an empty workspace; -> (its result, the profile records of the call)"""
    ctx.release_workspace()
    ctx.profile(True)
    try:
        r = fn(*a, **kw)
        return r, ctx.profile_read()
    finally:
        ctx.profile(False)


def revcomp_np(x, K):
    x = np.asarray(x, dtype=np.uint64)
    r = np.zeros_like(x)
    for i in range(K):
        r = (r << np.uint64(2)) | (np.uint64(3) - ((x >> np.uint64(2 * i)) & np.uint64(3)))
    return r


def n_canonical_of(kmers, K):
    """distinct canonical k-mers of a both-strand table: every k-mer and its mirror image, a palindrome once"""
    k = np.asarray(kmers, dtype=np.uint64)
    pal = int(np.count_nonzero(revcomp_np(k, K) == k)) if K % 2 == 0 else 0
    assert (len(k) + pal) % 2 == 0
    return (len(k) + pal) // 2


def canonical_of(kmers, counts, K):
    """the counted canonical list of a both-strand table: the entries with x <= rc x, a palindrome's count halved (it was counted
    twice per window)"""
    k = np.asarray(kmers, dtype=np.uint64)
    rc = revcomp_np(k, K)
    keep = k <= rc
    c = np.asarray(counts)[keep].astype(np.uint32)
    c[k[keep] == rc[keep]] //= 2
    return k[keep], c


def stream_of(reads):
    return ("".join(r + "\n" for r in reads)).encode()


# ---- zk_merge_n ---------------------------------------------------------------------------------------------------------------

def union_passes(k, fan_in):
    """passes of merge_many's level loop: groups of up to fan_in lists, a lone list sits out its level"""
    m, p = k, 0
    while m > 1:
        groups = [min(fan_in, m - i) for i in range(0, m, fan_in)]
        p += sum(1 for g in groups if g >= 2)
        m = len(groups)
    return p


def merge_lists(k, n, S, bits):
    """k sorted lists of n keys: list i holds (j*S + i % S)*3 + 1 for j < n -- disjoint when S == k, lists i and i + S the same keys
    otherwise.  -> (host lists [(keys, counts)], expected union keys, expected summed counts)"""
    dt = np.uint32 if bits == 32 else np.uint64
    j = np.arange(n, dtype=np.uint64)
    E = np.zeros((n, S), dtype=np.uint64)
    lists = []
    for i in range(k):
        keys = (j * np.uint64(S) + np.uint64(i % S)) * np.uint64(3) + np.uint64(1)
        c = np.uint64(1) + (j * np.uint64(5) + np.uint64(i)) % np.uint64(1009)
        if bits == 64 and i % 8 == 0:
            c = c + np.uint64(1 << 32)          # counts beyond 32 bits
        E[:, i % S] += c
        lists.append((keys, c.astype(dt)))
    want_k = np.arange(n * S, dtype=np.uint64) * np.uint64(3) + np.uint64(1)
    return lists, want_k, E.reshape(-1)


# (lists, pairs a list, key residues): 48 disjoint lists (two k-way levels), 40 lists of 4 Mi pairs with two of them repeated (two
# levels), 33 (one list sits out level 1, level 2 is a 3-list k-way pass), 17 (level 2 a 2-way pass)
MERGE_CASES = {"48x1Mi": (48, 1 * MiB, 48), "40x4Mi": (40, 4 * MiB, 38), "33x1Mi": (33, 1 * MiB, 33), "17x1Mi": (17, 1 * MiB, 17)}


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("case", list(MERGE_CASES))
def test_merge_n_fresh(ctx, case, bits):
    """zk_merge_n sizes its workspace up front: the two ping-pong regions and the scratch of one pass (merge_many).  On an empty
    workspace every level of k-way passes must fit -- with kway 1 (the default: k-way from 4 Mi pairs on), 2 (always) and 0 (the tree
    of 2-way passes) -- and give the union known by construction."""
    k, n, S = MERGE_CASES[case]
    lists, want_k, want_c = merge_lists(k, n, S, bits)
    acgt = [int(want_c[(want_k & np.uint64(3)) == np.uint64(b)].sum(dtype=np.uint64)) for b in range(4)]
    dev = [(ctx.upload(a), ctx.upload(b)) for a, b in lists]
    del lists
    try:
        for kway in (1, 2, 0):
            ctx.tune(kway=kway)
            (mk, mc, macgt), prof = fresh(ctx, ctx.merge_n, dev)
            assert mk.n == len(want_k), (case, bits, kway)
            assert np.array_equal(mk.to_host(), want_k), (case, bits, kway)
            assert np.array_equal(mc.to_host().astype(np.uint64), want_c), (case, bits, kway)
            assert macgt == acgt, (case, bits, kway)
            passes = union_passes(k, 2 if kway == 0 else 16)
            assert prof["union_sum"]["launches"] == passes, (case, bits, kway, prof.get("union_sum"))
            del mk, mc
    finally:
        ctx.tune(kway=1)


def test_merge_n_small_vs_oracle_fresh(ctx):
    """Two k-way levels on inputs small enough for the oracle (kway 2: k-way at any size), random keys that the lists share in part."""
    rng = np.random.default_rng(41)
    pool = np.sort(rng.choice(np.arange(1 << 24, dtype=np.uint64), size=1 << 21, replace=False)) << np.uint64(20)
    sets = []
    for s in range(35):
        x = np.sort(rng.choice(pool, size=int(rng.integers(1000, 120000)), replace=False))
        sets.append((x, rng.integers(1, 1 << 40, size=len(x), dtype=np.uint64)))
    zs, zc, acgt = zo.merge_n(25, sets)
    dev = [(ctx.upload(a), ctx.upload(b)) for a, b in sets]
    try:
        ctx.tune(kway=2)
        (gk, gc, gacgt), prof = fresh(ctx, ctx.merge_n, dev)
        assert np.array_equal(gk.to_host(), zs) and np.array_equal(gc.to_host(), zc) and gacgt == acgt
        assert prof["union_sum"]["launches"] == union_passes(35, 16)
    finally:
        ctx.tune(kway=1)


# ---- sorts, union, search, histogram ------------------------------------------------------------------------------------------

GOLD = np.uint64(0x9E3779B97F4A7C15)          # odd: i -> i * GOLD mod 2^64 is a bijection, the keys are distinct and spread


@pytest.mark.parametrize("tile_sort", [1, 0])
def test_sorts_fresh(ctx, tile_sort):
    """zk_sort_keys, zk_sort_pairs, zk_sort_count at 2^26 64-bit keys, with the tile sort and without.  The keys are i * GOLD, so a
    sorted pair (key, i) is checked by recomputing the key from its value."""
    n = 1 << 26
    idx = np.arange(n, dtype=np.uint64)
    keys = idx * GOLD
    try:
        ctx.tune(tile_sort=tile_sort)
        d = ctx.upload(keys)
        want = ctx.checksum(d)
        (sk, prof) = fresh(ctx, ctx.sort_keys, d, 64)
        assert ctx.first_descent(sk) == n and ctx.checksum(sk) == want
        assert ("tile_sort" in prof) == bool(tile_sort), prof
        del sk, d
        dk, dv = ctx.upload(keys), ctx.upload(idx.astype(np.uint32))
        (pk, pv), prof = fresh(ctx, ctx.sort_pairs, dk, dv, 64)
        kh, vh = pk.to_host(), pv.to_host()
        assert np.all(kh[1:] > kh[:-1]) and np.array_equal(kh, vh.astype(np.uint64) * GOLD)
        assert ("tile_sort" in prof) == bool(tile_sort), prof
        del dk, dv, pk, pv, kh, vh
        # every key four times
        q = n // 4
        dup = ctx.upload((idx % np.uint64(q)) * GOLD)
        (uk, uc), prof = fresh(ctx, ctx.sort_count, dup, 64)
        assert uk.n == q and ctx.first_descent(uk) == q
        assert np.all(uc.to_host() == 4)
        assert ctx.checksum(uk) == ctx.checksum(ctx.upload(idx[:q] * GOLD))
    finally:
        ctx.tune(tile_sort=1)


def test_union_sum_lower_bound_hist_fresh(ctx):
    """zk_union_sum (both count widths) of two lists of 2^26 keys, interleaved with a shared third; zk_lower_bound over the result;
    zk_hist of counts with more distinct values than its dense table (the side list)."""
    n = 1 << 26
    j = np.arange(n, dtype=np.uint64)
    xk, yk = j * np.uint64(4), j * np.uint64(4) + np.uint64(1)
    yk[::3] = xk[::3]                                    # every third key in both lists
    xc = np.uint64(1) + j % np.uint64(7)
    yc = np.uint64(2) + j % np.uint64(11)
    wk = np.union1d(xk, yk)
    wc = (np.bincount(np.searchsorted(wk, xk), weights=xc, minlength=len(wk)) +
          np.bincount(np.searchsorted(wk, yk), weights=yc, minlength=len(wk))).astype(np.uint64)          # (small sums: exact in doubles)
    dxk, dyk = ctx.upload(xk), ctx.upload(yk)
    for dt in (np.uint32, np.uint64):
        (uk, uc), _ = fresh(ctx, ctx.union_sum, dxk, ctx.upload(xc.astype(dt)), dyk, ctx.upload(yc.astype(dt)))
        assert np.array_equal(uk.to_host(), wk) and np.array_equal(uc.to_host().astype(np.uint64), wc), dt
    rng = np.random.default_rng(5)
    qs = rng.integers(0, int(wk[-1]) + 8, size=1 << 20, dtype=np.uint64)
    pos, _ = fresh(ctx, ctx.lower_bound, uk, qs)
    assert np.array_equal(pos.astype(np.int64), np.searchsorted(wk, qs, side="left"))
    # counts 1..2^22, spread: a thousand times more values than the dense table of zk_hist holds (4096), the rest in its side list
    cnt = (j * GOLD >> np.uint64(42)) + np.uint64(1)
    h, _ = fresh(ctx, ctx.hist, ctx.upload(cnt))
    v, f = np.unique(cnt, return_counts=True)
    assert h == {int(a): int(b) for a, b in zip(v, f)}


# ---- zk_mirror_expand ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [600, 560_000])
@pytest.mark.parametrize("packed", [1, 0])
def test_mirror_expand_fresh(ctx, R, packed):
    """zk_mirror_expand on the counted canonical list of R random reads (no genome: hardly a k-mer twice): R = 600 gives just above
    2^16 canonical k-mers, 560 000 more than 2^26 (where the estimate adds the tables of a 24-bit grouping).  packed = 1: the mirrored pairs
    travel as single words (the mirror copy books 20 bytes an entry), 0: as pairs.  Checked against zk_kmerize of both strands."""
    K, L = 25, 150
    d = ctx.synth_reads(synth.DEFAULT_SEED + 5, 0, R, L, genome=0)
    try:
        ctx.tune(packed_pairs=packed)
        ck, cc, _ = ctx.kmerize(d, K, native.KMERIZE_CANONICAL_ONLY)
        assert ck.n > (1 << 16 if R == 600 else 1 << 26)
        k, c, st = ctx.kmerize(d, K)
        (ek, ec), prof = fresh(ctx, ctx.mirror_expand, ck, cc, K)
        assert ek.n == k.n and ctx.checksum(ek, ec) == ctx.checksum(k, c) and ctx.first_descent(ek) == ek.n
        assert ctx.checksum(ek, ec) == ctx.stream_checksum(d, K)
        mirror = prof.get("mirror", {}).get("bytes", 0)
        assert (mirror == 20 * ck.n) == bool(packed), (R, packed, prof.get("mirror"))
    finally:
        ctx.tune(packed_pairs=1)


# ---- zk_kmerize around 2^29 stream bytes --------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [24, 25, 31, 32])
@pytest.mark.parametrize("side", ["below", "above"])
def test_kmerize_2p29_fresh(ctx, K, side):
    """zk_kmerize just below and just above 2^29 stream bytes (from there on the block dedupe with 2^18 blocks, and the estimate
    adds its tables), on genome reads (they repeat their k-mers): default,
    ZK_KMERIZE_BOTH, ZK_KMERIZE_CANONICAL_ONLY (+ zk_mirror_expand) and ZK_KMERIZE_SUBSAMPLE (= zk_subsample of the default's
    k-mers), each on an empty workspace.  The block dedupe's copy books 16 bytes a canonical k-mer on the strand-block route (odd K)
    and 24 where it writes the mirror words (even K) -- above the threshold only; K = 31, 32 have no room for a count beside the k-mer: no block dedupe, the
    copies are counted after the low passes and the pairs finish the sort."""
    L = 150
    R = ((1 << 29) // (L + 1)) + (3000 if side == "above" else -3000)
    cfg = synth.CONFIGS["config2"]
    d = ctx.synth_reads(synth.DEFAULT_SEED, 0, R, L, genome=cfg["genome"], sub_thr=synth.frac32(cfg["sub"]), n_thr=synth.frac32(cfg["n"]))
    assert (d.n >= 1 << 29) == (side == "above")
    want = ctx.stream_checksum(d, K)
    cap = int(2 * (cfg["genome"] + R * L * cfg["sub"] * (K - 3)) * 1.25) + MiB
    out = (ctx.empty(cap, np.uint64), ctx.empty(cap, np.uint32))
    (k, c, st), prof = fresh(ctx, ctx.kmerize, d, K, out=out)
    sel = prof.get("select", {}).get("bytes", 0)
    if K < 27:
        assert (sel == (16 if K & 1 else 24) * st.n_canonical) == (side == "above"), (K, side, prof)
    else:
        assert sel not in (16 * st.n_canonical, 24 * st.n_canonical) and "pass_pairs" in prof, (K, side, prof)
    assert ctx.checksum(k, c) == want and st.n_instances == want[0] and st.n_unique == k.n
    assert ctx.first_descent(k) == k.n and list(st.acgt) == list(ctx.stream_acgt(d, K))
    n_unique, n_can, ref = k.n, st.n_canonical, (st.n_windows, st.n_instances, list(st.acgt))
    keys_sum = ctx.checksum(k)
    sub = ctx.checksum(ctx.subsample(k, 5, 0.3))
    del k, c
    (kb, cb, stb), _ = fresh(ctx, ctx.kmerize, d, K, native.KMERIZE_BOTH, out=out)
    assert kb.n == n_unique and ctx.checksum(kb, cb) == want and ctx.first_descent(kb) == kb.n
    assert (stb.n_windows, stb.n_instances, list(stb.acgt)) == ref and stb.n_canonical == 0
    del kb, cb
    (ck, cc, stc), _ = fresh(ctx, ctx.kmerize, d, K, native.KMERIZE_CANONICAL_ONLY, cap=cap)
    assert stc.n_unique == n_can and stc.n_canonical == n_can and ctx.first_descent(ck) == ck.n
    (ek, ec), _ = fresh(ctx, ctx.mirror_expand, ck, cc, K, out=out)
    assert ek.n == n_unique and ctx.checksum(ek, ec) == want
    del ck, cc, ek, ec
    (ks, cs, sts), _ = fresh(ctx, ctx.kmerize, d, K, native.KMERIZE_SUBSAMPLE, p=0.3, seed=5, out=out)
    assert ctx.checksum(ks) == sub and sts.n_unique == ks.n and ctx.first_descent(ks) == ks.n
    assert sts.n_canonical == n_can and (sts.n_windows, sts.n_instances, list(sts.acgt)) == ref
    assert ctx.checksum(ks) != keys_sum


@pytest.mark.parametrize("K", [24, 25])
def test_kmerize_replan_2p29_fresh(ctx, K):
    """Reads that do not repeat their k-mers, just above 2^29 stream bytes: the look before the sort declines the block dedupe and
    the batch is planned again for the keys of both strands (twice the sort buffers, asked for on the empty workspace).  The
    result carries the stream's checksums, and n_canonical is the length of the counted canonical list."""
    L = 150
    R = ((1 << 29) // (L + 1)) + 3000
    d = ctx.synth_reads(synth.DEFAULT_SEED + 9, 0, R, L, genome=0, n_thr=synth.frac32(0.0005))
    want = ctx.stream_checksum(d, K)
    (k, c, st), prof = fresh(ctx, ctx.kmerize, d, K)
    assert "union_sum" not in prof and "mirror" not in prof and "tile_sort" in prof, prof
    assert ctx.checksum(k, c) == want and st.n_unique == k.n and ctx.first_descent(k) == k.n
    n_can = st.n_canonical
    del k, c
    (ck, cc, stc), prof = fresh(ctx, ctx.kmerize, d, K, native.KMERIZE_CANONICAL_ONLY)
    assert stc.n_unique == n_can and n_can > 0


# ---- first allocation ---------------------------------------------------------------------------------------------------------

def test_first_allocation_entries_fresh(ctx):
    """Calls that size the workspace by their first allocation, each at 2^27 elements on an empty workspace: zk_rle, zk_subsample,
    zk_sample and zk_trim (against the oracle), zk_undelta."""
    n = 1 << 27
    idx = np.arange(n, dtype=np.uint64)
    keys = ctx.upload(idx // np.uint64(3) * np.uint64(5))        # sorted, every key three times (the last twice or once)
    (uk, uc), _ = fresh(ctx, ctx.rle, keys)
    q = (n + 2) // 3
    assert uk.n == q and ctx.first_descent(uk) == q
    uch = uc.to_host()
    assert np.all(uch[:-1] == 3) and int(uch.sum()) == n
    del keys
    # zk_subsample keeps x where murmer(x, seed) / (2^61 - 1) < p: the kept keys are input keys in input order, and on a sample of
    # inputs membership is the oracle's predicate
    hk = idx * np.uint64(3)
    sk = ctx.upload(hk)
    (s1, _) = fresh(ctx, ctx.subsample, sk, 7, 0.25)
    sh = s1.to_host()
    assert np.all(sh[1:] > sh[:-1]) and np.all(sh % np.uint64(3) == 0) and 0 < len(sh) < n
    probe = np.random.default_rng(8).choice(hk, size=4096, replace=False)
    pos = np.minimum(np.searchsorted(sh, probe), len(sh) - 1)
    assert [bool(v) for v in sh[pos] == probe] == [zo.sub(7, 0.25, int(x)) for x in probe]
    del sk, s1, sh
    dk = ctx.upload(idx * np.uint64(3))
    dc = ctx.upload(np.uint64(1) + idx % np.uint64(100))
    (tk, tc), _ = fresh(ctx, ctx.trim, dk, dc, 50)
    hc = np.uint64(1) + idx % np.uint64(100)
    keep = hc >= np.uint64(50)
    assert tk.n == int(keep.sum()) and np.array_equal(tc.to_host(), hc[keep]) and np.array_equal(tk.to_host(), (idx * np.uint64(3))[keep])
    (pk, pc), _ = fresh(ctx, ctx.sample, dk, dc, 3, 0.5)
    zk_, zc_ = zo.sample_d(0.5, 3, idx * np.uint64(3), hc)
    assert np.array_equal(pk.to_host(), zk_) and np.array_equal(pc.to_host(), zc_)
    del zk_, zc_
    del dk, dc, tk, tc, pk, pc
    deltas = ctx.upload(np.full(n, 3, dtype=np.uint64))
    (u, _) = fresh(ctx, ctx.undelta, deltas, 11)
    uh = u.to_host()
    assert uh[0] == 14 and uh[-1] == 11 + 3 * n and np.all(np.diff(uh) == 3)


# ---- codec, partition, set operations, encode, FASTQ, capture ---------------------------------------------------------------

def fastq_text(seqs):
    """(R, L) uint8 sequence rows -> FASTQ text '@q\n' seq '\n+\n' seq '\n' per record (uint8, record r at r * (2L + 7))"""
    R, L = seqs.shape
    rec = np.empty((R, 2 * L + 7), dtype=np.uint8)
    rec[:, 0:3] = np.frombuffer(b"@q\n", np.uint8)
    rec[:, 3:3 + L] = seqs
    rec[:, 3 + L:6 + L] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 6 + L:6 + 2 * L] = seqs
    rec[:, -1] = ord("\n")
    return rec


def test_codec_dev_fresh(ctx):
    """zk_codec64_encode_dev (k-mer deltas and plain 64-bit values) and zk_codec64_encode_u32_dev against the host codec, and
    zk_codec64_decode_dev back, on 2^27 values each."""
    from zotmer_amd.library import vectors
    n = 1 << 27
    idx = np.arange(n, dtype=np.uint64)
    kmers = idx * np.uint64(7) + (idx & np.uint64(3))          # ascending, deltas of 4..10
    counts = (idx * GOLD) >> np.uint64(40)                     # up to 2^24
    for vals, delta in ((kmers, True), (counts, False), (counts.astype(np.uint32), False)):
        d = ctx.upload(vals)
        w, _ = fresh(ctx, ctx.codec_encode, d, delta)
        want = vectors._enc(vals.astype(np.uint64), delta)
        assert np.array_equal(w.to_host(), want), (vals.dtype, delta)
        back, _ = fresh(ctx, ctx.codec_decode, w, delta, n)
        assert np.array_equal(back.to_host(), vals.astype(np.uint64)), (vals.dtype, delta)
        del d, w, back


def test_hash_partition_fresh(ctx):
    """zk_hash_partition of a sorted table of 2^27 k-mers with 32-bit counts over 8 owners: a stable split (every part ascending,
    the pairs a permutation of the input's), and on a sample of every part the owner is murmer(x, seed) * world >> 64."""
    n, world, seed = 1 << 27, 8, 5
    idx = np.arange(n, dtype=np.uint64)
    dk = ctx.upload(idx * np.uint64(5) + np.uint64(2))
    dc = ctx.upload((np.uint64(1) + idx % np.uint64(977)).astype(np.uint32))
    (ok, oc, offs), _ = fresh(ctx, ctx.hash_partition, dk, dc, world, seed)
    assert offs[0] == 0 and offs[-1] == n and all(a <= b for a, b in zip(offs, offs[1:]))
    assert ctx.checksum_counts(ok, oc) == ctx.checksum_counts(dk, dc)
    kh = ok.to_host()
    rng = np.random.default_rng(6)
    for w in range(world):
        part = ok.view(offs[w + 1] - offs[w], offs[w])
        assert ctx.first_descent(part) == part.n, w
        for i in rng.integers(offs[w], offs[w + 1], size=256):
            assert (zo.murmer(int(kh[i]), seed) * world) >> 64 == w, (w, int(kh[i]))


def test_set_operations_fresh(ctx):
    """zk_project_dedupe, zk_split and zk_project at 2^27 k-mers against the oracle."""
    n = 1 << 27
    idx = np.arange(n, dtype=np.uint64)
    x = idx * np.uint64(6) + (idx & np.uint64(1))                # ascending
    y = idx * np.uint64(4)                                       # holds half of x: its keys 12 m
    yc = np.uint64(1) + idx % np.uint64(31)
    dx, dy = ctx.upload(x), ctx.upload(y)
    pd, _ = fresh(ctx, ctx.project_dedupe, dx, 6)
    assert np.array_equal(pd.to_host(), zo.project_dedupe(x, 6))
    del pd
    abc, _ = fresh(ctx, ctx.split, dx, dy)
    assert abc == zo.split(x, y)
    (pk, pc), _ = fresh(ctx, ctx.project, dx, dy, ctx.upload(yc))
    wk, wc = zo.project(x, y, yc)
    assert np.array_equal(pk.to_host(), wk) and np.array_equal(pc.to_host(), wc)


def test_encode_and_fastq_mask_fresh(ctx):
    """zk_encode (both strands) of a 2^27-byte base stream carries the stream's checksums and acgt; zk_fastq_mask of the FASTQ
    text of the same reads (2^28 bytes) keeps the sequence lines and turns every other byte into '\n'."""
    K, L = 25, 150
    R = (1 << 27) // (L + 1) + 1
    d = ctx.synth_reads(synth.DEFAULT_SEED + 3, 0, R, L, genome=1 << 20, sub_thr=synth.frac32(0.01), n_thr=synth.frac32(0.001))
    (keys, acgt), _ = fresh(ctx, ctx.encode, d, K)
    assert ctx.checksum(keys) == ctx.stream_checksum(d, K) and acgt == ctx.stream_acgt(d, K)
    del keys
    seqs = d.to_host().reshape(R, L + 1)[:, :L]
    text = fastq_text(seqs)
    want = np.full(text.shape, ord("\n"), dtype=np.uint8)
    want[:, 3:3 + L] = seqs
    (m, newlines), _ = fresh(ctx, ctx.fastq_mask, ctx.upload(text.reshape(-1)))
    assert newlines == 4 * R and np.array_equal(m.to_host(), want.reshape(-1))


def test_capture_fresh(ctx):
    """zk_capture_filter over a 2^27-byte base stream, the baits being every both-strand 31-mer of its first half (random reads:
    the first half is kept whole, the second blanked); zk_capture_hits and zk_capture_gather over the FASTQ text of 2^21 random reads
    with every 1024th read as a bait record: each bait hits exactly the read it was taken from, and the gathered records are those
    reads' records, bait by bait.  31-mers on both sides, so that two random reads share one with odds of about 10^-3 here."""
    K, L = 31, 150
    R = (1 << 27) // (L + 1) + 1
    R -= R & 1
    d = ctx.synth_reads(synth.DEFAULT_SEED + 4, 0, R, L, genome=0)
    half = d.view((R // 2) * (L + 1))
    bk, _, _ = ctx.kmerize(ctx.copy_of(half), K)
    (out, n_reads, n_kept), _ = fresh(ctx, ctx.capture_filter, d, K, bk)
    assert n_reads == R and n_kept == R // 2
    rows = out.to_host().reshape(R, L + 1)[:, :L]
    src = d.to_host().reshape(R, L + 1)[:, :L]
    assert np.array_equal(rows[:R // 2], src[:R // 2]) and np.all(rows[R // 2:] == ord("N"))
    del out, rows, src, bk, half, d
    R2, step = 1 << 21, 1024
    d2 = ctx.synth_reads(synth.DEFAULT_SEED + 6, 0, R2, L, genome=0)
    seqs = d2.to_host().reshape(R2, L + 1)[:, :L]
    picked = np.arange(0, R2, step)
    table = ctx.bait_table(ctx.upload_stream(b"".join(seqs[r].tobytes() + b"\n" for r in picked)), K)
    text = fastq_text(seqs)
    dt = ctx.upload(text.reshape(-1))
    lines = ctx.line_ends(dt)
    assert lines.n == 4 * R2
    pairs, _ = fresh(ctx, ctx.capture_hits, table, K, dt, lines, R2)
    want = (np.arange(len(picked), dtype=np.uint64) << np.uint64(32)) | picked.astype(np.uint64)
    assert np.array_equal(pairs.to_host(), want)
    (g, pair_spans, byte_spans), _ = fresh(ctx, ctx.capture_gather, pairs, len(picked), dt, lines)
    assert np.array_equal(pair_spans, np.arange(len(picked) + 1, dtype=np.uint64))
    assert g.to_host().tobytes() == text[picked].tobytes()
    assert int(byte_spans[-1]) == g.n


# ---- zk_kmerize_stats on every plan -------------------------------------------------------------------------------------------

# (name, tune): every plan tune() can force, and the default
PLANS = [("default", {}), ("short", dict(short_sort=1)), ("early_collapse0", dict(early_collapse=0)), ("early_collapse1", dict(early_collapse=1)),
         ("early_collapse2", dict(early_collapse=2)), ("early_collapse3", dict(early_collapse=3)), ("dedupe9", dict(dedupe_bits=9)),
         ("dedupe18_sb1", dict(dedupe_bits=18, strand_blocks=1)), ("dedupe18_sb0", dict(dedupe_bits=18, strand_blocks=0)),
         ("tile_sort0", dict(tile_sort=0)), ("tile_sort1", dict(tile_sort=1))]
DEFAULTS = dict(short_sort=0, early_collapse=1, packed_pairs=1, dedupe_bits=0, strand_blocks=1, tile_sort=1)


def _stats(st):
    return (st.n_windows, st.n_instances, st.n_unique, st.n_canonical, list(st.acgt))


@pytest.mark.parametrize("K", [24, 25, 31, 32])
def test_kmerize_stats_every_plan(ctx, K):
    """The keys, counts and all five stats fields of zk_kmerize are the same on every plan, and n_canonical is the oracle's number
    of distinct canonical k-mers (the short path counted its side list's entries, a k-mer once per group it was cut into).  The
    input that does not repeat its k-mers is the smallest that the look before the sort samples
    (4 Mi stream bytes): with the block dedupe over 9 bits it declines, and the batch is planned again for the keys of both strands
    (asserted from the profile; K = 31, 32 have no block dedupe, so there is no look and no replan).  ZK_KMERIZE_SUBSAMPLE agrees across the plans too, and its n_canonical is counted before the
    subsample."""
    deep = synth.read_strings(21, 0, 6000, 150, genome=12000, sub_thr=synth.frac32(0.004), n_thr=synth.frac32(0.001))
    flat = synth.read_strings(22, 0, 28000, 150, genome=0)
    try:
        for name, reads in (("deep", deep), ("flat", flat)):
            want = zo.kmerize(K, reads)
            n_can = n_canonical_of(want["kmers"], K)
            can_k, can_c = canonical_of(want["kmers"], want["counts"], K)
            data = stream_of(reads)
            if name == "flat":
                assert len(data) >= 4 * MiB
            d = ctx.upload_stream(data)
            ref = sub_ref = None
            for plan, knobs in PLANS:
                ctx.tune(**DEFAULTS)
                ctx.tune(**knobs)
                (k, c, st), prof = fresh(ctx, ctx.kmerize, d, K)
                assert np.array_equal(k.to_host(), want["kmers"]) and np.array_equal(c.to_host(), want["counts"]), (name, K, plan)
                assert st.n_canonical == n_can, (name, K, plan, st.n_canonical, n_can)
                assert list(st.acgt) == want["acgt"] and st.n_unique == len(want["kmers"]), (name, K, plan)
                if ref is None:
                    ref = _stats(st)
                assert _stats(st) == ref, (name, K, plan, _stats(st), ref)
                if name == "flat" and plan in ("default", "dedupe9") and K < 27:
                    assert "union_sum" not in prof and "tile_sort" in prof, (name, K, plan, prof)          # the replan
                if name == "flat" and plan in ("early_collapse0", "tile_sort0"):
                    assert "union_sum" in prof, (name, K, plan, prof)
                ks, cs, sts = ctx.kmerize(d, K, native.KMERIZE_SUBSAMPLE, p=0.4, seed=3)
                sub = (ks.to_host(), cs.to_host(), _stats(sts))
                if sub_ref is None:
                    sub_ref = sub
                    assert sts.n_canonical == n_can and sts.n_unique < len(want["kmers"])
                assert np.array_equal(sub[0], sub_ref[0]) and np.array_equal(sub[1], sub_ref[1]) and sub[2] == sub_ref[2], (name, K, plan)
                # the counted canonical list itself: every counting route has an exit of its own for it (counted straight into the
                # caller's arrays, or copied out of the aux region or a sort buffer)
                ck, cc, stc = ctx.kmerize(d, K, native.KMERIZE_CANONICAL_ONLY)
                assert np.array_equal(ck.to_host(), can_k) and np.array_equal(cc.to_host(), can_c), (name, K, plan)
                assert stc.n_canonical == stc.n_unique == len(can_k) and list(stc.acgt) == want["acgt"], (name, K, plan)
    finally:
        ctx.tune(**DEFAULTS)
