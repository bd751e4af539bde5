"""The output-capacity contract of the core entry points (include/zotk.h: "ZK_ENOSPC when the result exceeds cap: nothing is
written at or beyond index cap of any output array, *n_out = the length needed, and the call may be repeated with room").

Every case runs one entry with a capacity `cap` that may be short, exact or ample.  Each output array is allocated with
`needed + 64` entries whatever `cap` is, filled with a guard word, so that even a kernel that ignored `cap` altogether writes inside
the allocation: a wrong kernel fails the guard comparison, it cannot fault the device.  Short: ZK_ENOSPC, the count needed (where
the header promises it), the guard intact from `cap` on, and the same context then gives the oracle's result with room.  Exact or
ample: ZK_OK, the oracle's result bit for bit, the guard intact from `cap` on.  Capacities sit at 0, 1, around the output tile of
the entry's kernel and around the length needed; the inputs make that length about three of the largest tiles plus a few."""
import ctypes as C

import numpy as np
import pytest

from oracle import zkoracle as zo
from tests import _capture_restatement as R
from tests import _spectrum_host as H
from tests._core_cases import (CP_TILE, DEC_TILE, ENC_TILE, GUARD, KW_CAP, MRG_TILE, N, PAD, PS_TILE, RLE_TILE, SEL_TILE, U64, capture_case,
                               codec_case, counted_case, encode_case, guard, hist_case, kmerize_reads, kmerize_want, merge_case, mirror_case,
                               prefix_case, project_case, rle_case, stream_of, subsample_case, union_case)
from zotmer_amd import native

pytestmark = pytest.mark.gpu

OK, ENOSPC = native.ZK_OK, native.ZK_ENOSPC


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def caps_around(needed, *tiles):
    caps = {0, 1, needed - 1, needed, needed + 7}
    for t in tiles:
        caps |= {t - 1, t, t + 1}
    return sorted(c for c in caps if c >= 0)


def check(ctx, call, want, cap, needed=None, count=True, initial=None):
    """One call at capacity `cap`.  call(bufs, cap) -> (return code, count): runs the entry into the guarded device arrays `bufs`
    (one per array of `want`).  needed: the capacity the entry asks for when that is not the length of its result.  count: the
    header promises the count on a refusal.  initial: what the arrays hold before the call when that is not the guard (in-place
    forms), at least needed + PAD entries each.  -> whether the call had room"""
    want = [np.ascontiguousarray(w) for w in want]
    n_res = len(want[0])
    needed = n_res if needed is None else needed
    start = initial if initial is not None else [guard(needed + PAD, w.dtype) for w in want]
    assert all(len(s) >= needed + PAD for s in start) and cap <= needed + PAD          # the arrays hold more than any capacity used
    bufs = [ctx.upload(s) for s in start]
    rc, n = call(bufs, cap)
    got = [b.to_host() for b in bufs]
    for i, (g, s) in enumerate(zip(got, start)):
        assert np.array_equal(g[cap:], s[cap:]), "array %d written at or beyond the capacity %d (needed %d)" % (i, cap, needed)
    if cap < needed:
        assert rc == ENOSPC, (rc, cap, needed)
        if count:
            assert n == needed, (n, cap, needed)
        return False
    assert rc == OK, (rc, cap, needed, ctx.lib.zk_last_error(ctx.h))
    assert n == n_res, (n, n_res, cap)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g[:n_res], w), "array %d differs from the oracle at capacity %d" % (i, cap)
    return True


def sweep(ctx, call, want, caps, needed=None, **kw):
    """every capacity of `caps`; after each refusal the same context runs the same call with room"""
    room = (len(want[0]) if needed is None else needed) + 7
    for cap in caps:
        if not check(ctx, call, want, cap, needed=needed, **kw):
            assert check(ctx, call, want, room, needed=needed, **kw)


# ---- the selections and the list form of the encoder (select.hip) ---------------------------------------------------------------

def n_out_call(ctx, fn, before, after=()):
    """call(bufs, cap) for an entry whose arguments are: `before`, the output arrays, cap, &n_out, `after`"""
    def call(bufs, cap):
        n = C.c_uint64(0)
        rc = fn(ctx.h, *before, *[b.ptr for b in bufs], cap, C.byref(n), *after)
        return rc, n.value
    return call


@pytest.mark.parametrize("both", [0, 1])
def test_encode(ctx, both):
    stream, one, two = encode_case()
    want = two if both else one
    d = ctx.upload_stream(stream)
    acgt = (C.c_uint64 * 4)()
    sweep(ctx, n_out_call(ctx, ctx.lib.zk_encode, (d.ptr, d.n, 25, both), (acgt,)), [want],
          caps_around(len(want), SEL_TILE, 2 * SEL_TILE))
    assert list(acgt) == [int(np.sum((want & U64(3)) == U64(b))) for b in range(4)]


def test_subsample(ctx):
    kmers, want = subsample_case()
    d = ctx.upload(kmers)
    sweep(ctx, n_out_call(ctx, ctx.lib.zk_subsample, (d.ptr, d.n, 5, 4.2)), [want], caps_around(len(want), SEL_TILE // 2, SEL_TILE))


@pytest.mark.parametrize("in_place", [False, True])
def test_rle(ctx, in_place):
    keys, vals, cnt = rle_case()
    caps = caps_around(N, RLE_TILE, 5000, 5001)          # (5000: the run that crosses two tile edges is the first entry cut off)
    if not in_place:
        d = ctx.upload(keys)
        sweep(ctx, n_out_call(ctx, ctx.lib.zk_rle, (d.ptr, d.n)), [vals, cnt], caps)
        return
    # d_uniq == d_sorted: from cap on the array still holds its input
    start = [np.concatenate([keys, guard(PAD, U64)]), guard(N + PAD, np.uint32)]

    def call(bufs, cap):
        n = C.c_uint64(0)
        rc = ctx.lib.zk_rle(ctx.h, bufs[0].ptr, len(keys), bufs[0].ptr, bufs[1].ptr, cap, C.byref(n))
        return rc, n.value
    sweep(ctx, call, [vals, cnt], caps, initial=start)


def test_sort_count(ctx):
    keys, vals, cnt = rle_case()
    shuffled = np.random.default_rng(48).permutation(keys)

    def call(bufs, cap):
        d = ctx.upload(shuffled)          # (the sort destroys its input)
        n = C.c_uint64(0)
        rc = ctx.lib.zk_sort_count(ctx.h, d.ptr, d.n, 40, bufs[0].ptr, bufs[1].ptr, cap, C.byref(n))
        return rc, n.value
    sweep(ctx, call, [vals, cnt], caps_around(N, RLE_TILE))


@pytest.mark.parametrize("cdt", [np.uint32, np.uint64])
def test_trim(ctx, cdt):
    k, c = counted_case()
    ek, ec = zo.trim(k, c, 3, 7)
    assert len(ek) >= 3 * RLE_TILE
    dk, dc = ctx.upload(k), ctx.upload(c.astype(cdt))
    sweep(ctx, n_out_call(ctx, ctx.lib.zk_trim, (dk.ptr, dc.ptr, 8 * np.dtype(cdt).itemsize, dk.n, 3, 7)), [ek, ec.astype(cdt)],
          caps_around(len(ek), SEL_TILE // 2, SEL_TILE))


def test_sample(ctx):
    k, c = counted_case()
    ek, ec = zo.sample_d(0.5, 11, k, c)
    assert len(ek) >= 3 * RLE_TILE
    dk, dc = ctx.upload(k), ctx.upload(c)
    sweep(ctx, n_out_call(ctx, ctx.lib.zk_sample, (dk.ptr, dc.ptr, dk.n, 11, 0.5)), [ek, ec], caps_around(len(ek), SEL_TILE // 2, SEL_TILE))


@pytest.mark.parametrize("shift", [0, 20])
def test_project_dedupe(ctx, shift):
    k, _ = prefix_case()
    want = zo.project_dedupe(k, shift)
    assert len(want) == (N if shift else len(k))
    d = ctx.upload(k)
    sweep(ctx, n_out_call(ctx, ctx.lib.zk_project_dedupe, (d.ptr, d.n, shift)), [want], caps_around(len(want), SEL_TILE // 2, SEL_TILE))


# ---- merge-path union, projection, the k-way pass (setops.hip, kway.hip, pipeline.hip::merge_many) ----------------------------------

def refused_count(fn, *args):
    """the count a refused call leaves, for the entries reached through a wrapper that raises before it returns one"""
    n = C.c_uint64(0)
    rc = fn(*args, C.byref(n), None)
    return rc, n.value


@pytest.mark.parametrize("acgt", [False, True])
@pytest.mark.parametrize("cdt", [np.uint32, np.uint64])
def test_union_sum(ctx, cdt, acgt):
    x, xc, y, yc, zs, zc = union_case()
    xk, yk = ctx.upload(x), ctx.upload(y)
    dxc, dyc = ctx.upload(xc.astype(cdt)), ctx.upload(yc.astype(cdt))
    want_acgt = [int(zc[(zs & U64(3)) == U64(b)].sum()) for b in range(4)]

    def call(bufs, cap):
        try:
            r = ctx.union_sum(xk, dxc, yk, dyc, want_acgt=acgt, out=(bufs[0].view(cap), bufs[1].view(cap)))
        except native.ZotkError as e:
            assert e.code == ENOSPC
            return refused_count(ctx.lib.zk_union_sum, ctx.h, xk.ptr, dxc.ptr, xk.n, yk.ptr, dyc.ptr, yk.n, bufs[0].ptr, bufs[1].ptr,
                                 8 * np.dtype(cdt).itemsize, cap)
        assert not acgt or r[2] == want_acgt
        return OK, r[0].n
    sweep(ctx, call, [zs, zc.astype(cdt)], caps_around(N, MRG_TILE))


def test_project(ctx):
    ref, k, c, ek, ec = project_case()
    dr, dk, dc = ctx.upload(ref), ctx.upload(k), ctx.upload(c)
    sweep(ctx, n_out_call(ctx, ctx.lib.zk_project, (dr.ptr, dr.n, dk.ptr, dc.ptr, dk.n)), [ek, ec], caps_around(N, MRG_TILE // 2, MRG_TILE))


@pytest.mark.parametrize("k,kway", [(1, 1), (2, 1), (3, 0), (5, 2), (17, 2), (33, 2)])
def test_merge_n(ctx, k, kway):
    """k = 1: the copy; 2: one merge-path pass; 3 with the tree: a list sits out the first level; 5, 17 and 33 with the k-way pass
    forced: one k-way level, a k-way level under a 2-way pass, and two k-way levels.  Only the last level's pass sees the
    caller's capacity."""
    sets, zs, zc, acgt = merge_case(k)
    dev = [(ctx.upload(a), ctx.upload(b)) for a, b in sets]
    pk = (C.c_void_p * k)(*[s[0].ptr for s in dev])
    pc = (C.c_void_p * k)(*[s[1].ptr for s in dev])
    ns = (C.c_uint64 * k)(*[s[0].n for s in dev])

    def call(bufs, cap):
        try:
            gk, _, gacgt = ctx.merge_n(dev, out=(bufs[0].view(cap), bufs[1].view(cap)))
        except native.ZotkError as e:
            assert e.code == ENOSPC
            return refused_count(ctx.lib.zk_merge_n, ctx.h, k, pk, pc, ns, bufs[0].ptr, bufs[1].ptr, 64, cap)
        assert gacgt == acgt
        return OK, gk.n
    try:
        ctx.tune(kway=kway)
        sweep(ctx, call, [zs, zc], caps_around(N, MRG_TILE if kway != 2 else KW_CAP))
    finally:
        ctx.tune(kway=1)


@pytest.mark.parametrize("K", [25, 24])
def test_mirror_expand(ctx, K):
    """odd K: the two strands share no key, a tile's place in the union is its place in the merge (`disjoint`); even K: the
    palindromes of the list meet themselves, the table is shorter than 2 n"""
    c, n, keys, cnt, pal = mirror_case(K)
    assert pal == (0 if K & 1 else 200)
    dc, dn = ctx.upload(c), ctx.upload(n)
    sweep(ctx, n_out_call(ctx, ctx.lib.zk_mirror_expand, (dc.ptr, dn.ptr, dc.n, K)), [keys, cnt], caps_around(len(keys), MRG_TILE))


# ---- zk_project_sum (spectrum.hip) ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cdt", [np.uint32, np.uint64])
@pytest.mark.parametrize("shift", [0, 20])
def test_project_sum(ctx, shift, cdt):
    k, c = prefix_case()
    wk, ws, wt = H.host_project_sum(k, c.astype(cdt), shift)
    assert len(wk) == (N if shift else len(k))
    dk, dc = ctx.upload(k), ctx.upload(c.astype(cdt))
    total = C.c_uint64(0)
    sweep(ctx, n_out_call(ctx, ctx.lib.zk_project_sum, (dk.ptr, dc.ptr, 8 * np.dtype(cdt).itemsize, dk.n, shift), (C.byref(total),)),
          [np.asarray(wk, dtype=U64), np.asarray(ws, dtype=U64)], caps_around(len(wk), PS_TILE))
    assert total.value == int(wt)          # (the last call of the sweep had room; after a refusal *total is unspecified)


# ---- the device codec (codec.hip) -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["u64", "u32", "delta"])
def test_codec_encode(ctx, form):
    v, w, v32, w32, k, wk = codec_case()
    if form == "u32":
        d = ctx.upload(v32)
        call, want = n_out_call(ctx, ctx.lib.zk_codec64_encode_u32_dev, (d.ptr, d.n)), w32
    else:
        d = ctx.upload(k if form == "delta" else v)
        call, want = n_out_call(ctx, ctx.lib.zk_codec64_encode_dev, (d.ptr, d.n, int(form == "delta"))), (wk if form == "delta" else w)
    assert len(want) >= 3 * RLE_TILE
    sweep(ctx, call, [want], caps_around(len(want), ENC_TILE // 4, ENC_TILE))


@pytest.mark.parametrize("delta", [0, 1])
def test_codec_decode(ctx, delta):
    """delta = 1: the undelta scan runs over the decoded values in place; refused, it must not run at all (it would walk n > cap
    values: the guard behind cap is what shows that it did not)"""
    v, w, _, _, k, wk = codec_case()
    d = ctx.upload(wk if delta else w)
    want = k if delta else v
    sweep(ctx, n_out_call(ctx, ctx.lib.zk_codec64_decode_dev, (d.ptr, d.n, delta)), [want], caps_around(len(want), DEC_TILE, 3 * DEC_TILE))


# ---- zk_hist: host arrays, the first cap_bins bins are written --------------------------------------------------------------------

@pytest.mark.parametrize("cdt", [np.uint32, np.uint64])
def test_hist(ctx, cdt):
    counts = hist_case()
    wv, wf = zo.hist(counts)
    needed = len(wv)
    assert needed == 300 and int(np.count_nonzero(wv >= 4096)) == 4
    d = ctx.upload(counts.astype(cdt))
    u64p = C.POINTER(C.c_uint64)
    for cap in (0, 1, needed - 1, needed, needed + 7, needed - 4, 2):
        vals, freq = guard(needed + PAD, U64), guard(needed + PAD, U64)
        n = C.c_uint64(0)
        rc = ctx.lib.zk_hist(ctx.h, d.ptr, 8 * np.dtype(cdt).itemsize, d.n, vals.ctypes.data_as(u64p), freq.ctypes.data_as(u64p), cap, C.byref(n))
        assert np.all(vals[cap:] == U64(GUARD)) and np.all(freq[cap:] == U64(GUARD)), cap
        assert rc == (ENOSPC if cap < needed else OK) and n.value == needed, (rc, n.value, cap)
        m = min(cap, needed)
        assert np.array_equal(vals[:m], wv[:m]) and np.array_equal(freq[:m], wf[:m]), cap
    assert ctx.hist(d) == {int(a): int(b) for a, b in zip(wv, wf)}


# ---- the text kernels of `zot capture` (capture.hip) ------------------------------------------------------------------------------

def test_line_ends(ctx):
    text = capture_case()[0]
    want = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10).astype(U64)
    assert len(want) == 1600
    d = ctx.upload_stream(text)
    sweep(ctx, n_out_call(ctx, ctx.lib.zk_line_ends, (d.ptr, d.n)), [want], caps_around(len(want), 4, 400))


def test_capture_hits(ctx):
    """the capacity is that of the (bait, read) pairs BEFORE deduplication (one per bait and chunk of 64 windows), which is also
    the count a refusal returns; the result is the distinct pairs"""
    text, baits, pairs, raw, _, n_hit = capture_case()
    assert raw > len(pairs) and 100 <= n_hit <= 300
    d = ctx.upload_stream(text)
    lines = ctx.line_ends(d)
    table = ctx.bait_table(ctx.upload_stream(stream_of(baits)), R.READ_K)

    def call(bufs, cap):
        n = C.c_uint64(0)
        rc = ctx.lib.zk_capture_hits(ctx.h, table.h, None, R.READ_K, d.ptr, lines.ptr, None, None, 400, bufs[0].ptr, cap, C.byref(n))
        return rc, n.value
    sweep(ctx, call, [pairs], caps_around(raw, len(pairs) - 1, len(pairs)), needed=raw)


def test_capture_gather(ctx):
    """the capacity is in bytes"""
    text, baits, pairs, _, gathered, _ = capture_case()
    want = np.frombuffer(gathered, dtype=np.uint8)
    d = ctx.upload_stream(text)
    lines = ctx.line_ends(d)
    dp = ctx.upload(pairs)
    spans = np.zeros(2 * (len(baits) + 1), dtype=U64)

    def call(bufs, cap):
        n = C.c_uint64(0)
        rc = ctx.lib.zk_capture_gather(ctx.h, dp.ptr, dp.n, len(baits), d.ptr, lines.ptr, lines.n, bufs[0].ptr, cap,
                                       spans.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n))
        return rc, n.value
    first_record = gathered.index(b"\n@") + 1          # a capacity that ends with a record
    sweep(ctx, call, [want], caps_around(len(want), first_record, CP_TILE))
    bait_of = (pairs >> U64(32)).astype(np.int64)
    assert [int(v) for v in spans[:len(baits) + 1]] == [int(np.searchsorted(bait_of, b)) for b in range(len(baits) + 1)]
    assert int(spans[-1]) == len(want)


# ---- zk_kmerize: the flags, the inputs and every route that hands the caller's arrays on (pipeline.hip) ---------------------------

FLAGS = {"canonical": native.KMERIZE_CANONICAL, "both": native.KMERIZE_BOTH, "canonical_only": native.KMERIZE_CANONICAL_ONLY,
         "subsample": native.KMERIZE_CANONICAL | native.KMERIZE_SUBSAMPLE}
DEFAULT_KNOBS = dict(short_sort=0, side_div=8, early_collapse=1, tile_sort=1, dedupe_bits=0, tag_words=native.DEFAULT_TAG_WORDS)

KMERIZE_CASES = []
for _inp in ("deep", "flat"):
    KMERIZE_CASES += [(_inp, 25, f, {}) for f in ("canonical", "both", "canonical_only", "subsample")]
    KMERIZE_CASES += [(_inp, 24, f, {}) for f in ("canonical", "both", "canonical_only")]          # even K: palindromes
    KMERIZE_CASES += [(_inp, 25, "canonical", dict(short_sort=1))]
KMERIZE_CASES += [("deep", 24, "canonical", dict(short_sort=1))]
# the early collapse: off, in the tile-local ranking, as a pass of its own (1, as early as possible, is the default above)
KMERIZE_CASES += [("deep", 25, f, dict(early_collapse=e)) for e in (0, 2, 3) for f in ("canonical", "canonical_only")]
KMERIZE_CASES += [("flat", 25, "canonical", dict(early_collapse=0))]
# reads that do not repeat: the tile sort (the default above) and the passes over every bit
KMERIZE_CASES += [("flat", 25, f, dict(tile_sort=0)) for f in ("canonical", "canonical_only")]
# ... at K = 25 both come to the same passes on an input of this size; the tile sort counts straight into the caller's arrays at K >= 28,
# where a look before the sort finds that the reads do not repeat (K = 31: tile_sort_count with the canonical list alone, else the
# mirrored pairs are tile-sorted before the union)
KMERIZE_CASES += [("flat", 31, f, dict(tile_sort=t)) for t in (1, 0) for f in ("canonical", "canonical_only")]
# the block dedupe forced: at odd K the strands are rebuilt block by block (strand_blocks), else by the union of two packed lists
KMERIZE_CASES += [("deep", K, f, dict(dedupe_bits=18, tag_words=t)) for t in (1, 0) for K, f in ((25, "canonical"), (25, "canonical_only"), (24, "canonical"))]


def kmerize_id(case):
    inp, K, flags, knobs = case
    return "-".join([inp, "K%d" % K, flags] + ["%s%d" % kv for kv in sorted(knobs.items())])


@pytest.mark.parametrize("case", KMERIZE_CASES, ids=kmerize_id)
def test_kmerize(ctx, case):
    """one place short, exact, and a capacity inside the first output tile.  After a refusal the stats are unspecified (the header
    promises no count), so only the return code and the guard are asserted there."""
    inp, K, flags, knobs = case
    wk, wc, needed = kmerize_want(inp, K, flags)
    assert needed >= 3 * RLE_TILE
    d = ctx.upload_stream(stream_of(kmerize_reads(inp)))

    def call(bufs, cap):
        try:
            k, _, st = ctx.kmerize(d, K, FLAGS[flags], 0.5, 3, out=(bufs[0].view(cap), bufs[1].view(cap)))
        except native.ZotkError as e:
            return e.code, None
        return OK, k.n
    try:
        ctx.tune(**knobs)
        sweep(ctx, call, [wk, wc], [needed - 1, needed, 1000], needed=needed, count=False)
    finally:
        ctx.tune(**DEFAULT_KNOBS)
