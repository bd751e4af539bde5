"""
k-mer counts at the edges of every packed count field ("count fields").

zk_kmerize and zk_mirror_expand carry a k-mer and its count as one word, (k-mer << s) | count, wherever the count fits the s spare bits
above the 2K key bits, and several kernels decide on their own whether it does.  Here a count sits at 2^s - 2, 2^s - 1, 2^s and
2^s + 1 for every route that has such a decision (the inputs: tests/_count_edge_cases.py), and every result is compared bit for bit
with the C oracle, whose counts are plain 32-bit integers with no such field: k-mers, counts, acgt, n_unique, and zk_hist of the counts
against the oracle's histogram.  Where a profile record tells which side of an edge a call took, the route is asserted on both sides;
where none does, the test's docstring says so.

The rows of DESIGN.md's table and the tests that sit on their edge (s = 64 - 2K: K = 27: 10 ... 23: 18):
  rle_kernel / rle_fixup_kernel       test_packed_field[K-*-*] with early_collapse = 2: c = 2^s - 1 must stay words, 2^s and 2^s + 1 must
                                      step aside; `strided` deals the copies over the stream, `together` keeps them in one stretch
  collapse_kernel + reduce_by_key     test_packed_field with early_collapse = 3 (and 1 below a megabyte of stream);
                                      test_collapse_cut_every_512_slots[27|26-511 ... 1025]
  c > maxc, dedupe_kernel             test_forced_block_plan[K27-1024-*] (K = 27 has no tags: dedupe_kernel throughout),
                                      [K24-65536-*] and [K24-65535-one_block] (blocks of 2^16 keys and more), dedupe_variant = -1 anywhere
  c > maxc, dedupe2_kernel            test_forced_block_plan[K25-16383|16384-*]: strand_blocks 1 = the unsorted / mirror write-out,
                                      0 and 2 = the sorted one; [K24-65535-apart]: the largest block it takes, at the field's edge
  the `big` side list                 ...-apart: one entry per block; ...-one_block: two from one workgroup
  dedupe_bad_blocks (rle with field)  test_forced_block_plan_dense_block[25|27-2^s - 1|2^s]
  mirror_pack, max_count < 2^s        test_mirror_expand_at_the_field[K-2^s-1|2^s-first|middle|last], route asserted on both sides;
                                      test_packed_field[*-flat], [*-wide] (zk_kmerize and zk_mirror_expand, route asserted)
  the strand route                    test_forced_block_plan[K25-*], [K27-*]: taken at 2^s - 1, not at 2^s, asserted
  16-bit LDS count, dedupe_limit      test_sixteen_bit_lds_count[21|20-65535|65534+1|65536|65536+1]; test_forced_block_plan[K20-*-one_block]
  a palindrome's n + n                test_mirror_expand_palindrome_*; the palindrome target of test_packed_field at even K

Out of scope:
  - more than DEDUPE_BIG_CAP (65 536) k-mers beyond the field at once: that needs tens of millions of reads;
  - a 32-bit count overflowing through zk_kmerize itself: that needs 2^32 windows;
  - the mirror grouped into 2^24 groups: that needs lists of 2^26 entries.
"""
import numpy as np
import pytest

from tests import _count_edge_cases as E
from zotmer_amd import native

pytestmark = pytest.mark.gpu

DEFAULTS = dict(early_collapse=1, packed_pairs=1, dedupe_bits=0, strand_blocks=1, dedupe_variant=0, dedupe_limit=65536,
                tag_words=native.DEFAULT_TAG_WORDS)
EDGE = E.EDGE


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def profiled(ctx, call, knobs):
    """-> (what the call returns, its profile records); every knob back at its default afterwards"""
    ctx.tune(**knobs)
    ctx.profile(True)
    try:
        got = call()
        return got, ctx.profile_read()
    finally:
        ctx.profile(False)
        ctx.tune(**DEFAULTS)


def booked(prof, name):
    return prof.get(name, {}).get("bytes", 0)


def same_table(ctx, k, c, want, what):
    assert np.array_equal(k.to_host(), want["kmers"]), what
    assert np.array_equal(c.to_host(), want["counts"]), what
    assert ctx.hist(c) == want["hist"], what


def kmerize(ctx, d, K, want, flags, out, what, **knobs):
    """zk_kmerize against the oracle's table (CANONICAL_ONLY: only n_canonical; the caller expands the list) -> (k, c, stats, records)"""
    (k, c, st), prof = profiled(ctx, lambda: ctx.kmerize(d, K, flags, out=out), knobs)
    assert list(st.acgt) == want["acgt"], what
    if flags == native.KMERIZE_CANONICAL_ONLY:
        assert st.n_unique == want["n_canonical"] == k.n, what
    else:
        assert st.n_unique == len(want["kmers"]), what
        same_table(ctx, k, c, want, what)
    return k, c, st, prof


def outputs(ctx, want):
    n = len(want["kmers"])          # "a capacity equal to the table's length is enough on every plan"
    return (ctx.empty(n, np.uint64), ctx.empty(n, np.uint32)), (ctx.empty(n, np.uint64), ctx.empty(n, np.uint32))


def words_expected(K, want, packed):
    """the mirror of the counted list travels as words when every canonical count is below 2^s (pipeline.hip: mirror_pack) and the list
    has 2^16 entries (mirror_grouped); None: the list is too short for the records to tell"""
    if want["n_canonical"] < 1 << 16 or 2 * K < 26:
        return None
    return bool(packed) and want["max_canonical"] < 1 << E.pack_bits(K)


def assert_mirror_form(prof, n_can, words, what, always=True):
    """words: the grouping copy books 20 bytes an entry; pairs: it books 24, or the tile sort takes them, and pair passes follow.
    always=False: zk_kmerize may have sorted both strands outright when the sample found no repeats (no "union_sum" record: there
    was no counted list to mirror), which leaves nothing to assert"""
    if words is None or (not always and "union_sum" not in prof):
        return
    assert (booked(prof, "mirror") == 20 * n_can) == words, (what, prof)
    if not words:
        assert "pass_pairs" in prof, (what, prof)


# ---- (a) the packed field, every counting route ----------------------------------------------------------------------------------------

LAYOUTS = E.LAYOUTS


@pytest.mark.parametrize("layout", LAYOUTS, ids=["%s-%s" % l for l in LAYOUTS])
@pytest.mark.parametrize("edge", list(EDGE))
@pytest.mark.parametrize("K", E.PACKED_K)
def test_packed_field(ctx, K, edge, layout):
    """Three target k-mers (four at even K: a palindrome, whose table count is c + c) occur c = 2^s + {-2, -1, 0, 1} times: through the
    block dedupe / tile ranking the input's size chooses (early_collapse 1), collapse_kernel (3), the run-length pass (2: rle_kernel
    saturates and flags a run beyond the field, the pairs take over) and no collapse (0), with and without packed pairs, as
    ZK_KMERIZE_CANONICAL, ZK_KMERIZE_BOTH and ZK_KMERIZE_CANONICAL_ONLY + zk_mirror_expand.
    Route: on the backgrounds with 2^16 distinct canonical k-mers (flat, wide) the mirror must travel as words up to 2^s - 1 and as pairs
    from 2^s on, in zk_kmerize and in zk_mirror_expand.  No record tells whether the sample chose the collapse or which kernel met the
    count first (collapse_kernel and rle_kernel book the same "rle" record as a plain run-length pass): the counting routes are told
    apart by the knob alone."""
    spread, background = layout
    c = (1 << E.pack_bits(K)) + EDGE[edge]
    want = E.edge_want(K, c, spread, background)
    assert want["max_canonical"] == c
    reads, _ = E.edge_reads(K, c, spread, background)
    d = ctx.upload_stream(E.stream_of(reads))
    del reads
    out, out2 = outputs(ctx, want)
    for collapse in (1, 3, 2, 0):
        for packed in (1, 0):
            knobs = dict(early_collapse=collapse, packed_pairs=packed)
            what = (K, c, layout, knobs)
            words = words_expected(K, want, packed)
            _, _, st, prof = kmerize(ctx, d, K, want, native.KMERIZE_CANONICAL, out, what, **knobs)
            assert st.n_canonical == want["n_canonical"], what
            assert_mirror_form(prof, want["n_canonical"], words, what, always=collapse == 0)
            kmerize(ctx, d, K, want, native.KMERIZE_BOTH, out, (what, "both"), **knobs)
            ck, cc, _, _ = kmerize(ctx, d, K, want, native.KMERIZE_CANONICAL_ONLY, out2, (what, "canonical_only"), **knobs)
            assert int(cc.to_host().max()) == c, what
            (ek, ec), prof = profiled(ctx, lambda: ctx.mirror_expand(ck, cc, K, out=out), dict(packed_pairs=packed))
            same_table(ctx, ek, ec, want, (what, "mirror_expand"))
            assert_mirror_form(prof, want["n_canonical"], words, (what, "mirror_expand"))


# ---- (b) the cut every 512 slots -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", E.CUT_C)
@pytest.mark.parametrize("K", E.CUT_K)
def test_collapse_cut_every_512_slots(ctx, K, c):
    """K = 26 and 27 (2^s <= 8192): collapse_kernel cuts a run every 512 slots, and reduce_by_key adds the pieces.  The copies of a
    target lie in one stretch, so one run is cut inside a tile: c = 511, 512, 513 around one cut, 1023, 1024, 1025 around two (at
    K = 27 that is the field's bound as well).  No record distinguishes a cut run from a whole one."""
    want = E.edge_want(K, c, "together", "deep")
    reads, _ = E.edge_reads(K, c, "together", "deep")
    d = ctx.upload_stream(E.stream_of(reads))
    out, out2 = outputs(ctx, want)
    knobs = dict(early_collapse=3, packed_pairs=1)
    what = (K, c)
    kmerize(ctx, d, K, want, native.KMERIZE_CANONICAL, out, what, **knobs)
    ck, cc, _, _ = kmerize(ctx, d, K, want, native.KMERIZE_CANONICAL_ONLY, out2, what, **knobs)
    assert int(cc.to_host().max()) == c
    ek, ec = ctx.mirror_expand(ck, cc, K, out=out)
    same_table(ctx, ek, ec, want, (what, "mirror_expand"))


# ---- (c), (d) the forced block plan --------------------------------------------------------------------------------------------------

def forced_plan(ctx, K, reads, want, expect_fit, what):
    """the plan of a 50 M-read batch (ZK_TUNE_DEDUPE_BITS = 18) with every dedupe kernel (dedupe_variant), tag width (tag_words, K <= 25)
    and, at odd K, every way to the strands (strand_blocks).  Route, odd K: the strand route (strand_blocks.hip books 16 bytes a
    canonical k-mer under "select") is taken exactly when it is switched on and every count fits the field (expect_fit)."""
    d = ctx.upload_stream(E.stream_of(reads))
    out, out2 = outputs(ctx, want)
    n_can = want["n_canonical"]
    for sb in ((1, 4, 0, 2) if K & 1 else (1,)):
        for variant in (0, 2, 1, -1):
            for tw in ((0, 1, 2) if K <= 25 else (native.DEFAULT_TAG_WORDS,)):
                knobs = dict(dedupe_bits=18, strand_blocks=sb, dedupe_variant=variant, tag_words=tw)
                _, _, st, prof = kmerize(ctx, d, K, want, native.KMERIZE_CANONICAL, out, (what, knobs), **knobs)
                assert st.n_canonical == n_can, (what, knobs)
                if K & 1:
                    assert (booked(prof, "select") == 16 * n_can) == (sb != 0 and expect_fit), (what, knobs, prof)
    ck, cc, _, _ = kmerize(ctx, d, K, want, native.KMERIZE_CANONICAL_ONLY, out2, (what, "canonical_only"), dedupe_bits=18)
    assert int(cc.to_host().max()) == want["max_canonical"], what
    ek, ec = ctx.mirror_expand(ck, cc, K, out=out)
    same_table(ctx, ek, ec, want, (what, "mirror_expand"))


@pytest.mark.parametrize("K,c,same_block", E.FORCED, ids=["K%d-%d-%s" % (K, c, "one_block" if sb else "apart") for K, c, sb in E.FORCED])
def test_forced_block_plan(ctx, K, c, same_block):
    """The targets at 2^s - 1 (the word carries the count) and at 2^s (count 0 in the word, the pair in the `big` side list, put back by
    dedupe_big_kernel): every target in a block of its own, or two of them in one block -- two entries of the side list from one
    workgroup.  K = 24: a block of 2^16 - 1 or more keys, beyond dedupe2_kernel's 16-bit counts, goes to dedupe_kernel.  K = 20
    (s = 24, out of reach): 2^15 - 1 and 2^15 instead; two such targets in one block are 65 534 and 65 536 keys, either side of the
    largest block dedupe2_kernel counts.  Route: see forced_plan; at even K no record tells the two sides apart."""
    want = E.edge_want(K, c, "together", "deep", same_block)
    assert want["max_canonical"] == c
    reads, _ = E.edge_reads(K, c, "together", "deep", same_block)
    forced_plan(ctx, K, reads, want, c < 1 << E.pack_bits(K), (K, c, same_block))


@pytest.mark.parametrize("K,c", E.DENSE_CASES)
def test_forced_block_plan_dense_block(ctx, K, c):
    """Two targets at 2^s - 1 or 2^s in a block that also holds 14 000 distinct k-mers, more than any LDS table: the block is counted
    by sorting and a run-length pass with the field (dedupe_bad_blocks), where a count of 2^s - 1 must pass unsaturated and one of
    2^s sends the batch the long way.  Route: see forced_plan."""
    want = E.dense_block_want(K, c)
    assert want["max_canonical"] == c
    forced_plan(ctx, K, E.dense_block_reads(K, c)[0], want, c < 1 << E.pack_bits(K), (K, c, "dense"))


@pytest.mark.parametrize("copies", E.LDS_BLOCKS, ids=["+".join(map(str, b)) for b in E.LDS_BLOCKS])
@pytest.mark.parametrize("K", E.LDS_K)
def test_sixteen_bit_lds_count(ctx, K, copies):
    """dedupe2_kernel counts in 16-bit halves of LDS words and declines blocks of 65 536 keys or more.  One block of the forced plan
    holds exactly 65 535 keys of one k-mer (the largest count a block it takes can reach), 65 534 + 1, 65 536 and 65 536 + 1 keys (both
    declined: dedupe_kernel counts them) beside ordinary reads; the packed field (s = 22, 24) is far away.  Route: the strand route is
    taken at K = 21 whether or not the block is declined; no record tells which kernel counted the block."""
    want = E.block_want(K, copies)
    assert want["max_canonical"] == max(copies)
    reads, _ = E.block_reads(K, list(copies))
    forced_plan(ctx, K, reads, want, True, (K, copies))


# ---- (f) zk_mirror_expand on counted lists ---------------------------------------------------------------------------------------------

def expand(ctx, K, bound, where, palindrome=False):
    """zk_mirror_expand of mirror_lists(...) with and without packed pairs against the numpy table.  Route: words (20 bytes an entry under
    "mirror", "pass_packed" passes, no pair pass) exactly when the largest count of the list is below 2^s; else pairs."""
    c, n, keys, cnt, at = E.mirror_lists(K, bound, where, palindrome)
    assert int(cnt.max()) < 1 << 32
    dc, dn = ctx.upload(c), ctx.upload(n)
    for packed in (1, 0):
        what = (K, bound, where, palindrome, packed)
        (ek, ec), prof = profiled(ctx, lambda: ctx.mirror_expand(dc, dn, K), dict(packed_pairs=packed))
        assert np.array_equal(ek.to_host(), keys), what
        assert np.array_equal(ec.to_host(), cnt.astype(np.uint32)), what
        v, f = np.unique(cnt, return_counts=True)
        assert ctx.hist(ec) == {int(a): int(b) for a, b in zip(v, f)}, what
        words = bool(packed) and bound < 1 << E.pack_bits(K)
        assert (booked(prof, "mirror") == 20 * len(c)) == words, (what, prof)
        assert ("pass_packed" in prof and "pass_pairs" not in prof) == words, (what, prof)
        assert ("pass_pairs" in prof) == (not words), (what, prof)


@pytest.mark.parametrize("where", E.WHERES)
@pytest.mark.parametrize("edge", ["2^s-1", "2^s"])
@pytest.mark.parametrize("K", [25, 27, 24, 16])
def test_mirror_expand_at_the_field(ctx, K, edge, where):
    """the largest count of a list of 70 000 is 2^s - 1 or 2^s (K = 16: s = 31), in the first, middle or last entry"""
    expand(ctx, K, (1 << E.pack_bits(K)) + EDGE[edge], where)


@pytest.mark.parametrize("where", E.WHERES)
@pytest.mark.parametrize("n", [(1 << 15) - 1, 1 << 15, (1 << 16) - 1], ids=["2^15-1", "2^15", "2^16-1"])
def test_mirror_expand_palindrome_doubles_past_the_field(ctx, n, where):
    """K = 24 (s = 16): a palindrome of count n gets n + n = 2^16 - 2, 2^16, 2^17 - 2 in the table, while the packed maximum was taken
    before the doubling: all three travel as words"""
    expand(ctx, 24, n, where, palindrome=True)


def test_mirror_expand_palindrome_fills_u32(ctx):
    """K = 16: a palindrome of count 2^31 - 1 has the table count 2^32 - 2, which fits 32 bits"""
    expand(ctx, 16, (1 << 31) - 1, "middle", palindrome=True)


@pytest.mark.parametrize("packed", [1, 0])
def test_mirror_expand_palindrome_beyond_u32_is_refused(ctx, packed):
    """K = 16: a palindrome of count 2^31 would get 2^32 (the reference's array('I') raises OverflowError).  The call refuses with
    ZK_EOVERFLOW -- it does not hand out the wrapped count 0 as a result -- and the context works afterwards."""
    c, n, keys, cnt, at = E.mirror_lists(16, 1 << 31, "middle", True)
    assert int(cnt.max()) == 1 << 32
    dc, dn = ctx.upload(c), ctx.upload(n)
    try:
        ctx.tune(packed_pairs=packed)
        with pytest.raises(native.ZotkError) as e:
            ctx.mirror_expand(dc, dn, 16)
        assert e.value.code == -5, e.value          # ZK_EOVERFLOW
    finally:
        ctx.tune(**DEFAULTS)
    expand(ctx, 16, (1 << 31) - 1, "middle", palindrome=True)
