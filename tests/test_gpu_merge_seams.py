"""The set algebra, the k-way pass and the tile sort on inputs that stand exactly on their seams (tests/_seam_cases.py builds them,
tests/test_seam_cases_host.py shows that they are what they claim to be), bit for bit against the CPU oracle and numpy's sort:

  * setops.hip: an equal pair whose A element ends a tile and whose B element begins the next one (the one-element halos), a tile that
    is all A or all B with the partner in the neighbouring tile, a pair on every thread and wave seam, pairs at both ends, lengths
    around whole tiles -- through zk_union_sum (both count widths), zk_project, zk_split and the tree of two-way passes of zk_merge_n,
    and with the two lists in each other's role;
  * kway.hip: the fullest tile a sampled cut can hand out (1985 - k keys, and 1984 with the splitter k times in the sample), with runs
    of k equal keys all through it, the empty last tile when the sample count is a multiple of T, a tile that belongs to one list,
    a tile of the first and the last list with empty runs between them;
  * tilesort.hip: a block of exactly TS_SLACK keys that ends on a cut (a tile of CAP - 1 keys), one key more (declined: the long way),
    a block that starts on a cut, long blocks and repeated keys inside a tile -- and the route each call took, read from its launches;
    the counting form of the tile sort, which zk_kmerize alone reaches, on the same layouts spelt as reads of one k-mer each.
"""
import numpy as np
import pytest

from oracle import zkoracle as zo
from tests import _seam_cases as S
from tests._knob_cases import DEFAULTS
from zotmer_amd import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def acgt_of(zs, zc):
    return [int(zc[(zs & np.uint64(3)) == np.uint64(b)].sum()) for b in range(4)]


# ---- two lists ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("swap", [False, True], ids=["xy", "yx"])
@pytest.mark.parametrize("name", sorted(S.two_list_layouts()))
def test_two_way_seams(ctx, name, swap):
    x, xc, y, yc, _ = S.build_two_lists(name)
    if swap:          # the halo logic is not symmetric: the pair's first element is now the other list's
        x, xc, y, yc = y, yc, x, xc
    dx, dy = ctx.upload(x), ctx.upload(y)
    zs, zc = zo.union_sum(x, xc, y, yc)
    for cdt in (np.uint64, np.uint32):
        k, c, acgt = ctx.union_sum(dx, ctx.upload(xc.astype(cdt)), dy, ctx.upload(yc.astype(cdt)), want_acgt=True)
        assert c.dtype == cdt and k.n == len(zs), (k.n, len(zs))
        assert np.array_equal(k.to_host(), zs) and np.array_equal(c.to_host().astype(np.uint64), zc)
        assert acgt == acgt_of(zs, zc)
    pk, pc = ctx.project(dx, dy, ctx.upload(yc))          # the reference list as A: B's entries that A has, with B's counts
    ek, ec = zo.project(x, y, yc)
    assert pk.n == len(ek) and np.array_equal(pk.to_host(), ek) and np.array_equal(pc.to_host(), ec)
    assert ctx.split(dx, dy) == zo.split(x, y)
    # three lists through the tree of two-way passes; the third holds the keys x and y share: x and y meet on the seams in the first
    # level (x, y, z), and x + z -- which has x's keys -- meets y on them in the second (x, z, y)
    z, zc3 = S.third_list(x, xc, y, 5)
    try:
        ctx.tune(kway=0)
        for sets in ([(x, xc), (y, yc), (z, zc3)], [(x, xc), (z, zc3), (y, yc)]):
            ws, wc, wacgt = zo.merge_n(25, sets)
            gk, gc, gacgt = ctx.merge_n([(ctx.upload(a), ctx.upload(b)) for a, b in sets])
            assert np.array_equal(gk.to_host(), ws) and np.array_equal(gc.to_host(), wc) and gacgt == wacgt
    finally:
        ctx.tune(kway=DEFAULTS["kway"])


# ---- k lists in one pass --------------------------------------------------------------------------------------------------------------

KWAY_CASES = {v: (lambda k, v=v: S.kway_fullest(k, v, 1)) for v in S.KWAY_FULLEST_VARIANTS}
KWAY_CASES["sample_count_T"] = lambda k: S.kway_sample_multiple(k, 1, 1)
KWAY_CASES["sample_count_2T"] = lambda k: S.kway_sample_multiple(k, 2, 1)
KWAY_CASES["solo"] = lambda k: S.kway_solo(k, 1)
KWAY_CASES["first_and_last"] = lambda k: S.kway_first_and_last(k, 1)


# 2, 4, 5, 8, 9, 16: both ends of the three instantiations (4, 8, 16 lists) -- but two lists are a two-way pass whatever the knob
# says (merge_many), so the smallest k-way pass is three lists
@pytest.mark.parametrize("case", sorted(KWAY_CASES))
@pytest.mark.parametrize("k", [2, 3, 4, 5, 8, 9, 16])
def test_kway_seams(ctx, k, case):
    sets = KWAY_CASES[case](k)
    zs, zc, acgt = zo.merge_n(25, sets)
    keys = [ctx.upload(a) for a, _ in sets]
    try:
        ctx.tune(kway=2)
        for cdt in (np.uint64, np.uint32):
            gk, gc, gacgt = ctx.merge_n([(d, ctx.upload(b.astype(cdt))) for d, (_, b) in zip(keys, sets)])
            assert gc.dtype == cdt and gk.n == len(zs), (gk.n, len(zs))
            assert np.array_equal(gk.to_host(), zs) and np.array_equal(gc.to_host().astype(np.uint64), zc) and gacgt == acgt
    finally:
        ctx.tune(kway=DEFAULTS["kway"])


# ---- the tile sort --------------------------------------------------------------------------------------------------------------------

def launches(ctx, call):
    ctx.profile(True)
    try:
        out = call()
        return out, {tag: rec["launches"] for tag, rec in ctx.profile_read().items()}
    finally:
        ctx.profile(False)


@pytest.fixture(scope="module")
def lsd_passes(ctx):
    """the passes that sort one of these arrays with the tile sort switched off (all 64 bits by LSD passes), keys and pairs: a
    call that kept the tile route launches fewer, a call whose tiles were declined launches these on top of its own"""
    x, _ = S.build_tile_sort("keys", "block_of_S_ends_on_cut")
    v = np.arange(len(x), dtype=np.uint32)
    try:
        ctx.tune(tile_sort=0)
        got, prof_k = launches(ctx, lambda: ctx.sort_keys(ctx.upload(x), 64).to_host())
        assert np.array_equal(got, np.sort(x)) and "tile_sort" not in prof_k
        (dk, dv), prof_p = launches(ctx, lambda: ctx.sort_pairs(ctx.upload(x), ctx.upload(v), 64))
        assert np.array_equal(dk.to_host(), np.sort(x)) and np.array_equal(dv.to_host(), v[np.argsort(x, kind="stable")])
        assert "tile_sort" not in prof_p
        (u, c), prof_c = launches(ctx, lambda: ctx.sort_count(ctx.upload(x), 64))
        wu, wc = np.unique(x, return_counts=True)
        assert np.array_equal(u.to_host(), wu) and np.array_equal(c.to_host(), wc.astype(np.uint32)) and "tile_sort" not in prof_c
    finally:
        ctx.tune(tile_sort=DEFAULTS["tile_sort"])
    assert prof_c["pass_keys"] == prof_k["pass_keys"]
    return dict(keys=prof_k["pass_keys"], pairs=prof_p["pass_pairs"])


def check_route(prof, tag, lsd, flag, what):
    """the tile route was tried once; kept: only the passes over the top bits went before it; declined: those, and then every pass"""
    assert prof.get("tile_sort") == 1, (what, prof)
    assert prof[tag] != lsd and (prof[tag] > lsd) == flag, (what, prof, lsd, flag)


@pytest.mark.parametrize("name", sorted(S.tile_sort_layouts("keys")))
def test_tile_sort_keys_seams(ctx, lsd_passes, name):
    x, spec = S.build_tile_sort("keys", name)
    got, prof = launches(ctx, lambda: ctx.sort_keys(ctx.upload(x), 64).to_host())
    assert np.array_equal(got, np.sort(x))
    check_route(prof, "pass_keys", lsd_passes["keys"], spec["flag"], name)


@pytest.mark.parametrize("name", sorted(S.tile_sort_layouts("pairs")))
def test_tile_sort_pairs_seams(ctx, lsd_passes, name):
    """values = the places the keys came in: equal keys (S copies of one key among them) keep their order of arrival"""
    x, spec = S.build_tile_sort("pairs", name)
    v = np.arange(len(x), dtype=np.uint32)
    (dk, dv), prof = launches(ctx, lambda: ctx.sort_pairs(ctx.upload(x), ctx.upload(v), 64))
    assert np.array_equal(dk.to_host(), np.sort(x)) and np.array_equal(dv.to_host(), v[np.argsort(x, kind="stable")])
    check_route(prof, "pass_pairs", lsd_passes["pairs"], spec["flag"], name)


@pytest.mark.parametrize("name", sorted(S.tile_sort_layouts("keys")))
def test_sort_count_seams(ctx, lsd_passes, name):
    """zk_sort_count is zk_sort_keys and a run-length count: it meets the cuts of the keys form (tile_sort_count_kernel's own cuts are
    reached through zk_kmerize only, whose keys come out of a read stream)"""
    x, spec = S.build_tile_sort("keys", name)
    (u, c), prof = launches(ctx, lambda: ctx.sort_count(ctx.upload(x), 64))
    wu, wc = np.unique(x, return_counts=True)
    assert np.array_equal(u.to_host(), wu) and np.array_equal(c.to_host(), wc.astype(np.uint32))
    if name.startswith("S_identical"):
        assert int(c.to_host().max()) == S.TS_SLACK
    check_route(prof, "pass_keys", lsd_passes["keys"], spec["flag"], name)


@pytest.mark.parametrize("name", sorted(S.tile_sort_layouts("count")))
def test_kmerize_count_form_seams(ctx, name):
    """tile_sort_count_kernel (tiles of CAP 6144, T 5120) stands behind zk_kmerize alone: at K = 31 reads that do not repeat their
    k-mers are counted tile by tile.  The layout arrives as reads of one k-mer each, the smaller strand; the counted canonical list against
    numpy's unique.  Kept: the first pass from the stream and the passes over the top bits only; declined: every bit by passes after
    all, and 62 bits take seven passes or more of digits of up to 9 bits."""
    K = S.COUNT_K
    stream, keys, spec = S.count_form_reads(name)
    wu, wc = np.unique(keys, return_counts=True)
    (k, c, st), prof = launches(ctx, lambda: ctx.kmerize(ctx.upload_stream(stream), K, native.KMERIZE_CANONICAL_ONLY))
    assert st.n_unique == len(wu) and st.n_windows == len(keys), (st.n_unique, len(wu))
    assert np.array_equal(k.to_host(), wu) and np.array_equal(c.to_host(), wc.astype(np.uint32))
    if name.startswith("S_identical"):
        assert int(c.to_host().max()) == S.TS_SLACK
    assert prof.get("tile_sort") == 1, (name, prof)
    assert (prof.get("pass_stream", 0) + prof.get("pass_keys", 0) >= -(-2 * K // 9)) == spec["flag"], (name, prof)
