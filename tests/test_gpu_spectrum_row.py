"""
zk_spectrum_sums_row on the GPU: one spectrum against m others in one call.  Every pair of a row is compared with the host
statement (tests/_spectrum_host.py: Python integers, math.fsum) and with zk_spectrum_sums on the same pair: the integers equal,
the two doubles within (n_shared + 8) * 2**-52 * sum |term| -- what two summation orders of the same n_shared terms can differ by
(the form of tests/golden/make_golden_dist_spectrum.py); for S_js the sum of |term|, its terms have both signs.
"""
import math
import struct

import numpy as np
import pytest

from tests import _spectrum_host as H
from zotmer_amd import native

pytestmark = pytest.mark.gpu

TILE = 4096                # csrc/spectrum.hip: SP_TILE, the merged entries of a tile
ITEMS = 8                  # ... SP_ITEMS, the merged entries of a thread
GROUP = 4                  # ... SPR_GROUP_MIN, the tiles a workgroup takes of a pair of up to GROUPS_MAX * GROUP tiles
GROUPS_MAX = 2048          # ... SPR_GROUPS_MAX
INTS = ("n_shared", "S_min", "X_shared", "Y_shared", "S_xy")
ZERO = [0, 0, 0, 0, 0, 0.0, 0.0]


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def bits(d):
    return struct.pack("<dd", d["S_sqrt"], d["S_js"])


def spectrum(rng, pool, n, hi=2000, lo=1):
    k = np.sort(rng.choice(pool, n, replace=False)) if n else pool[:0]
    return k.astype(np.uint64), rng.integers(lo, hi, size=n, dtype=np.uint64)


def check_pair(got, want, pair=None):
    for f in INTS + ("cx", "cy"):
        assert got[f] == want[f], (f, got[f], want[f])
    eps = (want["n_shared"] + 8) * 2.0 ** -52
    print("n_shared %d S_sqrt %.17g (want %.17g, tol %.3g) S_js %.17g (want %.17g, tol %.3g)" % (
        want["n_shared"], got["S_sqrt"], want["S_sqrt"], eps * want["sqrt_abs"], got["S_js"], want["S_js"], eps * want["js_abs"]))
    assert abs(got["S_sqrt"] - want["S_sqrt"]) <= eps * want["sqrt_abs"]
    assert abs(got["S_js"] - want["S_js"]) <= eps * want["js_abs"]
    if pair is not None:
        for f in INTS:
            assert got[f] == pair[f], (f, got[f], pair[f])
        assert abs(got["S_sqrt"] - pair["S_sqrt"]) <= eps * want["sqrt_abs"]
        assert abs(got["S_js"] - pair["S_js"]) <= eps * want["js_abs"]


def check_row(ctx, x, ys, dev=None):
    """x = (keys, sums), ys = [(keys, sums)] as numpy arrays; dev = their device arrays when the caller placed them itself"""
    want = [H.host_spectrum_sums(x[0], x[1], yk, ys_) for yk, ys_ in ys]
    cx = sum(int(v) for v in x[1])
    if dev is None:
        dev = (ctx.upload(x[0]), ctx.upload(x[1])), [(ctx.upload(k), ctx.upload(s)) for k, s in ys]
    (dxk, dxs), dys = dev
    row = [(k, s, w["cy"]) for (k, s), w in zip(dys, want)]
    got = ctx.spectrum_sums_row((dxk, dxs, cx), row)
    assert len(got) == len(ys)
    for g, w, (k, s, cy) in zip(got, want, row):
        check_pair(g, w, ctx.spectrum_sums(dxk, dxs, cx, k, s, cy))
    again = ctx.spectrum_sums_row((dxk, dxs, cx), row)
    assert [bits(a) for a in again] == [bits(g) for g in got] and again == got
    return got


def test_row_against_host_and_pairs(ctx):
    """a row of eight spectra of different lengths, sums with zeros in them (absent k-mers), one list empty between the others"""
    rng = np.random.default_rng(3100)
    pool = np.unique(rng.integers(0, 1 << 30, size=40000, dtype=np.uint64))
    x = spectrum(rng, pool, 9000, hi=40, lo=0)
    ys = [spectrum(rng, pool, n, hi=40, lo=0) for n in (5000, 1, 0, 20000, 7, 12000, 0, 3000)]
    got = check_row(ctx, x, ys)
    assert [got[2][f] for f in INTS + ("S_sqrt", "S_js")] == ZERO and got[3]["n_shared"] > 1000
    zeros = H.host_spectrum_sums(x[0], x[1], *ys[0])
    both = len(np.intersect1d(x[0], ys[0][0]))
    assert zeros["n_shared"] < both          # keys in both lists with a zero sum are not shared


@pytest.mark.parametrize("nx", [1, 2000])
def test_row_merged_lengths(ctx, nx):
    """merged lengths 1, a tile less one, a tile, a tile and one, two tiles and one, in one row"""
    rng = np.random.default_rng(3200 + nx)
    pool = np.arange(3 * TILE, dtype=np.uint64) * np.uint64(3) + np.uint64(1)
    x = spectrum(rng, pool, nx)
    ys = [spectrum(rng, pool, total - nx) for total in (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1) if total - nx >= 0]
    got = check_row(ctx, x, ys)
    if nx == 1:
        assert [got[0][f] for f in INTS + ("S_sqrt", "S_js")] == ZERO          # merged length 1: y is empty


@pytest.mark.parametrize("tiles", [1, 2, GROUP, GROUP + 1, 2 * GROUP, 2 * GROUP + 1])
def test_row_equal_pairs_across_every_border(ctx, tiles):
    """x = one key of its own, then the keys of y: the merged order is x0, (x1 y0), (x2 y1), ..., every equal pair at an odd
    position and the next even one, so one lies across every thread seam (multiples of ITEMS) and every tile border; tile counts on
    both sides of the group a workgroup takes, with a last tile of one entry and a full one"""
    rng = np.random.default_rng(3300 + tiles)
    assert ITEMS % 2 == 0 and TILE % ITEMS == 0
    for total in (tiles * TILE, (tiles - 1) * TILE + 1, (tiles - 1) * TILE + 3):
        ny = (total - 1) // 2
        if ny < 1:
            continue
        yk = np.arange(ny, dtype=np.uint64) * np.uint64(7) + np.uint64(10)
        xk = np.concatenate([np.array([2], dtype=np.uint64), yk])
        if 1 + 2 * ny < total:          # an even total: one more key of x alone at the end
            xk = np.concatenate([xk, yk[-1:] + np.uint64(1)])
        assert len(xk) + ny == total
        x = xk, rng.integers(1, 5000, size=len(xk), dtype=np.uint64)
        y = yk, rng.integers(1, 5000, size=ny, dtype=np.uint64)
        got = check_row(ctx, x, [y])
        assert got[0]["n_shared"] == ny


@pytest.mark.parametrize("m", [1, 2, 64, 65])
def test_row_lengths_of_the_row(ctx, m):
    rng = np.random.default_rng(3400 + m)
    pool = np.unique(rng.integers(0, 1 << 20, size=6000, dtype=np.uint64))
    assert len(pool) > TILE
    x = spectrum(rng, pool, 600)
    ys = [spectrum(rng, pool, int(n)) for n in rng.integers(0, 900, size=m)]
    ys[m // 2] = spectrum(rng, pool, TILE + 5 - 600 if m > 1 else 300)
    check_row(ctx, x, ys)


def test_row_longer_than_the_bound(ctx):
    """the bound and one more pair through the binding (it cuts the row); the entry itself refuses"""
    import ctypes as C
    m = native.Context.SPECTRUM_ROW_MAX + 1
    assert m == 4097
    rng = np.random.default_rng(3500)
    pool = np.arange(64, dtype=np.uint64) * np.uint64(5)
    x = spectrum(rng, pool, 40)
    big_k = np.sort(rng.choice(pool, 48, replace=False)).astype(np.uint64)
    big_s = rng.integers(1, 99, size=48 + m, dtype=np.uint64)
    # y_j = 3 + j % 5 keys from offset j % 40 of one sorted array, sums from offset j of another
    ys = [(big_k[j % 40: j % 40 + 3 + j % 5], big_s[j: j + 3 + j % 5]) for j in range(m)]
    dk, ds = ctx.upload(big_k), ctx.upload(big_s)
    dev = (ctx.upload(x[0]), ctx.upload(x[1])), [(dk.view(3 + j % 5, j % 40), ds.view(3 + j % 5, j)) for j in range(m)]
    got = check_row(ctx, x, ys, dev=dev)
    assert len(got) == m and got[-1]["cy"] == int(ys[-1][1].sum())
    p = (C.c_void_p * m)(*[dk.ptr] * m)
    n = (C.c_uint64 * m)(*[3] * m)
    cy = (C.c_double * m)(*[1.0] * m)
    res = (native.Spectrum * m)()
    rc = ctx.lib.zk_spectrum_sums_row(ctx.h, dk.ptr, ds.ptr, 3, 1.0, m, p, p, n, cy, res)
    assert rc == native.ZK_EINVAL
    assert ctx.lib.zk_spectrum_sums_row(ctx.h, dk.ptr, ds.ptr, 3, 1.0, 0, None, None, None, None, None) == native.ZK_OK          # m = 0


def test_row_empty_x_and_one_array_for_every_y(ctx):
    rng = np.random.default_rng(3600)
    pool = np.unique(rng.integers(0, 1 << 24, size=12000, dtype=np.uint64))
    e = np.zeros(0, dtype=np.uint64)
    y = spectrum(rng, pool, 5000)
    got = check_row(ctx, (e, e), [y, (e, e), y])
    assert all([g[f] for f in INTS + ("S_sqrt", "S_js")] == ZERO for g in got)
    x = spectrum(rng, pool, 6000)
    dy = ctx.upload(y[0]), ctx.upload(y[1])
    got = check_row(ctx, x, [y] * 9, dev=((ctx.upload(x[0]), ctx.upload(x[1])), [dy] * 9))
    assert got[0]["n_shared"] > 0 and all(g == got[0] and bits(g) == bits(got[0]) for g in got)
    got = check_row(ctx, x, [x])          # x against itself, the same device arrays on both sides
    assert got[0]["n_shared"] == 6000 and got[0]["S_js"] == 0.0 and got[0]["S_min"] == got[0]["cx"]


def test_row_products_beyond_64_bits(ctx):
    """S_xy needs its high word: sums of 2^40 (their products 2^80), and three pairs of 2^62"""
    rng = np.random.default_rng(3700)
    k = np.unique(rng.integers(0, 1 << 34, size=9000, dtype=np.uint64))[:8000]
    xs = rng.integers(1 << 40, 1 << 41, size=len(k), dtype=np.uint64)
    ys = rng.integers(1 << 40, 1 << 41, size=len(k), dtype=np.uint64)
    big = np.full(3, 1 << 62, dtype=np.uint64)
    got = check_row(ctx, (k, xs), [(k[5:], ys[5:]), (k[:3], big)])
    assert got[0]["S_xy"] > 1 << 64
    got = check_row(ctx, (k[:3], big), [(k[:3], big)])
    assert got[0]["S_xy"] == 3 << 124


def test_row_same_pair_same_bits_in_any_row(ctx):
    """a pair of 2 * GROUP + 1 tiles (three workgroups' slots) first in a row of two, last in a row of forty and alone"""
    rng = np.random.default_rng(3800)
    pool = np.unique(rng.integers(0, 1 << 26, size=60000, dtype=np.uint64))
    x = spectrum(rng, pool, 20000)
    y = spectrum(rng, pool, (2 * GROUP + 1) * TILE - 20000 - 100)
    others = [spectrum(rng, pool, int(n)) for n in rng.integers(0, 30000, size=39)]
    cx = int(x[1].sum())
    dx = ctx.upload(x[0]), ctx.upload(x[1]), cx
    up = lambda s: (ctx.upload(s[0]), ctx.upload(s[1]), int(s[1].sum()))          # noqa: E731
    dy, do = up(y), [up(o) for o in others]
    alone = ctx.spectrum_sums_row(dx, [dy])[0]
    check_pair(alone, H.host_spectrum_sums(x[0], x[1], y[0], y[1]))
    assert alone["n_shared"] > 1000 and alone["S_js"] != 0.0
    first = ctx.spectrum_sums_row(dx, [dy, do[0]])[0]
    last = ctx.spectrum_sums_row(dx, do + [dy])[-1]
    twice = ctx.spectrum_sums_row(dx, [dy, do[3], dy])
    ctx.release_workspace()          # ... and on a workspace the call has to make
    fresh = ctx.spectrum_sums_row(dx, [do[1], dy])[1]
    for g in (first, last, twice[0], twice[2], fresh):
        assert g == alone and bits(g) == bits(alone)


def test_row_views_of_guarded_arrays(ctx):
    """x and every y are views at odd element offsets of larger arrays whose other entries would change every sum if read: keys
    equal to a key of the other side under sums of 2^50"""
    rng = np.random.default_rng(3900)
    pool = np.unique(rng.integers(1 << 8, 1 << 22, size=20000, dtype=np.uint64))
    assert len(pool) > 3 * TILE
    x = spectrum(rng, pool, TILE + 77)
    ys = [spectrum(rng, pool, n) for n in (TILE - 77, 901, 3 * TILE)]

    def guarded(k, s, other, off):
        """[off guards][the list][off guards]: guard keys taken from the other side, below and above the list's own"""
        gk = np.concatenate([other[:off], k, other[-off:]])
        gs = np.concatenate([np.full(off, 1 << 50, dtype=np.uint64), s, np.full(off, 1 << 50, dtype=np.uint64)])
        return ctx.upload(gk).view(len(k), off), ctx.upload(gs).view(len(s), off)

    dev = guarded(x[0], x[1], ys[2][0], 3), [guarded(k, s, x[0], 1 + 2 * i) for i, (k, s) in enumerate(ys)]
    check_row(ctx, x, ys, dev=dev)


def test_row_group_size_above_the_shortest(ctx):
    """more than GROUPS_MAX * GROUP tiles: a workgroup takes five tiles of the pair.  x against itself, so the host side is closed
    forms: every key shared, S_sqrt = sum of sqrt(s * s) = the sum of s (every term and every partial sum an integer below 2^53:
    exact in any order), every Jensen-Shannon term x/cx * log(1) = 0"""
    n = (GROUPS_MAX * GROUP * TILE) // 2 + 3 * TILE
    k = np.arange(n, dtype=np.uint64) * np.uint64(3)
    s = (np.arange(n, dtype=np.uint64) % np.uint64(13)) + np.uint64(1)
    total = int(s.sum())
    dk, ds = ctx.upload(k), ctx.upload(s)
    got = ctx.spectrum_sums_row((dk, ds, total), [(dk, ds, total), (dk.view(5, 1), ds.view(5, 1), 9)])
    pair = ctx.spectrum_sums(dk, ds, total, dk, ds, total)
    sq = sum(int(v) * int(v) * int(c) for v, c in zip(*np.unique(s, return_counts=True)))
    assert [got[0][f] for f in INTS] == [n, total, total, total, sq] == [pair[f] for f in INTS]
    assert got[0]["S_sqrt"] == float(total) and got[0]["S_js"] == 0.0
    assert got[1]["n_shared"] == 5 and got[1]["X_shared"] == int(s[1:6].sum())
