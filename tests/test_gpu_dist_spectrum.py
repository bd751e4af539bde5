"""
The spectrum measures of `zot dist` on the GPU: zk_project_sum against numpy (unique + add.at), zk_spectrum_sums against Python
integers (exact) and math.fsum (the two doubles, within (n_shared + 8) * 2**-52 * sum |term|: n_shared roundings of a sum taken in
any order, and the few inside a term), and the command end to end against what the reference printed for the same sets
(tests/golden/g11_dist_spectrum.json).
"""
import io
import math
from contextlib import redirect_stdout

import numpy as np
import pytest

from tests import _golden as G
from tests import _spectrum_host as H
from zotmer_amd import cli, native
from zotmer_amd.commands import dist as dist_cmd
from zotmer_amd.library import vectors
from zotmer_amd.library.container import KmerSet

pytestmark = pytest.mark.gpu

MERGE_TILE = 4096          # csrc/internal.hpp
SUM_TILE = 4096            # csrc/spectrum.hip: PS_TILE
U32MAX = (1 << 32) - 1


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def sorted_keys(rng, n, bits):
    k = np.unique(rng.integers(0, 1 << bits, size=int(n * 1.2) + 16, dtype=np.uint64))
    assert len(k) >= n
    return np.sort(rng.choice(k, size=n, replace=False)) if n else k[:0]


# ---- zk_project_sum -----------------------------------------------------------------------------------------------------------

def check_project_sum(ctx, keys, counts, shift):
    dk, dc = ctx.upload(keys), ctx.upload(counts)
    ok, os_, total = ctx.project_sum(dk, dc, shift)
    wk, ws, wt = H.host_project_sum(keys, counts, shift)
    assert ok.n == len(wk) and np.array_equal(ok.to_host(), wk), (len(keys), shift)
    assert np.array_equal(os_.to_host(), ws), (len(keys), shift)
    assert total == wt
    return ws


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
@pytest.mark.parametrize("shift", [0, 2, 20, 40])
def test_project_sum_random(ctx, dtype, shift):
    """40-bit keys: shift 40 leaves one segment over the whole array, shift 0 is a copy and a widen"""
    rng = np.random.default_rng(1100 + shift)
    keys = sorted_keys(rng, 300000, 40)
    counts = rng.integers(0, 1000, size=len(keys)).astype(dtype)
    ws = check_project_sum(ctx, keys, counts, shift)
    assert len(ws) == (1 if shift == 40 else len(ws))


@pytest.mark.parametrize("n", [0, 1, 2, SUM_TILE - 1, SUM_TILE, SUM_TILE + 1, (1 << 20) - 1, 1 << 20, (1 << 20) + 1])
def test_project_sum_sizes(ctx, n):
    rng = np.random.default_rng(1200 + n % 97)
    keys = sorted_keys(rng, n, 30)
    for dtype in (np.uint32, np.uint64):
        counts = rng.integers(1, 50, size=n).astype(dtype)
        for shift in (0, 9):
            check_project_sum(ctx, keys, counts, shift)


def test_project_sum_segments_over_many_tiles(ctx):
    """consecutive keys: segments of 2^14 entries lie over four or five tiles each, at K = 1 four segments cover everything;
    segments that end exactly at a tile border, and one entry past it"""
    n = 20 * SUM_TILE + 1234
    keys = np.arange(n, dtype=np.uint64) + np.uint64(7)
    counts = (np.arange(n, dtype=np.uint64) % np.uint64(13)) + np.uint64(1)
    for shift in (14, 12, 13, 17, 63):
        check_project_sum(ctx, keys, counts, shift)
    k1 = np.sort(np.concatenate([keys + (np.uint64(b) << np.uint64(48)) for b in range(4)]))          # K = 1 of 25: four prefixes
    ws = check_project_sum(ctx, k1, np.tile(counts, 4), 48)
    assert len(ws) == 4
    check_project_sum(ctx, np.arange(4 * SUM_TILE, dtype=np.uint64), np.ones(4 * SUM_TILE, dtype=np.uint32), 12)   # starts on the borders


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_project_sum_beyond_32_bits(ctx, dtype):
    """counts of 2^32 - 1: the sums pass 2^32 (the reference's array('I') raises there; these are 64-bit)"""
    n = 3 * SUM_TILE + 5
    keys = np.arange(n, dtype=np.uint64) * np.uint64(3)
    counts = np.full(n, U32MAX, dtype=dtype)
    ws = check_project_sum(ctx, keys, counts, 10)
    assert int(ws.max()) > 1 << 32


# ---- zk_spectrum_sums ---------------------------------------------------------------------------------------------------------

def np_sums(xk, xs, yk, ys):
    """the specification with numpy for the matching and the term arithmetic (IEEE, one rounding an operation, in the order of
    library/dist.py:138-139), Python integers and math.fsum for the sums"""
    cx, cy = sum(int(v) for v in xs), sum(int(v) for v in ys)
    _, ix, iy = np.intersect1d(xk, yk, assume_unique=True, return_indices=True)
    x, y = xs[ix], ys[iy]
    nz = (x != 0) & (y != 0)
    x, y = x[nz], y[nz]
    xo, yo = x.astype(object), y.astype(object)
    out = dict(cx=cx, cy=cy, n_shared=len(x), S_min=int(np.minimum(xo, yo).sum()) if len(x) else 0, X_shared=int(xo.sum()) if len(x) else 0,
               Y_shared=int(yo.sum()) if len(x) else 0, S_xy=int((xo * yo).sum()) if len(x) else 0)
    roots = [math.sqrt(int(a) * int(b)) for a, b in zip(x, y)] if len(x) < 100000 else list(np.sqrt(x.astype(np.float64) * y.astype(np.float64)))
    fx, fy, dx, dy = x.astype(np.float64), y.astype(np.float64), float(cx), float(cy)
    if len(x):
        t1 = fx / dx * np.log(2 * dy * fx / (dy * fx + dx * fy))
        t2 = fy / dy * np.log(2 * dx * fy / (dx * fy + dy * fx))
        js = list(t1) + list(t2)
    else:
        js = []
    out["S_sqrt"], out["S_js"] = math.fsum(roots), math.fsum(js)
    out["sqrt_abs"], out["js_abs"] = out["S_sqrt"], math.fsum(abs(t) for t in js)
    return out


def check_sums(ctx, xk, xs, yk, ys, want=None, fresh=False):
    xk, xs, yk, ys = (np.ascontiguousarray(a, dtype=np.uint64) for a in (xk, xs, yk, ys))
    want = want or np_sums(xk, xs, yk, ys)
    d = [ctx.upload(a) for a in (xk, xs, yk, ys)]
    if fresh:
        ctx.release_workspace()
    got = ctx.spectrum_sums(d[0], d[1], want["cx"], d[2], d[3], want["cy"])
    for f in ("n_shared", "S_min", "X_shared", "Y_shared", "S_xy"):
        assert got[f] == want[f], (f, got[f], want[f])
    eps = (want["n_shared"] + 8) * 2.0 ** -52
    print("n_shared %d S_sqrt %.17g (want %.17g, tol %.3g) S_js %.17g (want %.17g, tol %.3g)" % (
        want["n_shared"], got["S_sqrt"], want["S_sqrt"], eps * want["sqrt_abs"], got["S_js"], want["S_js"], eps * want["js_abs"]))
    assert abs(got["S_sqrt"] - want["S_sqrt"]) <= eps * want["sqrt_abs"]
    assert abs(got["S_js"] - want["S_js"]) <= eps * want["js_abs"]
    again = ctx.spectrum_sums(d[0], d[1], want["cx"], d[2], d[3], want["cy"])
    assert again == got and math.copysign(1, again["S_js"]) == math.copysign(1, got["S_js"])          # the same bits
    return got


def random_spectrum(rng, n, bits=34, hi=2000):
    return sorted_keys(rng, n, bits), rng.integers(1, hi, size=n, dtype=np.uint64)


def test_sums_small_against_python(ctx):
    """the numpy statement used below and the pure-Python one agree, and the device with both"""
    rng = np.random.default_rng(2100)
    pool = sorted_keys(rng, 3000, 20)
    xk, yk = pool[rng.random(3000) < 0.7], pool[rng.random(3000) < 0.6]
    xs, ys = rng.integers(0, 40, size=len(xk), dtype=np.uint64), rng.integers(0, 40, size=len(yk), dtype=np.uint64)   # zeros: absent k-mers
    a, b = np_sums(xk, xs, yk, ys), H.host_spectrum_sums(xk, xs, yk, ys)
    for f in ("cx", "cy", "n_shared", "S_min", "X_shared", "Y_shared", "S_xy"):
        assert a[f] == b[f]
    assert abs(a["S_js"] - b["S_js"]) <= 2.0 ** -50 * b["js_abs"] and a["S_sqrt"] == b["S_sqrt"]
    check_sums(ctx, xk, xs, yk, ys, want=b)


def test_sums_disjoint_identical_empty(ctx):
    rng = np.random.default_rng(2200)
    k, s = random_spectrum(rng, 50000)
    got = check_sums(ctx, k * np.uint64(2), s, k * np.uint64(2) + np.uint64(1), s)          # disjoint
    assert got["n_shared"] == 0 and got["S_sqrt"] == 0.0 and got["S_js"] == 0.0
    got = check_sums(ctx, k, s, k, s)                                                        # identical
    assert got["n_shared"] == len(k) and got["S_min"] == got["X_shared"] == got["Y_shared"] == got["cx"]
    assert got["S_js"] == 0.0          # every logarithm is log(1)
    e = np.zeros(0, dtype=np.uint64)
    for xk, xs, yk, ys in ((e, e, k, s), (k, s, e, e), (e, e, e, e)):
        got = ctx.spectrum_sums(ctx.upload(xk), ctx.upload(xs), int(xs.sum()), ctx.upload(yk), ctx.upload(ys), int(ys.sum()))
        assert [got[f] for f in ("n_shared", "S_min", "X_shared", "Y_shared", "S_xy", "S_sqrt", "S_js")] == [0, 0, 0, 0, 0, 0.0, 0.0]


@pytest.mark.parametrize("total", [1, 2, MERGE_TILE - 1, MERGE_TILE, MERGE_TILE + 1, 2 * MERGE_TILE - 1, 2 * MERGE_TILE, 2 * MERGE_TILE + 1,
                                   5 * MERGE_TILE + 1])
def test_sums_around_the_merge_tile(ctx, total):
    """nx + ny = a tile of the merge path, one less, one more: equal pairs lie across the tile borders"""
    rng = np.random.default_rng(2300 + total)
    for nx in sorted({total // 2, total - total // 3, total - 1, 1} - {0, total}) or [1]:
        ny = total - nx
        if ny <= 0:
            continue
        pool = np.arange(max(nx, ny) + 50, dtype=np.uint64) * np.uint64(5) + np.uint64(3)
        xk, yk = np.sort(rng.choice(pool, nx, replace=False)), np.sort(rng.choice(pool, ny, replace=False))
        check_sums(ctx, xk, rng.integers(1, 9999, size=nx, dtype=np.uint64), yk, rng.integers(1, 9999, size=ny, dtype=np.uint64))


def test_sums_products_beyond_64_bits(ctx):
    """S_xy is exact in 128 bits: sums of 2^40 and more (products of 2^80, their sum past 2^64 at once), and three pairs of 2^62"""
    rng = np.random.default_rng(2400)
    k, _ = random_spectrum(rng, 20000)
    xs = rng.integers(1 << 40, 1 << 41, size=len(k), dtype=np.uint64)
    ys = rng.integers(1 << 40, 1 << 41, size=len(k), dtype=np.uint64)
    got = check_sums(ctx, k, xs, k[5:], ys[5:])
    assert got["S_xy"] > 1 << 64
    big = np.full(3, 1 << 62, dtype=np.uint64)
    got = check_sums(ctx, k[:3], big, k[:3], big)
    assert got["S_xy"] == 3 << 124


def test_sums_millions_and_fresh_workspace(ctx):
    """two spectra of about three million prefixes, about half of each shared; the same pair again on a released workspace"""
    rng = np.random.default_rng(2500)
    pool = sorted_keys(rng, 4500000, 44)
    xk, yk = pool[rng.random(len(pool)) < 0.67], pool[rng.random(len(pool)) < 0.67]
    xs, ys = rng.integers(1, 300, size=len(xk), dtype=np.uint64), rng.integers(1, 300, size=len(yk), dtype=np.uint64)
    want = np_sums(xk, xs, yk, ys)
    assert want["n_shared"] > 1500000
    a = check_sums(ctx, xk, xs, yk, ys, want=want)
    b = check_sums(ctx, xk, xs, yk, ys, want=want, fresh=True)
    assert a == b


def test_project_sum_fresh_workspace(ctx):
    rng = np.random.default_rng(2600)
    keys = sorted_keys(rng, (1 << 21) + 77, 40)
    counts = rng.integers(1, 100, size=len(keys)).astype(np.uint32)
    dk, dc = ctx.upload(keys), ctx.upload(counts)
    ctx.release_workspace()
    ok, os_, total = ctx.project_sum(dk, dc, 16)
    wk, ws, wt = H.host_project_sum(keys, counts, 16)
    assert np.array_equal(ok.to_host(), wk) and np.array_equal(os_.to_host(), ws) and total == wt


def test_profile_tags(ctx):
    rng = np.random.default_rng(2700)
    k, s = random_spectrum(rng, 100000)
    dk, ds = ctx.upload(k), ctx.upload(s)
    ctx.profile(True)
    try:
        pk, ps, tot = ctx.project_sum(dk, ds, 8)
        ctx.spectrum_sums(pk, ps, tot, pk, ps, tot)
        rec = ctx.profile_read()
    finally:
        ctx.profile(False)
    assert rec["project_sum"]["launches"] == 2 and rec["project_sum"]["bytes"] == 8 * len(k) + 16 * len(k) + 16 * pk.n
    assert rec["spectrum"]["launches"] == 1 and rec["spectrum"]["bytes"] == 16 * 2 * pk.n


# ---- the command ---------------------------------------------------------------------------------------------------------------

CASES = G.load_json("g11_dist_spectrum")
NINE = sorted(m for m, v in dist_cmd.MEASURES.items() if v[1])


def zot(*args):
    buf = io.StringIO()
    with redirect_stdout(buf):
        cli.main_inner([str(a) for a in args])
    return buf.getvalue()


def write_set(path, K, kmers, counts=None):
    with KmerSet(str(path), "w") as z:
        if counts is None:
            z.add("kmers", vectors.encode_kmers(kmers))
        else:
            vectors.write_kmers_and_counts(z, kmers, counts)
        z.meta.update({"K": K, "kmers": "kmers", "counts": "counts"})
    return path


def golden_file(tmp_path, name, k=None, parity=None):
    info, km, ct, _, _ = G.load_case(name)
    tag = name
    if parity is not None:
        keep = ((km >> np.uint64(2 * (info["K"] - k))) & np.uint64(1)) == np.uint64(parity)
        km, ct, tag = km[keep], ct[keep], "%s_parity%d" % (name, parity)
    p = tmp_path / (tag + ".k%d" % info["K"])
    return p if p.exists() else write_set(p, info["K"], km, ct)


@pytest.mark.parametrize("c", CASES, ids=lambda c: "%s-%s-k%d%s" % (c["lhs"], c["rhs"], c["k"], "-disjoint" if "prefix_parity" in c else ""))
def test_dist_matches_the_reference_text(tmp_path, c):
    par = c.get("prefix_parity", [None, None])
    lhs, rhs = golden_file(tmp_path, c["lhs"], c["k"], par[0]), golden_file(tmp_path, c["rhs"], c["k"], par[1])
    out = zot("dist", "-M", "*.quant", "-M", "*.ab", "-M", "jensen.shannon", c["k"], lhs, rhs)
    vals = {m: c["values"][m]["g"] if m in c["values"] else "1" for m in NINE}          # disjoint: jaccard.ab, sorensen.ab = 1
    want = "\t".join(["lhs.name", "rhs.name"] + NINE) + "\n" + "\t".join([str(lhs), str(rhs)] + [vals[m] for m in NINE]) + "\n"
    assert out.split("\n") == want.split("\n")


def test_dist_all_measures(tmp_path):
    """-M '*': 17 columns, three files (every file prepared once, both ways); the *.qual columns are those of a *.qual run"""
    files = [golden_file(tmp_path, "g4_part%d" % i) for i in range(3)]
    rows = [l.split("\t") for l in zot("dist", "-M", "*", 8, *files).splitlines()]
    qual = [l.split("\t") for l in zot("dist", "-M", "*.qual", 8, *files).splitlines()]
    quant = [l.split("\t") for l in zot("dist", "-M", "*.quant", "-M", "*.ab", "-M", "jensen.shannon", 8, *files).splitlines()]
    assert len(rows) == 4 and all(len(r) == 2 + 17 for r in rows) and rows[0][2:] == sorted(dist_cmd.MEASURES)
    for r, a, b in zip(rows, qual, quant):
        assert [v for h, v in zip(rows[0], r) if h.endswith(".qual") or h.endswith(".name")] == a
        assert [v for h, v in zip(rows[0], r) if not h.endswith(".qual")] == b
    gold = {(c["lhs"], c["rhs"]): c for c in CASES if c["k"] == 8 and "prefix_parity" not in c}
    c = gold[("g4_part0", "g4_part1")]
    assert [v for h, v in zip(rows[0], rows[1]) if h in c["values"]] == [c["values"][m]["g"] for m in NINE]


def test_dist_errors(tmp_path):
    a, b = golden_file(tmp_path, "g4_part0"), golden_file(tmp_path, "g4_part1")
    with pytest.raises(dist_cmd.MismatchedK):
        zot("dist", "-M", "chord.quant", 26, a, b)
    info, km, ct, _, _ = G.load_case("g4_part0")
    bare = write_set(tmp_path / "bare.k25", 25, km)
    with pytest.raises(SystemExit) as e:
        zot("dist", "-M", "jensen.shannon", 8, a, bare)
    assert "no counts" in str(e.value.code)
    assert zot("dist", "-M", "jaccard.qual", 8, a, bare).count("\n") == 2          # the set measures never needed them
    empty = write_set(tmp_path / "empty.k25", 25, km[:0], ct[:0])
    with pytest.raises(SystemExit) as e:
        zot("dist", "-M", "bray.curtis.quant", 8, a, empty)
    assert e.value.code not in (0, None) and "no k-mers" in str(e.value.code)
