"""`zot ksnp` on the GPU: zk_ksnp_flank and zk_ksnp_components against the plain-Python restatement (tests/_ksnp_restatement.py)
and, on the fixture's cases, against what the reference's generators yielded (tests/golden/k1_ksnp.json), exactly.

Where the restatement would take more than about a second -- groups of a thousand k-mers and more, at (K + 1)^2 table cells a
pair under -L -- the NumPy brute force (tests/_ksnp_brute.py) stands in for it: it shares no code with the restatement and
tests/test_ksnp_host.py holds the two against each other and against the fixture.  `expected` below says which one a shape gets.

Shapes: every size at which csrc/ksnp.hip takes another path (include/zotk.h: ZK_KSNP_WAVE_GROUP, ZK_KSNP_LDS_GROUP, a tile
edge of ZK_KSNP_PAIR_TILE above it, the 4096 of the flat passes), as three groups of t - 1, t and t + 1 members that straddle a
tile edge of the flat passes; chains; the middle-base rule; pairs on which the two distances differ; capacity; views."""
import contextlib
import ctypes as C
import functools
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _ksnp_brute as B
from tests import _ksnp_restatement as R
from tests._ksnp_cases import DEFAULT, HAMMING, LEVENSHTEIN, around, chain_lows, fixture_cases, geometry, group, random_lows, random_set

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = {c["name"]: c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "k1_ksnp.json")))}
CASES = fixture_cases()
IDS = [c["name"] for c in CASES]
SENTINEL = np.uint64(0x5A5A5A5A5A5A5A5A)


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    from zotmer_amd.library import engine
    yield engine.context()
    engine.close()


def metric_of(mode):
    from zotmer_amd import native
    return {DEFAULT: None, HAMMING: native.KSNP_HAMMING, LEVENSHTEIN: native.KSNP_LEVENSHTEIN}[mode]


def device(ctx, K, mode, d, xs):
    got = ctx.ksnp(ctx.upload(np.asarray(xs, dtype=np.uint64)), K, metric_of(mode), d).to_host()
    assert got.dtype == np.uint64
    return got.tolist()


def expected(K, mode, d, xs):
    """the restatement, or the brute force where the restatement's pair loop is too long for a test"""
    xs = np.asarray(xs, dtype=np.uint64)
    pairs = sum((b - a) * (b - a - 1) // 2 for a, b in B.group_slices(K, xs)) if len(xs) else 0
    cells = pairs * ((K + 1) ** 2 if mode == LEVENSHTEIN else 1)
    if mode == DEFAULT or cells <= 300000:
        return R.run(K, mode, d, xs.tolist())
    return B.run(K, mode, d, xs).tolist()


def check(ctx, K, mode, d, xs):
    want = expected(K, mode, d, xs)
    got = device(ctx, K, mode, d, xs)
    assert got == want, (K, mode, d, len(xs), len(got), len(want))
    return want


ALL_MODES = ((DEFAULT, 0), (HAMMING, 0), (HAMMING, 1), (HAMMING, 2), (LEVENSHTEIN, 1), (LEVENSHTEIN, 2))


# ---- the fixture ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixture_on_the_device(ctx, case):
    got = device(ctx, case["K"], case["mode"], case["d"], case["kmers"])
    assert got == GOLD[case["name"]]["kept"]          # what the reference's generator yielded


# ---- sizes and K ----------------------------------------------------------------------------------------------------------------

def test_nothing_and_one(ctx):
    from zotmer_amd import native
    fill = np.full(8, SENTINEL, dtype=np.uint64)
    out = ctx.upload(fill)
    for call in (lambda n: ctx.lib.zk_ksnp_flank(ctx.h, None, 0, 25, out.ptr, out.n, C.byref(n)),
                 lambda n: ctx.lib.zk_ksnp_components(ctx.h, None, 0, 25, native.KSNP_HAMMING, 1, out.ptr, out.n, C.byref(n)),
                 lambda n: ctx.lib.zk_ksnp_components(ctx.h, None, 0, 25, native.KSNP_LEVENSHTEIN, 2, None, 0, C.byref(n))):
        n = C.c_uint64(99)
        assert call(n) == native.ZK_OK and n.value == 0
    assert np.array_equal(out.to_host(), fill)
    for K in (1, 2, 13, 32):
        for mode, d in ALL_MODES:
            assert device(ctx, K, mode, d, [3]) == []
            assert device(ctx, K, mode, d, [0]) == []


@pytest.mark.parametrize("K", [1, 2])
def test_every_set_of_the_shortest_kmers(ctx, K):
    """J = 0: no tail, the last base is the middle base"""
    every = 4 ** K
    subsets = range(1, 1 << every) if K == 1 else [s for s in range(1, 1 << every, 97)] + [(1 << every) - 1]
    for s in subsets:
        xs = [x for x in range(every) if (s >> x) & 1]
        for mode, d in ALL_MODES + ((HAMMING, K), (LEVENSHTEIN, K)):
            assert device(ctx, K, mode, d, xs) == R.run(K, mode, d, xs), (K, s, mode, d)


def test_k32_with_the_prefix_in_the_top_bits(ctx):
    K = 32
    _, S, T = geometry(K)
    xs = []
    for p in (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF):
        lows = random_lows(K, 12, seed=p & 0xFFFF)
        lows += [lows[0] ^ (1 << T), lows[1] ^ 3, lows[2] ^ (2 << T) ^ 1, ((lows[3] << 2) & ((1 << S) - 1)) | 2]
        xs += group(K, p, set(lows))
    xs += [(0xFFFFFFFF << S) | ((1 << S) - 1), (0xFFFFFFFF << S) | ((1 << S) - 1 - (1 << T))]          # the last k-mer there is
    xs = sorted(set(xs))
    assert xs[-1] == (1 << 64) - 1
    for mode, d in ALL_MODES + ((HAMMING, 32), (LEVENSHTEIN, 32)):
        want = check(ctx, K, mode, d, xs)
        assert mode == HAMMING and d == 0 or want


def test_even_k_against_odd_k(ctx):
    """K = 12 and K = 13 cut the same low bases differently: J = 5 and J = 6"""
    lows = sorted(set(random_lows(12, 300, seed=12)))          # values below 4^6: low bases of both
    for K in (12, 13):
        xs = sorted(group(K, 1, lows) + group(K, 2, lows[::2]) + group(K, 3, lows[:1]))
        for mode, d in ALL_MODES:
            check(ctx, K, mode, d, xs)
    low = lambda K, kept: sorted(x & ((1 << geometry(K)[1]) - 1) for x in kept if x >> geometry(K)[1] == 1)
    assert low(12, R.run(12, DEFAULT, 0, group(12, 1, lows))) != low(13, R.run(13, DEFAULT, 0, group(13, 1, lows)))


def test_one_group_that_is_the_whole_input(ctx):
    for K, n in ((5, 64), (5, 37), (12, 700), (13, 3000)):
        _, S, _ = geometry(K)
        xs = sorted(group(K, (1 << (2 * K - S)) - 1, random_lows(K, n, seed=n)))
        for mode, d in ((DEFAULT, 0), (HAMMING, 1), (HAMMING, 2)) + (((LEVENSHTEIN, 1), (LEVENSHTEIN, 2)) if n <= 700 else ()):
            check(ctx, K, mode, d, xs)


def test_groups_of_one_only(ctx):
    for K, xs in ((13, around_shape(64)[:4000]), (32, np.unique(np.random.default_rng(32).integers(0, 1 << 63, size=4096 + 77, dtype=np.uint64)))):
        assert all(b - a == 1 for a, b in B.group_slices(K, xs)) and len(xs) >= 4000
        for mode, d in ALL_MODES + ((HAMMING, 10 ** 6),):
            assert device(ctx, K, mode, d, xs) == []


# ---- the thresholds between the kernels ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def around_shape(t):
    return around(13, t, seed=t)


def thresholds():
    from zotmer_amd import native
    w, l, p = native.KSNP_WAVE_GROUP, native.KSNP_LDS_GROUP, native.KSNP_PAIR_TILE
    assert (w, l, p) == (64, 1024, 256)
    return [w, l, l + p, 4096]


@pytest.mark.parametrize("t,mode,d", [(t, m, d) for t in (64, 1024, 1280, 4096)
                                      for m, d in ((DEFAULT, 0), (HAMMING, 1), (HAMMING, 2), (LEVENSHTEIN, 1), (LEVENSHTEIN, 2))
                                      if m != LEVENSHTEIN or t <= 1024 and (d == 1 or t == 64)])
def test_groups_around_every_threshold(ctx, t, mode, d):
    """t - 1, t and t + 1 members: the wave kernel against the workgroup kernel, that against the tile pairs (1025 members: four
    tiles of 256 and one of 1), a last tile of 255, 256 and 1 members, and the tile of the flat passes.  -L up to 1025 members,
    where the brute force's table of all pairs is affordable: the pair schedule is the same code for both distances."""
    assert t in thresholds()
    xs = around_shape(t)
    sizes = [b - a for a, b in B.group_slices(13, xs)]
    assert sizes[-3:] == [t - 1, t, t + 1] and set(sizes[:-3]) == {1}
    first = len(xs) - sum(sizes[-3:])
    assert first // 4096 != (first + t - 2) // 4096          # the first of the three straddles a tile edge of the flat passes
    want = check(ctx, 13, mode, d, xs)
    assert want and len(want) < len(xs)


def test_the_same_call_returns_the_same_list(ctx):
    xs = around_shape(1280)
    a = device(ctx, 13, HAMMING, 2, xs)
    assert a == device(ctx, 13, HAMMING, 2, xs) == device(ctx, 13, HAMMING, 2, xs)


# ---- chains ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("padded", [False, True], ids=["wave", "tiles"])
def test_chain(ctx, d, padded):
    """consecutive members exactly d apart, all others farther: one component only through every link, and the order of the
    list is not the order of the chain"""
    K = 13
    lows = chain_lows(K, d)[:-1]
    assert len(lows) >= 13 and lows != sorted(lows)
    assert all(R.ham(a, b) == d for a, b in zip(lows, lows[1:]))
    assert all(R.ham(lows[i], lows[j]) > d for i in range(len(lows)) for j in range(i + 2, len(lows)))
    members = set(lows)
    if padded:          # past the LDS threshold: the links cross the tiles of the pair kernel
        members |= set(random_lows(K, 1100, seed=d))
        assert len(members) > 1024 + 64
    xs = sorted(group(K, 77, members) + group(K, 78, lows[:len(lows) // 2] + lows[len(lows) // 2 + 1:]))
    want = check(ctx, K, HAMMING, d, xs)
    assert set(group(K, 77, lows)) <= set(want)                      # the whole chain, both ends
    if d == 2:
        assert not set(group(K, 77, lows)) <= set(expected(K, HAMMING, 1, xs))
    check(ctx, K, LEVENSHTEIN, d, sorted(group(K, 77, lows) + group(K, 78, lows[::-1][:9])))


# ---- the middle-base rule ---------------------------------------------------------------------------------------------------------

def test_components_of_one_middle_base_are_not_kept(ctx):
    K = 13
    J, S, T = geometry(K)
    one_base = [(2 << T) | t for t in (0, 1, 2, 3, 1 << 2, 2 << 4)]                       # middle G, tails one base apart: a component
    two_bases = [(0 << T) | 0xFFF, (3 << T) | 0xFFF, (3 << T) | 0xFFE, (3 << T) | 0xBFE]  # A and T over one tail, and two more T
    lone = [(1 << T) | 0x555]
    xs = sorted(group(K, 9, one_base + two_bases + lone) + group(K, 10, one_base))
    want = check(ctx, K, HAMMING, 1, xs)
    assert want == sorted(group(K, 9, two_bases))
    assert check(ctx, K, DEFAULT, 0, xs) == sorted(group(K, 9, two_bases[:2]))
    assert check(ctx, K, LEVENSHTEIN, 1, xs) == want
    assert check(ctx, K, HAMMING, 0, xs) == []
    for d in (K, 10 ** 6, (1 << 64) - 1):          # everything of a group is joined: whole groups where two middle bases occur
        assert check(ctx, K, HAMMING, min(d, 10 ** 6), xs) == sorted(group(K, 9, one_base + two_bases + lone))
        got = ctx.ksnp(ctx.upload(np.array(xs, dtype=np.uint64)), K, metric_of(LEVENSHTEIN), d).to_host().tolist()
        assert got == sorted(group(K, 9, one_base + two_bases + lone)) == R.run(K, LEVENSHTEIN, K, xs)


# ---- -L against -H -----------------------------------------------------------------------------------------------------------------

def test_pairs_on_which_the_two_distances_differ(ctx):
    K = 13
    kmer = lambda s: sum("ACGT".index(c) << (2 * (len(s) - 1 - i)) for i, c in enumerate(s))
    a, b = kmer("ACGTACG"), kmer("CGTACGT")                  # the low 7 bases, shifted by one: every base differs
    c, e = kmer("GGGGTTT"), kmer("TGGGTTT")                  # one substituted base, the middle one
    assert R.ham(a, b) == 7 and R.lev(7, min(a, b), max(a, b)) <= 2 and R.ham(c, e) == 1 == R.lev(7, min(c, e), max(c, e))
    xs = sorted(group(K, 100, [a, b]) + group(K, 200, [c, e]))
    for d in (1, 2, 6):
        assert check(ctx, K, HAMMING, d, xs) == sorted(group(K, 200, [c, e]))
    assert check(ctx, K, HAMMING, 7, xs) == xs
    assert check(ctx, K, LEVENSHTEIN, 2, xs) == xs
    lev1 = check(ctx, K, LEVENSHTEIN, 1, xs)
    assert set(group(K, 200, [c, e])) <= set(lev1)
    # basics.lev is not symmetric: the k-mer that comes first in the list is its first argument, wherever the kernels meet the pair
    x, y = kmer("ACCCCCG"), kmer("CCCCCGT")                  # (two middle bases: kept as soon as they are joined)
    assert x < y and R.lev(7, x, y) == 1 and R.lev(7, y, x) == 2
    for n_pad in (0, 70, 1100):
        pad = [v for v in random_lows(K, n_pad, seed=n_pad) if R.ham(v, x) > 3 and R.ham(v, y) > 3] if n_pad else []
        zs = sorted(group(K, 5, [x, y] + pad))
        want = check(ctx, K, LEVENSHTEIN, 1, zs)
        assert set(group(K, 5, [x, y])) <= set(want)


# ---- capacity and views -----------------------------------------------------------------------------------------------------------

def call_into(ctx, K, mode, d, d_in, n, out_ptr, cap):
    from zotmer_amd import native
    got = C.c_uint64(0)
    if mode == DEFAULT:
        rc = ctx.lib.zk_ksnp_flank(ctx.h, d_in, n, K, out_ptr, cap, C.byref(got))
    else:
        rc = ctx.lib.zk_ksnp_components(ctx.h, d_in, n, K, metric_of(mode), d, out_ptr, cap, C.byref(got))
    return rc, got.value


@pytest.mark.parametrize("mode,d", [(DEFAULT, 0), (HAMMING, 1), (LEVENSHTEIN, 1)])
def test_capacity(ctx, mode, d):
    from zotmer_amd import native
    K, xs = 13, around_shape(64)
    want = expected(K, mode, d, xs)
    need = len(want)
    assert need > 2
    d_in = ctx.upload(xs)
    for cap in (0, need - 1, need, need + 1):
        fill = np.full(need + 64, SENTINEL, dtype=np.uint64)
        out = ctx.upload(fill)
        rc, got = call_into(ctx, K, mode, d, d_in.ptr, len(xs), out.ptr if cap else None, cap)
        host = out.to_host()
        assert got == need
        if cap < need:
            assert rc == native.ZK_ENOSPC and (host[cap:] == SENTINEL).all()          # nothing at or beyond cap
        else:
            assert rc == native.ZK_OK and host[:need].tolist() == want and (host[need:] == SENTINEL).all()
    assert np.array_equal(d_in.to_host(), xs)
    # the binding repeats the call with the length reported
    assert ctx.ksnp(d_in, K, metric_of(mode), d, out=ctx.empty(1, np.uint64)).to_host().tolist() == want


@pytest.mark.parametrize("mode,d", [(DEFAULT, 0), (HAMMING, 2), (LEVENSHTEIN, 1)])
def test_views_at_odd_offsets(ctx, mode, d):
    """input and output inside larger guarded arrays, at odd element offsets, the last place before a 128-byte line among them"""
    from zotmer_amd import native
    K, xs = 13, around_shape(64)
    want = expected(K, mode, d, xs)
    for off_in, off_out in ((1, 3), (15, 15), (7, 1)):
        big_in = np.full(len(xs) + 40, SENTINEL, dtype=np.uint64)
        big_in[off_in:off_in + len(xs)] = xs
        d_in = ctx.upload(big_in)
        big_out = np.full(len(want) + 40, SENTINEL, dtype=np.uint64)
        d_out = ctx.upload(big_out)
        assert d_in.ptr % 128 == 0 and d_out.ptr % 128 == 0
        rc, got = call_into(ctx, K, mode, d, d_in.ptr + 8 * off_in, len(xs), d_out.ptr + 8 * off_out, len(want))
        assert rc == native.ZK_OK and got == len(want)
        host = d_out.to_host()
        assert host[off_out:off_out + len(want)].tolist() == want
        assert (host[:off_out] == SENTINEL).all() and (host[off_out + len(want):] == SENTINEL).all()
        assert np.array_equal(d_in.to_host(), big_in)          # the input is unchanged


def test_refused_arguments(ctx):
    from zotmer_amd import native
    d_in, out = ctx.upload(np.arange(8, dtype=np.uint64)), ctx.upload(np.full(8, SENTINEL, dtype=np.uint64))
    n = C.c_uint64(0)
    for K in (0, 33, -1):
        assert ctx.lib.zk_ksnp_flank(ctx.h, d_in.ptr, 8, K, out.ptr, 8, C.byref(n)) == native.ZK_EINVAL
        assert ctx.lib.zk_ksnp_components(ctx.h, d_in.ptr, 8, K, 0, 1, out.ptr, 8, C.byref(n)) == native.ZK_EINVAL
    assert ctx.lib.zk_ksnp_components(ctx.h, d_in.ptr, 8, 5, 2, 1, out.ptr, 8, C.byref(n)) == native.ZK_EINVAL          # no such metric
    for big in ((1 << 32) - 1, 1 << 40):                                                                      # refused before any launch
        assert ctx.lib.zk_ksnp_flank(ctx.h, d_in.ptr, big, 5, out.ptr, 8, C.byref(n)) == native.ZK_EINVAL
        assert ctx.lib.zk_ksnp_components(ctx.h, d_in.ptr, big, 5, 0, 1, out.ptr, 8, C.byref(n)) == native.ZK_EINVAL
    assert ctx.lib.zk_ksnp_flank(ctx.h, d_in.ptr, 8, 5, None, 8, C.byref(n)) == native.ZK_EINVAL
    assert (out.to_host() == SENTINEL).all()
    assert device(ctx, 5, DEFAULT, 0, list(range(8))) == R.run(5, DEFAULT, 0, list(range(8)))          # the context is as good as before


# ---- a randomised run against the brute force --------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,n", [(5, 700), (8, 3000), (9, 6000)])
def test_random_sets_against_the_brute_force(ctx, K, n):
    xs = random_set(K, n, seed=K * n)
    for mode, d in ALL_MODES:
        got = device(ctx, K, mode, d, xs)
        assert got == B.run(K, mode, d, xs).tolist(), (K, mode, d)


def test_profile_records(ctx):
    xs = ctx.upload(around_shape(1024))          # 1023 and 1024 members for the workgroup kernel, 1025 for the tile pairs
    out = ctx.empty(xs.n, np.uint64)          # room for everything: one call each
    ctx.profile(True)
    ctx.ksnp(xs, 13, out=out)
    ctx.ksnp(xs, 13, metric_of(HAMMING), 1, out=out)
    rec = ctx.profile_read()
    ctx.profile(False)
    assert rec["ksnp_flank"]["launches"] == 1 and rec["ksnp_flank"]["bytes"] == 8 * xs.n + 8 * ((xs.n + 63) // 64)
    assert rec["ksnp_pairs"]["launches"] == 3 and rec["ksnp_pairs"]["bytes"] == 16 * xs.n          # wave, workgroup and tile-pair kernels


# ---- the command -------------------------------------------------------------------------------------------------------------------

def run(args):
    from zotmer_amd import cli
    out, err = io.StringIO(), io.StringIO()
    code = None
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            code = cli.main_inner(args)
        except SystemExit as e:
            code = e.code
    return code, out.getvalue(), err.getvalue()


def write_set(path, K, xs, counts=True):
    from zotmer_amd.library import vectors
    from zotmer_amd.library.container import KmerSet
    xs = np.array(xs, dtype=np.uint64)
    with KmerSet(str(path), "w") as z:
        if counts:
            vectors.write_kmers_and_counts(z, xs, np.arange(1, len(xs) + 1, dtype=np.uint64))
            z.meta.update({"K": K, "kmers": "kmers", "counts": "counts", "hist": {"1": 1}})
        else:
            z.add("kmers", vectors.encode_kmers(xs))
            z.meta.update({"K": K, "kmers": "kmers"})
    return str(path)


def options(case):
    return {DEFAULT: [], HAMMING: ["-H", str(case["d"])], LEVENSHTEIN: ["-L", str(case["d"])]}[case["mode"]]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_command_on_the_fixture(ctx, case, tmp_path):
    from zotmer_amd.commands.dump import render
    from zotmer_amd.library import vectors
    from zotmer_amd.library.container import KmerSet
    K, want = case["K"], GOLD[case["name"]]["kept"]
    inp, out = write_set(tmp_path / "in.k", K, case["kmers"]), str(tmp_path / "out.k")
    assert run(["ksnp"] + options(case) + [out, inp]) == (0, "", "")
    with KmerSet(out, "r") as z:
        assert z.meta == {"K": K, "kmers": "kmers"} and sorted(z.toc) == ["__meta__", "kmers"]
        assert vectors.read_kmers(z).tolist() == want
    code, text, err = run(["dump", out])
    assert err == "" and text.split() == render(K, np.array(want, dtype=np.uint64))
    # counts are ignored: the same input without them gives the same file
    bare, out2 = write_set(tmp_path / "bare.k", K, case["kmers"], counts=False), str(tmp_path / "out2.k")
    assert run(["ksnp"] + options(case) + [out2, bare]) == (0, "", "")
    assert open(out, "rb").read() == open(out2, "rb").read()


def test_the_zot_script(ctx, tmp_path):
    """./zot ksnp in a process of its own, then ./zot dump and ./zot info on what it wrote"""
    case = CASES[IDS.index("k25_levenshtein_2")]
    inp, out = write_set(tmp_path / "in.k", 25, case["kmers"]), str(tmp_path / "out.k")
    zot = os.path.join(ROOT, "zot")
    p = subprocess.run([sys.executable, zot, "ksnp", "-L", "2", out, inp], capture_output=True, text=True, timeout=120)
    assert (p.returncode, p.stdout, p.stderr) == (0, "", "")
    p = subprocess.run([sys.executable, zot, "dump", out], capture_output=True, text=True, timeout=120)
    from zotmer_amd.commands.dump import render
    assert p.returncode == 0 and p.stdout.split() == render(25, np.array(GOLD[case["name"]]["kept"], dtype=np.uint64))
    p = subprocess.run([sys.executable, zot, "info", out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "25" in p.stdout


def test_command_on_an_empty_set(ctx, tmp_path):
    from zotmer_amd.library.container import KmerSet
    inp, out = write_set(tmp_path / "e.k", 11, []), str(tmp_path / "out.k")
    for opt in ([], ["-H", "1"], ["-L", "1"]):
        assert run(["ksnp"] + opt + [out, inp]) == (0, "", "")
        with KmerSet(out, "r") as z:
            assert z.meta == {"K": 11, "kmers": "kmers"} and z.member_size("kmers") == 0
