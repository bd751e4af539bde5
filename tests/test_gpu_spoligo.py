"""`zot spoligo` on the device: zk_probe_scan (csrc/probe_scan.hip) against a numpy brute force (the n x W table of Hamming
distances) at the sizes where the kernel changes path, and the command against the reference's fixtures
(tests/golden/sp1_spoligo.json) and the restatement of the reference's route (tests/_spoligo_restatement.py)."""
import contextlib
import io
import json
import os

import numpy as np
import pytest

from tests import _spoligo_restatement as R
from tests._spoligo_cases import make_cases

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sp1_spoligo.json")
INPUTS = {c["name"]: c for c in make_cases()}
CASES = [dict(INPUTS[c["name"]], **c) for c in json.load(open(GOLD)) if c["name"] in INPUTS]
IDS = [c["name"] for c in CASES]
LOW = 0x5555555555555555


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    from zotmer_amd.library import engine
    yield engine.context()
    engine.close()


def consts():
    from zotmer_amd import native
    return native.PROBE_TILE, native.PROBE_MAX_WINDOWS


def test_constants_match_the_header():
    import re
    T, W = consts()
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zotk.h")).read()
    assert int(re.search(r"#define ZK_PROBE_TILE (\d+)", text).group(1)) == T
    assert int(re.search(r"#define ZK_PROBE_MAX_WINDOWS (\d+)", text).group(1)) == W


# ---- the brute force ---------------------------------------------------------------------------------------------------

def ham(x, v):
    """basics.ham over a uint64 array"""
    z = x ^ np.uint64(v)
    m = (z | (z >> np.uint64(1))) & np.uint64(LOW)
    return np.unpackbits(m.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1)


def brute(kmers, K, windows):
    out = np.zeros((len(windows), 3), dtype=np.uint64)
    for w, (J, v) in enumerate(windows):
        d = ham(kmers >> np.uint64(2 * (K - J)), v)
        out[w] = [np.count_nonzero(d == i) for i in range(3)]
    return out


def entry(ctx, kmers, K, windows, n=None):
    """zk_probe_scan itself -> (return code, (W, 3) tallies)"""
    from zotmer_amd import native
    arr = (native.ProbeWindow * max(len(windows), 1))(*[native.ProbeWindow(int(v), int(J), 0) for J, v in windows])
    t = np.full(3 * len(windows) + 1, 0xABCD, dtype=np.uint64)
    rc = ctx.lib.zk_probe_scan(ctx.h, kmers.ptr if kmers is not None else None, kmers.n if n is None else n, K, arr, len(windows),
                               t.ctypes.data_as(native.C.POINTER(native.C.c_uint64)))
    assert t[-1] == 0xABCD          # nothing written past the 3 W words
    return rc, t[:-1].reshape(-1, 3)


def substitute(rng, v, J, d):
    """v with d of its J bases substituted (each by one of the three other bases)"""
    for i in rng.choice(J, size=d, replace=False):
        v ^= int(rng.integers(1, 4)) << (2 * int(i))
    return v


def make_problem(seed, K, Js, W, n):
    """W windows with J cycling through Js, and n distinct k-mers, a share of them planted at distance 0 .. 3 of a window"""
    rng = np.random.default_rng(seed)
    rnd = lambda bits: int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)) >> (64 - bits) if bits else 0
    windows = [(Js[w % len(Js)], rnd(2 * Js[w % len(Js)])) for w in range(W)]
    pool = set()
    for w in range(min(W, 40)):
        J, v = windows[w]
        for d in (0, 1, 2, 3, 1, 2):
            if d <= J:
                pool.add((substitute(rng, v, J, d) << (2 * (K - J))) | rnd(2 * (K - J)))
    planted = sorted(pool)
    while len(pool) < min(n + len(planted), 1 << (2 * K)):
        pool.add(rnd(2 * K))
    rest = sorted(pool - set(planted))
    rng.shuffle(rest)
    take = (planted + rest)[:n] if n >= len(planted) else list(rng.permutation(np.array(planted, dtype=np.uint64))[:n])
    return windows, np.sort(np.array(take, dtype=np.uint64))


def sizes():
    T, _ = consts()
    return [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]


@pytest.mark.parametrize("W", [1, 2, 65])
@pytest.mark.parametrize("n", range(9))
def test_probe_scan_sizes(ctx, n, W):
    n = sizes()[n]
    windows, kmers = make_problem(1000 + 7 * n + W, 25, [25, 13, 24, 1], W, n)
    assert len(kmers) == n
    rc, got = entry(ctx, ctx.upload(kmers), 25, windows)
    want = brute(kmers, 25, windows)
    assert rc == 0 and np.array_equal(got, want)
    if n >= 64:
        assert want.sum() > 0
    # the wrapper says the same
    assert np.array_equal(ctx.probe_scan(ctx.upload(kmers), 25, windows), want)


@pytest.mark.parametrize("K,Js", [(25, [1, 13, 24, 25]), (32, [1, 31, 32]), (1, [1]), (2, [1, 2]), (16, [16, 5])])
def test_probe_scan_k_and_j(ctx, K, Js):
    T, _ = consts()
    for n in (65, T + 1):
        n = min(n, 1 << (2 * K))
        windows, kmers = make_problem(77 + K, K, Js, 65, n)
        rc, got = entry(ctx, ctx.upload(kmers), K, windows)
        want = brute(kmers, K, windows)
        assert rc == 0 and np.array_equal(got, want), (K, n)
        for J in Js:          # every J saw something
            assert sum(int(want[w].sum()) for w in range(65) if windows[w][0] == J) > 0, J


@pytest.mark.parametrize("K,J", [(32, 32), (32, 31), (25, 25), (25, 13)])
def test_planted_distances(ctx, K, J):
    """entries at distance exactly 0, 1, 2 and 3 of one window: mismatches in the top base, the bottom base, the upper and the
    lower half of the word, and a base changed in both bits; the entries at distance 3 move no tally"""
    rng = np.random.default_rng(5 + K + J)
    s = 2 * (K - J)
    v = int(rng.integers(0, 1 << 62)) >> (62 - 2 * J) if J < 32 else int(rng.integers(0, 1 << 63)) * 2 + 1
    base = lambda i: 2 * i                      # bit place of base i of the window, counted from its bottom base
    top, bottom = J - 1, 0
    upper = max(i for i in range(J) if base(i) + s >= 32)          # a base in the upper half of the k-mer's word
    lower = min(range(J), key=lambda i: abs(base(i) + s - 20))     # ... and one in (or nearest to) the lower half
    low = lambda: int(rng.integers(0, 1 << s)) if s else 0
    d1 = [v ^ (1 << base(top)), v ^ (2 << base(bottom)), v ^ (3 << base(upper)), v ^ (1 << base(lower)), v ^ (3 << base(J // 2))]
    d2 = [v ^ (1 << base(top)) ^ (3 << base(bottom)), v ^ (2 << base(upper)) ^ (1 << base(3)), v ^ (3 << base(top)) ^ (3 << base(1))]
    d3 = [v ^ (1 << base(top)) ^ (2 << base(bottom)) ^ (3 << base(J // 2)), v ^ (3 << base(5)) ^ (3 << base(6)) ^ (3 << base(7)),
          v ^ (1 << base(0)) ^ (1 << base(1)) ^ (1 << base(2))]
    assert len(set(d1)) == 5 and len(set(d2)) == 3 and len(set(d3)) == 3
    near = [(v << s) | low()] + [(y << s) | low() for y in d1 + d2]
    far = [(y << s) | low() for y in d3]
    far += [int(x) for x in rng.integers(0, 1 << 62, size=300, dtype=np.uint64) >> np.uint64(62 - 2 * K if K < 32 else 0)
            if ham(np.array([int(x) >> s], dtype=np.uint64), v)[0] > 3]
    for entries, want in ((near + far, [1, 5, 3]), (near, [1, 5, 3]), (far, [0, 0, 0])):
        kmers = np.unique(np.array(entries, dtype=np.uint64))
        rc, got = entry(ctx, ctx.upload(kmers), K, [(J, v)])
        assert rc == 0 and got.tolist() == [want] and np.array_equal(got, brute(kmers, K, [(J, v)]))


def test_entries_that_differ_only_below_the_window(ctx):
    K, J = 25, 16
    rng = np.random.default_rng(16)
    v = int(rng.integers(0, 1 << 32))
    others = rng.integers(0, 1 << 50, size=500, dtype=np.uint64)
    others = others[ham(others >> np.uint64(18), v) > 2]
    same = (np.uint64(v) << np.uint64(18)) | rng.choice(1 << 18, size=16, replace=False).astype(np.uint64)
    kmers = np.unique(np.concatenate([others, same]))
    rc, got = entry(ctx, ctx.upload(kmers), K, [(J, v), (J, v ^ 1)])
    assert rc == 0 and got.tolist() == [[16, 0, 0], [0, 16, 0]]


def test_every_entry_of_two_tiles_within_distance(ctx):
    """T + 1 entries, all within distance 2 of the window: the tallies add up to n (the flush of both tiles' LDS tallies)"""
    T, _ = consts()
    K, J, n = 25, 13, T + 1
    rng = np.random.default_rng(4097)
    v = int(rng.integers(0, 1 << 26))
    pool = set()
    while len(pool) < n:
        pool.add((substitute(rng, v, J, int(rng.integers(0, 3))) << 24) | int(rng.integers(0, 1 << 24)))
    kmers = np.sort(np.array(sorted(pool), dtype=np.uint64))
    rc, got = entry(ctx, ctx.upload(kmers), K, [(J, v)])
    assert rc == 0 and int(got.sum()) == n and np.array_equal(got, brute(kmers, K, [(J, v)]))
    assert all(int(t) > 0 for t in got[0])


def test_same_call_same_bits_and_a_fresh_context(ctx):
    from zotmer_amd import native
    T, _ = consts()
    windows, kmers = make_problem(31, 25, [25, 13, 1], 65, 3 * T + 17)
    want = brute(kmers, 25, windows)
    d = ctx.upload(kmers)
    first = entry(ctx, d, 25, windows)[1]
    # a call with other windows in between: nothing carries over
    entry(ctx, d, 25, [(1, 0), (1, 3)])
    again = entry(ctx, d, 25, windows)[1]
    assert np.array_equal(first, want) and np.array_equal(again, want)
    with native.Context(0) as fresh:
        assert np.array_equal(entry(fresh, fresh.upload(kmers), 25, windows)[1], want)


def test_bad_arguments_launch_nothing(ctx):
    from zotmer_amd import native
    _, MAXW = consts()
    kmers = ctx.upload(np.arange(100, dtype=np.uint64))
    ctx.profile(True)
    try:
        for K, windows in ((25, [(0, 0)]), (25, [(26, 0)]), (25, [(13, 1), (-1, 0)]), (33, [(25, 0)]), (0, [(1, 0)]),
                           (25, [(13, 1 << 26)]), (25, [(1, 4)]), (32, [(31, 1 << 62)]), (25, [(25, 0)] * (MAXW + 1))):
            rc, _ = entry(ctx, kmers, K, windows)
            assert rc == native.ZK_EINVAL, (K, windows[:2])
            assert b"zk_probe_scan" in ctx.lib.zk_last_error(ctx.h)
        assert "probe_scan" not in ctx.profile_read()
        # the limits themselves are fine, and nothing at all is fine too
        assert entry(ctx, kmers, 32, [(32, (1 << 64) - 1), (1, 3)])[0] == 0
        assert entry(ctx, kmers, 25, [(25, 0)] * MAXW)[0] == 0
        assert ctx.profile_read()["probe_scan"] == dict(launches=2, ms=ctx.profile_read()["probe_scan"]["ms"], bytes=2 * 800)
        rc, t = entry(ctx, kmers, 25, [])
        assert rc == 0 and t.shape == (0, 3)
        rc, t = entry(ctx, None, 25, [(25, 0), (1, 0)], n=0)
        assert rc == 0 and t.tolist() == [[0, 0, 0], [0, 0, 0]]
    finally:
        ctx.profile(False)


def test_wrapper_splits_long_window_lists(ctx):
    _, MAXW = consts()
    windows, kmers = make_problem(9, 6, [6, 3], MAXW + 1, 65)
    got = ctx.probe_scan(ctx.upload(kmers), 6, windows)
    assert got.shape == (MAXW + 1, 3) and got.dtype == np.uint64
    want = brute(kmers, 6, windows)
    assert np.array_equal(got, want) and want[MAXW].sum() > 0 and want[:MAXW].sum() > 0


# ---- the command ----------------------------------------------------------------------------------------------------

def zot(args):
    from zotmer_amd import cli
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        code = cli.main_inner(args)
    return code, out.getvalue(), err.getvalue()


def write_set(path, K, kmers):
    """a k-mer set through the project's own container code"""
    from zotmer_amd.library import vectors
    from zotmer_amd.library.container import KmerSet
    with KmerSet(str(path), "w") as z:
        z.meta = {"K": K, "kmers": len(kmers)}
        vectors.write_kmers_and_counts(z, np.array(kmers, dtype=np.uint64), np.ones(len(kmers), dtype=np.uint64))
    return str(path)


def write_case(d, case):
    pf = d / (case["name"] + ".probes")
    pf.write_text(case["probe_text"])
    return str(pf), write_set(d / (case["name"] + ".k%d" % case["K"]), case["K"], case["kmers"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixture(ctx, tmp_path, case):
    pf, ks = write_case(tmp_path, case)
    code, out, err = zot(["spoligo", "-p", pf, ks])
    assert code == 0 and err == "" and out == ks + "\t" + case["present"] + "\n"
    code, out, err = zot(["spoligo", "-l", "-p", pf, ks])
    assert code == 0 and err == ""
    assert out == "".join("%s\t%s\t%s\n" % (ks, p["name"], b) for p, b in zip(case["probes"], case["present"]))
    assert zot(["spoligo", "-d", "2", "-p", pf, ks])[1] == ks + "\t" + case["present"] + "\n"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_smaller_distances_equal_the_restatement(ctx, tmp_path, case):
    pf, ks = write_case(tmp_path, case)
    seqs = [p["seq"] for p in case["probes"]]
    seen = set()
    for D in (0, 1):
        want = R.spoligo(case["K"], case["kmers"], seqs, D)
        code, out, err = zot(["spoligo", "-d", str(D), "-p", pf, ks])
        assert code == 0 and err == "" and out == ks + "\t" + want + "\n", D
        seen.add(want)
    assert len(seen | {case["present"]}) >= 2          # the bound matters


def test_inputs_of_different_k_and_an_empty_set(ctx, tmp_path):
    a, b = CASES[0], CASES[2]
    assert a["K"] != b["K"]
    pf, ka = write_case(tmp_path, a)
    kb = write_set(tmp_path / "other.k", b["K"], b["kmers"])
    ke = write_set(tmp_path / "empty.k", a["K"], [])
    seqs = [p["seq"] for p in a["probes"]]
    code, out, err = zot(["spoligo", "-p", pf, ka, kb, ke, ka])
    assert code == 0 and err == ""
    line_a = ka + "\t" + a["present"] + "\n"
    assert out == line_a + kb + "\t" + R.spoligo(b["K"], b["kmers"], seqs) + "\n" + ke + "\t" + "0" * len(seqs) + "\n" + line_a
    code, out, _ = zot(["spoligo", "-l", "-p", pf, ke])
    assert out == "".join("%s\t%s\t0\n" % (ke, p["name"]) for p in a["probes"])
