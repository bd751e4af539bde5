"""`zot contigs` on the GPU: zk_debruijn_links against a NumPy brute force (searchsorted over the whole array) bit for bit, at
sizes around the tile, at both ends of the key range, on skewed sets that stage nothing and on a million keys; zk_contig_render
against the restatement's text; the command against the reference's fixture (tests/golden/k1_contigs.json); refused input."""
import contextlib
import ctypes as C
import functools
import io
import json
import os
import re

import numpy as np
import pytest

from tests import _contigs_restatement as R
from tests._contigs_cases import make_cases
from tests._contigs_links import NO_LINK, np_links, np_rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = {c["name"]: c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "k1_contigs.json")))}
CASES = make_cases()
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    from zotmer_amd.library import engine
    yield engine.context()
    engine.close()


def tile():
    from zotmer_amd import native
    return native.LINKS_TILE


def test_constants_match_the_header():
    from zotmer_amd import native
    text = open(os.path.join(ROOT, "include", "zotk.h")).read()
    assert int(re.search(r"#define ZK_LINKS_TILE (\d+)", text).group(1)) == tile()
    assert int(re.search(r"#define ZK_NO_LINK (0x[0-9A-Fa-f]+)u", text).group(1), 16) == native.NO_LINK == NO_LINK
    assert int(re.search(r"#define ZK_PROF_LINKS (\d+)", text).group(1)) == native.Context.PROF_TAGS["links"] == 24


# ---- sets ---------------------------------------------------------------------------------------------------------------------

def mask(K):
    return np.uint64((1 << (2 * K)) - 1)


def genome_kmers(K, length, seed, both=True):
    """the ascending distinct k-mers of a random genome (and of its reverse complement: a set closed under rc)"""
    codes = np.random.default_rng(seed).integers(0, 4, size=length, dtype=np.uint64)
    x = np.zeros(length - K + 1, dtype=np.uint64)
    for j in range(K):
        x = (x << np.uint64(2)) | codes[j:j + len(x)]
    if both:
        x = np.concatenate([x, np_rc(K, x)])
    return np.unique(x)


def random_keys(K, n, seed):
    """n distinct random keys below 4^K, ascending (fewer where 4^K is less): not closed under rc"""
    rng = np.random.default_rng(seed)
    if 4 ** K <= 4 * n + 64:
        every = np.arange(4 ** K, dtype=np.uint64)
        return np.sort(rng.choice(every, size=min(n, len(every)), replace=False))
    x = np.unique(rng.integers(0, 1 << 63, size=2 * n + 64, dtype=np.uint64) * np.uint64(2) & mask(K) | rng.integers(0, 2, size=2 * n + 64, dtype=np.uint64))
    return np.sort(rng.choice(x, size=n, replace=False))


def window_entries(K, xs):
    """per tile, the entries of the (at most four) successor windows that the kernel has to look at"""
    x = np.asarray(xs, dtype=np.uint64)
    T, out = tile(), []
    for t0 in range(0, len(x), T):
        seg = x[t0:t0 + T]
        first = seg >> np.uint64(2 * K - 2)
        total = 0
        for b in range(4):
            s = seg[first == b]
            if len(s):
                lo = np.searchsorted(x, (s[0] << np.uint64(2)) & mask(K), side="left")
                hi = np.searchsorted(x, ((s[-1] << np.uint64(2)) & mask(K)) | np.uint64(3), side="right")
                total += int(hi - lo)
        out.append(total)
    return out


def device_links(ctx, K, xs):
    d = ctx.upload(np.asarray(xs, dtype=np.uint64))
    nx, rc = ctx.debruijn_links(d, K)
    return nx.to_host(), rc.to_host()


def check(ctx, K, xs):
    xs = np.asarray(xs, dtype=np.uint64)
    want_next, want_rc = np_links(K, xs)
    got_next, got_rc = device_links(ctx, K, xs)
    assert got_next.dtype == np.uint32 and got_rc.dtype == np.uint32
    assert np.array_equal(got_next, want_next), (K, len(xs), np.flatnonzero(got_next != want_next)[:5])
    assert np.array_equal(got_rc, want_rc), (K, len(xs), np.flatnonzero(got_rc != want_rc)[:5])
    return want_next, want_rc


def sizes():
    T = tile()
    return [0, 1, 2, T - 1, T, T + 1, 3 * T + 5]


@functools.lru_cache(maxsize=None)
def closed_pool(K):
    """a set closed under rc with more than 3 TILE + 5 entries (every K-mer where there are not that many)"""
    if 4 ** K <= 4 * tile():
        return np.arange(4 ** K, dtype=np.uint64)
    return genome_kmers(K, 2 * tile(), seed=K)


# ---- zk_debruijn_links ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 2, 5, 11, 16, 25, 31, 32])
def test_links_on_sets_closed_under_rc(ctx, K):
    """the graph of a genome: most nodes have one successor; the first n entries of the set for the sizes around the tile (cut
    sets are no longer closed: ranks reach n), and the whole set"""
    pool = closed_pool(K)
    linked = 0
    for n in sizes() + [len(pool)]:
        xs = pool[:min(n, len(pool))]
        nxt, rank = check(ctx, K, xs)
        linked += int((nxt != NO_LINK).sum())
        if len(xs) == len(pool) and len(xs):
            assert int(rank.max()) < len(xs) and np.array_equal(np.sort(rank), np.arange(len(xs)))          # closed: rc is a permutation
    assert linked > (tile() if K >= 11 else 0)


def open_subset(K, n, seed):
    """n random keys (2 <= n <= 4^K - 4, K >= 2) that hold rc(AA..AC) but neither AA..AA nor AA..AC, and rc(TT..TG) but
    neither TT..TG nor TT..TT: the first has rank 0 and the second rank n by construction"""
    top = (1 << (2 * K)) - 1
    forced = {int(np_rc(K, [1])[0]), int(np_rc(K, [top - 1])[0])}
    pool = [int(v) for v in random_keys(K, min(n + 6, 4 ** K), seed) if int(v) not in (0, 1, top - 1, top) and int(v) not in forced]
    return np.array(sorted(forced | set(pool[:n - 2])), dtype=np.uint64)


@pytest.mark.parametrize("K", [1, 2, 5, 11, 16, 25, 31, 32])
def test_links_on_random_subsets(ctx, K):
    """not closed under rc: the ranks include 0 and n"""
    for n in sizes():
        check(ctx, K, random_keys(K, n, seed=1000 * K + n))
        if K >= 2 and n >= 2:
            xs = open_subset(K, min(n, 4 ** K - 4), seed=2000 * K + n)
            assert len(xs) == min(n, 4 ** K - 4)
            _, rank = check(ctx, K, xs)
            assert (rank == 0).any() and (rank == len(xs)).any()


def test_links_where_every_kmer_is_present(ctx):
    xs = np.arange(4 ** 6, dtype=np.uint64)
    nxt, rank = check(ctx, 6, xs)
    assert (nxt == NO_LINK).all() and len(xs) == 4 * tile()
    # ... and with three of every four successors taken out: everything links
    xs = np.arange(0, 4 ** 6, 4, dtype=np.uint64)
    nxt, _ = check(ctx, 6, xs)
    assert (nxt != NO_LINK).all()


@pytest.mark.parametrize("K", [1, 2, 5, 11, 16, 25, 31, 32])
def test_links_at_the_ends_of_the_key_range(ctx, K):
    top = (1 << (2 * K)) - 1
    xs = {0, top} | {int(v) for v in random_keys(K, min(300, 4 ** K // 2), seed=K)}
    if K >= 2:
        xs |= {1, 2, top - 1, top >> 2, (top >> 2) + 1, top - 3}
    if K == 32:
        # keys whose y0 is 2^64 - 4: the bound y0 | 3 is 2^64 - 1 and y0 + 4 would wrap
        xs |= {(b << 62) | ((1 << 62) - 1) for b in range(4)}
        assert all(((x << 2) & top) == (1 << 64) - 4 for x in ((b << 62) | ((1 << 62) - 1) for b in range(4)))
    xs = np.array(sorted(xs), dtype=np.uint64)
    check(ctx, K, xs)
    # the two ends alone: poly-A and poly-T are their own successors (at K = 1 each has both)
    nxt, rank = check(ctx, K, np.array([0, top], dtype=np.uint64))
    assert nxt.tolist() == ([0, 1] if K > 1 else [NO_LINK, NO_LINK]) and rank.tolist() == [1, 0]


def test_links_when_all_keys_begin_with_one_base(ctx):
    K = 11
    pool = genome_kmers(K, 8 * tile(), seed=5)
    for b in (0, 2, 3):
        xs = pool[(pool >> np.uint64(2 * K - 2)) == b]
        assert len(xs) > 3 * tile()
        nxt, _ = check(ctx, K, xs)
        assert (nxt != NO_LINK).any()


def test_links_when_a_window_is_too_large_to_stage(ctx):
    """sparse keys under first base A, dense ones elsewhere: the successors of the first tile range over the whole set"""
    K, T = 16, tile()
    rng = np.random.default_rng(9)
    quarter = 4 ** (K - 1)
    sparse = (np.arange(T, dtype=np.uint64) * np.uint64(quarter // T)) + rng.integers(0, 1000, size=T, dtype=np.uint64)
    dense = np.uint64(quarter) + rng.integers(0, 3 * quarter, size=12 * T, dtype=np.uint64)
    planted = ((sparse[::3] << np.uint64(2)) & mask(K)) | rng.integers(0, 4, size=len(sparse[::3]), dtype=np.uint64)
    planted = planted[(planted >> np.uint64(2 * K - 2)) != 0]                  # (keep the first tile sparse)
    twins = ((sparse[1::7] << np.uint64(2)) & mask(K))
    twins = twins[(twins >> np.uint64(2 * K - 2)) != 0]
    xs = np.unique(np.concatenate([sparse, dense, planted, twins, twins | np.uint64(1)]))
    w = window_entries(K, xs)
    assert w[0] > 8 * T and min(w[1:]) <= 5 * T                                # the first tile searches in place, others stage
    nxt, _ = check(ctx, K, xs)
    first = nxt[:T]
    assert (first != NO_LINK).sum() > T // 8 and (first == NO_LINK).sum() > T // 8


@functools.lru_cache(maxsize=None)
def million():
    K = 16
    xs = genome_kmers(K, 505000, seed=77)[:1000003]
    assert len(xs) == 1000003
    return K, xs


def test_links_on_a_million_keys(ctx):
    K, xs = million()
    nxt, _ = check(ctx, K, xs)
    assert (nxt != NO_LINK).sum() > 900000
    w = window_entries(K, xs[:64 * tile()])
    assert max(w[:-1]) <= 5 * tile()                                            # ... through the staged path


def test_the_same_call_returns_the_same_bits(ctx):
    K, xs = 25, closed_pool(25)
    a, b = device_links(ctx, K, xs), device_links(ctx, K, xs)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_links_refuse_bad_input_and_leave_the_outputs_alone(ctx):
    from zotmer_amd import native
    good = closed_pool(11)[:2 * tile() + 3].copy()
    n = len(good)
    fill = np.full(n, 0xABCDEF01, dtype=np.uint32)

    def call(xs, K):
        d, nx, rc = ctx.upload(xs), ctx.upload(fill), ctx.upload(fill)
        r = ctx.lib.zk_debruijn_links(ctx.h, d.ptr, len(xs), K, nx.ptr, rc.ptr)
        return r, nx.to_host(), rc.to_host()

    swapped = good.copy()
    swapped[[tile(), tile() + 1]] = swapped[[tile() + 1, tile()]]
    twice = good.copy()
    twice[n - 1] = twice[n - 2]
    beyond = good.copy()
    beyond[n - 1] = np.uint64(1 << 22)                                          # 4^11: one past the largest 11-mer
    for xs, K in ((swapped, 11), (twice, 11), (beyond, 11), (good, 33), (good, 0), (good, -1), (good, 10)):
        r, nx, rc = call(xs, K)
        assert r == native.ZK_EINVAL, K
        assert np.array_equal(nx, fill) and np.array_equal(rc, fill)
    r, nx, rc = call(good, 11)                                                  # the context is as good as before
    want = np_links(11, good)
    assert r == native.ZK_OK and np.array_equal(nx, want[0]) and np.array_equal(rc, want[1])
    # nothing: valid, writes nothing
    d1 = ctx.upload(fill)
    assert ctx.lib.zk_debruijn_links(ctx.h, None, 0, 11, d1.ptr, d1.ptr) == native.ZK_OK and np.array_equal(d1.to_host(), fill)


# ---- zk_contig_render ---------------------------------------------------------------------------------------------------------

def render(ctx, K, xs, paths, out=None):
    d = ctx.upload(np.asarray(xs, dtype=np.uint64))
    nodes = np.array([j for p in paths for j in p], dtype=np.uint32)
    offs = np.cumsum([0] + [len(p) for p in paths]).astype(np.uint64)
    return ctx.contig_render(d, K, ctx.upload(nodes), ctx.upload(offs), out=out).to_host().tobytes().decode("ascii")


def test_render_contigs_of_one_node(ctx):
    for K in (1, 2, 11, 32):
        xs = random_keys(K, 50, seed=K).tolist()
        paths = [[i] for i in range(len(xs))]
        assert render(ctx, K, xs, paths) == R.text_of(K, xs, paths)


@pytest.mark.parametrize("K", [1, 32])
def test_render_at_the_ends_of_k(ctx, K):
    rng = np.random.default_rng(K)
    xs = random_keys(K, 3000, seed=40 + K).tolist()
    paths, at = [], 0
    order = rng.permutation(len(xs)).tolist() * (1 if K == 32 else 300)
    for ln in [1, 2, 3, 64, 65, 255, 256, 257, 1, 100]:
        paths.append(order[at:at + ln])
        at += ln
    assert at <= len(order)
    assert render(ctx, K, xs, paths) == R.text_of(K, xs, paths)


def test_render_a_contig_across_many_workgroups(ctx):
    K = 25
    xs = genome_kmers(K, 80000, seed=3, both=False).tolist()
    rng = np.random.default_rng(4)
    long = rng.integers(0, len(xs), size=64 * 1024 + 777).tolist()
    paths = [[5, 6], long, [len(xs) - 1], long[:300]]
    text = render(ctx, K, xs, paths)
    assert text == R.text_of(K, xs, paths) and len(text.split("\n")[3]) == K + len(long) - 1


def test_render_start_indices_of_one_to_seven_digits(ctx):
    K, xs = million()
    starts = [0, 7, 42, 777, 1234, 54321, 654321, 1000002, 999999, 100000, 99999, 10, 9, 99, 100, 999, 1000, 9999, 10000]
    paths = [[s] + [(s * 31 + j) % len(xs) for j in range(1, 1 + i % 4)] for i, s in enumerate(starts)]
    text = render(ctx, K, xs, paths)
    assert text == R.text_of(K, xs.tolist(), paths)
    assert sorted({len(h) - len(">contig_") for h in text.split("\n")[0::2] if h}) == [1, 2, 3, 4, 5, 6, 7]


def test_render_nothing(ctx):
    from zotmer_amd import native
    d = ctx.upload(np.arange(10, dtype=np.uint64))
    offs = ctx.upload(np.zeros(1, dtype=np.uint64))
    n = C.c_uint64(99)
    fill = np.full(64, 0x5A, dtype=np.uint8)
    out = ctx.upload(fill)
    assert ctx.lib.zk_contig_render(ctx.h, d.ptr, 10, 2, None, 0, offs.ptr, 0, out.ptr, out.n, C.byref(n)) == native.ZK_OK
    assert n.value == 0 and np.array_equal(out.to_host(), fill)


def test_render_capacity_one_byte_short(ctx):
    from zotmer_amd import native
    K = 11
    xs = closed_pool(K)
    paths = [[3, 4, 5], [100], list(range(200, 1500))]
    want = R.text_of(K, xs.tolist(), paths)
    d = ctx.upload(xs)
    nodes = ctx.upload(np.array([j for p in paths for j in p], dtype=np.uint32))
    offs = ctx.upload(np.cumsum([0] + [len(p) for p in paths]).astype(np.uint64))
    n = C.c_uint64(0)
    fill = np.full(len(want) + 8, 0x5A, dtype=np.uint8)
    out = ctx.upload(fill)
    args = (ctx.h, d.ptr, len(xs), K, nodes.ptr, nodes.n, offs.ptr, len(paths), out.ptr)
    assert ctx.lib.zk_contig_render(*args, len(want) - 1, C.byref(n)) == native.ZK_ENOSPC
    assert n.value == len(want) and np.array_equal(out.to_host(), fill)          # the size needed; nothing written
    assert ctx.lib.zk_contig_render(*args, len(want), C.byref(n)) == native.ZK_OK and n.value == len(want)
    got = out.to_host()
    assert got[:len(want)].tobytes().decode() == want and (got[len(want):] == 0x5A).all()
    # the binding grows a buffer that is too small
    small = ctx.empty(10, np.uint8)
    assert render(ctx, K, xs, paths, out=small) == want


def test_render_refuses_damaged_arrays(ctx):
    from zotmer_amd import native
    K, xs = 11, closed_pool(11)[:500]
    d = ctx.upload(xs)
    n = C.c_uint64(0)
    out = ctx.empty(4096, np.uint8)
    for nodes, offs in (([1, 2, 500], [0, 3]), ([1, 2, 3], [0, 2]), ([1, 2, 3], [1, 3]), ([1, 2, 3], [0, 2, 2, 3]), ([1, 2, 3], [0, 2, 1, 3]),
                        ([1, 2, 3], [0, 4])):
        dn, do = ctx.upload(np.array(nodes, dtype=np.uint32)), ctx.upload(np.array(offs, dtype=np.uint64))
        r = ctx.lib.zk_contig_render(ctx.h, d.ptr, len(xs), K, dn.ptr, len(nodes), do.ptr, len(offs) - 1, out.ptr, out.n, C.byref(n))
        assert r == native.ZK_EINVAL, (nodes, offs)
    assert render(ctx, K, xs, [[1, 2], [3]]) == R.text_of(K, xs.tolist(), [[1, 2], [3]])


# ---- links, walk and text together -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 3, 4, 11, 32])
def test_the_three_stages_reproduce_the_restatement(ctx, K):
    """also K < 5, where the reference dies: the same definitions"""
    from zotmer_amd.library import debruijn
    xs = closed_pool(K) if K >= 11 else random_keys(K, 4 ** K * 3 // 5, seed=K)
    for l in (None, 1, K + 2):
        got = debruijn.contigs_text(ctx, ctx.upload(xs), K, l)
        assert got.decode("ascii") == R.stdout_text(K, xs.tolist(), l), (K, l)


# ---- the command -------------------------------------------------------------------------------------------------------------

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


def write_set(path, K, xs):
    from zotmer_amd.library import vectors
    from zotmer_amd.library.container import KmerSet
    with KmerSet(str(path), "w") as z:
        vectors.write_kmers_and_counts(z, np.array(xs, dtype=np.uint64), np.arange(1, len(xs) + 1, dtype=np.uint64))
        z.meta.update({"K": K, "kmers": "kmers", "counts": "counts"})
    return str(path)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_command_on_the_fixture(ctx, case, tmp_path):
    inp = write_set(tmp_path / "in.k", case["K"], case["kmers"])
    args = ["contigs"] + ([] if case["l"] is None else ["-l", str(case["l"])]) + [inp]
    code, out, err = run(args)
    assert code == 0 and err == ""
    assert out == GOLD[case["name"]]["stdout"]                                  # the reference's bytes
    assert run(args) == (code, out, err)                                        # ... and the same bytes again


def test_command_on_two_inputs(ctx, tmp_path):
    a, b = CASES[0], CASES[2]
    fa, fb = write_set(tmp_path / "a.k", a["K"], a["kmers"]), write_set(tmp_path / "b.k", b["K"], b["kmers"])
    code, out, err = run(["contigs", fa, fb])
    assert code == 0 and err == "" and out == GOLD[a["name"]]["stdout"] + GOLD[b["name"]]["stdout"]
    code, out, err = run(["contigs", fb, fa, fb])
    assert out == GOLD[b["name"]]["stdout"] + GOLD[a["name"]]["stdout"] + GOLD[b["name"]]["stdout"]


def test_command_on_an_empty_set(ctx, tmp_path):
    f = write_set(tmp_path / "e.k", 11, [])
    assert run(["contigs", f]) == (0, "", "")
