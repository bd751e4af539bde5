"""`zot hgvs-find` on the device: zk_capture_kmers against the restatement's multiset (tests/_hgvsfind_restatement.py),
zk_path_scan against a numpy brute force, and the command end to end against the reference's fixtures
(tests/golden/h1_hgvsfind.json)."""
import contextlib
import ctypes as C
import functools
import io
import json
import math
import os
import random

import numpy as np
import pytest

from tests import _hgvsfind_restatement as R
from tests._capture_restatement import kmers as kmers_list
from tests._hgvsfind_cases import make_cases

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "h1_hgvsfind.json")
GUARD32, GUARD64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
M1 = 0x5555555555555555


@functools.lru_cache(maxsize=None)
def cases():
    inputs = {c["name"]: c for c in make_cases()}
    return [dict(inputs[g["name"]], gold=g["stdout"]) for g in json.load(open(GOLD))]


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    from zotmer_amd.library import engine
    yield engine.context()
    engine.close()


# ---- zk_capture_kmers ------------------------------------------------------------------------------------------------------

def fastq(seqs, tag):
    return "".join("@%s%d\n%s\n+\n%s\n" % (tag, i, s, "I" * len(s)) for i, s in enumerate(seqs))


@functools.lru_cache(maxsize=None)
def reads_for(K):
    """two mates per read: the line lengths around K and around a step of 64 window starts, N at the first, a middle and the
    last byte and at every K-th byte, lower case and U"""
    rng = random.Random(1000 + K)

    def rnd(n):
        return "".join(rng.choice("ACGT") for _ in range(n))

    def with_n(s, *at):
        return "".join("N" if i in at else c for i, c in enumerate(s))
    m1 = [rnd(n) for n in (max(K - 1, 0), K, 63 + K, 64 + K, 65 + K)]
    m1 += [with_n(rnd(100), 0), with_n(rnd(100), 50), with_n(rnd(100), 99), with_n(rnd(100), *range(K - 1, 100, K)), rnd(150).lower(),
           rnd(70).replace("T", "U"), rnd(130)]
    m2 = [rnd(rng.choice((0, K - 1, K, 64 + K, 90))) for _ in m1]
    m2[-1] = with_n(rnd(140), 3, 70)
    return m1, m2


def expect_kmers(K, pair_words, mates):
    """the multiset as sorted (bait, k-mer) arrays"""
    out = []
    for w in pair_words:
        b, r = int(w) >> 32, int(w) & 0xffffffff
        for m in mates:
            out += [(b, x) for x in kmers_list(K, m[r], True)]
    out.sort()
    return np.array([b for b, _ in out], np.uint32), np.array([x for _, x in out], np.uint64)


def sorted_pairs(baits, kms):
    o = np.lexsort((kms, baits))
    return baits[o], kms[o]


class Reads:
    def __init__(self, ctx, K, single=False):
        self.mates = reads_for(K)[:1] if single else reads_for(K)
        self.texts = [ctx.upload_stream(fastq(m, "r/%d " % i).encode()) for i, m in enumerate(self.mates)]
        self.lines = [ctx.line_ends(t) for t in self.texts]
        self.n = len(self.mates[0])

    def call(self, ctx, pairs, K, out=None):
        t2, l2 = (self.texts[1], self.lines[1]) if len(self.mates) == 2 else (None, None)
        return ctx.capture_kmers(pairs, self.texts[0], self.lines[0], self.n, K, t2, l2, out=out)

    def raw(self, ctx, pairs, K, ob, ok, cap, n_reads=None):
        n = C.c_uint64(0)
        two = len(self.mates) == 2
        rc = ctx.lib.zk_capture_kmers(ctx.h, pairs.ptr, pairs.n, self.texts[0].ptr, self.lines[0].ptr, self.texts[1].ptr if two else None,
                                      self.lines[1].ptr if two else None, self.n if n_reads is None else n_reads, K,
                                      ob.ptr if ob is not None else None, ok.ptr if ok is not None else None, cap, C.byref(n))
        return rc, n.value


def all_pairs(n_reads):
    """every read under bait r % 3, and read 5 under three baits; ascending as zk_capture_hits gives them"""
    words = {((r % 3) << 32) | r for r in range(n_reads)} | {(b << 32) | 5 for b in (0, 1, 2)}
    return np.array(sorted(words), np.uint64)


@pytest.mark.parametrize("K", [1, 25, 31, 32])
@pytest.mark.parametrize("single", [False, True], ids=["paired", "single"])
def test_capture_kmers_against_the_restatement(ctx, K, single):
    rd = Reads(ctx, K, single)
    words = all_pairs(rd.n)
    gb, gk = rd.call(ctx, ctx.upload(words), K)
    wb, wk = expect_kmers(K, words, rd.mates)
    assert len(wb) > 0 and gb.n == len(wb)
    sb, sk = sorted_pairs(gb.to_host(), gk.to_host())
    assert np.array_equal(sb, wb) and np.array_equal(sk, wk)
    # the same call returns the same bits once sorted
    gb2, gk2 = rd.call(ctx, ctx.upload(words), K)
    sb2, sk2 = sorted_pairs(gb2.to_host(), gk2.to_host())
    assert np.array_equal(sb2, sb) and np.array_equal(sk2, sk)


def test_capture_kmers_zero_pairs_one_pair_and_no_window(ctx):
    K = 25
    rd = Reads(ctx, K)
    gb, gk = rd.call(ctx, ctx.upload(np.zeros(0, np.uint64)), K)
    assert gb.n == 0 and gk.n == 0
    one = np.array([(7 << 32) | 2], np.uint64)
    gb, gk = rd.call(ctx, ctx.upload(one), K)
    wb, wk = expect_kmers(K, one, rd.mates)
    sb, sk = sorted_pairs(gb.to_host(), gk.to_host())
    assert np.array_equal(sb, wb) and np.array_equal(sk, wk) and set(wb.tolist()) == {7}
    # read 8 has an N at every K-th byte of mate 1: with single reads it has no window at all
    rs = Reads(ctx, K, single=True)
    gb, gk = rs.call(ctx, ctx.upload(np.array([(1 << 32) | 8, (2 << 32) | 0], np.uint64)), K)     # read 0: K - 1 bytes
    assert gb.n == 0


def test_capture_kmers_on_an_offset_view(ctx):
    K = 25
    rd = Reads(ctx, K)
    words = all_pairs(rd.n)
    big = ctx.upload(np.concatenate([np.full(3, GUARD64, np.uint64), words, np.full(5, GUARD64, np.uint64)]))
    view = big.view(len(words) - 2, offset=4)                   # not 16-byte aligned; the guards and the cut pairs stay out
    gb, gk = rd.call(ctx, view, K)
    wb, wk = expect_kmers(K, words[1:-1], rd.mates)
    sb, sk = sorted_pairs(gb.to_host(), gk.to_host())
    assert np.array_equal(sb, wb) and np.array_equal(sk, wk)
    assert np.array_equal(big.to_host()[3:-5], words)            # the input is left as it is


def test_capture_kmers_capacity_and_errors(ctx):
    from zotmer_amd import native
    K = 25
    rd = Reads(ctx, K)
    words = all_pairs(rd.n)
    pairs = ctx.upload(words)
    wb, wk = expect_kmers(K, words, rd.mates)
    need = len(wb)
    rc, n = rd.raw(ctx, pairs, K, None, None, 0)                 # cap = 0 sizes the output
    assert rc == native.ZK_ENOSPC and n == need
    for cap in (need - 1, need):
        ob, ok = ctx.upload(np.full(need + 16, GUARD32, np.uint32)), ctx.upload(np.full(need + 16, GUARD64, np.uint64))
        rc, n = rd.raw(ctx, pairs, K, ob, ok, cap)
        hb, hk = ob.to_host(), ok.to_host()
        assert np.all(hb[cap:] == GUARD32) and np.all(hk[cap:] == GUARD64), cap
        if cap < need:
            assert rc == native.ZK_ENOSPC and n == need
            continue
        assert rc == native.ZK_OK and n == need
        sb, sk = sorted_pairs(hb[:n], hk[:n])
        assert np.array_equal(sb, wb) and np.array_equal(sk, wk)
    ob, ok = ctx.upload(np.full(need, GUARD32, np.uint32)), ctx.upload(np.full(need, GUARD64, np.uint64))
    for bad_k in (0, 33):
        assert rd.raw(ctx, pairs, bad_k, ob, ok, need)[0] == native.ZK_EINVAL
    assert rd.raw(ctx, pairs, K, ob, ok, need, n_reads=rd.n - 1)[0] == native.ZK_EINVAL      # the last read is none of the batch's
    assert np.all(ob.to_host() == GUARD32) and np.all(ok.to_host() == GUARD64)
    assert rd.raw(ctx, pairs, K, ob, ok, need) == (native.ZK_OK, need)                        # the context stays usable


# ---- zk_path_scan ----------------------------------------------------------------------------------------------------------

def ham_np(a, v):
    z = a ^ np.uint64(v)
    y = (z | (z >> np.uint64(1))) & np.uint64(M1)
    d = np.zeros(len(a), np.uint32)
    for i in range(0, 64, 2):
        d += ((y >> np.uint64(i)) & np.uint64(1)).astype(np.uint32)
    return d


def brute(baits, kms, counts, windows):
    ws, es = [], []
    for w, (b, v, m, h, q) in enumerate(windows):
        hit = (baits == b) & ((kms & np.uint64(m)) == np.uint64(v & m)) & (ham_np(kms, v) <= h) & (counts >= q)
        e = np.nonzero(hit)[0]
        ws.append(np.full(len(e), w, np.uint32))
        es.append(e.astype(np.uint32))
    if not ws:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    return np.concatenate(ws), np.concatenate(es)


def mutate(rng, K, x, d):
    """x with d bases changed; a changed base differs in one bit or in both"""
    for i in rng.sample(range(K), d):
        x ^= rng.choice((1, 2, 3)) << (2 * i)
    return x


def entry_list(rng, K, segments):
    """segments: [(bait, size)] ascending -> (baits, k-mers, counts, {bait: seeds}): every segment is a crowd of neighbours of
    three seeds at distances 0 .. 3 among random k-mers, ascending and distinct"""
    top = 1 << (2 * K)
    B, X, seeds = [], [], {}
    for b, size in segments:
        sd = [rng.randrange(top) for _ in range(3)]
        seeds[b] = sd
        xs = set(sd[:min(size, 3)])
        while len(xs) < size:
            xs.add(mutate(rng, K, rng.choice(sd), rng.randrange(0, min(K, 3) + 1)) if rng.random() < 0.5 and K > 1 else rng.randrange(top))
        B += [b] * size
        X += sorted(xs)
    counts = np.array([rng.choice((1, 2, 3, 9, 10, 11, 50)) for _ in X], np.uint32)
    return np.array(B, np.uint32), np.array(X, np.uint64), counts, seeds


def get_masks(K):
    full = (1 << (2 * K)) - 1
    return [0, full, (1 << (2 * 3)) - 1 if K >= 3 else full, full ^ ((1 << (2 * (K // 2))) - 1)]


def window_list(rng, K, seeds, baits_with_windows):
    wins = []
    masks = get_masks(K)
    for b in baits_with_windows:
        for s in seeds.get(b, [rng.randrange(1 << (2 * K))]):
            for h in (0, 1, 2, K):
                wins.append((b, s, masks[len(wins) % 4], h, rng.choice((0, 1, 10, 11))))
            wins.append((b, mutate(rng, K, s, 1), 0, 1, 0))
    return wins


def scan(ctx, B, X, Cn, K, wins, out=None):
    return ctx.path_scan(ctx.upload(B), ctx.upload(X), ctx.upload(Cn), K, wins, out=out)


def check(ctx, B, X, Cn, K, wins):
    gw, ge = scan(ctx, B, X, Cn, K, wins)
    ww, we = brute(B, X, Cn, wins)
    assert gw.dtype == np.uint32 and ge.dtype == np.uint32
    assert np.array_equal(gw, ww) and np.array_equal(ge, we)
    return len(ww)


def tile_sizes():
    from zotmer_amd import native
    T = native.PATH_TILE
    return [T - 1, T, T + 1, 2 * T + 3]


@pytest.mark.parametrize("which", range(4))
def test_path_scan_sizes_around_the_tile(ctx, which):
    """one bait's segment lies across every tile boundary; bait 1 has windows and no entries, bait 4 entries and no windows"""
    n = tile_sizes()[which]
    K = 25
    rng = random.Random(77 + which)
    segs = [(0, 300), (2, n - 300 - 500 - 7), (4, 500), (6, 7)]
    B, X, Cn, seeds = entry_list(rng, K, segs)
    assert len(B) == n
    wins = window_list(rng, K, seeds, [0, 1, 2, 6, 9])
    assert check(ctx, B, X, Cn, K, wins) > 20


def test_path_scan_small_baits_share_a_tile(ctx):
    K = 21
    rng = random.Random(5)
    segs = [(b, rng.randrange(1, 400)) for b in range(0, 60, 2)]
    B, X, Cn, seeds = entry_list(rng, K, segs)
    wins = window_list(rng, K, seeds, list(range(0, 60)))
    assert check(ctx, B, X, Cn, K, wins) > 100


def test_path_scan_one_window_more_than_a_chunk(ctx):
    from zotmer_amd import native
    K = 25
    rng = random.Random(9)
    B, X, Cn, seeds = entry_list(rng, K, [(3, 700), (5, 5000)])
    base = window_list(rng, K, seeds, [3, 5])
    w5 = [w for w in base if w[0] == 5]
    wins = [w for w in base if w[0] == 3] + [w5[i % len(w5)] for i in range(native.PATH_CHUNK + 1)]
    assert sum(1 for w in wins if w[0] == 5) == native.PATH_CHUNK + 1
    assert check(ctx, B, X, Cn, K, wins) > native.PATH_CHUNK


def test_path_scan_masks_bounds_and_counts(ctx):
    K = 25
    full = (1 << (2 * K)) - 1
    x = 0x123456789ABC & full
    near1 = x ^ (3 << 20)                 # both bits of one base: distance 1
    near1b = x ^ (1 << 48)                # the top base, one bit
    near2 = x ^ (2 << 4) ^ (1 << 30)
    far = x ^ full
    X = np.array(sorted([x, near1, near1b, near2, far]), np.uint64)
    B = np.full(len(X), 4, np.uint32)
    Cn = np.array([10] * len(X), np.uint32)
    at = {int(v): i for i, v in enumerate(X)}

    def hits(win):
        gw, ge = scan(ctx, B, X, Cn, K, [win])
        assert np.all(gw == 0)
        return set(ge.tolist())
    assert hits((4, x, 0, 0, 0)) == {at[x]}
    assert hits((4, x, 0, 1, 0)) == {at[x], at[near1], at[near1b]}
    assert hits((4, x, 0, 2, 0)) == {at[x], at[near1], at[near1b], at[near2]}
    assert hits((4, x, 0, K, 0)) == set(range(len(X)))
    assert hits((4, x, full, K, 0)) == {at[x]}
    low = (1 << (2 * 6)) - 1              # get_mask's low-2(i+1)-bits form: near2 differs below it, near1 and near1b above
    assert hits((4, x, low, K, 0)) == {at[x], at[near1], at[near1b]}
    high = full ^ ((1 << (2 * 12)) - 1)   # ... and its high-bits form: only near1b and near2's upper base differ there
    assert hits((4, x, high, K, 0)) == {at[x], at[near1]}
    assert hits((4, x, 0, K, 10)) == set(range(len(X))) and hits((4, x, 0, K, 11)) == set()
    assert hits((5, x, 0, K, 0)) == set() and hits((3, x, 0, K, 0)) == set()
    # ... against the brute force as well
    for win in [(4, x, m, h, q) for m in (0, full, low, high) for h in (0, 1, 2, K) for q in (10, 11)]:
        assert check(ctx, B, X, Cn, K, [win]) >= 0


def test_path_scan_k32_top_base(ctx):
    K = 32
    x = 0x0123456789ABCDEF
    X = np.array(sorted([x, x ^ (3 << 62), x ^ (1 << 62) ^ 1]), np.uint64)
    B = np.zeros(3, np.uint32)
    Cn = np.ones(3, np.uint32)
    for h, want in ((0, 1), (1, 2), (2, 3), (32, 3)):
        assert check(ctx, B, X, Cn, K, [(0, x, 0, h, 0)]) == want
    assert check(ctx, B, X, Cn, K, [(0, x, 3 << 62, 32, 0)]) == 1
    assert check(ctx, B, X, Cn, K, [(0, x, (1 << 64) - 1, 32, 1)]) == 1


def raw_scan(ctx, dB, dX, dC, K, wins, ow, oe, cap):
    from zotmer_amd import native
    arr = (native.PathWindow * max(len(wins), 1))(*[native.PathWindow(v, m, b, h, q, 0) for b, v, m, h, q in wins])
    n = C.c_uint64(0)
    rc = ctx.lib.zk_path_scan(ctx.h, dB.ptr if dB is not None else None, dX.ptr if dX is not None else None, dC.ptr if dC is not None else None,
                              dB.n if dB is not None else 0, K, arr, len(wins), ow.ptr if ow is not None else None,
                              oe.ptr if oe is not None else None, cap, C.byref(n))
    return rc, n.value


def test_path_scan_empty_inputs_errors_and_capacity(ctx):
    from zotmer_amd import native
    K = 25
    rng = random.Random(3)
    B, X, Cn, seeds = entry_list(rng, K, [(1, 900), (2, 4000)])
    wins = window_list(rng, K, seeds, [1, 2])
    dB, dX, dC = ctx.upload(B), ctx.upload(X), ctx.upload(Cn)
    ww, we = brute(B, X, Cn, wins)
    need = len(ww)
    assert need > 10
    assert raw_scan(ctx, None, None, None, K, wins, None, None, 0) == (native.ZK_OK, 0)        # n = 0
    assert raw_scan(ctx, dB, dX, dC, K, [], None, None, 0) == (native.ZK_OK, 0)                # no windows
    assert raw_scan(ctx, dB, dX, dC, K, wins, None, None, 0) == (native.ZK_ENOSPC, need)       # cap = 0 sizes the output
    for cap in (need - 1, need):
        ow, oe = ctx.upload(np.full(need + 16, GUARD32, np.uint32)), ctx.upload(np.full(need + 16, GUARD32, np.uint32))
        rc, n = raw_scan(ctx, dB, dX, dC, K, wins, ow, oe, cap)
        hw, he = ow.to_host(), oe.to_host()
        if cap < need:
            assert (rc, n) == (native.ZK_ENOSPC, need)
            assert np.all(hw == GUARD32) and np.all(he == GUARD32)                             # nothing written at all
            continue
        assert (rc, n) == (native.ZK_OK, need)
        assert np.array_equal(hw[:n], ww) and np.array_equal(he[:n], we)
        assert np.all(hw[n:] == GUARD32) and np.all(he[n:] == GUARD32)
    # every ZK_EINVAL rule, before any launch: nothing is written
    ow, oe = ctx.upload(np.full(need, GUARD32, np.uint32)), ctx.upload(np.full(need, GUARD32, np.uint32))
    top = 1 << (2 * K)
    bad = [[(2, 0, 0, 0, 0), (1, 0, 0, 0, 0)],            # not ascending by bait
           [(1, top, 0, 0, 0)],                            # a value of 4^K
           [(1, 0, top, 0, 0)]]                            # a mask of 4^K
    for w in bad:
        assert raw_scan(ctx, dB, dX, dC, K, w, ow, oe, need)[0] == native.ZK_EINVAL
    for bad_k in (0, 33):
        assert raw_scan(ctx, dB, dX, dC, bad_k, wins[:1], ow, oe, need)[0] == native.ZK_EINVAL
    assert np.all(ow.to_host() == GUARD32) and np.all(oe.to_host() == GUARD32)
    # the order, and two runs give the same bits
    a = scan(ctx, B, X, Cn, K, wins)
    b = scan(ctx, B, X, Cn, K, wins)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    key = a[0].astype(np.uint64) << np.uint64(32) | a[1].astype(np.uint64)
    assert np.all(key[1:] > key[:-1])


# ---- the command -----------------------------------------------------------------------------------------------------------

def write_case(d, case, index_name="index.json"):
    d.mkdir(parents=True, exist_ok=True)
    (d / index_name).write_text(json.dumps(case["index"]))          # JSON is YAML: no PyYAML needed here
    fns = []
    for i, text in enumerate(case["inputs"]):
        (d / ("in%d.fastq" % i)).write_bytes(text.encode())
        fns.append("in%d.fastq" % i)
    return ["hgvs-find"] + list(case["opts"]) + [index_name] + fns


def zot(args):
    from zotmer_amd import cli
    out, err = io.StringIO(), io.StringIO()
    code = 0
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            code = cli.main_inner(args) or 0
        except SystemExit as e:
            code = e.code
    return code, out.getvalue(), err.getvalue()


FLOAT_COLUMNS = ("wtD", "mutD", "wtQ", "mutQ")


def same_table(got, want):
    """text-identical but for the columns that come from exp / log / pow printed with %g, made with another libm: those may
    differ by one unit in the sixth significant digit"""
    g, w = [l.split("\t") for l in got.splitlines()], [l.split("\t") for l in want.splitlines()]
    assert len(g) == len(w) and g[0] == w[0]
    for a, b in zip(g[1:], w[1:]):
        assert len(a) == len(b)
        for col, x, y in zip(g[0], a, b):
            if col in FLOAT_COLUMNS and x != y:
                fx, fy = float(x), float(y)
                unit = 10.0 ** (math.floor(math.log10(max(abs(fx), abs(fy)))) - 5)
                assert abs(fx - fy) <= unit * 1.0000001, (col, x, y)
            else:
                assert x == y, (col, x, y)
    return True


@pytest.mark.parametrize("case", cases(), ids=[c["name"] for c in cases()])
def test_command_against_the_reference(ctx, tmp_path, monkeypatch, case):
    monkeypatch.chdir(tmp_path)
    code, out, err = zot(write_case(tmp_path, case))
    assert code == 0 and err == ""
    if any(c in out.splitlines()[0].split("\t") for c in FLOAT_COLUMNS):
        assert same_table(out, case["gold"])
    else:
        assert out == case["gold"]


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


def test_batches_and_slices_do_not_matter(ctx, tmp_path, monkeypatch):
    from zotmer_amd.library import hgvsfind
    case = by_name("two_close")
    monkeypatch.chdir(tmp_path)
    args = write_case(tmp_path, case)
    items, variants = hgvsfind.read_index("index.json")
    res = []
    for batch, budget in ((16 << 10, 6000), (64 << 20, hgvsfind.EMIT_BUDGET)):
        out, stats = io.StringIO(), hgvsfind.new_stats()
        hgvsfind.run(ctx, items, variants, args[-2:], 25, 2, 10, 0.05, {"rds", "vaf"}, batch, out, budget=budget, stats=stats)
        res.append((out.getvalue(), stats))
    small, whole_ = res[0][1], res[1][1]
    assert small["batches"] >= 3 and small["slices"] >= 2 * small["batches"]      # every batch's pair list was cut
    assert whole_["batches"] == 1 and whole_["slices"] == 1
    assert small["entries"] == whole_["entries"] and small["read_pairs"] == whole_["read_pairs"] == 260
    assert res[0][0] == res[1][0] == case["gold"]


def test_a_pair_beyond_the_budget_is_refused(ctx, tmp_path, monkeypatch):
    from zotmer_amd.library import hgvsfind
    case = by_name("het_sub")
    monkeypatch.chdir(tmp_path)
    args = write_case(tmp_path, case)
    items, variants = hgvsfind.read_index("index.json")
    with pytest.raises(hgvsfind.InputError, match="more than a call takes"):
        hgvsfind.run(ctx, items, variants, args[-2:], 25, 2, 10, 0.05, {"rds", "vaf"}, 64 << 20, io.StringIO(), budget=100)


def test_unequal_mates_end_the_pair_with_a_warning(ctx, tmp_path, monkeypatch):
    case = dict(by_name("het_sub"))
    m1, m2 = case["inputs"]
    short = "".join(m2.splitlines(True)[:4 * 200])
    monkeypatch.chdir(tmp_path)
    code, out, err = zot(write_case(tmp_path, dict(case, inputs=[m1, short])))
    assert code == 0 and err == "warning: files had unequal length\n"
    assert out == R.find(case["index"], [m1, short])
    code, out2, err = zot(write_case(tmp_path, dict(case, inputs=[short, m1])))                   # mate 1 ends first: no warning
    assert code == 0 and err == "" and out2 == R.find(case["index"], [short, m1])


def test_kmers_come_in_ascending_order_and_o_names_a_file(ctx, tmp_path, monkeypatch):
    case = by_name("two_close")
    monkeypatch.chdir(tmp_path)
    args = write_case(tmp_path, case)
    code, out, err = zot(args[:1] + ["-F", "kmers,rds,vaf", "-o", "table.txt"] + args[1:])
    assert code == 0 and err == ""
    want = R.find(case["index"], case["inputs"], F="kmers,rds,vaf")
    table = [l for l in want.splitlines(True) if not l.split("\t")[1][:1] in "ACGT" or l.startswith("n\t")]
    kms = [l for l in want.splitlines(True) if l not in table]
    assert len(kms) > 2000 and "".join(table) == case["gold"]
    assert out == "".join(kms)                                   # the k-mers go to stdout, ascending by (variant, k-mer)
    assert (tmp_path / "table.txt").read_text() == case["gold"]
    keys = [(int(l.split("\t")[0]), l.split("\t")[1]) for l in out.splitlines()]
    assert keys == sorted(keys)


def test_an_empty_index_and_no_hits(ctx, tmp_path, monkeypatch):
    case = by_name("uncovered")
    monkeypatch.chdir(tmp_path)
    code, out, err = zot(write_case(tmp_path, dict(case, index=[])))
    assert (code, out, err) == (0, "", "")
    code, out, err = zot(write_case(tmp_path, dict(case, opts=["-D", "0"])))
    assert code == 0 and out == R.find(case["index"], case["inputs"], D=0)
    het = by_name("het_sub")
    code, out, err = zot(write_case(tmp_path, dict(het, opts=["-D", "0"])))                       # no candidates at all, as in the reference
    assert code == 0 and out == R.find(het["index"], het["inputs"], D=0) and "\tnull\t" in out
