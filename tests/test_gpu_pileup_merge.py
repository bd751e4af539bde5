"""zk_pileup_merge, zk_narrow_counts and alufinder.DevicePileup on the GPU, against the numpy restatement
(tests/_pileup_merge_cases.py) as exact arrays: sizes around the tile with each side empty, six layouts of the two lists, an equal
pair across every tile boundary (and one element either way), the comparison order at the ends of both key fields, counts that
carry and wrap, both widths of B's counts, capacities and refusals; the accumulator against the host Pileup, with and without
the handover to the host; then the four commands that use it, every fixture case through `run` with a host Pileup and with the
default, in batches small enough for several merges.  Every device array of every entry call is a view at an odd element offset
of a larger guarded array; guards and inputs are checked after every call."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from tests import _pileup_merge_cases as M
from zotmer_amd import native
from zotmer_amd.library import alufinder as A

pytestmark = pytest.mark.gpu

T = native.PILEUP_MERGE_TILE
OK, EINVAL, ENOSPC = native.ZK_OK, native.ZK_EINVAL, native.ZK_ENOSPC
G32, G64 = 0xABCDABCD, 0xABCDABCDABCDABCD
SIZES = (0, 1, 2, T - 1, T, T + 1, 3 * T + 5)
U32, U64 = np.uint32, np.uint64


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    from zotmer_amd.library import engine
    yield engine.context()
    engine.close()


@pytest.fixture(scope="module")
def uni():
    return M.universe(4096)          # 32 768 keys: room for two lists of 3 T + 5


# ---- one call on guarded views --------------------------------------------------------------------------------------------------
def guarded(ctx, a, lead, room=7):
    a = np.asarray(a)
    g = G64 if a.dtype.itemsize == 8 else G32
    host = np.concatenate((np.full(lead, g, a.dtype), a, np.full(room, g, a.dtype)))
    return host, ctx.upload(host)


def at(dev, lead):
    return dev.ptr + lead * dev.dtype.itemsize


def call(ctx, a, b, cap, bits=None, room=7):
    """zk_pileup_merge(a, b) into guarded arrays of cap entries -> (rc, n_out, (oc, ok, on) as written); every array a view at an
    odd offset; the guards and the inputs are checked here"""
    bits = 8 * np.asarray(b[2]).dtype.itemsize if bits is None else bits
    ins = [guarded(ctx, v, lead) for v, lead in zip(tuple(a) + tuple(b), (1, 3, 5, 3, 5, 1))]
    outs = [guarded(ctx, np.full(cap, G64 if dt == U64 else G32, dt), lead) for dt, lead in ((U32, 5), (U64, 1), (U64, 3))]
    got = C.c_uint64(12345)
    leads = (1, 3, 5, 3, 5, 1)
    p = [at(d, lead) for (_, d), lead in zip(ins, leads)]
    o = [at(d, lead) for (_, d), lead in zip(outs, (5, 1, 3))]
    rc = ctx.lib.zk_pileup_merge(ctx.h, p[0], p[1], p[2], len(a[0]), p[3], p[4], p[5], bits, len(b[0]), o[0], o[1], o[2], cap, C.byref(got))
    for h, d in ins:
        assert np.array_equal(d.to_host(), h)                               # inputs are left as they are
    wrote = got.value if rc == OK else 0
    res = []
    for (h, d), lead in zip(outs, (5, 1, 3)):
        v = d.to_host()
        g = G64 if v.dtype.itemsize == 8 else G32
        assert np.all(v[:lead] == g) and np.all(v[lead + wrote:] == g), rc      # a refusal writes nothing at all
        res.append(v[lead:lead + wrote])
    return rc, got.value, tuple(res)


def check(ctx, a, b):
    """with exactly the room the union needs: the restatement's arrays"""
    want = M.merge_lists(a, b)
    rc, n, got = call(ctx, a, b, len(want[0]))
    assert (rc, n) == (OK, len(want[0])), (rc, n, len(want[0]), ctx.lib.zk_last_error(ctx.h))
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    return want


def test_header_and_binding_agree():
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zotk.h")).read()
    assert int(re.search(r"#define ZK_PILEUP_MERGE_TILE (\d+)", text).group(1)) == T


# ---- sizes and layouts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", M.LAYOUTS)
def test_sizes_around_the_tile_in_every_layout(ctx, uni, name, bits):
    """every (na, nb) of SIZES x SIZES: each side empty, both empty, one tile exactly, one more, several tiles"""
    rng = np.random.default_rng(1000 + 7 * M.LAYOUTS.index(name) + bits)
    for na in SIZES:
        for nb in SIZES:
            a, b = M.layout(uni, name, na, nb, rng, bits)
            want = check(ctx, a, b)
            if name == "equal":
                assert len(want[0]) == na
            if name == "disjoint":
                assert len(want[0]) == na + nb


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("shift", [-1, 0, 1])
def test_an_equal_pair_across_every_tile_boundary(ctx, uni, shift, bits):
    """4 tiles; for t = 1, 2, 3 merged input t T - 1 is an A element and input t T its B twin (shift 0): the pair belongs to tile
    t - 1, which reads the twin through its halo, and tile t drops its first B element.  Shifted by one either way the pair lies
    inside one tile."""
    rng = np.random.default_rng(50 + shift + bits)
    a, b = M.boundary_pairs(uni, T, 4, shift, rng, bits)
    want = check(ctx, a, b)
    assert len(want[0]) == 4 * T + shift - 3
    if bits == 64:                      # the lists in each other's place: the same cut, the other list's elements end the tiles
        check(ctx, b, a)


def one(c, x, n, bits=64):
    return np.array(c, U32), np.array(x, U64), np.array(n, U32 if bits == 32 else U64)


def test_comparison_order(ctx):
    """pairs that differ only in the coordinate, only in the k-mer, and (1, 2^63) against (2, 0): a signed or a 64-bit-only
    comparison merges these in another order, which the partition and the walk would both show"""
    top32, top64 = (1 << 32) - 1, (1 << 64) - 1
    cases = [
        (one([1], [1 << 63], [5]), one([2], [0], [6])),
        (one([0, 1 << 31], [9, 9], [1, 2]), one([(1 << 31) - 1, top32], [9, 9], [3, 4])),
        (one([1 << 31], [5], [1]), one([0, top32], [5, 5], [2, 3])),
        (one([7, 7], [0, 1 << 63], [1, 2]), one([7, 7], [(1 << 63) - 1, top64], [3, 4])),
        (one([7], [1 << 63], [1]), one([7, 7], [0, top64], [2, 3])),
        (one([0, 1 << 31, top32], [top64, 1 << 63, 0], [1, 2, 3]), one([0, 1 << 31, top32], [0, 1 << 63, top64], [4, 5, 6])),
        (one([0], [0], [1]), one([0], [0], [2])),
        (one([top32], [top64], [1]), one([top32], [top64], [2])),
    ]
    for a, b in cases:
        for x, y in ((a, b), (b, a)):
            want = check(ctx, x, y)
            keys = list(zip(want[0].tolist(), want[1].tolist()))
            assert keys == sorted(keys)
            check(ctx, x, (y[0], y[1], y[2].astype(U32)))


def test_counts_carry_and_wrap(ctx):
    key = ([3], [1 << 40])
    want = check(ctx, one(*key, [1]), one(*key, [0xFFFFFFFF], bits=32))          # a carry into the high word
    assert want[2].tolist() == [1 << 32]
    want = check(ctx, one(*key, [(1 << 40) + 3]), one(*key, [0xFFFFFFFF], bits=32))
    assert want[2].tolist() == [(1 << 40) + 3 + 0xFFFFFFFF]
    want = check(ctx, one(*key, [(1 << 64) - 1]), one(*key, [2]))                # modulo 2^64
    assert want[2].tolist() == [1]
    want = check(ctx, one(*key, [1 << 63]), one(*key, [(1 << 63) + 9]))
    assert want[2].tolist() == [9]
    want = check(ctx, one(*key, [0]), one(*key, [0], bits=32))
    assert want[2].tolist() == [0]


@pytest.mark.parametrize("bits", [32, 64])
def test_capacities(ctx, uni, bits):
    rng = np.random.default_rng(77 + bits)
    a, b = M.layout(uni, "interleaved", T + 1, 3 * T + 5, rng, bits)
    want = M.merge_lists(a, b)
    need = len(want[0])
    assert need < len(a[0]) + len(b[0])
    for cap in (0, 1, need - 1):
        rc, n, _ = call(ctx, a, b, cap)
        assert (rc, n) == (ENOSPC, need), cap                                   # ... and call() saw that nothing was written
        assert b"zk_pileup_merge" in ctx.lib.zk_last_error(ctx.h)
    for cap in (need, need + 1):
        rc, n, got = call(ctx, a, b, cap)                                       # repeated with room
        assert (rc, n) == (OK, need)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)


def test_einval_before_any_launch(ctx, uni):
    rng = np.random.default_rng(3)
    a, b = M.layout(uni, "interleaved", 10, 10, rng, 32)
    for bits in (16, 0, 33, -32):
        rc, n, _ = call(ctx, a, b, 20, bits=bits)
        assert rc == EINVAL, bits
    rc = ctx.lib.zk_pileup_merge(ctx.h, None, None, None, 0, None, None, None, 32, 0, None, None, None, 0, None)
    assert rc == EINVAL
    n = C.c_uint64(9)
    assert ctx.lib.zk_pileup_merge(ctx.h, None, None, None, 0, None, None, None, 64, 0, None, None, None, 0, C.byref(n)) == OK and n.value == 0


def test_the_binding_and_the_profile_record(ctx, uni):
    rng = np.random.default_rng(8)
    a, b = M.layout(uni, "interleaved", 3 * T + 5, T + 1, rng, 32)
    want = M.merge_lists(a, b)
    da, db = tuple(ctx.upload(v) for v in a), tuple(ctx.upload(v) for v in b)
    small = (ctx.empty(10, U32), ctx.empty(10, U64), ctx.empty(10, U64))
    assert ctx.pileup_merge_into(da, db, small) == (len(want[0]), False)
    ctx.profile(True)
    got = ctx.pileup_merge(da, db, out=small)                                   # grown once
    rec = ctx.profile_read()
    ctx.profile(False)
    for g, w in zip(got, want):
        assert np.array_equal(g.to_host(), w)
    na, nb, m = len(a[0]), len(b[0]), len(want[0])
    assert rec["pileup_merge"]["launches"] == 2                                 # the refusal and the call with room: one record each
    assert rec["pileup_merge"]["bytes"] == 2 * 12 * (na + nb) + 20 * na + 16 * nb + 20 * m
    # a merged list is a valid A and a valid B (u64 counts)
    again = ctx.pileup_merge(got, got)
    assert np.array_equal(again[2].to_host(), want[2] * U64(2)) and np.array_equal(again[1].to_host(), want[1])


# ---- zk_narrow_counts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 70001])
def test_narrow_counts(ctx, n):
    rng = np.random.default_rng(n)
    edges = np.array([0, (1 << 32) - 1, 1 << 32, (1 << 64) - 1, 1, (1 << 32) + 1], dtype=U64)
    for top in ((1 << 64) - 1, 1 << 32, (1 << 32) - 1, 0):
        pool = edges[edges <= U64(top)]
        v = pool[rng.integers(0, len(pool), size=n)]
        if n:
            v[rng.integers(0, n)] = top
        hi, di = guarded(ctx, v, 3)
        ho, do = guarded(ctx, np.full(n, G32, U32), 1)
        mx = C.c_uint64(777)
        assert ctx.lib.zk_narrow_counts(ctx.h, at(di, 3), at(do, 1), n, C.byref(mx)) == OK
        assert np.array_equal(di.to_host(), hi)
        out = do.to_host()
        assert np.all(out[:1] == G32) and np.all(out[1 + n:] == G32)
        assert np.array_equal(out[1:1 + n], np.minimum(v, U64((1 << 32) - 1)).astype(U32))
        assert mx.value == (int(v.max()) if n else 0)
    narrow, mx = ctx.narrow_counts(ctx.upload(np.array([5, 1 << 33], U64)))
    assert narrow.to_host().tolist() == [5, (1 << 32) - 1] and mx == 1 << 33 and narrow.dtype == U32
    assert ctx.lib.zk_narrow_counts(ctx.h, None, None, 0, None) == EINVAL


# ---- DevicePileup ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lists():
    return M.random_lists(20, 9000, 60000, 21)          # 180 K pairs; from the fourth list on about half of a list's keys are known


def add_all(ctx, pile, lists):
    for c, x, n in lists:
        pile.add_device(ctx.upload(c), ctx.upload(x), ctx.upload(n))


def same(got, want):
    return all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want)) and len(got) == len(want) == 3


def test_device_pileup_is_the_host_pileup(ctx, lists):
    host, dev = A.Pileup(merge_at=1), A.DevicePileup(ctx)
    for c, x, n in lists:
        host.add(c, x, n)
    add_all(ctx, dev, lists)
    want = host.result()
    assert len(want[0]) < 60000 and dev.host is None
    assert same(dev.result(), want) and same(tuple(a.to_host() for a in dev.device_result()), want)
    assert dev.merges == 19 and host.merges >= 19 and dev.pairs == host.pairs == 180000 and dev.merge_seconds > 0
    assert [a.dtype for a in dev.device_result()] == [np.dtype(U32), np.dtype(U64), np.dtype(U64)]
    # a list from the host, and more after a result was taken
    dev.add(*lists[0])
    host.add(*lists[0])
    assert same(dev.result(), host.result()) and dev.merges == 20


@pytest.mark.parametrize("limit", [None, 0], ids=["device", "handed_over"])
def test_device_pileup_first_list_with_u64_counts(ctx, lists, limit):
    """add() as the first call, and add_device with u64 counts first: the first list is copied, not merged, whatever its counts' width"""
    big = (lists[0][0], lists[0][1], lists[0][2].astype(U64) + U64(1 << 32))          # counts that need their high words
    for first in (lists[0], big):
        host = A.Pileup(merge_at=1)
        by_add, by_device = A.DevicePileup(ctx, limit=limit), A.DevicePileup(ctx, limit=limit)
        host.add(*first)
        by_add.add(*first)
        by_device.add_device(ctx.upload(first[0]), ctx.upload(first[1]), ctx.upload(first[2].astype(U64)))
        want = (first[0], first[1], first[2].astype(U64))
        for dev in (by_add, by_device):
            assert same(dev.result(), want) and same(tuple(a.to_host() for a in dev.device_result()), want) and dev.merges == 0
        for l in lists[1:3]:
            host.add(*l)
            by_add.add(*l)
            by_device.add_device(ctx.upload(l[0]), ctx.upload(l[1]), ctx.upload(l[2]))
        for dev in (by_add, by_device):
            assert same(dev.result(), host.result()) and dev.pairs == host.pairs and (dev.host is None) == (limit is None)


def test_device_pileup_hands_over_at_its_byte_limit(ctx, lists):
    sizes, acc = [], ([], [], [])
    for l in lists:
        acc = M.merge_lists(acc, l)
        sizes.append(len(acc[0]))
    limit = 2 * A.DevicePileup.ENTRY_BYTES * sizes[6]          # both triples may hold what the first seven lists come to
    dev = A.DevicePileup(ctx, limit=limit)
    add_all(ctx, dev, lists)
    assert dev.host is not None and 3 <= dev._merges <= 7 and dev.cur is None and dev.alt is None      # after about a third of the lists
    assert same(dev.result(), acc)
    assert dev.merges >= dev._merges + 1 and dev.pairs == 180000          # the host's merges count as well
    up = dev.device_result()                                   # uploaded after a handover
    assert same(tuple(a.to_host() for a in up), acc)
    tiny = A.DevicePileup(ctx, limit=0)                        # no room at all: the host from the first list on
    add_all(ctx, tiny, lists[:3])
    assert tiny.host is not None and tiny._merges == 0 and same(tiny.result(), M.merge_lists(M.merge_lists(lists[0], lists[1]), lists[2]))


def test_device_pileup_empty_and_single(ctx, lists):
    dev = A.DevicePileup(ctx)
    assert 0 < dev.limit <= ctx.mem_info()[1] // 2           # half of what was free when it was created
    assert [len(a) for a in dev.result()] == [0, 0, 0] and [a.n for a in dev.device_result()] == [0, 0, 0]
    assert [a.dtype for a in dev.result()] == [np.dtype(U32), np.dtype(U64), np.dtype(U64)]
    e = (ctx.empty(0, U32), ctx.empty(0, U64), ctx.empty(0, U32))
    dev.add_device(*e)
    assert (dev.merges, dev.pairs, dev.n) == (0, 0, 0)
    add_all(ctx, dev, lists[:1])
    want = (lists[0][0], lists[0][1], lists[0][2].astype(U64))
    assert dev.merges == 0 and same(dev.result(), want) and same(tuple(a.to_host() for a in dev.device_result()), want)
    dev.add_device(*e)
    assert same(dev.result(), want)
    handed = A.DevicePileup(ctx, limit=0)
    assert [len(a) for a in handed.result()] == [0, 0, 0] and [a.n for a in handed.device_result()] == [0, 0, 0]
    add_all(ctx, handed, lists[:1])
    assert handed.host is not None and same(handed.result(), want) and same(tuple(a.to_host() for a in handed.device_result()), want)


# ---- the four commands ---------------------------------------------------------------------------------------------------------------
class CountingPileup(A.Pileup):
    """the host Pileup, counting the lists that are not empty"""
    lists = 0

    def add_device(self, oc, ok, cnt):
        self.lists += 1 if oc.n else 0
        super().add_device(oc, ok, cnt)


def small_batch(paths):
    """a batch size that cuts the inputs into about six batches, never below two of their longest records"""
    longest, size = 0, 0
    for p in paths:
        data = open(p, "rb").read()
        size = max(size, len(data))
        lines = data.split(b"\n")
        longest = max([longest] + [sum(len(l) + 2 for l in lines[i:i + 4]) for i in range(0, len(lines), 4)])
    return max(2 * longest + 64, size // 6)


def both_ways(monkeypatch, module, zot, args):
    """the command line `args` twice, its library `run` given small batches and (1) a host Pileup, (2) the default ->
    [(code, stdout, stderr, stats), ...] and the lists the host Pileup took"""
    orig = module.run
    res, piles = [], []
    for host in (True, False):
        stats = {}

        def run(*a, **kw):
            ba = inspect.signature(orig).bind(*a, **kw)
            ba.arguments["batch"] = small_batch(ba.arguments["inputs"])
            ba.arguments["stats"] = stats
            if host:
                piles.append(CountingPileup())
                ba.arguments["pileup"] = piles[-1]
            assert host or ba.arguments.get("pileup") is None
            return orig(*ba.args, **ba.kwargs)
        monkeypatch.setattr(module, "run", run)
        res.append(zot(args) + (stats,))
        monkeypatch.setattr(module, "run", orig)
    assert len(piles) == 1
    return res, piles[0].lists


def check_both(res, n_lists):
    (code1, out1, err1, st1), (code2, out2, err2, st2) = res
    assert code1 == code2 and code1 in (0, None) and out1 == out2 and err1 == err2
    assert st2["merges"] == max(n_lists - 1, 0)                 # one device merge per list after the first
    return st2["merges"]


# The one fixture case whose reads come to fewer than four counted lists however small the batches are (`uncovered`: no read
# hits a bait, no list at all), with the lists it gives.  Every other case must show three merges or more in its stats.
FEW_LISTS = {("hgvs-find", "uncovered"): 0}


def enough(command, case, n_lists, merges):
    few = FEW_LISTS.get((command, case))
    if few is None:
        assert merges >= 3, (command, case, n_lists, merges)
    else:
        assert n_lists == few < 4, (command, case, n_lists)


def alu_cases():
    from tests import test_gpu_alufinder as TA
    return TA.CASES


@pytest.mark.parametrize("i", range(len(alu_cases())), ids=[c["name"] for c in alu_cases()])
def test_alu_finder_both_ways(ctx, monkeypatch, tmp_path, i):
    from tests import test_gpu_alufinder as TA
    case = TA.CASES[i]
    res, n_lists = both_ways(monkeypatch, A, TA.run, ["alu-finder"] + TA.write_case(case, str(tmp_path)))
    merges = check_both(res, n_lists)
    assert res[1][2] == "" and TA.expected(case)(res[1][1])
    enough("alu-finder", case["name"], n_lists, merges)


def hgvs_cases():
    from tests import test_gpu_hgvsfind as TH
    return TH.cases()


@pytest.mark.parametrize("i", range(len(hgvs_cases())), ids=[c["name"] for c in hgvs_cases()])
def test_hgvs_find_both_ways(ctx, monkeypatch, tmp_path, i):
    from tests import test_gpu_hgvsfind as TH
    from zotmer_amd.library import hgvsfind
    case = TH.cases()[i]
    monkeypatch.chdir(tmp_path)
    res, n_lists = both_ways(monkeypatch, hgvsfind, TH.zot, TH.write_case(tmp_path, case))
    merges = check_both(res, n_lists)
    out = res[1][1]
    assert res[1][2] == ""
    if any(c in out.splitlines()[0].split("\t") for c in TH.FLOAT_COLUMNS):
        assert TH.same_table(out, case["gold"])
    else:
        assert out == case["gold"]
    enough("hgvs-find", case["name"], n_lists, merges)


def stop_cases():
    from tests import test_gpu_stop as TS
    return TS.CASES


@pytest.mark.parametrize("i", range(len(stop_cases())), ids=[c["name"] for c in stop_cases()])
def test_stop_both_ways(ctx, monkeypatch, tmp_path, i):
    from tests import test_gpu_stop as TS
    from zotmer_amd.library import stopscan
    case = TS.CASES[i]
    res, n_lists = both_ways(monkeypatch, stopscan, TS.run, ["stop"] + TS.write_case(case, str(tmp_path)))
    merges = check_both(res, n_lists)
    assert res[1][2] == "" and TS.same_lines(case, res[1][1])
    assert res[1][1] == "".join(l + "\n" for l in TS.R.run(case["K"], case["fasta"], case["inputs"], case["S"]))
    enough("stop", case["name"], n_lists, merges)


def vardyger_cases():
    from tests import test_gpu_vardyger as TV
    return TV.GOLD


@pytest.mark.parametrize("i", range(len(vardyger_cases())), ids=[c["name"] for c in vardyger_cases()])
def test_vardyger_both_ways(ctx, monkeypatch, tmp_path, i):
    from tests import test_gpu_vardyger as TV
    from zotmer_amd.library import vardyger
    gold = TV.GOLD[i]
    case = TV.CASES[gold["name"]]
    res, n_lists = both_ways(monkeypatch, vardyger, TV.zot, ["vardyger", "-v"] + TV.write_case(case, str(tmp_path)))
    merges = check_both(res, n_lists)
    out, err = res[1][1], res[1][2]
    want_cover, want_rows = TV.split_gold(gold["stdout"])
    rows = out.split("\n")[:-1][1:]
    assert sorted(r.split("\t", 1)[1] for r in rows) == sorted(r.split("\t", 1)[1] for r in want_rows)
    assert [r.split("\t")[0] for r in rows] == [str(k + 1) for k in range(len(want_rows))]
    elines = err.split("\n")[:-1]
    assert sorted(l for l in elines if l.startswith("warning: ")) == sorted(gold["stderr"])
    assert [l for l in elines if l == "" or set(l) <= set(".X")] == want_cover
    enough("vardyger", gold["name"], n_lists, merges)
