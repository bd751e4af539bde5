"""`zot scan` on the device: zk_lcp_resolve against the restatement of the reference's two sequential passes
(tests/_scan_restatement.py: resolve_all), zk_scan_place against its placement loop, both on arrays inside guarded allocations
at element offsets (tests/_frames.py), and the command end to end against the reference's fixture (tests/golden/s1_scan.json)."""
import contextlib
import functools
import io
import json
import math
import os
import re

import numpy as np
import pytest

from tests import _scan_cases as cases
from tests import _scan_restatement as R
from tests._frames import Frame, lead_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "s1_scan.json")
TILE = 256
EINVAL, ERANGE = -1, -7


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    from zotmer_amd.library import engine
    yield engine.context()
    engine.close()


def test_the_tile_and_the_tags_are_the_headers():
    from zotmer_amd import native
    text = open(os.path.join(ROOT, "include", "zotk.h")).read()
    assert int(re.search(r"#define ZK_LCP_TILE (\d+)", text).group(1)) == native.LCP_TILE == TILE
    assert int(re.search(r"#define ZK_PROF_LCP_RESOLVE (\d+)", text).group(1)) == native.Context.PROF_TAGS["lcp_resolve"] == 32
    assert int(re.search(r"#define ZK_PROF_SCAN_PLACE (\d+)", text).group(1)) == native.Context.PROF_TAGS["scan_place"] == 33


# ---- zk_lcp_resolve ---------------------------------------------------------------------------------------------------------------

PLACEMENTS = ("P0", "P1", "P2", "P3")


def resolve_on_device(ctx, K, S, X, placement):
    """the call on framed arrays -> (rc, L, Y); guards and inputs checked untouched"""
    fS = Frame(ctx, np.array(S, dtype=np.uint64), lead_of("u64", placement))
    fX = Frame(ctx, np.array(X, dtype=np.uint64), lead_of("u64", placement))
    fL = Frame.output(ctx, np.uint8, len(S), lead_of("byte", placement, output=True))
    fY = Frame.output(ctx, np.uint64, len(S), lead_of("u64", placement, output=True))
    rc = ctx.lib.zk_lcp_resolve(ctx.h, fS.arr.ptr, len(S), fX.arr.ptr, len(X), K, fL.arr.ptr, fY.arr.ptr)
    assert fS.unchanged() and fX.unchanged()
    assert fL.outside_intact() and fY.outside_intact()
    return rc, fL, fY


def check_resolve(ctx, K, S, X, placement):
    rc, fL, fY = resolve_on_device(ctx, K, S, X, placement)
    assert rc == 0, ctx.lib.zk_last_error(ctx.h)
    L, Y = R.resolve_all(K, S, X)
    gotL, gotY = fL.result().tolist(), fY.result().tolist()
    bad = [i for i in range(len(S)) if gotL[i] != L[i] or gotY[i] != Y[i]]
    assert not bad, (len(bad), bad[:5], [(gotL[i], L[i], gotY[i], Y[i]) for i in bad[:5]])


SIZES = (1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)


def _random_grid():
    out, seen = [], set()
    for a, K in enumerate((1, 2, 13, 27, 31, 32)):
        for b, nS in enumerate(SIZES):
            nS_ = min(nS, 4 ** K)
            nX = (1, 2, 7, nS_)[(a + b) % 4]
            if (K, nS_, min(nX, 4 ** K)) not in seen:
                seen.add((K, nS_, min(nX, 4 ** K)))
                out.append((K, nS_, nX))
    return out


@pytest.mark.parametrize("K,nS,nX", _random_grid())
def test_resolve_random(ctx, K, nS, nX):
    S, X = cases.random_lists(7 * K + nS, K, nS, nX)
    check_resolve(ctx, K, S, X, PLACEMENTS[(K + nS + nX) % 4])


@pytest.mark.parametrize("K", [13, 27, 31, 32])
@pytest.mark.parametrize("nS", [TILE - 1, TILE + 1, 3 * TILE + 5])
def test_resolve_clustered(ctx, K, nS):
    """pass 2 changes at least 1 entry in 20, and at least 1 in 20 is not the better of the two neighbours (the builder asserts both)"""
    S, X = cases.clustered_lists(100 * K + nS, K, nS, nS)
    check_resolve(ctx, K, S, X, PLACEMENTS[(K + nS) % 4])


@pytest.mark.parametrize("K", [13, 27])
@pytest.mark.parametrize("nX", [1, 2, 7])
def test_resolve_clustered_against_a_short_sample(ctx, K, nX):
    S, _ = cases.clustered_lists(31 * K, K, 2 * TILE + 3, 2 * TILE)
    _, X = cases.random_lists(K + nX, K, 1, nX)
    check_resolve(ctx, K, S, X, "P1")


@pytest.mark.parametrize("shape", ["S above X", "S below X", "S equals X", "disjoint first bases", "disjoint first bases, 0 in X"])
@pytest.mark.parametrize("K,n", [(2, 3), (13, TILE + 1), (27, 3 * TILE + 5), (32, TILE)])
def test_resolve_shapes(ctx, shape, K, n):
    if K == 2 and shape.startswith("disjoint"):
        n = 2
    S, X = cases.shaped_lists(shape, K, n, TILE)
    check_resolve(ctx, K, S, X, "P3")


@pytest.mark.parametrize("K", [13, 27, 32])
@pytest.mark.parametrize("brk", [3 * TILE, 4 * TILE - 1], ids=["break on a tile's first entry", "break on a tile's last entry"])
def test_resolve_a_value_carried_over_whole_tiles(ctx, K, brk):
    S, X = cases.long_carry(K, brk)
    check_resolve(ctx, K, S, X, "P2")


def test_resolve_a_value_carried_over_256_tiles_at_once(ctx):
    """the walk steps over a whole group of 256 tiles only from an index that is a multiple of 65536: one carried run that
    crosses two such indices and stops behind the second"""
    S, X = cases.long_carry(27, 2 * 65536 + 777)
    check_resolve(ctx, 27, S, X, "P1")


@pytest.mark.parametrize("K", [13, 27, 32])
def test_resolve_the_degenerate_two_element_sample(ctx, K):
    S, X = cases.shaped_lists("two-element X", K, 4 * TILE, TILE)
    check_resolve(ctx, K, S, X, "P0")


def test_resolve_argument_rules(ctx):
    S, X = cases.random_lists(3, 13, 40, 9)
    rc, fL, fY = resolve_on_device(ctx, 13, S, [], "P1")
    assert rc == EINVAL and fL.unchanged() and fY.unchanged()
    for K in (0, 33, -1):
        rc, fL, fY = resolve_on_device(ctx, K, S, X, "P1")
        assert rc == EINVAL and fL.unchanged() and fY.unchanged()
    rc, fL, fY = resolve_on_device(ctx, 13, [], X, "P1")
    assert rc == 0
    assert ctx.lib.zk_lcp_resolve(ctx.h, None, 0, None, 0, 13, None, None) == 0
    fS = Frame(ctx, np.array(S, dtype=np.uint64), 1)
    assert ctx.lib.zk_lcp_resolve(ctx.h, fS.arr.ptr, 1 << 32, fS.arr.ptr, 5, 13, fS.arr.ptr, fS.arr.ptr) == ERANGE and fS.unchanged()


def test_resolve_returns_the_same_bits(ctx):
    S, X = cases.clustered_lists(2731, 27, 3 * TILE + 5, 3 * TILE)
    a = resolve_on_device(ctx, 27, S, X, "P0")
    b = resolve_on_device(ctx, 27, S, X, "P2")
    assert a[0] == b[0] == 0 and np.array_equal(a[1].result(), b[1].result()) and np.array_equal(a[2].result(), b[2].result())


# ---- zk_scan_place ----------------------------------------------------------------------------------------------------------------

def place_frames(ctx, c, placement):
    K, slots = c["K"], c["slots"]
    off = np.concatenate(([0], np.cumsum(slots))).astype(np.uint64)
    f = dict(L=Frame(ctx, np.array(c["L"], dtype=np.uint8), lead_of("byte", placement)),
             Y=Frame(ctx, np.array(c["Y"], dtype=np.uint64), lead_of("u64", placement)),
             T=Frame(ctx, np.array(c["T"], dtype=np.uint32), lead_of("u32", placement)),
             U=Frame(ctx, np.array(c["U"], dtype=np.uint32), lead_of("u32", placement)),
             V=Frame(ctx, np.array(c["V"], dtype=np.int32).view(np.uint32), lead_of("u32", placement)),
             off=Frame(ctx, np.array(c.get("off", off), dtype=np.uint64), lead_of("u64", placement)),
             P=Frame.output(ctx, np.uint64, int(off[-1]), lead_of("u64", placement, output=True)),
             Q=Frame.output(ctx, np.uint8, int(off[-1]), lead_of("byte", placement, output=True)),
             cnt=Frame.output(ctx, np.uint32, len(slots) * (K + 1), lead_of("u32", placement, output=True)))
    return f


def place_on_device(ctx, c, placement):
    f = place_frames(ctx, c, placement)
    rc = ctx.lib.zk_scan_place(ctx.h, f["L"].arr.ptr, f["Y"].arr.ptr, len(c["L"]), f["T"].arr.ptr, f["U"].arr.ptr, f["V"].arr.ptr, len(c["U"]),
                               f["off"].arr.ptr, len(c["slots"]), c["K"], f["P"].arr.ptr, f["Q"].arr.ptr, f["cnt"].arr.ptr)
    for nm in ("L", "Y", "T", "U", "V", "off"):
        assert f[nm].unchanged(), nm
    for nm in ("P", "Q", "cnt"):
        assert f[nm].outside_intact(), nm
    return rc, f


def check_place(ctx, c, placement):
    rc, f = place_on_device(ctx, c, placement)
    assert rc == 0, ctx.lib.zk_last_error(ctx.h)
    K, slots = c["K"], c["slots"]
    P, Q, cnt = R.place(K, c["L"], c["Y"], c["T"], c["U"], c["V"], slots)
    assert f["P"].result().tolist() == [x for r in P for x in r]
    assert f["Q"].result().tolist() == [x for r in Q for x in r]
    got = f["cnt"].result().reshape(len(slots), K + 1)
    assert got.tolist() == cnt
    assert got.sum(axis=1).tolist() == np.bincount(np.array(c["U"], dtype=np.int64), minlength=len(slots)).tolist()


@pytest.mark.parametrize("K", [27, 32, 4, 1])
@pytest.mark.parametrize("n_rec", [1, 2, 300])
def test_place_random(ctx, K, n_rec):
    """records of K, K + 1 and K + 70 bases: ties between the strands won by either side, both L equal to 0, slots without entries,
    reverse palindromes at even K (the builder asserts them where the case has 60 slots or more)"""
    slots = [(1, 2, 71)[(n + n_rec) % 3] for n in range(n_rec)]
    if n_rec <= 2:
        slots[-1] = 71
    c = cases.place_case(1000 * K + n_rec, K, slots, nS=max(3, sum(slots) // 2))
    check_place(ctx, c, PLACEMENTS[(K + n_rec) % 4])


@pytest.mark.parametrize("n_entries", [TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_place_entry_counts_around_the_tile(ctx, n_entries):
    c = cases.place_case(n_entries, 27, [400, 2000, 7], nS=900, density=1.0, pairs=1.0)
    assert len(c["U"]) > n_entries
    c["U"], c["V"] = c["U"][:n_entries], c["V"][:n_entries]
    c["T"] = [min(t, n_entries) for t in c["T"]]
    check_place(ctx, c, "P1")


def test_place_all_l_zero_and_no_entries(ctx):
    check_place(ctx, cases.place_case(5, 27, [71, 1, 2], nS=40, max_l=0), "P2")
    c = cases.place_case(6, 27, [71, 3], nS=10)
    c.update(T=[0] * 11, U=[], V=[])
    check_place(ctx, c, "P3")
    check_place(ctx, dict(K=27, L=[], Y=[], T=[0], U=[], V=[], slots=[5]), "P1")


def test_place_ties_between_strands_by_rank(ctx):
    """one slot, a forward and a reverse entry under two k-mers with the same L: the lower rank wins whichever strand it is;
    under ONE k-mer the order within its list decides"""
    K, y0, y1 = 32, 0x0123456789ABCDEF, 0xFEDCBA9876543210
    for V, want in (([1, -1], y0), ([-1, 1], R.rc(K, y0))):
        c = dict(K=K, L=[9, 9], Y=[y0, y1], T=[0, 1, 2], U=[0, 0], V=V, slots=[1])
        rc, f = place_on_device(ctx, c, "P1")
        assert rc == 0 and f["P"].result().tolist() == [want] and f["Q"].result().tolist() == [9]
        c = dict(K=K, L=[9, 3], Y=[y0, y1], T=[0, 2, 2], U=[0, 0], V=V, slots=[1])
        rc, f = place_on_device(ctx, c, "P2")
        assert rc == 0 and f["P"].result().tolist() == [want] and f["Q"].result().tolist() == [9]
        check_place(ctx, c, "P3")


@pytest.mark.parametrize("what", ["record", "position", "position 0", "T descends", "T short of the entries", "T from 1", "L above K",
                                  "offsets descend", "offsets from 1", "K"])
def test_place_refusals_write_nothing(ctx, what):
    c = cases.place_case(77, 27, [71, 2, 1], nS=30)
    j = len(c["U"]) // 2
    if what == "record":
        c["U"][j] = 3
    elif what == "position":
        c["V"][j] = -(c["slots"][c["U"][j]] + 1)
    elif what == "position 0":
        c["V"][j] = 0
    elif what == "T descends":
        i = next(i for i in range(1, 30) if c["T"][i] < c["T"][i + 1])
        c["T"][i] = c["T"][i + 1] + 1
    elif what == "T short of the entries":
        c["T"][-1] -= 1
    elif what == "T from 1":
        c["T"][0] = 1
    elif what == "L above K":
        c["L"][3] = 28
    elif what == "offsets descend":
        c["off"] = [0, 71, 70, 74]
    elif what == "offsets from 1":
        c["off"] = [1, 71, 73, 74]
    elif what == "K":
        c["K"] = 33
    rc, f = place_on_device(ctx, c, "P1")
    assert rc == EINVAL, what
    for nm in ("P", "Q", "cnt"):
        assert f[nm].unchanged(), (what, nm)


# ---- the command ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def golden():
    inputs = {c["name"]: c for c in cases.golden_cases()}
    return [dict(inputs[g["name"]], gold=g) for g in json.load(open(GOLD))]


def run_cli(args):
    from zotmer_amd import cli
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        code = cli.main_inner(args)
    return code, out.getvalue(), err.getvalue()


def same_lines(got, want):
    """identical but for the three '%g' columns, which may differ by one unit of the sixth significant digit"""
    assert len(got) == len(want), (got, want)
    for a, b in zip(got, want):
        a, b = a.split("\t"), b.split("\t")
        assert len(a) == len(b) == 8
        for col, (x, y) in enumerate(zip(a, b)):
            if col in (3, 4, 5) and x != y:
                fx, fy = float(x), float(y)
                unit = 10.0 ** (math.floor(math.log10(max(abs(fx), abs(fy)))) - 5)
                assert abs(fx - fy) <= unit * 1.0000001, (col, x, y)
            else:
                assert x == y, (col, x, y)
    return True


@pytest.mark.parametrize("k", range(2))
def test_the_command_against_the_fixture(ctx, k, tmp_path):
    from tests._scan_files import write_fasta, write_set
    case = golden()[k]
    g = case["gold"]
    genes = str(tmp_path / "genes")
    code, out, _ = run_cli(["scan", "-X", genes] + write_fasta(tmp_path, case))
    assert code == 0 and out == ""
    from zotmer_amd.library.container import Container
    with Container(genes, "r") as z:
        assert json.loads(z.read("__meta__").decode()) == g["meta"]
        for n in "STUV":
            assert z.read(n).hex() == g["members"][n], n
    sets = [write_set(tmp_path / (nm + ".k"), 27, acgt, X) for nm, acgt, X in case["samples"]]
    code, out, err = run_cli(["scan", "-A", genes] + sets)
    assert code == 0
    want = [l for nm in g["inputs"] for l in g["stdout"][nm]]
    assert same_lines(out.splitlines(), want)
    assert err.startswith("loading...\ndone.\ng = ") and err.count("g = ") == len(sets)
