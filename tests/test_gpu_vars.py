"""`zot vars` on the device: zk_vars_scan against a Python brute force of its definition (include/zotk.h) -- bracketed between the
groups the host flags exactly and the groups that pass the predicate with twice the guard --, at the tile borders, at the
threshold, at the ends of the count range; the command against the reference's fixture (tests/golden/v1_vars.json) and, for
the documented deviations, against the restatement."""
import bisect
import contextlib
import ctypes as C
import functools
import io
import json
import math
import os
import random
import re

import numpy as np
import pytest

from tests import _vars_restatement as R
from tests._vars_cases import make_cases, missing_case
from tests._vars_compare import same_lines

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = {c["name"]: c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "v1_vars.json")))}
CASES = make_cases()
IDS = [c["name"] for c in CASES]
THR = -10.0


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    from zotmer_amd.library import engine
    yield engine.context()
    engine.close()


def tile():
    from zotmer_amd import native
    return native.VARS_TILE


def test_tile_matches_the_header():
    text = open(os.path.join(ROOT, "include", "zotk.h")).read()
    assert int(re.search(r"#define ZK_VARS_TILE (\d+)", text).group(1)) == tile()


# ---- the brute force --------------------------------------------------------------------------------------------------------

def groups_of(pairs):
    """{context: [c0, c1, c2, c3]} and {context: entries} of an ascending (k-mer, count) list"""
    g, n = {}, {}
    for x, c in pairs:
        g.setdefault(x >> 2, [0, 0, 0, 0])[x & 3] = c
        n[x >> 2] = n.get(x >> 2, 0) + 1
    return g, n


@functools.lru_cache(maxsize=None)
def lane_candidates(sx, gx, thr, guards):
    from zotmer_amd.library import varscan
    st, gt = sum(sx), sum(gx)
    return any(varscan.candidate(sx[j], st, gx[j], gt, thr, guards) for j in range(4))


def brute(ref, sam, thr=THR, guards=0.0):
    """(rows [(context, sx, gx)] of the joined groups with >= 2 reference entries and a candidate base, stats as the device
    reports them)"""
    rg, rn = groups_of(ref)
    sg, _ = groups_of(sam)
    rows, missing, mixed = [], [], 0
    for c in sorted(sg):
        if c not in rg:
            missing.append(c)
            continue
        if rn[c] < 2:
            continue
        mixed += 1
        if lane_candidates(tuple(sg[c]), tuple(rg[c]), thr, guards):
            rows.append((c, tuple(sg[c]), tuple(rg[c])))
    return rows, dict(n_groups=len(sg), n_missing=len(missing), first_missing=missing[0] if missing else 0, n_mixed=mixed)


def upload(ctx, pairs, bits):
    keys = np.array([x for x, _ in pairs], dtype=np.uint64)
    cnts = np.array([c for _, c in pairs], dtype=np.uint32 if bits == 32 else np.uint64)
    return ctx.upload(keys), ctx.upload(cnts)


def scan(ctx, ref, sam, K, thr=THR, rbits=64, sbits=64, cap=None):
    rk, rc = upload(ctx, ref, rbits)
    sk, sc = upload(ctx, sam, sbits)
    ctxs, rows, st = ctx.vars_scan(rk, rc, sk, sc, K, thr, cap_rows=cap)
    r = rows.to_host().reshape(-1, 8).tolist()
    got = [(int(c), tuple(x[:4]), tuple(x[4:])) for c, x in zip(ctxs.to_host().tolist(), r)]
    assert st.n_rows == len(got)
    return got, dict(n_groups=st.n_groups, n_missing=st.n_missing, first_missing=st.first_missing, n_mixed=st.n_mixed)


def check_exact(ctx, ref, sam, K, thr=THR, rbits=64, sbits=64):
    """the device's rows are the brute force's, where no base lies between the threshold and twice the guard above it"""
    lower, stats = brute(ref, sam, thr, 0.0)
    upper, _ = brute(ref, sam, thr, 2.0)
    assert lower == upper, "the test's data has a base inside the guard band"
    got, gstats = scan(ctx, ref, sam, K, thr, rbits, sbits)
    assert gstats == stats
    assert got == lower
    return got


# ---- sandwich against the exact values ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def random_lists(K):
    """(reference list, sample list, the contexts the host flags exactly): groups of every size on both sides, sample contexts
    the reference lacks, counts small enough for the exact tail sums"""
    from zotmer_amd.library import varscan
    rng = random.Random(1000 + K)
    space = 1 << (2 * (K - 1))
    n_ctx = min(space, 1400)
    ctxs = sorted(rng.sample(range(space), n_ctx)) if space > 1 << 20 else sorted(rng.sample(range(space), min(space, n_ctx)))
    if K >= 31:
        ctxs = sorted(set(ctxs[1:-1]) | {0, space - 1})
    ref, sam = [], []
    for c in ctxs:
        in_ref = rng.random() < 0.9 or space <= 4
        in_sam = rng.random() < 0.7 or space <= 4
        if in_ref:
            for b in sorted(rng.sample(range(4), rng.randint(2 if space <= 4 else 1, 4))):
                ref.append(((c << 2) | b, rng.choice([1, 1, 2, 5, 25])))
        if in_sam:
            for b in sorted(rng.sample(range(4), rng.randint(1, 4))):
                sam.append(((c << 2) | b, rng.choice([1, 2, 12, 25])))
    rg, rn = groups_of(ref)
    sg, _ = groups_of(sam)
    flagged = [c for c in sorted(sg) if c in rg and varscan.eval_row(sg[c], rg[c], THR)[0] > 0]
    return ref, sam, flagged


@pytest.mark.parametrize("bits", [(32, 32), (64, 64), (32, 64), (64, 32)], ids=lambda b: "ref%d_sam%d" % b)
@pytest.mark.parametrize("K", [1, 2, 13, 31, 32])
def test_rows_between_the_exact_flags_and_the_guarded_predicate(ctx, K, bits):
    ref, sam, flagged = random_lists(K)
    if K == 13:
        assert len(ref) + len(sam) > tile() and len(flagged) > 20
    got, stats = scan(ctx, ref, sam, K, THR, *bits)
    upper, want_stats = brute(ref, sam, THR, 2.0)
    assert stats == want_stats
    cs = [c for c, _, _ in got]
    assert cs == sorted(set(cs))                                        # ascending, one row per group
    assert set(flagged) <= set(cs)                                      # nothing the host would print is lost
    by_ctx = {c: (sx, gx) for c, sx, gx in upper}
    for c, sx, gx in got:                                               # nothing comes back that the predicate cannot explain
        assert c in by_ctx and by_ctx[c] == (sx, gx), c
    if K == 13:
        assert len(got) < stats["n_mixed"]                             # the predicate does select


# ---- tile borders ------------------------------------------------------------------------------------------------------------

BORDER_K = 13


def merged_of(layout, lead):
    """the merged sequence [(k-mer, side, count)] (side 0 = reference, first on equal keys) of a layout, long enough for the
    largest size, after `lead` reference entries of contexts of their own"""
    rng = random.Random(77)
    out = [(x, 0, 7) for x in range(lead)]
    n_ctx = (3 * tile() + 5) // 4 + 8
    for i in range(n_ctx):
        c = 1000 + 3 * i
        if layout == "full4":
            rb, sb = [0, 1, 2, 3], [0, 1, 2, 3]
        else:               # group sizes cycling 1..4, the two lists out of phase: the reference's first bases, the sample's last
            rb, sb = list(range(i % 4 + 1)), list(range(3 - (i + 1) % 4, 4))
        rc = [rng.choice([60, 3, 2, 1]) for _ in rb]
        sc = [rng.choice([1, 2, 30]) for _ in sb]
        ent = [((c << 2) | b, 0, n) for b, n in zip(rb, rc)] + [((c << 2) | b, 1, n) for b, n in zip(sb, sc)]
        out += sorted(ent)
    return out


def lists_of(layout, lead, total):
    m = merged_of(layout, lead)[:total]
    return [(x, n) for x, s, n in m if s == 0], [(x, n) for x, s, n in m if s == 1]


def cuts_of(ref, sam):
    """include/zotk.h: a_t = the reference entries among the first t * tile merged elements, the reference first on ties"""
    T = tile()
    side = [s for _, s in sorted([(x, 0) for x, _ in ref] + [(x, 1) for x, _ in sam])]
    pre = [0]
    for s in side:
        pre.append(pre[-1] + (1 - s))
    return [(pre[min(t * T, len(side))], min(t * T, len(side)) - pre[min(t * T, len(side))]) for t in range(len(side) // T + 2)]


def border_classes(ref, sam):
    """what the tile borders of a pair of lists split: {"sample": offsets into a sample group, "reference": offsets into a
    reference group, "before" / "after": reference entries of a sample group's context that lie before / after the tile that
    holds the group's first entry}"""
    seen = {"sample": set(), "reference": set(), "before": set(), "after": set()}
    cuts = cuts_of(ref, sam)
    rctx, sctx = [x >> 2 for x, _ in ref], [x >> 2 for x, _ in sam]
    for a, b in cuts[1:-1]:
        if 0 < b < len(sam) and sctx[b] == sctx[b - 1]:
            seen["sample"].add(sum(1 for q in range(max(0, b - 3), b) if sctx[q] == sctx[b]))
        if 0 < a < len(ref) and rctx[a] == rctx[a - 1]:
            seen["reference"].add(sum(1 for q in range(max(0, a - 3), a) if rctx[q] == rctx[a]))
    for t in range(len(cuts) - 1):
        (a0, b0), (a1, b1) = cuts[t], cuts[t + 1]
        for q in range(b0, b1):
            if q and sctx[q] == sctx[q - 1]:
                continue
            lo, hi = bisect.bisect_left(rctx, sctx[q]), bisect.bisect_right(rctx, sctx[q])          # the reference group
            seen["before"].add(max(0, min(hi, a0) - lo))
            seen["after"].add(max(0, hi - max(lo, a1)))
    return {k: v - {0} for k, v in seen.items()}


def border_sizes():
    T = tile()
    return [T - 1, T, T + 1, 3 * T + 5]


LEADS = {"full4": range(8), "cycling": range(0, 20)}


def test_the_border_cases_split_what_they_are_for():
    seen = {"sample": set(), "reference": set(), "before": set(), "after": set()}
    for layout in LEADS:
        for lead in LEADS[layout]:
            ref, sam = lists_of(layout, lead, 3 * tile() + 5)
            for k, v in border_classes(ref, sam).items():
                seen[k] |= v
    for k in seen:
        assert {1, 2, 3} <= seen[k], (k, seen[k])
    assert 4 in seen["before"]                  # the whole reference group in the tile before its sample group


@pytest.mark.parametrize("layout", ["full4", "cycling"])
@pytest.mark.parametrize("which", range(4))
def test_tile_borders(ctx, layout, which):
    total = border_sizes()[which]
    rows = 0
    for lead in LEADS[layout]:
        ref, sam = lists_of(layout, lead, total)
        assert len(ref) + len(sam) == total
        rows += len(check_exact(ctx, ref, sam, BORDER_K))
    assert rows > 10 * len(LEADS[layout])


# ---- missing contexts, empty lists -------------------------------------------------------------------------------------------

def test_missing_contexts(ctx):
    m = missing_case()
    got = check_exact(ctx, m["ref"], m["sample"], m["K"])
    assert [c for c, _, _ in got] == [10, 20, 30]
    _, st = scan(ctx, m["ref"], m["sample"], m["K"])
    assert st == dict(n_groups=6, n_missing=3, first_missing=3, n_mixed=3)
    for keep in ([3], [25], [200], [25, 200]):                         # before the first, between two, after the last
        sam = [(x, c) for x, c in m["sample"] if (x >> 2) in keep + [10, 20, 30]]
        _, st = scan(ctx, m["ref"], sam, m["K"])
        assert (st["n_missing"], st["first_missing"]) == (len(keep), keep[0])
    # the context 0 can be the missing one
    _, st = scan(ctx, m["ref"], [(1, 5)] + m["shared"], m["K"])
    assert (st["n_missing"], st["first_missing"], st["n_groups"]) == (1, 0, 4)


def test_empty_lists(ctx):
    m = missing_case()
    got, st = scan(ctx, [], m["sample"], m["K"])
    assert got == [] and st == dict(n_groups=6, n_missing=6, first_missing=3, n_mixed=0)
    for ref in (m["ref"], []):
        got, st = scan(ctx, ref, [], m["K"])
        assert got == [] and st == dict(n_groups=0, n_missing=0, first_missing=0, n_mixed=0)
    # more than a tile of sample entries against an empty reference
    sam = [(4 * i + (i % 4), 3) for i in range(tile() + 100)]
    got, st = scan(ctx, [], sam, 13)
    assert got == [] and st == dict(n_groups=len(sam), n_missing=len(sam), first_missing=0, n_mixed=0)


# ---- the threshold edge ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 30, 1000, 10 ** 6, 1 << 31])
@pytest.mark.parametrize("g", [(1, 2), (3, 1000), (1 << 20, 1)])
def test_threshold_edge_at_k_equal_n(ctx, n, g):
    """the sample holds one base only: the tail is its first term, v == F == n log(p) on the host"""
    from zotmer_amd.library import varscan
    K, c = 9, 4321
    ref = [((c << 2) | 1, g[0]), ((c << 2) | 2, g[1])]
    sam = [((c << 2) | 1, n)]
    p = float(g[0]) / float(sum(g))
    v = varscan.log_bin_ge(p, n, n)
    assert v == varscan.first_term(p, n, n) == math.log(p) * n
    G = varscan.guard(n, n, p)
    assert G > 0 and v - 3 * G < v
    bits = 32 if n < 1 << 32 else 64
    got, _ = scan(ctx, ref, sam, K, np.nextafter(v, math.inf), sbits=bits)
    assert got == [(c, (0, n, 0, 0), (0, g[0], g[1], 0))]               # v < threshold: the host prints it
    got, _ = scan(ctx, ref, sam, K, v - 3 * G, sbits=bits)
    assert got == []                                                    # three guards below: out of the device's reach


# ---- exact comparison, widths, overflow --------------------------------------------------------------------------------------

def two_by_two(a, b, g, h, c=77):
    """sample {0: a, 1: b} against reference {0: g, 2: h}: base 0 is the only possible candidate, and is one iff a h > b g"""
    return [((c << 2) | 0, g), ((c << 2) | 2, h)], [((c << 2) | 0, a), ((c << 2) | 1, b)]


def test_products_are_compared_in_128_bits(ctx):
    K = 9
    # the two products share their low 64 bits
    for a, b, g, h, row in ((1 << 33, 1 << 33, (1 << 32) + 1, (1 << 33) + 1, True), (1 << 33, 1 << 33, (1 << 33) + 1, (1 << 32) + 1, False)):
        ref, sam = two_by_two(a, b, g, h)
        x, y = a * (g + h), (a + b) * g
        assert x & (2 ** 64 - 1) == y & (2 ** 64 - 1) and (x > y) == row and x >> 64 != y >> 64
        assert len(check_exact(ctx, ref, sam, K)) == int(row)
    # the two products differ by one unit at 2^81: equal as doubles
    for a, b, g, h, row in ((1 << 40, (1 << 40) + 1, (1 << 40) - 1, 1 << 40, True), ((1 << 40) + 1, 1 << 40, 1 << 40, (1 << 40) - 1, False)):
        ref, sam = two_by_two(a, b, g, h)
        x, y = a * (g + h), (a + b) * g
        assert float(x) == float(y) and (x > y) == row
        assert len(check_exact(ctx, ref, sam, K, thr=-5.0)) == int(row)


def test_counts_at_the_ends_of_their_widths(ctx):
    K, top = 9, (1 << 32) - 1
    ref = [((5 << 2) | b, top) for b in range(4)] + [((9 << 2) | 0, top), ((9 << 2) | 3, 1)]
    sam = [((5 << 2) | 1, top), ((9 << 2) | 0, 1), ((9 << 2) | 3, top)]
    got = check_exact(ctx, ref, sam, K, rbits=32, sbits=32)
    assert got == [(5, (0, top, 0, 0), (top, top, top, top)), (9, (1, 0, 0, top), (top, 0, 0, 1))]
    assert check_exact(ctx, ref, sam, K, rbits=64, sbits=32) == got
    big = (1 << 40) + 12345
    ref = [((5 << 2) | 0, 3 * big), ((5 << 2) | 1, big)]
    sam = [((5 << 2) | 0, big), ((5 << 2) | 1, 2 * big)]
    assert check_exact(ctx, ref, sam, K) == [(5, (big, 2 * big, 0, 0), (3 * big, big, 0, 0))]
    # the largest sums that fit
    ref = [((5 << 2) | 0, (1 << 63) - 1), ((5 << 2) | 1, 1 << 63)]
    sam = [((5 << 2) | 0, 1 << 63), ((5 << 2) | 2, (1 << 63) - 1)]
    _, st = scan(ctx, ref, sam, K)
    assert st["n_mixed"] == 1


def test_a_group_sum_that_wraps(ctx):
    from zotmer_amd import native
    K = 9
    good_ref = [((5 << 2) | 0, 10), ((5 << 2) | 1, 20)]
    good_sam = [((5 << 2) | 0, 10), ((5 << 2) | 1, 1)]
    for ref, sam in ((good_ref, [((5 << 2) | 0, 1 << 63), ((5 << 2) | 1, 1 << 63)]),
                     ([((5 << 2) | 0, (1 << 64) - 1), ((5 << 2) | 3, 1)], good_sam)):
        with pytest.raises(native.ZotkError) as e:
            scan(ctx, ref, sam, K)
        assert e.value.code == native.ZK_EOVERFLOW
        check_exact(ctx, good_ref, good_sam, K)                        # the context is as good as before
    # a reference group that no sample group joins is not added up
    ref = good_ref + [((6 << 2) | 0, (1 << 64) - 1), ((6 << 2) | 3, 1)]
    check_exact(ctx, ref, good_sam, K)


# ---- capacities and refusals -------------------------------------------------------------------------------------------------

def raw_call(ctx, rk, rc, sk, sc, K, thr, cap, rbits=64, sbits=64):
    from zotmer_amd import native
    ctxs, rows = ctx.empty(cap, np.uint64), ctx.empty(8 * cap, np.uint64)
    st = native.VarsStats()
    rc_ = ctx.lib.zk_vars_scan(ctx.h, rk.ptr, rc.ptr, rbits, rk.n, sk.ptr, sc.ptr, sbits, sk.n, K, thr, ctxs.ptr, rows.ptr, cap, C.byref(st))
    return rc_, st, ctxs, rows


def test_enospc_and_the_binding_grows(ctx):
    from zotmer_amd import native
    ref, sam = lists_of("cycling", 3, tile() + 1)
    want, stats = brute(ref, sam)
    n = len(want)
    assert n > 100
    rk, rc = upload(ctx, ref, 64)
    sk, sc = upload(ctx, sam, 64)
    for cap in (0, 1, n - 1):
        rc_, st, _, _ = raw_call(ctx, rk, rc, sk, sc, BORDER_K, THR, cap)
        assert rc_ == native.ZK_ENOSPC
        assert dict(n_groups=st.n_groups, n_missing=st.n_missing, first_missing=st.first_missing, n_mixed=st.n_mixed) == stats
        assert st.n_rows == n and b"%d rows" % n in ctx.lib.zk_last_error(ctx.h)
    rc_, st, ctxs, rows = raw_call(ctx, rk, rc, sk, sc, BORDER_K, THR, n)           # the size reported is enough
    assert rc_ == 0 and ctxs.to_host().tolist() == [c for c, _, _ in want]
    first = (ctxs.to_host().tobytes(), rows.to_host().tobytes())
    rc_, st, ctxs, rows = raw_call(ctx, rk, rc, sk, sc, BORDER_K, THR, n)           # the same call, the same bits
    assert rc_ == 0 and (ctxs.to_host().tobytes(), rows.to_host().tobytes()) == first
    got, _ = scan(ctx, ref, sam, BORDER_K)                                           # the binding grows what was too small
    assert got == want
    got, _ = scan(ctx, ref, sam, BORDER_K, cap=1)
    assert got == want


def test_refused_arguments(ctx):
    from zotmer_amd import native
    m = missing_case()
    rk, rc = upload(ctx, m["ref"], 64)
    sk, sc = upload(ctx, m["sample"], 64)
    for K, thr, rb, sb in ((0, THR, 64, 64), (33, THR, 64, 64), (-1, THR, 64, 64), (5, math.nan, 64, 64), (5, math.inf, 64, 64),
                           (5, -math.inf, 64, 64), (5, THR, 16, 64), (5, THR, 64, 0), (5, THR, 33, 32)):
        rc_, st, _, _ = raw_call(ctx, rk, rc, sk, sc, K, thr, 16, rb, sb)
        assert rc_ == native.ZK_EINVAL, (K, thr, rb, sb)
    check_exact(ctx, m["ref"], m["sample"], m["K"])                    # the context is as good as before


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


def write_set(path, K, pairs):
    from zotmer_amd.library import vectors
    from zotmer_amd.library.container import KmerSet
    with KmerSet(str(path), "w") as z:
        vectors.write_kmers_and_counts(z, np.array([x for x, _ in pairs], dtype=np.uint64), np.array([c for _, c in pairs], dtype=np.uint64))
        z.meta.update({"K": K, "kmers": "kmers", "counts": "counts"})
    return str(path)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_command_on_the_fixture(ctx, case, tmp_path):
    K = case["K"]
    ref = write_set(tmp_path / "ref.k", K, case["ref"])
    inputs = [write_set(tmp_path / (nm + ".k"), K, pairs) for nm, pairs in case["samples"]]
    code, out, err = run(["vars", "-r", ref] + inputs)
    assert code == 0 and err == ""
    want = [l for _, pairs in case["samples"] for l in R.stdout_lines(K, case["ref"], pairs)]
    assert out.splitlines() == want                                     # the restatement, in this process: exact text
    gold = [l for nm in GOLD[case["name"]]["inputs"] for l in GOLD[case["name"]]["stdout"][nm]]
    assert same_lines(out.splitlines(), gold, GOLD[case["name"]]["noise"])


def test_command_skips_missing_contexts(ctx, tmp_path):
    m = missing_case()
    ref = write_set(tmp_path / "ref.k", m["K"], m["ref"])
    sam = write_set(tmp_path / "sam.k", m["K"], m["sample"])
    shared = write_set(tmp_path / "shared.k", m["K"], m["shared"])
    with pytest.raises(AssertionError):
        R.stdout_lines(m["K"], m["ref"], m["sample"])                   # where the reference dies
    code, out, err = run(["vars", "-r", ref, sam, shared])
    want = R.stdout_lines(m["K"], m["ref"], m["sample"], skip_missing=True)
    assert code == 0 and len(want) == 3 and out.splitlines() == want + R.stdout_lines(m["K"], m["ref"], m["shared"])
    assert err == "zot vars: %s: 3 of 6 contexts are not in the reference (first: %s)\n" % (sam, R.render(m["K"] - 1, 3))


def test_command_refusals(ctx, tmp_path):
    m = missing_case()
    ref = write_set(tmp_path / "ref.k", m["K"], m["ref"])
    shared = write_set(tmp_path / "shared.k", m["K"], m["shared"])
    other = write_set(tmp_path / "other.k", m["K"] + 1, m["shared"])
    code, out, err = run(["vars", shared])                              # no -r
    assert code == 1 and out == "" and "zot vars -r ref <input>..." in err
    code, out, err = run(["vars", "-r", other, shared])                 # a reference set of another K
    assert code == 1 and out == "" and "reference set" in err
    code, out, err = run(["vars", "-r", ref, shared])
    assert code == 0 and len(out.splitlines()) == 3 and err == ""
