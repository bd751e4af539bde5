"""`zot alu-finder` on the GPU: zk_anchor_pileup against a pure-Python brute force of the reference's `hits` (every window of a
list once per distinct diagonal of the list), bit for bit as sorted multisets, on the line shapes, hit patterns, diagonal counts
(around ZK_PILEUP_DIAGS, where the kernel changes its path), coordinates, capacities and refusals the entry's contract names;
zk_pileup_count against NumPy on runs placed around ZK_PILEUP_TILE; and the command end to end on every fixture the reference
produced (tests/golden/a1_alufinder.json), in one batch and in several."""
import contextlib
import ctypes as C
import io
import json
import os
import random
import re

import numpy as np
import pytest

from tests import _alufinder_restatement as R
from tests._alufinder_cases import make_cases, write_case
from zotmer_amd import native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "a1_alufinder.json")
OK, EINVAL, ENOSPC, ERANGE = native.ZK_OK, native.ZK_EINVAL, native.ZK_ENOSPC, native.ZK_ERANGE
DIAGS, TILE = native.PILEUP_DIAGS, native.PILEUP_TILE
G32, G64 = 0xABCDABCD, 0xABCDABCDABCDABCD
CODE = {c: i for i, c in enumerate("ACGT")}
CODE.update({c.lower(): i for c, i in list(CODE.items())})
CODE.update(U=3, u=3)


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "zotk.h")).read()
    assert int(re.search(r"#define ZK_PILEUP_DIAGS (\d+)", text).group(1)) == DIAGS
    assert int(re.search(r"#define ZK_PILEUP_TILE (\d+)", text).group(1)) == TILE
    assert int(re.search(r"#define ZK_PROF_PILEUP (\d+)", text).group(1)) == native.Context.PROF_TAGS["pileup"] == 27
    assert int(re.search(r"#define ZK_PROF_PILEUP_CUT (\d+)", text).group(1)) == native.Context.PROF_TAGS["pileup_cut"] == 28


# ---- the brute force ------------------------------------------------------------------------------------------------------------
def rc_str(s):
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def kmer(w):
    x = 0
    for ch in w:
        x = (x << 2) | CODE[ch]
    return x


def rc_int(K, x):
    y = 0
    for _ in range(K):
        y = (y << 2) | (3 - (x & 3))
        x >>= 2
    return y


def index_of(K, zones, pad):
    """zones: [sequence, ...] laid out one after another with 2 * pad between them -> ({k-mer: ascending anchors}, total)"""
    idx, base = {}, 0
    for seq in zones:
        for i in range(len(seq) - K + 1):
            w = seq[i:i + K]
            if all(ch in CODE for ch in w):
                idx.setdefault(kmer(w), set()).add(base + pad + i)
        base += max(len(seq) - K + 1, 1) + 2 * pad
    return {x: sorted(a) for x, a in idx.items()}, base


def brute(K, idx, fastq, diag_counts=None):
    """the pairs (coordinate, k-mer) of every list of every read of a FASTQ text, sorted"""
    out = []
    lines = fastq.split("\n")
    for r in range(len(lines) // 4):
        seq = lines[4 * r + 1].strip()
        L = len(seq)
        wins = [(kmer(seq[i:i + K]), i) for i in range(L - K + 1) if all(ch in CODE for ch in seq[i:i + K])]
        for lst in (wins, [(rc_int(K, x), L - i - K) for x, i in wins]):
            D = {a - p for x, p in lst for a in idx.get(x, ())}
            if diag_counts is not None:
                diag_counts.append(len(D))
            out += [(d + p, x) for d in D for x, p in lst]
    return sorted(out)


def fastq_of(seqs, eol="\n"):
    return "".join("@r%d%s%s%s+%s%s%s" % (i, eol, s, eol, eol, "I" * len(s.strip()), eol) for i, s in enumerate(seqs))


def table_of(ctx, K, idx, total):
    keys = np.array(sorted(idx), dtype=np.uint64)
    offs = np.zeros(len(keys) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(idx[int(x)]) for x in keys])
    ids = np.array([a for x in keys for a in idx[int(x)]], dtype=np.uint32)
    return ctx.bait_table_from_arrays(K, ctx.upload(keys), ctx.upload(offs), ctx.upload(ids), max(total, 1))


def pileup(ctx, table, fastq, K, pad, cap=None, room=64, n_reads=None):
    """one zk_anchor_pileup into guarded arrays -> (rc, count, coordinates, k-mers) with the whole arrays"""
    text = ctx.upload(np.frombuffer(fastq.encode(), dtype=np.uint8))
    lines = ctx.line_ends(text)
    n_reads = lines.n // 4 if n_reads is None else n_reads
    size = (cap or 0) + room
    oc, ok = ctx.upload(np.full(size, G32, np.uint32)), ctx.upload(np.full(size, G64, np.uint64))
    n = C.c_uint64(0)
    rc = ctx.lib.zk_anchor_pileup(ctx.h, table.h, text.ptr, lines.ptr, n_reads, K, pad, oc.ptr, ok.ptr, size - room if cap is not None else 0,
                                  C.byref(n))
    return rc, n.value, oc.to_host(), ok.to_host()


def check_pileup(ctx, table, fastq, K, pad, idx, diag_counts=None):
    """size the output with cap = 0, run with exactly that room, compare with the brute force -> the sorted pairs"""
    want = brute(K, idx, fastq, diag_counts)
    rc, n, oc, ok = pileup(ctx, table, fastq, K, pad)
    assert (rc, n) == ((ENOSPC if want else OK), len(want)), (rc, n, len(want), ctx.lib.zk_last_error(ctx.h))
    assert np.all(oc == G32) and np.all(ok == G64)
    rc, n, oc, ok = pileup(ctx, table, fastq, K, pad, cap=len(want))
    assert (rc, n) == (OK, len(want)), (rc, n, len(want), ctx.lib.zk_last_error(ctx.h))
    assert np.all(oc[n:] == G32) and np.all(ok[n:] == G64)
    got = sorted(zip(oc[:n].tolist(), ok[:n].tolist()))
    assert got == want
    return want


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


# ---- zk_anchor_pileup -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 25, 32])
def test_line_shapes(ctx, K):
    """lines shorter than K, of K bases, with 63, 64, 65 and 129 window starts; a byte that is no base first, last and in the middle;
    lower case and U; blanks, tabs and CR around the line; reads of both strands"""
    rng = random.Random(100 + K)
    zone = rand_seq(rng, 600)
    idx, total = index_of(K, [zone], 256)
    reads = [zone[7:7 + K - 1], "", zone[11:11 + K]]
    for w in (63, 64, 65, 129):
        s = zone[20:20 + w + K - 1]
        reads += [s, rc_str(s)]
    s = zone[100:100 + 90]
    reads += ["N" + s[1:], s[:-1] + "N", s[:45] + "n" + s[46:], s[:30] + "-" + s[31:60] + "." + s[61:], rc_str(s)[:50] + "N" + rc_str(s)[51:]]
    reads += [s.lower(), s.replace("T", "U"), rc_str(s).lower().replace("t", "u")]
    reads += [s + "  ", "\t " + s, " " + rc_str(s) + " \t", s[:40] + " " + s[41:]]
    table = table_of(ctx, K, idx, total)
    counts = []
    want = check_pileup(ctx, table, fastq_of(reads), K, 256, idx, counts)
    assert want and counts[0] == counts[1] == 0 and counts[4] == 1
    check_pileup(ctx, table, fastq_of(reads, eol="\r\n"), K, 256, idx)
    table.free()


@pytest.mark.parametrize("K", [5, 25, 32])
def test_hits_by_orientation_and_the_reads_that_hit_nothing(ctx, K):
    rng = random.Random(200 + K)
    zone = rand_seq(rng, 300)
    both = rand_seq(rng, 60)
    zones = [zone, both + "G" + rc_str(both)]                 # the second zone holds a stretch and its reverse complement
    idx, total = index_of(K, zones, 128)
    table = table_of(ctx, K, idx, total)
    fwd, rev, two, none = zone[50:130], rc_str(zone[150:230]), both[5:55], rand_seq(rng, 90)
    for reads, diags in (([fwd], [1, 0]), ([rev], [0, 1]), ([none], [0, 0]), ([none, none[::-1]], [0] * 4)):
        counts = []
        want = check_pileup(ctx, table, fastq_of(reads), K, 128, idx, counts)
        if K > 5:                                             # (5-mers of a random read also hit by chance)
            assert counts == diags and len(want) == sum(diags) * (80 - K + 1)
    counts = []
    check_pileup(ctx, table, fastq_of([two]), K, 128, idx, counts)
    assert min(counts) >= 1
    # a pair whose first mate hits nothing: one call per mate, the pairs come from the second alone
    assert check_pileup(ctx, table, fastq_of([none]), K, 128, idx) == [] or K == 5
    assert check_pileup(ctx, table, fastq_of([rev]), K, 128, idx)
    # many reads, more than one per wave of the grid's first round
    reads = [zone[i:i + 70] if i % 3 else rc_str(zone[i:i + 70]) for i in range(0, 200)] + [rand_seq(rng, 70) for _ in range(40)]
    rng.shuffle(reads)
    check_pileup(ctx, table, fastq_of(reads), K, 128, idx)
    table.free()


@pytest.mark.parametrize("K", [5, 25, 32])
def test_diagonals(ctx, K):
    """many windows on one diagonal count once; a read with one base more than the zone lies on two; a k-mer anchored in two zones and
    twice in one zone gives one diagonal per anchor"""
    rng = random.Random(300 + K)
    a, shared = rand_seq(rng, 200), rand_seq(rng, 70)
    zones = [a[:100] + shared + a[100:], rand_seq(rng, 50) + shared + rand_seq(rng, 40) + shared + rand_seq(rng, 30)]
    idx, total = index_of(K, zones, 128)
    table = table_of(ctx, K, idx, total)
    clean = zones[0][10:95]
    counts = []
    want = check_pileup(ctx, table, fastq_of([clean]), K, 128, idx, counts)
    if K > 5:
        assert counts == [1, 0] and len(want) == 85 - K + 1
    more = zones[0][5:45] + "T" + zones[0][45:95]
    counts = []
    check_pileup(ctx, table, fastq_of([more, rc_str(more)]), K, 128, idx, counts)
    if K > 5:
        assert counts == [2, 0, 0, 2]
    counts = []
    check_pileup(ctx, table, fastq_of([shared[3:68], rc_str(shared)]), K, 128, idx, counts)
    if K > 5:
        assert counts == [3, 0, 0, 3]
    table.free()


def tandem(K, period, target, rng):
    """a zone of a repeated unit and a read of it with exactly `target` diagonals -> (zone, read)"""
    unit = rand_seq(rng, period)
    while len({unit[i:] + unit[:i] for i in range(period)}) < period:
        unit = rand_seq(rng, period)
    read = (unit * (K // period + 4))[:K + 2 * period]
    n = max(1, target - 4)
    while True:
        zone = (unit * (n + K // period + 2))[:n * period + K - 1]
        counts = []
        brute(K, index_of(K, [zone], 64)[0], fastq_of([read]), counts)
        if counts[0] >= target:
            assert counts[0] == target, (counts, target)
            return zone, read
        n += 1


@pytest.mark.parametrize("K", [5, 25, 32])
@pytest.mark.parametrize("target", [DIAGS - 1, DIAGS, DIAGS + 1, 4 * DIAGS + 3])
def test_tandem_repeats_around_the_register_bound(ctx, K, target):
    """a read on a tandem repeat with DIAGS - 1, DIAGS, DIAGS + 1 and about 4 x DIAGS diagonals: the list in registers, full, and the
    path beyond it -- forward, reverse, with a byte that is no base, and beside reads that take the register path"""
    rng = random.Random(400 + K)
    zone, read = tandem(K, 7, target, rng)
    other = rand_seq(rng, 150)
    idx, total = index_of(K, [zone, other], 128)
    table = table_of(ctx, K, idx, total)
    broken = read[:K + 3] + "N" + read[K + 4:] + read[:K + 2]
    reads = [read, other[20:20 + 60], rc_str(read), broken.lower(), rc_str(other[40:110]), read[:K]]
    counts = []
    check_pileup(ctx, table, fastq_of(reads), K, 128, idx, counts)
    assert counts[0] == target and counts[5] == target and (K == 5 or (counts[1] == 0 and counts[4] == 0))
    table.free()


def test_coordinates_in_the_pad_and_a_line_longer_than_the_pad(ctx):
    K, pad = 25, 100
    rng = random.Random(500)
    zones = [rand_seq(rng, 120), rand_seq(rng, 90)]
    idx, total = index_of(K, zones, pad)
    table = table_of(ctx, K, idx, total)
    # reads that hang over the first and the last anchor of a zone: their other windows lie in the pad, up to pad - K from an anchor
    left, right = rand_seq(rng, 70) + zones[1][:30], zones[0][-30:] + rand_seq(rng, 70)
    want = check_pileup(ctx, table, fastq_of([left, right, rc_str(left), rc_str(right)]), K, pad, idx)
    first1 = (120 - K + 1) + 2 * pad + pad                     # zone 1's first anchor
    last0 = pad + 120 - K                                      # zone 0's last anchor
    assert min(c for c, _ in want if c > last0 + pad) == first1 - 70 and max(c for c, _ in want if c < first1 - pad) == last0 + 70
    # a line of pad bytes that hits is the longest allowed; one more is refused before anything is written; one that hits nothing is not
    at = zones[0][:40] + rand_seq(rng, pad - 40)
    check_pileup(ctx, table, fastq_of([at]), K, pad, idx)
    for long_read in (at + "A", rc_str(at + "A"), "  " + at + "C\t"):
        text = fastq_of([zones[0][:60], long_read])
        rc, n, oc, ok = pileup(ctx, table, text, K, pad, cap=500)
        assert rc == ERANGE and b"longer than pad" in ctx.lib.zk_last_error(ctx.h)
        assert np.all(oc == G32) and np.all(ok == G64)
    check_pileup(ctx, table, fastq_of([zones[0][:60], rand_seq(rng, 3 * pad), " " + at + "  "]), K, pad, idx)
    table.free()


def test_empty_and_invalid_inputs(ctx):
    K = 25
    rng = random.Random(600)
    zone = rand_seq(rng, 100)
    idx, total = index_of(K, [zone], 64)
    table = table_of(ctx, K, idx, total)
    empty = table_of(ctx, K, {}, 0)
    text = fastq_of([zone[:60]])
    rc, n, oc, ok = pileup(ctx, empty, text, K, 64, cap=10)
    assert (rc, n) == (OK, 0) and np.all(oc == G32) and np.all(ok == G64)
    rc, n, oc, ok = pileup(ctx, table, text, K, 64, cap=10, n_reads=0)
    assert (rc, n) == (OK, 0) and np.all(oc == G32) and np.all(ok == G64)
    n64 = C.c_uint64(7)
    assert ctx.lib.zk_anchor_pileup(ctx.h, table.h, None, None, 0, K, 64, None, None, 0, C.byref(n64)) == OK and n64.value == 0
    for bad in (0, 33, -1, 24):                                # out of range, and not the table's K
        rc, n, oc, ok = pileup(ctx, table, text, bad, 64, cap=100)
        assert rc == EINVAL and np.all(oc == G32) and np.all(ok == G64), bad
    assert ctx.lib.zk_anchor_pileup(ctx.h, None, None, None, 0, K, 64, None, None, 0, C.byref(n64)) == EINVAL
    for bad in (0, 33):
        assert ctx.lib.zk_pileup_count(ctx.h, None, None, 0, bad, None, None, None, 0, C.byref(n64)) == EINVAL
    check_pileup(ctx, table, text, K, 64, idx)                 # the context is still good
    table.free()
    empty.free()


def test_pileup_capacity(ctx):
    """one short of the pairs needed, exactly them, and more: nothing at or beyond cap, the count needed, repeatable"""
    K = 25
    rng = random.Random(700)
    zone = rand_seq(rng, 400)
    idx, total = index_of(K, [zone], 128)
    table = table_of(ctx, K, idx, total)
    text = fastq_of([zone[i:i + 90] if i % 2 else rc_str(zone[i:i + 90]) for i in range(0, 300, 7)])
    want = brute(K, idx, text)
    need = len(want)
    for cap in (0, 1, need // 2, need - 1):
        rc, n, oc, ok = pileup(ctx, table, text, K, 128, cap=cap, room=need + 64)
        assert (rc, n) == (ENOSPC, need), cap
        assert np.all(oc[cap:] == G32) and np.all(ok[cap:] == G64), cap
    for cap in (need, need + 1, need + 50):
        rc, n, oc, ok = pileup(ctx, table, text, K, 128, cap=cap, room=64)
        assert (rc, n) == (OK, need), cap
        assert np.all(oc[need:] == G32) and np.all(ok[need:] == G64) and sorted(zip(oc[:n].tolist(), ok[:n].tolist())) == want
    table.free()


def test_pileup_on_views_at_odd_offsets(ctx):
    """the text 5 bytes into a larger buffer, the outputs 3 elements into guarded arrays: nothing in front of either is touched"""
    K, pad = 25, 128
    rng = random.Random(750)
    zone = rand_seq(rng, 300)
    idx, total = index_of(K, [zone], pad)
    table = table_of(ctx, K, idx, total)
    fq = fastq_of([zone[i:i + 80] for i in range(0, 200, 11)] + [rc_str(zone[30:120])])
    want = brute(K, idx, fq)
    raw = np.frombuffer(fq.encode(), dtype=np.uint8)
    buf = ctx.upload(np.concatenate((np.full(5, ord("A"), np.uint8), raw, np.full(7, ord("C"), np.uint8))))
    text = buf.view(len(raw), 5)
    lines = ctx.line_ends(text)
    oc, ok = ctx.upload(np.full(len(want) + 70, G32, np.uint32)), ctx.upload(np.full(len(want) + 70, G64, np.uint64))
    n = C.c_uint64(0)
    rc = ctx.lib.zk_anchor_pileup(ctx.h, table.h, text.ptr, lines.ptr, lines.n // 4, K, pad, oc.ptr + 4 * 3, ok.ptr + 8 * 3, len(want), C.byref(n))
    assert (rc, n.value) == (OK, len(want))
    hc, hk = oc.to_host(), ok.to_host()
    assert np.all(hc[:3] == G32) and np.all(hk[:3] == G64) and np.all(hc[3 + n.value:] == G32) and np.all(hk[3 + n.value:] == G64)
    assert sorted(zip(hc[3:3 + n.value].tolist(), hk[3:3 + n.value].tolist())) == want
    assert np.array_equal(buf.to_host()[5:5 + len(raw)], raw)
    table.free()


# ---- zk_pileup_count --------------------------------------------------------------------------------------------------------------
def count_oracle(coords, kmers):
    order = np.lexsort((kmers, coords))
    c, x = coords[order], kmers[order]
    heads = np.ones(len(c), dtype=bool)
    heads[1:] = (c[1:] != c[:-1]) | (x[1:] != x[:-1])
    starts = np.nonzero(heads)[0]
    return c[starts], x[starts], np.diff(np.append(starts, len(c))).astype(np.uint32)


def run_count(ctx, coords, kmers, K, cap=None, offset=0):
    """zk_pileup_count on views `offset` elements into larger arrays, into guarded outputs -> (rc, count, oc, ok, cnt) whole arrays"""
    n = len(coords)
    dc = ctx.upload(np.concatenate((np.full(offset, G32, np.uint32), coords, np.full(3, G32, np.uint32))))
    dk = ctx.upload(np.concatenate((np.full(offset, G64, np.uint64), kmers, np.full(3, G64, np.uint64))))
    size = n + 64
    cap = n if cap is None else cap
    oc, ok, cnt = ctx.upload(np.full(size, G32, np.uint32)), ctx.upload(np.full(size, G64, np.uint64)), ctx.upload(np.full(size, G32, np.uint32))
    m = C.c_uint64(0)
    rc = ctx.lib.zk_pileup_count(ctx.h, dc.ptr + 4 * offset, dk.ptr + 8 * offset, n, K, oc.ptr, ok.ptr, cnt.ptr, cap, C.byref(m))
    assert np.array_equal(dc.to_host()[offset:offset + n], coords) and np.array_equal(dk.to_host()[offset:offset + n], kmers)   # inputs stay
    return rc, m.value, oc.to_host(), ok.to_host(), cnt.to_host()


def check_count(ctx, coords, kmers, K, offset=0):
    coords, kmers = np.asarray(coords, np.uint32), np.asarray(kmers, np.uint64)
    wc, wk, wn = count_oracle(coords, kmers)
    rc, m, oc, ok, cnt = run_count(ctx, coords, kmers, K, offset=offset)
    assert (rc, m) == (OK, len(wc)), (rc, m, len(wc), ctx.lib.zk_last_error(ctx.h))
    assert np.array_equal(oc[:m], wc) and np.array_equal(ok[:m], wk) and np.array_equal(cnt[:m], wn)
    assert np.all(oc[m:] == G32) and np.all(ok[m:] == G64) and np.all(cnt[m:] == G32)
    return m


def runs_of(lengths, rng, K):
    """runs of equal pairs of the given lengths, distinct from one another, shuffled"""
    mask = (1 << (2 * K)) - 1
    pairs = set()
    while len(pairs) < len(lengths):
        pairs.add((rng.randrange(1 << 12), rng.getrandbits(64) & mask))
    pairs = sorted(pairs)
    c = np.repeat(np.array([p[0] for p in pairs], np.uint32), lengths)
    x = np.repeat(np.array([p[1] for p in pairs], np.uint64), lengths)
    order = np.random.default_rng(rng.randrange(1 << 30)).permutation(len(c))
    return c[order], x[order]


@pytest.mark.parametrize("K", [5, 25, 32])
def test_count_small_and_degenerate(ctx, K):
    rng = random.Random(800 + K)
    top = (1 << (2 * K)) - 1
    m = C.c_uint64(9)
    assert ctx.lib.zk_pileup_count(ctx.h, None, None, 0, K, None, None, None, 0, C.byref(m)) == OK and m.value == 0
    assert check_count(ctx, [77], [top], K) == 1
    assert check_count(ctx, [5] * 1000, [top] * 1000, K) == 1                                   # all equal
    assert check_count(ctx, np.arange(3000)[::-1] // 2, (np.arange(3000, dtype=np.uint64) * np.uint64(7)) % np.uint64(top), K, offset=3)
    # equal coordinates with different k-mers, equal k-mers at different coordinates; at K = 32 with bit 63 set and clear
    xs = [top, top - 1, top >> 1, 1, 0]
    c = [9] * 5 + [1, 2, 3, 4, 5] + [9, 9, 4]
    x = xs + [top] * 5 + [top, 0, top]
    assert check_count(ctx, c, x, K, offset=1) == 10
    c, x = runs_of([rng.randrange(1, 9) for _ in range(700)], rng, K)
    check_count(ctx, c, x, K, offset=5)


@pytest.mark.parametrize("K", [25, 32])
def test_count_runs_across_the_tiles(ctx, K):
    """runs that end one short of, at and one past the first and the second tile border of the sorted pairs; runs longer than a tile"""
    rng = random.Random(900 + K)
    for first in (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1):
        c, x = runs_of([1] * 3 + [2, 5], rng, K)
        lengths = [first - 40, 40 - 12, 3, 2 * TILE + 5, 1, 1, 700]
        c2, x2 = runs_of(lengths, rng, K)
        # the coordinates of the second set lie above the first's, in the order given: the borders fall where `first` puts them
        c2 = np.repeat(np.arange(len(lengths), dtype=np.uint32) + (1 << 13), lengths)
        x2 = np.repeat(np.array([rng.getrandbits(2 * K) for _ in lengths], np.uint64), lengths)
        order = np.random.default_rng(first).permutation(len(c2) + len(c))
        check_count(ctx, np.concatenate((c, c2))[order], np.concatenate((x, x2))[order], K, offset=first % 3)


def test_count_capacity(ctx):
    rng = random.Random(1000)
    c, x = runs_of([rng.randrange(1, 5) for _ in range(TILE + 50)], rng, 25)
    wc, wk, wn = count_oracle(c, x)
    need = len(wc)
    for cap in (0, 1, TILE, need - 1):
        rc, m, oc, ok, cnt = run_count(ctx, c, x, 25, cap=cap)
        assert (rc, m) == (ENOSPC, need), cap
        assert np.all(oc[cap:] == G32) and np.all(ok[cap:] == G64) and np.all(cnt[cap:] == G32), cap
    for cap in (need, need + 9):
        rc, m, oc, ok, cnt = run_count(ctx, c, x, 25, cap=cap)
        assert (rc, m) == (OK, need)
        assert np.array_equal(oc[:m], wc) and np.array_equal(ok[:m], wk) and np.array_equal(cnt[:m], wn)
        assert np.all(oc[m:] == G32) and np.all(ok[m:] == G64) and np.all(cnt[m:] == G32)


def test_pileup_then_count_is_the_references_accumulator(ctx):
    """both entries in a row on a fixture's reads against the restatement's acc (before the filter), through the product's layout"""
    from zotmer_amd.library import alufinder as A
    case = next(c for c in make_cases() if c["name"] == "one_base_more_raw")
    keep = {}
    R.alu_finder(case, keep=keep)
    zones = A.Zones(case["k"])
    for line in case["bed"].splitlines():
        ch, s, e, nm = line.split()
        zones.add(ch, int(s), int(e), nm, case["genomes"][ch].encode())
    layout = A.layout_of(zones, pad=128)
    table = A.anchor_table(ctx, zones, layout)
    pile = A.Pileup()
    for fq in case["inputs"]:
        text = ctx.upload(np.frombuffer(fq.encode(), dtype=np.uint8))
        lines = ctx.line_ends(text)
        coords, kmers = ctx.anchor_pileup(table, text, lines, lines.n // 4, case["k"], layout.pad)
        oc, ok, cnt = ctx.pileup_count(coords, kmers, case["k"])
        pile.add(oc.to_host(), ok.to_host(), cnt.to_host())
    table.free()
    assert A.decode_acc(layout, *pile.result()) == keep["acc"]


# ---- the command ------------------------------------------------------------------------------------------------------------------
INPUTS = {c["name"]: c for c in make_cases()}
CASES = [dict(INPUTS[c["name"]], **c) for c in json.load(open(GOLD))]


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


def expected(case):
    import hashlib
    if "lines" in case:
        return lambda text: text == "".join(l + "\n" for l in case["lines"])
    return lambda text: text.count("\n") == case["n_lines"] and hashlib.sha256(text.encode()).hexdigest() == case["sha256"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_command_on_the_fixture(ctx, case, tmp_path):
    args = write_case(case, str(tmp_path))
    code, out, err = run(["alu-finder"] + args)
    assert code in (0, None) and err == "", err
    assert expected(case)(out)
    if case["name"] in ("batches", "insertion_two_zones_raw", "one_base_more_raw"):          # several batches and the host merge
        code, small, err = run(["alu-finder", "-m", "1"] + args)
        assert code in (0, None) and err == "" and small == out


def test_command_when_mate_2_ends_first_and_when_a_read_is_too_long(ctx, tmp_path):
    from zotmer_amd.library import alufinder as A
    case = dict(INPUTS["insertion_raw"], C=2)
    m1, m2 = (t.split("\n") for t in case["inputs"])
    case["inputs"] = ["\n".join(m1[:4 * 500]) + "\n", "\n".join(m2[:4 * 320]) + "\n"]
    args = write_case(case, str(tmp_path))
    code, out, err = run(["alu-finder"] + args)
    assert code in (0, None) and err == "warning: files had unequal length\n"
    assert out == "".join(l + "\n" for l in R.alu_finder(case)) and out.count("\n") > 1
    # the longest line that may hit a zone is the pad: the library's run with a pad below the reads' length refuses
    bed = args[-3]
    zones = A.load_zones(bed, os.path.dirname(bed), case["k"])
    with pytest.raises(A.InputError, match="longer than pad = 64"):
        A.run(ctx, zones, args[-2:], 2, 29, 5, 0.05, True, 1 << 20, io.StringIO(), pad=64)
