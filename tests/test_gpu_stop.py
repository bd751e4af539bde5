"""`zot stop` on the GPU: zk_stop_frames against the restatement of the reference's loop (tests/_stop_restatement.py), bit for bit
as sorted multisets of (transcript, k-mer), on the line shapes, frame patterns, vote counts (around ZK_STOP_VOTES, where the
selection changes its path), draws on both sides of a frame boundary, batch cuts, capacities and refusals the entry's contract
names; zk_stop_nearest against NumPy on list and entry counts around its tiles; and the command end to end on every fixture
case the reference's main produced (tests/golden/s1_stop.json)."""
import contextlib
import ctypes as C
import io
import json
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import _stop_restatement as R
from tests._stop_cases import fixture_cases, rc, write_case
from zotmer_amd import native, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "s1_stop.json")
OK, EINVAL, ENOSPC, ERANGE = native.ZK_OK, native.ZK_EINVAL, native.ZK_ENOSPC, native.ZK_ERANGE
VOTES, ENTRIES, TILE = native.STOP_VOTES, native.STOP_NEAR_ENTRIES, native.STOP_NEAR_TILE
G32, G64, G8 = 0xABCDABCD, 0xABCDABCDABCDABCD, 0xAB


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "zotk.h")).read()
    assert int(re.search(r"#define ZK_STOP_VOTES (\d+)", text).group(1)) == VOTES
    assert int(re.search(r"#define ZK_STOP_NEAR_ENTRIES (\d+)", text).group(1)) == ENTRIES
    assert int(re.search(r"#define ZK_STOP_NEAR_TILE (\d+)", text).group(1)) == TILE
    for name, tag in (("STOP_FRAMES", 39), ("STOP_EMIT", 40), ("STOP_NEAREST", 41)):
        assert int(re.search(r"#define ZK_PROF_%s (\d+)" % name, text).group(1)) == native.Context.PROF_TAGS[name.lower()] == tag
    assert synth.T_STOP == 24 and "SF_T_STOP = 24" in open(os.path.join(ROOT, "zotmer_amd", "csrc", "stop_frames.hip")).read()


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def fastq_of(seqs, eol="\n"):
    return "".join("@r%d%s%s%s+%s%s%s" % (i, eol, s, eol, eol, "I" * len(s.strip()), eol) for i, s in enumerate(seqs))


class Placed:
    """transcripts [(name, sequence)] as the product lays them out (library/stopscan.py) and as the restatement indexes them"""

    def __init__(self, ctx, K, records, pad):
        from zotmer_amd.library import stopscan
        self.ctx, self.K, self.pad = ctx, K, pad
        self.ref = R.Index(K, records)
        self.index = stopscan.Index(K, [(nm, seq.encode("latin-1")) for nm, seq in records])
        self.layout = stopscan.layout_of(self.index, pad)
        self.table = stopscan.anchor_table(ctx, self.index, self.layout)
        self.starts = ctx.upload(stopscan.starts_of(self.layout))
        self.t_of = {nm: t for t, nm in enumerate(self.index.names)}

    def want(self, reads, seed, first=0, frames=None):
        out = []
        for g, seq in enumerate(reads, first):
            stops, frame = R.read_stops(self.ref, seq.strip(R.WS), seed, g)
            out += [(self.t_of[nm], x) for nm, x in stops]
            if frames is not None:
                frames.append(frame)
        return sorted(out)

    def call(self, fastq, seed, first=0, cap=None, room=64, n_reads=None, K=None, lead=0):
        """one zk_stop_frames into guarded arrays -> (rc, count, transcripts, k-mers) with the whole arrays"""
        ctx = self.ctx
        text = ctx.upload(np.frombuffer(fastq.encode("latin-1"), dtype=np.uint8))
        lines = ctx.line_ends(text)
        n_reads = lines.n // 4 if n_reads is None else n_reads
        size = lead + (cap or 0) + room
        ot, ok = ctx.upload(np.full(size, G32, np.uint32)), ctx.upload(np.full(size, G64, np.uint64))
        n = C.c_uint64(0)
        rc = ctx.lib.zk_stop_frames(ctx.h, self.table.h, self.starts.ptr, self.starts.n, text.ptr, lines.ptr, n_reads, self.K if K is None else K,
                                    self.pad, seed, first, ot.ptr + 4 * lead, ok.ptr + 8 * lead, cap or 0, C.byref(n))
        return rc, n.value, ot.to_host(), ok.to_host()

    def check(self, reads, seed, first=0, eol="\n", frames=None):
        """size the output with cap = 0, run with exactly that room, compare with the restatement -> the sorted stops"""
        want = self.want(reads, seed, first, frames)
        fastq = fastq_of(reads, eol)
        rc, n, ot, ok = self.call(fastq, seed, first)
        assert (rc, n) == ((ENOSPC if want else OK), len(want)), (rc, n, len(want), self.ctx.lib.zk_last_error(self.ctx.h))
        assert np.all(ot == G32) and np.all(ok == G64)
        rc, n, ot, ok = self.call(fastq, seed, first, cap=len(want))
        assert (rc, n) == (OK, len(want)), (rc, n, len(want), self.ctx.lib.zk_last_error(self.ctx.h))
        assert np.all(ot[n:] == G32) and np.all(ok[n:] == G64)
        assert sorted(zip(ot[:n].tolist(), ok[:n].tolist())) == want
        return want

    def free(self):
        self.table.free()


def stoppy(rng, n):
    """random bases with a stop codon every few: every frame and orientation of a read has some"""
    out = []
    while sum(len(s) for s in out) < n:
        out.append(rand_seq(rng, rng.randrange(2, 9)) + rng.choice(("TAA", "TAG", "TGA", "TTA", "CTA", "TCA")))
    return "".join(out)[:n]


# ---- zk_stop_frames ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 25, 27, 31, 32])
def test_line_shapes(ctx, K):
    """lines shorter than K, of K bases, with 64 and 65 windows; a byte that is no base first, last and inside; lower case and U;
    blanks, tabs and CR around the line; both orientations; reads that hang over the transcript's start and its end"""
    rng = random.Random(100 + K)
    n = 120 if K == 3 else 400
    a, b = stoppy(rng, n), stoppy(rng, n - 33)
    p = Placed(ctx, K, [("b", a), ("a", b)], 256)
    reads = [a[7:7 + K - 1], "", a[11:11 + K], rc(b[5:5 + K])]
    for w in (64, 65):
        s = a[20:20 + w + K - 1]
        reads += [s, rc(s)]
    s = a[30:30 + 80]
    reads += ["N" + s[1:], s[:-1] + "N", s[:45] + "n" + s[46:], s[:30] + "-" + s[31:60] + "." + s[61:], rc(s)[:50] + "N" + rc(s)[51:]]
    reads += [s.lower(), s.replace("T", "U"), rc(s).lower().replace("t", "u")]
    reads += [s + "  ", "\t " + s, " " + rc(s) + " \t", s[:40] + " " + s[41:]]
    reads += [stoppy(rng, 40) + a[:50], rc(stoppy(rng, 40) + b[:50]), a[-50:] + stoppy(rng, 40), rc(b[-45:] + stoppy(rng, 30))]
    for seed in (17, 3):
        frames = []
        want = p.check(reads, seed, frames=frames)
        assert want and frames[0] is None and frames[1] is None
        if K > 3:
            assert frames[2] == ("b", 11, 0) and frames[3] == ("a", 5, 1)
            assert frames[-4][1] == -40 and frames[-3][2] == 1 and frames[-3][1] < 0
    p.check(reads, 17, eol="\r\n")
    p.free()


@pytest.mark.parametrize("K", [25, 32])
def test_frames_and_the_reads_that_hit_nothing(ctx, K):
    """one frame; two frames in one orientation (a base more than the transcript); one in each orientation (a transcript that holds
    a stretch and its reverse complement); a k-mer with anchors in two transcripts; many reads, more than a wave's share"""
    rng = random.Random(200 + K)
    a, shared, both = stoppy(rng, 300), stoppy(rng, 90), stoppy(rng, 70)
    records = [("m", a[:150] + shared + a[150:]), ("c", stoppy(rng, 60) + shared + stoppy(rng, 50)), ("x", both + "G" + rc(both))]
    p = Placed(ctx, K, records, 128)
    one, none = records[0][1][10:100], rand_seq(rng, 90)
    more = records[0][1][5:50] + "T" + records[0][1][50:110]
    for seed in range(6):
        frames = []
        p.check([one, none, more, rc(more), both[3:68], shared[2:88], rc(shared)], seed, frames=frames)
        assert frames[0] == ("m", 10, 0) and frames[1] is None
        assert frames[2] in (("m", 5, 0), ("m", 4, 0)) and frames[3][2] == 1 and frames[4][0] == "x" and frames[5][0] in "mc"
    kinds = {(tuple(f[:1]) + (f[2],)) for seed in range(12) for f in [R.read_stops(p.ref, both[3:68], seed, 0)[1]]}
    assert kinds == {("x", 0), ("x", 1)}                      # the draw reaches the frame of either orientation
    reads = [records[i % 3][1][j:j + 70] if j % 3 else rc(records[i % 3][1][j:j + 70]) for i, j in enumerate(range(0, 230, 1))]
    reads += [rand_seq(rng, 70) for _ in range(40)]
    rng.shuffle(reads)
    assert len(p.check(reads, 17)) > 100
    p.free()


def tandem(K, target, rng):
    """a transcript of a repeated 7-mer and a read of it whose votes number exactly `target`: with a read of seven windows
    every base more of the transcript is one vote more; other read lengths are tried where 7-mers repeat inside the unit"""
    unit = rand_seq(rng, 7)
    while len({unit[i:] + unit[:i] for i in range(7)}) < 7:
        unit = rand_seq(rng, 7)
    for extra in (6, 13, 7, 9):
        read = (unit * (K // 7 + 5))[:K + extra]
        z = max(K, target * 7 // (extra + 1) - 21)
        n = 0
        while n < target:
            zone = (unit * (z // 7 + 2))[:z]
            n = sum(R.frames_of(R.Index(K, [("rep", zone)]), read)[0].values())
            z += 1
        if n == target:
            return zone, read
    raise AssertionError("no transcript gives %d votes" % target)


@pytest.mark.parametrize("K", [5, 27, 32])
@pytest.mark.parametrize("target", [VOTES - 1, VOTES, VOTES + 1, 3 * VOTES + 5])
def test_tandem_repeats_around_the_vote_bound(ctx, K, target):
    """a read on a tandem repeat with VOTES - 1, VOTES, VOTES + 1 and about 3 x VOTES votes: the keys in LDS, full, and the walk per
    probe -- forward, reverse, with a byte that is no base, beside reads that have one frame; every draw against the restatement"""
    rng = random.Random(400 + K)
    zone, read = tandem(K, target, rng)
    other = stoppy(rng, 150)
    p = Placed(ctx, K, [("rep", zone), ("other", other)], 128)
    assert sum(R.frames_of(p.ref, read)[0].values()) == target or K == 5
    broken = read[:K + 3] + "N" + read[K + 4:] + read[:K + 2]
    reads = [read, other[20:20 + 60], rc(read), broken.lower(), rc(other[40:110]), read[:K]] * 3
    for seed in (17, 1, 2):
        p.check(reads, seed)
    p.free()


def test_the_draw_on_both_sides_of_a_frame_boundary(ctx):
    """seeds found on the CPU that put r on the last vote of the first frame and on the first vote of the next"""
    K = 27
    rng = random.Random(500)
    body = stoppy(rng, 200)
    p = Placed(ctx, K, [("t", body)], 128)
    read = body[5:60] + "T" + body[60:120]                    # two frames: offsets 5 and 4
    frames, _ = R.frames_of(p.ref, read)
    order = sorted(frames)
    assert len(order) == 2
    first_votes, n = frames[order[0]], sum(frames.values())
    found = {}
    for seed in range(100000):
        r = synth.stop_draw(seed, 0, n)
        if r in (first_votes - 1, first_votes) and r not in found:
            found[r] = seed
            if len(found) == 2:
                break
    assert len(found) == 2
    for r, frame in ((first_votes - 1, order[0]), (first_votes, order[1])):
        got = []
        p.check([read], found[r], frames=got)
        assert got == [frame]
    # the same read as read g of a run: the draw follows the ordinal
    for g in (1, 7, (1 << 32) + 5):
        got = []
        p.check([read], 17, first=g, frames=got)
        assert got[0] == R.pick(frames, synth.stop_draw(17, g, n))
    p.free()


def test_a_batch_cut_at_every_read_number(ctx):
    K = 25
    rng = random.Random(600)
    a = stoppy(rng, 260)
    p = Placed(ctx, K, [("t1", a), ("t2", a[:100] + stoppy(rng, 90))], 128)
    reads = [a[i:i + 60] if i % 2 else rc(a[i:i + 60]) for i in range(0, 130, 10)]
    whole = p.check(reads, 17)
    assert whole
    for cut in range(len(reads) + 1):
        parts = []
        for first, part in ((0, reads[:cut]), (cut, reads[cut:])):
            rc_, n, ot, ok = p.call(fastq_of(part), 17, first, cap=len(whole)) if part else (OK, 0, np.empty(0), np.empty(0))
            assert rc_ == OK
            parts += list(zip(ot[:n].tolist(), ok[:n].tolist()))
        assert sorted(parts) == whole, cut
    p.free()


def test_capacity_and_views(ctx):
    """one short of the stops needed, exactly them, and more: nothing written beyond, the count needed, repeatable; the text 5
    bytes into a larger buffer and the outputs 3 elements into guarded arrays"""
    K = 25
    rng = random.Random(700)
    a = stoppy(rng, 400)
    p = Placed(ctx, K, [("t", a)], 128)
    reads = [a[i:i + 90] if i % 2 else rc(a[i:i + 90]) for i in range(0, 300, 7)]
    text = fastq_of(reads)
    want = p.want(reads, 17)
    need = len(want)
    assert need > 20
    for cap in (1, need // 2, need - 1):
        rc_, n, ot, ok = p.call(text, 17, cap=cap, room=need + 64)
        assert (rc_, n) == (ENOSPC, need), cap
        assert np.all(ot[cap:] == G32) and np.all(ok[cap:] == G64), cap
    for cap in (need, need + 1, need + 50):
        rc_, n, ot, ok = p.call(text, 17, cap=cap)
        assert (rc_, n) == (OK, need), cap
        assert np.all(ot[need:] == G32) and np.all(ok[need:] == G64) and sorted(zip(ot[:n].tolist(), ok[:n].tolist())) == want
    rc_, n, ot, ok = p.call(text, 17, cap=need, lead=3)
    assert (rc_, n) == (OK, need) and np.all(ot[:3] == G32) and np.all(ok[:3] == G64)
    assert np.all(ot[3 + n:] == G32) and np.all(ok[3 + n:] == G64) and sorted(zip(ot[3:3 + n].tolist(), ok[3:3 + n].tolist())) == want
    raw = np.frombuffer(text.encode(), dtype=np.uint8)
    buf = ctx.upload(np.concatenate((np.full(5, ord("A"), np.uint8), raw, np.full(7, ord("C"), np.uint8))))
    view = buf.view(len(raw), 5)
    lines = ctx.line_ends(view)
    tx, kmers = ctx.stop_frames(p.table, p.starts, view, lines, lines.n // 4, K, 128, 17, 0)
    assert sorted(zip(tx.to_host().tolist(), kmers.to_host().tolist())) == want
    assert np.array_equal(buf.to_host()[5:5 + len(raw)], raw)
    p.free()


def test_empty_invalid_and_too_long(ctx):
    K, pad = 25, 100
    rng = random.Random(800)
    a = stoppy(rng, 150)
    p = Placed(ctx, K, [("t", a), ("u", stoppy(rng, 90))], pad)
    empty = Placed(ctx, K, [("t", "ACGT")], pad)                # a transcript shorter than K: a table without keys
    text = fastq_of([a[:60]])
    rc_, n, ot, ok = empty.call(text, 17, cap=10)
    assert (rc_, n) == (OK, 0) and np.all(ot == G32) and np.all(ok == G64)
    rc_, n, ot, ok = p.call(text, 17, cap=10, n_reads=0)
    assert (rc_, n) == (OK, 0) and np.all(ot == G32) and np.all(ok == G64)
    n64 = C.c_uint64(7)
    assert ctx.lib.zk_stop_frames(ctx.h, p.table.h, p.starts.ptr, p.starts.n, None, None, 0, K, pad, 17, 0, None, None, 0, C.byref(n64)) == OK
    assert n64.value == 0
    for bad in (2, 33, -1, 24):                                 # out of range, and not the table's K
        rc_, n, ot, ok = p.call(text, 17, cap=100, K=bad)
        assert rc_ == EINVAL and np.all(ot == G32) and np.all(ok == G64), bad
    assert ctx.lib.zk_stop_frames(ctx.h, None, None, 0, None, None, 0, K, pad, 17, 0, None, None, 0, C.byref(n64)) == EINVAL
    # a line of pad bytes that hits is the longest allowed; one more is refused before anything is written; one that hits nothing is not
    at = a[:40] + rand_seq(rng, pad - 40)
    p.check([at], 17)
    for long_read in (at + "A", rc(at + "A"), "  " + at + "C\t"):
        rc_, n, ot, ok = p.call(fastq_of([a[:60], long_read]), 17, cap=500)
        assert rc_ == ERANGE and b"longer than pad" in ctx.lib.zk_last_error(ctx.h)
        assert np.all(ot == G32) and np.all(ok == G64)
    p.check([a[:60], rand_seq(rng, 3 * pad), " " + at + "  "], 17)      # the context is still good
    p.free()
    empty.free()


# ---- zk_stop_nearest --------------------------------------------------------------------------------------------------------------
def popcount64(v):
    v = v - ((v >> np.uint64(1)) & np.uint64(0x5555555555555555))
    v = (v & np.uint64(0x3333333333333333)) + ((v >> np.uint64(2)) & np.uint64(0x3333333333333333))
    v = (v + (v >> np.uint64(4))) & np.uint64(0x0F0F0F0F0F0F0F0F)
    return (v * np.uint64(0x0101010101010101)) >> np.uint64(56)


def np_nearest(K, tx, kmers, lists, known):
    dist, near = np.empty(len(tx), np.uint32), np.empty(len(tx), np.uint64)
    for i, (t, x) in enumerate(zip(tx.tolist(), kmers.tolist())):
        ys = lists[t]
        if not len(ys):
            dist[i], near[i] = K + 1, x
            continue
        z = (ys >> np.uint64(3)) ^ np.uint64(x >> 3)
        d = popcount64((z | (z >> np.uint64(1))) & np.uint64(R.M1))
        j = int(np.argmin(d))                                   # the first minimum of an ascending list: the smallest y
        dist[i], near[i] = d[j], ys[j]
    return dist, near, np.isin(kmers, known).astype(np.uint8)


def run_nearest(ctx, K, tx, kmers, lists, known):
    """zk_stop_nearest into guarded arrays, checked against NumPy -> (dist, near, flags)"""
    tx, kmers, known = np.asarray(tx, np.uint32), np.asarray(kmers, np.uint64), np.asarray(known, np.uint64)
    lists = [np.asarray(l, np.uint64) for l in lists]
    offs = np.concatenate(([0], np.cumsum([len(l) for l in lists]))).astype(np.uint64)
    tk = np.concatenate(lists) if lists else np.empty(0, np.uint64)
    m = len(tx)
    d_tx, d_k, d_tk, d_offs, d_known = ctx.upload(tx), ctx.upload(kmers), ctx.upload(tk), ctx.upload(offs), ctx.upload(known)
    dist, near, flags = ctx.upload(np.full(m + 9, G32, np.uint32)), ctx.upload(np.full(m + 9, G64, np.uint64)), ctx.upload(np.full(m + 9, G8, np.uint8))
    rc_ = ctx.lib.zk_stop_nearest(ctx.h, d_tx.ptr, d_k.ptr, m, K, d_tk.ptr, d_offs.ptr, len(lists), d_known.ptr, len(known), dist.ptr, near.ptr, flags.ptr)
    assert rc_ == OK, ctx.lib.zk_last_error(ctx.h)
    hd, hn, hf = dist.to_host(), near.to_host(), flags.to_host()
    assert np.all(hd[m:] == G32) and np.all(hn[m:] == G64) and np.all(hf[m:] == G8)
    wd, wn, wf = np_nearest(K, tx, kmers, lists, known)
    assert np.array_equal(hd[:m], wd) and np.array_equal(hn[:m], wn) and np.array_equal(hf[:m], wf)
    assert np.array_equal(d_tx.to_host(), tx) and np.array_equal(d_k.to_host(), kmers)
    return hd[:m], hn[:m], hf[:m]


def rand_kmers(rng, K, n):
    return np.unique(np.array([rng.getrandbits(2 * K) for _ in range(n)], dtype=np.uint64))


@pytest.mark.parametrize("K", [3, 27, 32])
def test_nearest_list_sizes(ctx, K):
    """transcript lists of 0, 1, 63, 64, 65 and TILE - 1, TILE, TILE + 1, 2 TILE + 1 k-mers (at K = 3 as many as there are), a few
    entries each, all in one entry tile; an exact member; known and unknown"""
    rng = random.Random(900 + K)
    sizes = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
    lists = [rand_kmers(rng, K, s)[:s] if s else np.empty(0, np.uint64) for s in sizes]
    tx, kmers = [], []
    for t, l in enumerate(lists):
        xs = {rng.getrandbits(2 * K) for _ in range(4)} | ({int(l[len(l) // 2]), int(l[0]), int(l[-1])} if len(l) else set())
        tx += [t] * len(xs)
        kmers += sorted(xs)
    known = sorted(set(kmers[::3]))
    d, y, f = run_nearest(ctx, K, tx, kmers, lists, known)
    assert d[0] == K + 1 and y[0] == kmers[0] and 0 in d[4:] and f.sum() == sum(x in known for x in kmers) > 0
    assert len(tx) < ENTRIES


@pytest.mark.parametrize("m", [0, 1, ENTRIES - 1, ENTRIES, ENTRIES + 1, 3 * ENTRIES + 7])
def test_nearest_entry_counts(ctx, m):
    """entry counts around the entry tile, over transcripts of very different sizes, several of them inside one tile and one that
    spans tiles; K = 32 with the top bits set"""
    K = 32
    rng = random.Random(1000 + m)
    lists = [rand_kmers(rng, K, s) | np.uint64(1 << 63 if s % 2 else 0) for s in (5, 300, 0, TILE + 40, 70)]
    lists = [np.unique(l) for l in lists]
    tx = np.sort(np.array([rng.choice((0, 1, 1, 2, 3, 3, 3, 4)) for _ in range(m)], dtype=np.uint32))
    kmers = np.array([rng.getrandbits(64) | (1 << 63) for _ in range(m)], dtype=np.uint64)
    order = np.lexsort((kmers, tx))
    run_nearest(ctx, K, tx[order], kmers[order], lists, kmers[::2][np.argsort(kmers[::2])] if m else [])
    if m == 0:
        assert ctx.lib.zk_stop_nearest(ctx.h, None, None, 0, K, None, None, 0, None, 0, None, None, None) == OK
        assert ctx.lib.zk_stop_nearest(ctx.h, None, None, 0, 2, None, None, 0, None, 0, None, None, None) == EINVAL


def test_nearest_ties_go_to_the_smallest(ctx):
    """constructed ties: k-mers at the same distance in different parts of a tile, in different tiles, and two that differ only in
    the three bits the distance does not see"""
    K = 27
    x = 0x2AAAAAAAAAAAA8 & ((1 << (2 * K)) - 1)
    near = sorted({x ^ (1 << 10), x ^ (2 << 20), x ^ (3 << 40), x ^ 5, x ^ 2})        # all at distance 1 but the last two (0)
    rng = random.Random(1100)
    far = [int(v) for v in rand_kmers(rng, K, 2 * TILE + 300)]
    for keep in (near, near[:3], [near[0], near[4]], near[2:]):
        ys = np.unique(np.array(far + keep, dtype=np.uint64))
        d, y, f = run_nearest(ctx, K, [0], [x], [ys], [])
        best = min(R.ham(x >> 3, int(v) >> 3) for v in ys.tolist())
        assert d[0] == best and y[0] == min(int(v) for v in ys.tolist() if R.ham(x >> 3, int(v) >> 3) == best)
        assert R.nearest3(K, ys.tolist(), x)[:2] == (int(d[0]), int(y[0]))


def test_both_entries_in_a_row_are_the_restatements_rows(ctx):
    case = next(c for c in fixture_cases() if c["name"] == "k27_isoform")
    K, S = case["K"], case["S"]
    records = R.read_fasta(case["fasta"])
    p = Placed(ctx, K, records, 128)
    reads = R.read_fastq(case["inputs"][0])
    text = ctx.upload(np.frombuffer(case["inputs"][0].encode(), dtype=np.uint8))
    lines = ctx.line_ends(text)
    tx, kmers = ctx.stop_frames(p.table, p.starts, text, lines, lines.n // 4, K, 128, S, 0)
    ot, ok, cnt = ctx.pileup_count(tx, kmers, K)
    tk, offs = p.index.transcript_kmers()
    dist, near, flags = ctx.stop_nearest(ot, ok, K, ctx.upload(tk), ctx.upload(offs), ctx.upload(p.index.known_stops()))
    rows = R.rows(p.ref, R.count_stops(p.ref, reads, S))
    got = list(zip(flags.to_host().tolist(), ok.to_host().tolist(), cnt.to_host().tolist(), dist.to_host().tolist(), near.to_host().tolist(),
                   [p.index.names[t] for t in ot.to_host().tolist()]))
    assert got == [(int(r[0] == "known"),) + r[1:6] for r in rows] and len(rows) > 30
    p.free()


# ---- the command ------------------------------------------------------------------------------------------------------------------
INPUTS = {c["name"]: c for c in fixture_cases()}
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


def same_lines(case, text):
    """the fixture's lines, but for the nearest k-mer of the lines whose minimum is tied (the reference's choice is its set order)"""
    got, want = sorted(text.split("\n")[:-1]), case["lines"]
    strip = lambda l: l.split("\t")[:4] + l.split("\t")[5:]
    differ = sum(a != b for a, b in zip(got, want))
    return len(got) == len(want) and sorted(map(strip, got)) == sorted(map(strip, want)) and differ <= 2 * case["tied"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_command_on_the_fixture(ctx, case, tmp_path):
    args = write_case(case, str(tmp_path))
    code, out, err = run(["stop"] + args)
    assert code in (0, None) and err == "", err
    assert same_lines(case, out)
    assert out == "".join(l + "\n" for l in R.run(case["K"], case["fasta"], case["inputs"], case["S"]))      # order and ties included


def test_command_in_batches_and_in_a_process_of_its_own(ctx, tmp_path):
    from zotmer_amd.library import stopscan
    case = CASES[[c["name"] for c in CASES].index("k27_repeat_tail_two_files")]
    args = write_case(case, str(tmp_path))
    want = "".join(l + "\n" for l in R.run(case["K"], case["fasta"], case["inputs"], case["S"]))
    out, stats = io.StringIO(), {}
    index = stopscan.load_index(args[5], case["K"])
    stopscan.run(ctx, index, args[6:], case["S"], 4096, out, stats=stats)          # a few reads per batch, two files
    assert out.getvalue() == want and stats["reads"] == 200 and stats["lines"] == len(case["lines"])
    with pytest.raises(stopscan.InputError, match="longer than pad = 64"):
        stopscan.run(ctx, index, args[6:], case["S"], 1 << 20, io.StringIO(), pad=64)
    zot = os.path.join(ROOT, "zot")
    p = subprocess.run([sys.executable, zot, "stop"] + args, capture_output=True, text=True, timeout=120)
    assert (p.returncode, p.stdout, p.stderr) == (0, want, "")
