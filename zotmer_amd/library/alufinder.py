"""
`zot alu-finder` (zotmer/commands/alu-finder.py): insertion spurs from a pile-up of reads on reference zones.

The reference indexes every K-mer of its BED zones by (zone, position) (alu-finder.py:288-307), places each orientation of
each mate of every read pair on the diagonals its k-mers' anchors give and counts every window of the read at its place on
every diagonal (hits, alu-finder.py:116-147, 309-322), filters the counts (324-350) and walks the filtered pile-up for paths
that leave the reference (forwardSpurs / reverseSpurs, 164-218) -- printed raw, or shifted and joined (352-434).

Here the zones and the index are read on the host (load_zones); the index goes to the device as a bait table whose ids are
anchors on one u32 axis (Layout, anchor_table); the reads stream through in batches (fastq_batches.record_batches), one
zk_anchor_pileup and one zk_pileup_count per mate and batch; the counted lists are merged on the device (DevicePileup: one
zk_pileup_merge per list into a resident accumulator; Pileup is the host form: a lexsort and an add.reduceat over the
concatenation) and decoded back to acc[zone][position][k-mer]; the filter runs on the merged list (filter_counted); the spurs,
the shifts, the join and the printing are the reference's, restated.  What is printed does not depend on where the batches
are cut.
"""
import contextlib
import os
import sys
import time

import numpy as np

from zotmer_amd import native
from zotmer_amd.library import seqio
from zotmer_amd.library.fastq_batches import record_batches, whole

PAD = 1 << 16                   # free coordinates on either side of a zone: the longest sequence line that may hit one
MERGE_AT = 1 << 24              # counted pairs held before the host merges them

_BASES = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _BASES[ord(_c)] = _BASES[ord(_c.lower())] = _i
_BASES[ord("U")] = _BASES[ord("u")] = 3


class InputError(Exception):
    """an input the command refuses (the message goes to stderr, the exit status is 1)"""


# ---- zones --------------------------------------------------------------------------------------------------------------
def read_bed(path):
    """readBED (alu-finder.py:50-70) without the chromosome renaming: [(chrom, s, e, name), ...] in file order.  A first line
    that starts with `track` or `browser` is skipped; blank lines are skipped; a line without a name is refused."""
    zones = []
    with seqio.open_binary(path) as f:
        for n, raw in enumerate(f):
            t = raw.decode("latin-1").split()
            if not t or (n == 0 and t[0] in ("track", "browser")):
                continue
            if len(t) < 4:
                raise InputError("%s, line %d: a region needs a chromosome, a start, an end and a name" % (path, n + 1))
            try:
                s, e = int(t[1]), int(t[2])
            except ValueError:
                raise InputError("%s, line %d: start and end must be integers" % (path, n + 1))
            zones.append((t[0], s, e, t[3]))
    return zones


def read_chromosome(home, chrom):
    """SequenceFactory (alu-finder.py:72-95): the first record of <home>/<chrom>.fa, else of <home>/<chrom>.fa.gz, as bytes"""
    path = home + "/" + chrom + ".fa"
    if not os.path.exists(path):
        path += ".gz"
    if not os.path.exists(path):
        raise InputError("no reference sequence %s/%s.fa or .fa.gz" % (home, chrom))
    name, seq = None, []
    with seqio.open_binary(path) as f:
        for line in f:
            line = line.strip()
            if line[:1] == b">":
                if name is not None:
                    break
                name, seq = line, []
            else:
                seq.append(line)
    if name is None:
        raise InputError("%s: no FASTA record" % path)
    return b"".join(seq)


def kmers_with_pos(K, seq):
    """basics.kmersWithPosList(K, seq, False) with 0-based positions: (k-mers u64, positions i64) of the windows that hold
    only AaCcGgTtUu"""
    codes = _BASES[np.frombuffer(seq, dtype=np.uint8)]
    n = len(codes) - K + 1
    if n <= 0:
        return np.empty(0, np.uint64), np.empty(0, np.int64)
    bad = np.concatenate(([0], np.cumsum(codes == 4)))
    ok = (bad[K:] - bad[:-K]) == 0
    x = np.zeros(n, dtype=np.uint64)
    c = codes.astype(np.uint64) & np.uint64(3)
    for j in range(K):
        x = (x << np.uint64(2)) | c[j:j + n]
    pos = np.nonzero(ok)[0].astype(np.int64)
    return x[pos], pos


class Zones:
    """ref[name][p] = the reference k-mer at position p of the zone (refTbl), where[name] = (chrom, s, e) (zoneIdx), and the
    anchors (k-mer, name, p) of every window (refIdx)"""

    def __init__(self, K):
        self.K, self.ref, self.where = K, {}, {}
        self.xs, self.names, self.ps = [], [], []

    def add(self, chrom, s, e, name, chrom_seq):
        if name in self.where and self.where[name][0] != chrom:
            raise InputError("zone %s lies on %s and on %s" % (name, self.where[name][0], chrom))
        self.where[name] = (chrom, s, e)
        tbl = self.ref.setdefault(name, {})
        x, pos = kmers_with_pos(self.K, chrom_seq[s - 1:e])          # the reference's own slice, whatever s is
        pos = pos + s
        tbl.update(zip(pos.tolist(), x.tolist()))
        self.xs.append(x)
        self.ps.append(pos)
        self.names.append((name, len(x)))


def load_zones(bed, home, K):
    """alu-finder.py:286-307"""
    zones = Zones(K)
    seqs = {}
    for chrom, s, e, name in read_bed(bed):
        if chrom not in seqs:
            seqs[chrom] = read_chromosome(home, chrom)
        zones.add(chrom, s, e, name, seqs[chrom])
    return zones


# ---- the coordinate axis ---------------------------------------------------------------------------------------------------
class Layout:
    """Every (zone, position) that a read placed on an anchor can reach, on one u32 axis: the zones that have anchors, in name
    order, zone z at [base[z], base[z] + span[z] + 2 * pad), position p at base[z] + pad + (p - lo[z]).  An anchor's diagonal
    moved by less than pad either way stays inside its zone's piece, so a coordinate decodes to one (zone, position)."""

    def __init__(self, ranges, pad=PAD):
        """ranges: {name: (lowest, highest anchor position)}"""
        self.pad = int(pad)
        self.names = sorted(ranges)
        self.lo = np.array([ranges[nm][0] for nm in self.names], dtype=np.int64)
        span = np.array([ranges[nm][1] - ranges[nm][0] + 1 for nm in self.names], dtype=np.int64)
        ends = np.cumsum(span + 2 * self.pad)
        self.base = np.concatenate(([0], ends[:-1])).astype(np.int64) if len(ends) else np.empty(0, np.int64)
        self.total = int(ends[-1]) if len(ends) else 0
        if self.total >= (1 << 32) - 1:
            raise InputError("the zones and their margins span %d coordinates (at most 2^32 - 2)" % self.total)
        self.index = {nm: i for i, nm in enumerate(self.names)}

    def encode(self, name, pos):
        z = self.index[name]
        return self.base[z] + self.pad + (np.asarray(pos, dtype=np.int64) - self.lo[z])

    def decode(self, coords):
        """coordinates -> (zone numbers, positions)"""
        g = np.asarray(coords).astype(np.int64)
        z = np.searchsorted(self.base, g, side="right") - 1
        return z, g - self.base[z] - self.pad + self.lo[z]


def layout_of(zones, pad=PAD):
    ranges = {}
    for (name, n), pos in zip(zones.names, zones.ps):
        if n:
            lo, hi = int(pos.min()), int(pos.max())
            if name in ranges:
                lo, hi = min(lo, ranges[name][0]), max(hi, ranges[name][1])
            ranges[name] = (lo, hi)
    return Layout(ranges, pad)


def anchor_arrays(zones, layout):
    """the index as a bait table's arrays: (sorted distinct k-mers u64, offsets u32, anchors u32 ascending per k-mer)"""
    if not layout.names:
        return np.empty(0, np.uint64), np.zeros(1, np.uint32), np.empty(0, np.uint32)
    x = np.concatenate(zones.xs)
    g = np.concatenate([layout.encode(name, pos) if n else np.empty(0, np.int64) for (name, n), pos in zip(zones.names, zones.ps)])
    order = np.lexsort((g, x))
    x, g = x[order], g[order]
    keep = np.ones(len(x), dtype=bool)
    keep[1:] = (x[1:] != x[:-1]) | (g[1:] != g[:-1])
    x, g = x[keep], g[keep]
    heads = np.ones(len(x), dtype=bool)
    heads[1:] = x[1:] != x[:-1]
    starts = np.nonzero(heads)[0]
    return x[starts], np.concatenate((starts, [len(x)])).astype(np.uint32), g.astype(np.uint32)


def anchor_table(ctx, zones, layout):
    keys, offs, ids = anchor_arrays(zones, layout)
    return ctx.bait_table_from_arrays(zones.K, ctx.upload(keys), ctx.upload(offs), ctx.upload(ids), max(layout.total, 1))


# ---- the pile-up -------------------------------------------------------------------------------------------------------------
class Pileup:
    """The counted (coordinate, k-mer) pairs of everything added so far, on the host.  Lists wait in `parts` until MERGE_AT
    pairs have gathered, then one lexsort and one add.reduceat over their concatenation make them one."""

    def __init__(self, merge_at=MERGE_AT):
        self.parts, self.waiting, self.merge_at = [], 0, merge_at
        self.merge_seconds, self.merges, self.pairs = 0.0, 0, 0

    def add(self, coords, kmers, counts):
        if len(coords):
            self.parts.append((coords, kmers, counts.astype(np.uint64)))
            self.waiting += len(coords)
            self.pairs += len(coords)
        if self.waiting >= self.merge_at:
            self.merge()

    def merge(self):
        if len(self.parts) > 1:
            t0 = time.perf_counter()
            c = np.concatenate([p[0] for p in self.parts])
            x = np.concatenate([p[1] for p in self.parts])
            n = np.concatenate([p[2] for p in self.parts])
            order = np.lexsort((x, c))
            c, x, n = c[order], x[order], n[order]
            heads = np.ones(len(c), dtype=bool)
            heads[1:] = (c[1:] != c[:-1]) | (x[1:] != x[:-1])
            starts = np.nonzero(heads)[0]
            self.parts = [(c[starts], x[starts], np.add.reduceat(n, starts))]
            self.merge_seconds += time.perf_counter() - t0
            self.merges += 1
        self.waiting = 0

    def add_device(self, oc, ok, cnt):
        """the three views of Context.pileup_count"""
        self.add(oc.to_host(), ok.to_host(), cnt.to_host())

    def result(self):
        self.merge()
        if not self.parts:
            return np.empty(0, np.uint32), np.empty(0, np.uint64), np.empty(0, np.uint64)
        return self.parts[0]


class DevicePileup:
    """Pileup with the list kept on the device: every counted list is merged straight into one accumulated list
    (zk_pileup_merge), which lives in one of two array triples and is written into the other.  The triples grow geometrically
    to na + nb before a merge, so a merge never needs a second try.  When the next pair of triples would take more than
    `limit` bytes (default: half of the device memory free now), or an allocation fails, the list goes down into a host
    Pileup once and the run continues there."""

    DTYPES = (np.uint32, np.uint64, np.uint64)
    ENTRY_BYTES = 20

    def __init__(self, ctx, limit=None):
        self.ctx = ctx
        self.limit = int(limit) if limit is not None else ctx.mem_info()[0] // 2
        self.cur, self.alt, self.n = None, None, 0
        self.host, self._down = None, None
        self._merge_seconds, self._merges, self.pairs = 0.0, 0, 0

    @property
    def merges(self):
        return self._merges + (self.host.merges if self.host is not None else 0)

    @property
    def merge_seconds(self):
        return self._merge_seconds + (self.host.merge_seconds if self.host is not None else 0.0)

    @staticmethod
    def _cap(triple):
        return triple[0].n if triple is not None else 0

    def _triple(self, need, other):
        """a triple of need + need / 2 entries, or None: beside `other` it would pass the limit, or the device has no room"""
        cap = need + need // 2
        if self.ENTRY_BYTES * (cap + self._cap(other)) > self.limit:
            cap = need
            if self.ENTRY_BYTES * (cap + self._cap(other)) > self.limit:
                return None
        got = []
        try:
            for dt in self.DTYPES:
                got.append(self.ctx.empty(cap, dt))
        except native.ZotkError as e:
            if e.code != native.ZK_ENOMEM:
                raise
            for a in got:
                a.free()
            return None
        return tuple(got)

    def _hand_over(self):
        self.host = Pileup()
        if self.n:
            self.host.add(*[a.to_host(self.n) for a in self.cur])
        for t in (self.cur, self.alt):
            for a in t or ():
                a.free()
        self.cur, self.alt, self.n = None, None, 0

    def add_device(self, oc, ok, cnt):
        """the three views of Context.pileup_count, or any counted list on the device with u32 or u64 counts"""
        nb = oc.n
        assert ok.n == nb == cnt.n and oc.dtype.itemsize == 4 and ok.dtype.itemsize == 8 and cnt.dtype.itemsize in (4, 8)
        if nb == 0:
            return
        self.pairs += nb
        self._down = None
        if self.host is not None:
            return self.host.add(oc.to_host(), ok.to_host(), cnt.to_host())
        ctx = self.ctx
        if self.n == 0:
            if self._cap(self.cur) < nb:
                for a in self.cur or ():
                    a.free()
                self.cur = None
                self.cur = self._triple(nb, self.alt)
                if self.cur is None:
                    self._hand_over()
                    return self.host.add(oc.to_host(), ok.to_host(), cnt.to_host())
            ctx._check(ctx.lib.zk_copy(ctx.h, self.cur[0].ptr, oc.ptr, 4 * nb))
            ctx._check(ctx.lib.zk_copy(ctx.h, self.cur[1].ptr, ok.ptr, 8 * nb))
            if cnt.dtype.itemsize == 8:                         # a list that was merged before, or one from the host
                ctx._check(ctx.lib.zk_copy(ctx.h, self.cur[2].ptr, cnt.ptr, 8 * nb))
            else:
                ctx._check(ctx.lib.zk_widen_counts(ctx.h, cnt.ptr, self.cur[2].ptr, nb))
            ctx.sync()
            self.n = nb
            return
        t0 = time.perf_counter()
        if self._cap(self.alt) < self.n + nb:
            for a in self.alt or ():
                a.free()
            self.alt = None
            self.alt = self._triple(self.n + nb, self.cur)
            if self.alt is None:
                self._hand_over()
                return self.host.add(oc.to_host(), ok.to_host(), cnt.to_host())
        n, fit = ctx.pileup_merge_into(tuple(a.view(self.n) for a in self.cur), (oc, ok, cnt), self.alt)
        assert fit
        self.cur, self.alt, self.n = self.alt, self.cur, n
        self._merge_seconds += time.perf_counter() - t0
        self._merges += 1

    def add(self, coords, kmers, counts):
        """a list from the host (as Pileup.add takes it)"""
        if len(coords):
            self.add_device(self.ctx.upload(coords, np.uint32), self.ctx.upload(kmers, np.uint64), self.ctx.upload(counts, np.uint64))

    def result(self):
        """the merged list on the host: one download"""
        if self.host is not None:
            return self.host.result()
        if self._down is None:
            self._down = tuple(a.to_host(self.n) if self.n else np.empty(0, dt) for a, dt in zip(self.cur or self.DTYPES, self.DTYPES))
        return self._down

    def device_result(self):
        """the merged list as three DeviceArray views (u32, u64, u64 counts); uploaded after a handover.  The views lie in the
        accumulator's own arrays: they are valid until the next add or add_device, which may write over them or free them."""
        if self.host is not None:
            return tuple(self.ctx.upload(a, dt) for a, dt in zip(self.host.result(), self.DTYPES))
        if self.cur is None:
            return tuple(self.ctx.empty(0, dt) for dt in self.DTYPES)
        return tuple(a.view(self.n) for a in self.cur)


def pile_inputs(ctx, table, K, pad, inputs, batch, pileup, verbose=False):
    """alu-finder.py:309-322: the inputs in pairs (1,2), (3,4), ... (a trailing unpaired one is ignored, reads.py:78), both
    mates of every pair piled up.  Returns the number of read pairs."""
    n_reads = 0
    bufs = None
    for i in range(0, len(inputs) - 1, 2):
        paths = inputs[i:i + 2]
        with contextlib.closing(record_batches(ctx, paths, batch, warn_unequal=True)) as batches:
            for texts, lines, r, _ in batches:
                for text, ln in zip(texts, lines):
                    try:
                        coords, kmers = ctx.anchor_pileup(table, text, ln, r, K, pad, out=bufs)
                    except native.ZotkError as e:
                        if e.code != native.ZK_ERANGE:
                            raise
                        raise InputError("%s: %s" % (" & ".join(paths), str(e).split(": ", 1)[-1]))
                    bufs = (whole(coords), whole(kmers))
                    pileup.add_device(*ctx.pileup_count(coords, kmers, K))
                n_reads += r
                if verbose:
                    sys.stderr.write("%s: %d read pairs processed\n" % (" & ".join(os.path.basename(p) for p in paths), n_reads))
    return n_reads


def decode_acc(layout, coords, kmers, counts):
    """the counted list as the reference's acc[zone][position][k-mer] = count"""
    acc = {}
    z, pos = layout.decode(coords)
    for zi, p, x, c in zip(z.tolist(), pos.tolist(), np.asarray(kmers).tolist(), np.asarray(counts).tolist()):
        acc.setdefault(layout.names[zi], {}).setdefault(p, {})[x] = c
    return acc


def filter_counted(coords, kmers, counts, V, C):
    """alu-finder.py:324-350 on the counted list, ascending by (coordinate, k-mer): within a position, the k-mers that share
    all but their last base form a group; a k-mer with fewer than C copies, or fewer than V times its group's, is dropped.
    The k-mers of a group are neighbours in the list, so a group's sum is one add.reduceat; the comparisons are the reference's
    (an int against V times an int, in doubles: exact while the counts stay below 2^53) -> the entries that stay"""
    if not len(coords):
        return coords, kmers, counts
    g = np.asarray(kmers) >> np.uint64(2)
    heads = np.ones(len(g), dtype=bool)
    heads[1:] = (coords[1:] != coords[:-1]) | (g[1:] != g[:-1])
    starts = np.nonzero(heads)[0]
    sums = np.add.reduceat(np.asarray(counts, dtype=np.uint64), starts)[np.cumsum(heads) - 1]
    c = np.asarray(counts).astype(np.float64)
    keep = ~((c < V * sums.astype(np.float64)) | (np.asarray(counts).astype(np.int64) < C))
    return coords[keep], kmers[keep], counts[keep]


# ---- the reference's host stages, restated -----------------------------------------------------------------------------------
def _follows(K, x, y):
    return (x & ((1 << (2 * (K - 1))) - 1)) == (y >> 2)


def _spurs(K, ref, Z, step):
    """forwardSpurs (step = 1) / reverseSpurs (step = -1), alu-finder.py:164-218: from every position whose reference k-mer was
    seen, the paths through the pile-up that follow one another base by base and never step onto the reference k-mer of their
    position; a path ends where nothing follows.  Yields (position, sorted paths of (k-mer, count))."""
    for p0 in sorted(ref):
        x0 = ref[p0]
        if p0 not in Z or x0 not in Z[p0]:
            continue
        done, live = [], [[(x0, Z[p0][x0])]]
        p = p0 + step
        while p in Z and live:
            grown = []
            for path in live:
                tip = path[-1][0] if step > 0 else path[0][0]
                extended = False
                for y, c in Z[p].items():
                    if not (_follows(K, tip, y) if step > 0 else _follows(K, y, tip)):
                        continue
                    if ref.get(p) == y:
                        continue
                    grown.append(path + [(y, c)] if step > 0 else [(y, c)] + path)
                    extended = True
                if not extended:
                    done.append(path)
            live = grown
            p += step
        yield p0, sorted(done + live)


def _shifts(ref, Z, S, p, path, step):
    """shiftForwardSpur (step = -1: the anchor moves left, reference k-mers join the front) / shiftReverseSpur (step = 1),
    alu-finder.py:227-255"""
    for i in range(S):
        yield p, path, i
        p += step
        if p not in ref or p not in Z or ref[p] not in Z[p]:
            return
        link = [(ref[p], Z[p][ref[p]])]
        path = link + path if step < 0 else path + link


def _text(K, xs):
    """renderPath (alu-finder.py:156-162)"""
    first = "".join("ACGT"[(xs[0] >> (2 * (K - 1 - j))) & 3] for j in range(K))
    return first + "".join("ACGT"[x & 3] for x in xs[1:])


RAW_HEADER = "\t".join(["chrom", "pos", "side", "label", "anchor", "insSeq"])
JOIN_HEADER = "\t".join(["chrom", "after", "before", "label", "rhsShift", "lhsShift", "lhsAnc", "rhsAnc", "lhsSeq", "rhsSeq"])


def report_lines(K, acc, zones, L, S, raw):
    """alu-finder.py:352-434 over the filtered acc: the lines the reference prints, without their newlines"""
    yield RAW_HEADER if raw else JOIN_HEADER
    for z in sorted(acc):
        ch, st, en = zones.where[z]
        Z, ref = acc[z], zones.ref[z]
        after, before = {}, {}
        for p, paths in _spurs(K, ref, Z, 1):
            if p + K - 1 == en:
                continue
            for path in paths:
                if len(path) < L:
                    continue
                if raw:
                    seq = _text(K, [x for x, _ in path])
                    yield "%s\t%d\t%s\t%s\t%s\t%s\t%s" % (ch, p + K - 1, "after", z, seq[:K], seq[K:], ",".join(str(c) for _, c in path))
                    continue
                for q, shifted, v in _shifts(ref, Z, S, p, path, -1):
                    seq = _text(K, [x for x, _ in shifted])
                    after.setdefault(q + K - 1, []).append((v, seq[:K], seq[K:]))
        for p, paths in _spurs(K, ref, Z, -1):
            if p == st:
                continue
            for path in paths:
                if len(path) < L:
                    continue
                if raw:
                    seq = _text(K, [x for x, _ in path])
                    yield "%s\t%d\t%s\t%s\t%s\t%s\t%s" % (ch, p, "before", z, seq[-K:], seq[:-K], ",".join(str(c) for _, c in path))
                    continue
                for q, shifted, v in _shifts(ref, Z, S, p, path, 1):
                    seq = _text(K, [x for x, _ in shifted])
                    before.setdefault(q, []).append((v, seq[-K:], seq[:-K]))
        for p0 in sorted(after):
            for av, a_anc, a_ins in after[p0]:
                for bv, b_anc, b_ins in before.get(p0 + 1, ()):
                    if b_anc in a_ins or a_anc in b_ins:
                        continue
                    yield "%s\t%d\t%d\t%s\t%d\t%d\t%s\t%s\t%s\t%s" % (ch, p0, p0 + 1, z, av, bv, a_anc, b_anc, a_ins, b_ins)


def run(ctx, zones, inputs, C, L, S, V, raw, batch, out, pad=PAD, verbose=False, stats=None, pileup=None):
    """the whole command behind its argument checks.  pileup: where the counted lists gather (None: a DevicePileup)"""
    K = zones.K
    layout = layout_of(zones, pad)
    pileup = pileup if pileup is not None else DevicePileup(ctx)
    n_reads = 0
    t0 = time.perf_counter()
    if layout.names:
        table = anchor_table(ctx, zones, layout)
        try:
            n_reads = pile_inputs(ctx, table, K, layout.pad, inputs, batch, pileup, verbose)
        finally:
            table.free()
    coords, kmers, counts = pileup.result()
    t1 = time.perf_counter()
    acc = decode_acc(layout, *filter_counted(coords, kmers, counts, V, C))
    t2 = time.perf_counter()
    for line in report_lines(K, acc, zones, L, S, raw):
        out.write(line + "\n")
    if stats is not None:
        stats.update(read_pairs=n_reads, counted_pairs=pileup.pairs, distinct_pairs=len(coords), merges=pileup.merges,
                     merge_seconds=pileup.merge_seconds, pile_up_seconds=t1 - t0, decode_filter_seconds=t2 - t1,
                     report_seconds=time.perf_counter() - t2)
    return 0
