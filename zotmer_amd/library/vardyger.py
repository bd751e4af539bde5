"""
`zot vardyger` (zotmer/commands/vardyger.py): in-frame tandem duplications over a panel of sequences, from single reads.

The reference's main ends at line 401 in debugging traces; the caller proper (lines 403-506) is complete but nothing reaches
it.  This is that caller.  Per FASTA record n the reference keeps the forward K-mers as baits and, with J = K / 2, the two
halves of each (lines 289-334).  A read counts for every record that holds one of its K-mers of either strand, and all its
K-mers of both strands are counted for that record (lines 338-354); K-mers counted at least ten times stay (line 361).
findDup (lines 82-94) then names the tuples (a, b, c, d) of half-mers with ab and cd K-mers of the record, cb and cd counted,
a != c and b != d, and positions (lines 115-133) places ab and cd on the record, cd more than J behind ab.

Here the reads go through `zot hgvs-find`'s capture on single reads (zk_capture_hits with read_K = K against a both-strand
bait table, zk_capture_kmers, zk_pileup_count, zk_pileup_merge into alufinder.DevicePileup), and one zk_dup_join (csrc/dup_join.hip) turns the merged list
and the records' occurrence table into the rows of findDup + positions and the coverage of every window.  The same kernel,
given the records' own K-mers as the counted list, gives the phantom warnings of line 332.  The filters, the strict path check
(hgvsfind.paths) and the table are the reference's, restated over the rows.  What is printed does not depend on where the
batches are cut.
"""
import contextlib
import os
import sys
import time

import numpy as np

from zotmer_amd.library import capture, hgvsfind, seqio
from zotmer_amd.library.alufinder import DevicePileup
from zotmer_amd.library.fastq_batches import record_batches, whole
from zotmer_amd.library.hgvsfind import EMIT_BUDGET, InputError, render

THRESHOLD = 10          # vardyger.py:361: a constant, not -m
HEADER = ("n", "left", "leftCov", "mid", "midCov", "right", "rightCov", "len", "vaf", "hgvs")


# ---- the index ---------------------------------------------------------------------------------------------------------------
_CODES = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODES[ord(_c)] = _CODES[ord(_c.lower())] = _i
_CODES[ord("U")] = _CODES[ord("u")] = 3


def _windows(K, seqs):
    """basics.kmersWithPosList(K, seq, False) of every sequence at once -> (record u32, K-mer u64, 1-based position u32) of the
    windows that hold only AaCcGgTtUu, in (record, position) order"""
    text = np.frombuffer("\n".join(seqs).encode("latin-1", "replace"), dtype=np.uint8)
    n = len(text) - K + 1
    if n <= 0:
        return np.empty(0, np.uint32), np.empty(0, np.uint64), np.empty(0, np.uint32)
    codes = _CODES[text]
    bad = np.concatenate(([0], np.cumsum(codes == 4)))
    x = np.zeros(n, dtype=np.uint64)
    for t in range(K):
        x = (x << np.uint64(2)) | (codes[t:t + n] & 3).astype(np.uint64)
    ok = np.nonzero(bad[K:K + n] == bad[:n])[0]
    starts = np.cumsum([0] + [len(s) + 1 for s in seqs])[:-1]
    rec = np.searchsorted(starts, ok, side="right") - 1
    return rec.astype(np.uint32), x[ok], (ok - starts[rec] + 1).astype(np.uint32)


class Index:
    """vardyger.py:289-334 without the dicts: the records, and every window of every record as (record, K-mer, 1-based
    position) ascending -- the occurrence table of zk_dup_join -- with its order by (record, second half, first half,
    position) and, per record, its windows in position order (the coverage line walks them so)."""

    def __init__(self, K, records):
        if K < 2 or K > 32 or K & 1:
            raise InputError("K must be even, 2..32")
        self.K, self.J = K, K // 2
        self.names = [nm for nm, _ in records]
        seen = set()
        for nm in self.names:
            if nm in seen:
                raise InputError("two sequences are named %s" % nm)
            seen.add(nm)
        self.seqs = [seq for _, seq in records]
        rs, rk, rp = _windows(K, self.seqs)          # in (record, position) order
        cuts = np.searchsorted(rs, np.arange(len(self.seqs) + 1, dtype=np.uint32)).tolist()
        order = np.lexsort((rp, rk, rs))
        self.rseq, self.rkmer, self.rpos = rs[order], rk[order], rp[order]
        low = np.uint64((1 << K) - 1)                # a half is J bases = K bits
        self.first, self.second = self.rkmer >> np.uint64(K), self.rkmer & low
        self.by_second = np.lexsort((self.rpos, self.first, self.second, self.rseq)).astype(np.uint32)
        self.cuts = cuts                             # record n's windows are occurrences walk[cuts[n]:cuts[n + 1]], by position
        self.walk = np.empty(len(order), dtype=np.int64)
        self.walk[order] = np.arange(len(order))

    @property
    def m(self):
        return len(self.rseq)

    def own_list(self):
        """the records' own K-mers as a counted list: distinct (record, K-mer), every count 1"""
        heads = np.ones(self.m, dtype=bool)
        heads[1:] = (self.rseq[1:] != self.rseq[:-1]) | (self.rkmer[1:] != self.rkmer[:-1])
        return self.rseq[heads], self.rkmer[heads], np.ones(int(heads.sum()), dtype=np.uint32)


def load_index(path, K):
    return Index(K, [(nm, seq.decode("latin-1")) for nm, seq in seqio.fasta_records(path)])


class DeviceIndex:
    """the occurrence table on the device"""

    def __init__(self, ctx, index):
        self.arrays = tuple(ctx.upload(a) for a in (index.rseq, index.rkmer, index.rpos, index.by_second))


# ---- the join ----------------------------------------------------------------------------------------------------------------
def join(ctx, dev, index, baits, kmers, counts, min_count, bufs=None):
    """one zk_dup_join -> (cover per occurrence, rows): rows is an int64 array [r, 3] of (entry, occurrence of ab, occurrence
    of cd) in ascending (record, c, b, d, a, pa, pc) order.  The kernel's order is (record, c, b, a, pa, d, pc)."""
    if index.m == 0:
        return np.zeros(0, np.uint32), np.zeros((0, 3), np.int64)
    return join_device(ctx, dev, index, (ctx.upload(baits.astype(np.uint32)), ctx.upload(kmers.astype(np.uint64)), ctx.upload(counts.astype(np.uint32))),
                       min_count, bufs)


def join_device(ctx, dev, index, counted, min_count, bufs=None):
    """join with the counted list on the device already: (baits u32, k-mers u64, counts u32) DeviceArrays"""
    if index.m == 0:
        return np.zeros(0, np.uint32), np.zeros((0, 3), np.int64)
    cover, e, i, j = ctx.dup_join(*counted, *dev.arrays, index.K, min_count, out=bufs)
    return cover, order_rows(index, e, i, j)


def order_rows(index, e, i, j):
    """the rows of zk_dup_join in ascending (record, c, b, d, a, pa, pc) order, as an int64 array [r, 3]"""
    e, i, j = np.asarray(e, np.int64), np.asarray(i, np.int64), np.asarray(j, np.int64)
    order = np.lexsort((index.rpos[j], index.rpos[i], index.first[i], index.second[j], e))      # e ascends by (record, c, b)
    return np.stack([e[order], i[order], j[order]], axis=1)


def phantom_warnings(index, rows):
    """vardyger.py:323-332 from the rows of the records' own K-mers (spelling kept)"""
    K = index.K
    for _, i, j in rows.tolist():
        ab, cd = int(index.rkmer[i]), int(index.rkmer[j])
        cb = (cd >> K) << K | (ab & ((1 << K) - 1))
        yield "warning: phantom dumplication: %s-%s-%s (%d)" % (render(K, ab), render(K, cb), render(K, cd), int(index.rpos[j]) - int(index.rpos[i]))


# ---- the capture -------------------------------------------------------------------------------------------------------------
def capture_inputs(ctx, table, K, inputs, batch, budget, pileup, read_counts, stats, verbose=False, err=None):
    """vardyger.py:338-354: reads.reads(inputs, both=True), single reads, file by file, through hgvs-find's capture"""
    err = err or sys.stderr
    emitter = hgvsfind.Emitter(ctx, K, budget, pileup, stats)
    pairs_buf = None
    for path in inputs:
        n_reads = 0
        with contextlib.closing(record_batches(ctx, [path], batch)) as batches:
            for texts, lines, r, _ in batches:
                t0 = time.perf_counter()
                pairs_buf = ctx.capture_hits(table, K, texts[0], lines[0], r, out=whole(pairs_buf))
                stats["lookup_seconds"] += time.perf_counter() - t0
                stats["batches"] += 1
                if pairs_buf.n:
                    hit = (pairs_buf.to_host() >> np.uint64(32)).astype(np.int64)
                    read_counts += np.bincount(hit, minlength=len(read_counts))
                    emitter.emit(pairs_buf, (texts[0], None), (lines[0], None), r)
                n_reads += r
                if verbose:
                    err.write("%s: %d reads\n" % (os.path.basename(path), n_reads))
        stats["reads"] += n_reads


# ---- the filters and the table -----------------------------------------------------------------------------------------------
def coverage_line(index, cover, n):
    """vardyger.py:371-376: '.' for a window whose K-mer stayed, 'X' for one that did not"""
    c = cover[index.walk[index.cuts[n]:index.cuts[n + 1]]]
    return "".join("." if v >= THRESHOLD else "X" for v in c.tolist())


def best_path(K, xs, xb, xe, n):
    """Interpolator.interpolate (debruijn.py:164-176): the path of n K-mers with the largest summed coverage, the first of
    equals in hgvsfind.paths' ascending order; None without a path of positive coverage"""
    best, best_sum = None, 0
    for p in hgvsfind.paths(K, xs, xb, xe, n):
        s = sum(xs[x] for x in p)
        if s > best_sum:
            best, best_sum = p, s
    return best


def table_rows(index, counted, cover, rows, min_cov, report_all, strict, stats):
    """vardyger.py:420-506 -> the lines of the table without the column n"""
    K, J = index.K, index.J
    kept = {}
    t_strict = 0.0
    for e, i, j in rows.tolist():
        n = int(index.rseq[i])
        ab, cd, cb = int(index.rkmer[i]), int(index.rkmer[j]), int(counted.kmers[e])
        pa, pc = int(index.rpos[i]), int(index.rpos[j])
        dd = pc - pa
        if not report_all and dd % 3 != 0:
            continue
        if strict:
            t0 = time.perf_counter()
            if n not in kept:
                seg = counted.segment(n)
                keep = seg.counts >= THRESHOLD
                kept = {n: dict(zip(seg.kmers[keep].tolist(), seg.counts[keep].tolist()))}      # the rows ascend by record: one at a time
            xs = kept[n]
            fst = best_path(K, xs, ab, cb, dd + 1)
            snd = best_path(K, xs, cb, cd, dd + 1) if fst is not None else None
            t_strict += time.perf_counter() - t0
            if fst is None or snd is None or fst[J:-J] != snd[J:-J]:
                continue
        cov = lambda c: c if c >= THRESHOLD else 0                  # xs.get(x, 0)
        cab, ccb, ccd = cov(int(cover[i])), cov(int(counted.counts[e])), cov(int(cover[j]))
        if cab < min_cov or ccb < min_cov or ccd < min_cov:
            continue
        w = ccb / ((cab + ccd) / 2.0)
        pb, pd = pa + J, pc + J
        yield "%s\t%d\t%s\t%d\t%s\t%d\t%d\t%g\t%s:c.%d_%ddup" % (render(K, ab), cab, render(K, cb), ccb, render(K, cd), ccd, dd, w,
                                                                  index.names[n], pb, pd - 1)
    stats["strict_seconds"] += t_strict


def new_stats():
    return dict(reads=0, batches=0, slices=0, entries=0, lookup_seconds=0.0, emission_seconds=0.0, count_seconds=0.0, merge_seconds=0.0,
                join_seconds=0.0, strict_seconds=0.0, format_seconds=0.0, distinct_entries=0, occurrences=0, candidate_rows=0, rows=0,
                phantoms=0)


def run(ctx, index, inputs, min_cov, report_all, strict, batch, out, budget=EMIT_BUDGET, verbose=False, err=None, stats=None, pileup=None):
    """the whole command behind its argument checks.  pileup: where the counted lists gather (None: a DevicePileup)"""
    err = err or sys.stderr
    stats = stats if stats is not None else new_stats()
    for k, v in new_stats().items():
        stats.setdefault(k, v)
    K, N = index.K, len(index.names)
    stats["occurrences"] = index.m
    pileup = pileup if pileup is not None else DevicePileup(ctx)
    read_counts = np.zeros(N, dtype=np.int64)
    dev = DeviceIndex(ctx, index)
    t0 = time.perf_counter()
    _, rows = join(ctx, dev, index, *index.own_list(), 1)
    stats["join_seconds"] += time.perf_counter() - t0
    stats["phantoms"] = len(rows)
    for line in phantom_warnings(index, rows):
        err.write(line + "\n")
    if index.m:
        table = capture.build_table(ctx, [(nm.encode("latin-1"), seq.encode("latin-1")) for nm, seq in zip(index.names, index.seqs)], K)
        try:
            capture_inputs(ctx, table, K, inputs, batch, budget, pileup, read_counts, stats, verbose, err)
        finally:
            table.free()
    baits, kmers, counts = pileup.result()
    stats["merge_seconds"] = pileup.merge_seconds
    stats["merges"] = pileup.merges
    stats["distinct_entries"] = len(baits)
    on_device = None
    if isinstance(pileup, DevicePileup):
        on_device = hgvsfind.device_list(ctx, pileup, "join")
    elif len(counts) and int(counts.max()) >= 1 << 32:
        raise InputError("a k-mer was counted %d times, more than the join's 32-bit counts hold" % int(counts.max()))
    counted = hgvsfind.Counted(baits, kmers, counts, N)
    t0 = time.perf_counter()
    cover, rows = join_device(ctx, dev, index, on_device, THRESHOLD) if on_device is not None else join(ctx, dev, index, baits, kmers, counts, THRESHOLD)
    stats["join_seconds"] += time.perf_counter() - t0
    stats["candidate_rows"] = len(rows)
    t0 = time.perf_counter()
    if verbose:
        for n in range(N):
            err.write(coverage_line(index, cover, n) + "\n")
    vn = 0
    for line in table_rows(index, counted, cover, rows, min_cov, report_all, strict, stats):
        if vn == 0:
            out.write("\t".join(HEADER) + "\n")
        vn += 1
        out.write("%d\t%s\n" % (vn, line))
    out.flush()
    stats["rows"] = vn
    stats["format_seconds"] += time.perf_counter() - t0 - stats["strict_seconds"]
    return 0
