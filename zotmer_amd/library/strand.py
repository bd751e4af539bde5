"""
`zot strand` on the device (zotmer/commands/strand.py, the mode without -r): per-k-mer counts with the orientation kept.

The reference walks every read pair's k-mers -- mate 1 forward, mate 2 reverse-complemented (strand.py:59) -- through a
dict keyed by the oriented k-mer, keeping the k-mers whose canonical form passes a hash sample (strand.py:130-140), and
prints per canonical k-mer the two orientations' counts (strand.py:142-155).  Here the input text streams onto the device
in batches cut at record ends (fastq_batches.record_batches); each batch is one zk_strand_keys per mate (the kept windows
as tagged keys (c << 1) | (oriented != c), into one buffer) and one zk_sort_count on 2K + 1 bits; the batch tables are
union-summed into a running table like a binary counter (two tables of a level make one of the next, as
engine.KmerTable does); at the end zk_strand_pairs pairs the neighbours and zk_format_pairs writes the lines, which the
host prints chunk by chunk.  The output does not depend on where the batches are cut.
"""
import contextlib
import os
import sys

import numpy as np

from zotmer_amd import native
from zotmer_amd.library.fastq_batches import record_batches, whole
from zotmer_amd.library.timing import Phase

SEED = 17                   # strand.py:137,148
FORMAT_CHUNK = 1 << 22      # pairs formatted and printed at a time


def threshold(K, p):
    """strand.py:66,72-73: M = 4**K - 1 and T = int(M * p), in Python's own arithmetic.  (z & M) <= M always, so a T above M
    is M; a negative T keeps nothing (None)."""
    M = (1 << (2 * K)) - 1
    T = int(M * p)
    return None if T < 0 else min(T, M)


class StrandTable:
    """Sorted distinct tagged keys + counts on the device, grown batch by batch.  The tables sit on a stack and are
    union-summed pairwise like a binary counter (engine.KmerTable._merge_top): n batches cost O(n log n) table traffic.
    Counts are 32-bit, as zk_sort_count leaves them, while the windows counted into the two tables of a merge add up to less
    than 2^32 (no count can wrap then); from there on they are widened to 64 bits first."""

    def __init__(self, ctx, K, T):
        self.ctx, self.K, self.T = ctx, K, T
        self.stack = []             # [(keys, counts, level, windows counted into it)]
        self.keys_buf = self.uniq_buf = self.cnt_buf = None
        self.windows = 0

    def _keys(self, text, lines, r, reverse, offset, est):
        """one mate's kept keys into keys_buf[offset:] -> how many"""
        ctx = self.ctx
        if self.keys_buf is None or self.keys_buf.n < offset + est:
            grown = ctx.empty(offset + est, np.uint64)
            if offset:
                ctx._check(ctx.lib.zk_copy(ctx.h, grown.ptr, self.keys_buf.ptr, 8 * offset))
                ctx.sync()
            self.keys_buf = grown
        n, fits = ctx.strand_keys(text, lines, r, self.K, reverse, self.T, self.keys_buf, offset, SEED)
        if not fits:                # the estimate was too small: once more with the room it asked for
            return self._keys(text, lines, r, reverse, offset, n)
        return n

    def add_batch(self, texts, lines, r, reverse):
        """texts / lines: the mates of one batch of r records; reverse[m]: mate m contributes reverse complements"""
        ctx = self.ctx
        n = 0
        with Phase(ctx, "strand keys (%d reads)" % r, sum(t.n for t in texts)):
            for text, ln, rev in zip(texts, lines, reverse):
                # a window per sequence byte at most, and sequence lines are under half of a FASTQ text; the sample keeps
                # about T / M of them
                est = int(text.n // 2 * min(1.0, 1.2 * (self.T + 1) / float(1 << (2 * self.K)) + 0.01)) + 1024
                n += self._keys(text, ln, r, rev, n, est)
        self.windows += n
        if n == 0:
            return
        if self.uniq_buf is None or self.uniq_buf.n < n:
            self.uniq_buf = self.cnt_buf = None
            self.uniq_buf, self.cnt_buf = ctx.empty(n + n // 4, np.uint64), ctx.empty(n + n // 4, np.uint32)
        nu = native.C.c_uint64(0)
        with Phase(ctx, "sort + count", 8 * n):
            ctx._check(ctx.lib.zk_sort_count(ctx.h, self.keys_buf.ptr, n, 2 * self.K + 1, self.uniq_buf.ptr, self.cnt_buf.ptr,
                                             self.uniq_buf.n, native.C.byref(nu)))
        self.stack.append((ctx.copy_of(self.uniq_buf.view(nu.value)), ctx.copy_of(self.cnt_buf.view(nu.value)), 0, n))
        while len(self.stack) >= 2 and self.stack[-1][2] == self.stack[-2][2]:
            self._merge_top()

    def _merge_top(self):
        ctx = self.ctx
        bk, bc, lb, wb = self.stack.pop()
        ak, ac, la, wa = self.stack.pop()
        if wa + wb >= 1 << 32 or ac.dtype.itemsize == 8 or bc.dtype.itemsize == 8:
            ac = ac if ac.dtype.itemsize == 8 else ctx.widen(ac)
            bc = bc if bc.dtype.itemsize == 8 else ctx.widen(bc)
        with Phase(ctx, "union_sum %d + %d" % (ak.n, bk.n)):
            mk, mc = ctx.union_sum(ak, ac, bk, bc)
            ctx.sync()
        del ak, ac, bk, bc
        self.stack.append((mk, mc, max(la, lb) + 1, wa + wb))

    def result(self):
        """(ascending distinct tagged keys, counts u32 | u64) of everything added"""
        self.keys_buf = self.uniq_buf = self.cnt_buf = None
        if not self.stack:
            return self.ctx.empty(0, np.uint64), self.ctx.empty(0, np.uint32)
        while len(self.stack) > 1:
            self._merge_top()
        return self.stack[0][0], self.stack[0][1]


def count_inputs(ctx, table, inputs, single, batch, verbose=False):
    """parseFiles (strand.py:39-60): the files in pairs (1,2), (3,4), ... -- mate 1 forward, mate 2 reverse-complemented, a
    pair ending where the shorter file ends; single: every file alone, forward.  Returns the number of reads (pairs)."""
    step = 1 if single else 2
    n_reads = 0
    for i in range(0, len(inputs), step):
        paths = inputs[i:i + step]
        with contextlib.closing(record_batches(ctx, paths, batch, warn_unequal=False)) as batches:
            for texts, lines, r, _ in batches:
                table.add_batch(texts, lines, r, [False, True][:len(texts)])
                n_reads += r
                if verbose:
                    sys.stderr.write("%s: %d %s processed\n" % (" & ".join(os.path.basename(p) for p in paths), n_reads,
                                                                 "reads" if single else "read pairs"))
    return n_reads


def write_lines(ctx, keys, counts, K, orphans, out):
    """strand.py:142-155 over the final table: the lines in ascending canonical k-mer order, written to `out` (a binary or a
    text stream) chunk by chunk -> StrandStats"""
    with Phase(ctx, "pairs", keys.n * (8 + counts.dtype.itemsize)):
        a, b, st = ctx.strand_pairs(keys, counts, K, orphans, SEED)
    buf = None
    binary = getattr(out, "buffer", None)
    for lo in range(0, a.n, FORMAT_CHUNK):
        m = min(FORMAT_CHUNK, a.n - lo)
        with Phase(ctx, "format", 16 * m):
            buf = ctx.format_pairs(a.view(m, lo), b.view(m, lo), out=whole(buf))
        with Phase(ctx, "download", buf.n):
            host = buf.to_host()
        with Phase(ctx, "print", buf.n):
            if binary is not None:
                out.flush()
                binary.write(host.tobytes())
            elif "b" in getattr(out, "mode", ""):
                out.write(host.tobytes())
            else:
                out.write(host.tobytes().decode("ascii"))
    return st
