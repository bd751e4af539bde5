"""
`zot stop` (zotmer/commands/stop.py): the in-frame stop codons of reads placed on transcripts.

The reference indexes every K-mer of its transcripts by (name, position) (stop.py:92-110), lets every window of a read vote
for the frames its anchors name, draws one frame (112-150) and counts the k-mers of the drawn orientation that end in frame
with a stop; each counted k-mer is printed with the nearest k-mer of its transcript (151-158).

Here the transcripts are read and indexed on the host (load_index); the index goes to the device as a bait table whose ids are
anchors on one u32 axis, the transcripts in name order (alufinder.Layout, alufinder.anchor_arrays); the reads stream through in
batches (fastq_batches.record_batches), one zk_stop_frames and one zk_pileup_count per batch, the ordinal of a batch's first
read carried across batches and files; the counted lists are merged on the device (alufinder.DevicePileup); one zk_stop_nearest after
the last batch gives the distance, the nearest k-mer and the known flag of every line.  What is printed does not depend on
where the batches are cut: the draw of a read is a function of (seed, ordinal) (synth.stop_draw).
"""
import contextlib
import os
import re
import sys
import time

import numpy as np

from zotmer_amd import native
from zotmer_amd.library import seqio
from zotmer_amd.library.alufinder import DevicePileup, InputError, Layout, anchor_arrays, kmers_with_pos
from zotmer_amd.library.fastq_batches import record_batches, whole

PAD = 1 << 12                   # free coordinates on either side of a transcript: the longest sequence line that may hit one
DEFAULT_SEED = 17
_POLY_A = re.compile(b"AAAAAA*$")
_STOPS = (48, 50, 56)           # TAA, TAG, TGA
_LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def trim_poly_a(seq):
    """re.sub('AAAAAA*$', '', seq) (stop.py:97): a trailing run of five or more upper-case A goes"""
    return _POLY_A.sub(b"", seq)


class Index:
    """The transcripts in ascending byte order of their names: names[t], xs[t] / ps[t] = the k-mers and 0-based starts of the
    windows of the trimmed sequence of transcript t, span[t] = its length"""

    def __init__(self, K, records):
        self.K = K
        seen = {}
        for name, seq in records:
            if name in seen:
                raise InputError("two records are named %s" % name)
            seen[name] = trim_poly_a(seq)
        self.names = sorted(seen)                   # latin-1 str: code point order is byte order
        self.xs, self.ps, self.span = [], [], []
        for nm in self.names:
            x, pos = kmers_with_pos(K, seen[nm])
            self.xs.append(x)
            self.ps.append(pos)
            self.span.append(len(seen[nm]))

    def known_stops(self):
        """the k-mers with an occurrence at p % 3 == 0 that end with a stop (stop.py:102-110; p, not p + K - 3), ascending"""
        out = [x[(p % 3 == 0) & np.isin(x & np.uint64(63), np.array(_STOPS, dtype=np.uint64))] for x, p in zip(self.xs, self.ps)]
        return np.unique(np.concatenate(out)) if out else np.empty(0, np.uint64)

    def transcript_kmers(self):
        """seqKmers as (every transcript's distinct k-mers ascending, one after the other; offsets u64[n + 1])"""
        parts = [np.unique(x) for x in self.xs]
        offs = np.zeros(len(parts) + 1, dtype=np.uint64)
        if parts:
            offs[1:] = np.cumsum([len(p) for p in parts])
        return (np.concatenate(parts) if parts else np.empty(0, np.uint64)), offs


class _Zones:
    """an Index as anchor_arrays takes its zones"""

    def __init__(self, index):
        self.K, self.xs, self.ps = index.K, index.xs, index.ps
        self.names = [(nm, len(x)) for nm, x in zip(index.names, index.xs)]


def load_index(path, K):
    return Index(K, seqio.fasta_records(path))


def layout_of(index, pad=PAD):
    """every transcript on the axis, position 0 at base + pad: refuses an axis of 2^32 - 1 coordinates or more"""
    try:
        return Layout({nm: (0, max(n - 1, 0)) for nm, n in zip(index.names, index.span)}, pad)
    except InputError:
        raise InputError("the transcripts and their margins span 2^32 - 1 coordinates or more")


def starts_of(layout):
    return (layout.base + layout.pad).astype(np.uint32)


def anchor_table(ctx, index, layout):
    keys, offs, ids = anchor_arrays(_Zones(index), layout)
    return ctx.bait_table_from_arrays(index.K, ctx.upload(keys), ctx.upload(offs), ctx.upload(ids), max(layout.total, 1))


def scan_inputs(ctx, table, starts, K, pad, seed, inputs, batch, pileup, verbose=False):
    """stop.py:112-150: every input in order, single reads.  Returns the number of reads."""
    first = 0
    bufs = None
    for path in inputs:
        with contextlib.closing(record_batches(ctx, [path], batch)) as batches:
            for texts, lines, r, _ in batches:
                try:
                    tx, kmers = ctx.stop_frames(table, starts, texts[0], lines[0], r, K, pad, seed, first, out=bufs)
                except native.ZotkError as e:
                    if e.code != native.ZK_ERANGE:
                        raise
                    raise InputError("%s: %s" % (path, str(e).split(": ", 1)[-1]))
                bufs = (whole(tx), whole(kmers))
                if tx.n:
                    pileup.add_device(*ctx.pileup_count(tx, kmers, K))
                first += r
                if verbose:
                    sys.stderr.write("%s: %d reads processed\n" % (os.path.basename(path), first))
    return first


def render(K, x):
    return "".join("ACGT"[(x >> (2 * (K - 1 - j))) & 3] for j in range(K))


def render_all(K, xs):
    """render of every k-mer of an array, through one [n, K] matrix of letters"""
    xs = np.asarray(xs, dtype=np.uint64)
    shifts = (2 * (K - 1 - np.arange(K))).astype(np.uint64)
    text = _LETTERS[((xs[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.intp)].tobytes().decode("ascii")
    return [text[i:i + K] for i in range(0, len(text), K)]


def report_lines(K, names, tx, kmers, counts, dist, near, flags):
    """stop.py:151-158, ordered by transcript name and k-mer"""
    kinds = ("novel", "known")
    for t, x, c, d, y, f in zip(tx.tolist(), render_all(K, kmers), counts.tolist(), dist.tolist(),
                                render_all(K, np.asarray(near, dtype=np.uint64) >> np.uint64(3)), flags.tolist()):
        yield "%s\t%s\t%d\t%d\t%s\t%s" % (kinds[f], x, c, d, y, names[t])


def run(ctx, index, inputs, seed, batch, out, pad=PAD, verbose=False, stats=None, pileup=None):
    """the whole command behind its argument checks.  pileup: where the counted lists gather (None: a DevicePileup)"""
    K = index.K
    layout = layout_of(index, pad)
    pileup = pileup if pileup is not None else DevicePileup(ctx)
    n_reads = 0
    t0 = time.perf_counter()
    if index.names:
        table = anchor_table(ctx, index, layout)
        try:
            n_reads = scan_inputs(ctx, table, ctx.upload(starts_of(layout)), K, layout.pad, seed, inputs, batch, pileup, verbose)
        finally:
            table.free()
    tx, kmers, counts = pileup.result()
    t1 = time.perf_counter()
    if len(tx):
        tk, offs = index.transcript_kmers()
        d_tx, d_kmers = pileup.device_result()[:2] if isinstance(pileup, DevicePileup) else (ctx.upload(tx, np.uint32), ctx.upload(kmers, np.uint64))
        dist, near, flags = ctx.stop_nearest(d_tx, d_kmers, K, ctx.upload(tk), ctx.upload(offs), ctx.upload(index.known_stops()))
        dist, near, flags = dist.to_host(), near.to_host(), flags.to_host()
    else:
        dist, near, flags = np.empty(0, np.uint32), np.empty(0, np.uint64), np.empty(0, np.uint8)
    t2 = time.perf_counter()
    for line in report_lines(K, index.names, tx, kmers, counts, dist, near, flags):
        out.write(line + "\n")
    if stats is not None:
        stats.update(reads=n_reads, stops=int(np.sum(counts)) if len(counts) else 0, lines=len(tx), merges=pileup.merges, merge_seconds=pileup.merge_seconds,
                     scan_seconds=t1 - t0, nearest_seconds=t2 - t1, report_seconds=time.perf_counter() - t2)
    return 0
