"""
`zot capture` on the device (zotmer/commands/capture.py): FASTQ reads binned by the bait sequences they touch.

The reference builds a dict from every bait K-mer (both strands) to the set of baits holding it (capture.py:85-95), walks
every read's forward 25-mers through it (capture.py:97-116; reads.py:38 fixes the read K at 25 whatever `-k` says) and
appends each hit read to a per-bait buffer that is flushed to `<prefix>/<name>.fastq` (ReadCache, capture.py:26-69).
Here the bait table is built on the device (zk_bait_table_build), the input text streams onto the device in batches cut
at record ends, and each batch is one zk_line_ends (the record structure), one zk_capture_hits (the distinct
(bait, read) pairs in (bait, read) order) and one zk_capture_gather per mate (the stripped records, bait by bait); the
host copies the gathered bytes back once and appends each bait's span to its file.  The output does not depend on
where the batches are cut.
"""
import gzip
import os
import sys

import numpy as np

from zotmer_amd import native
from zotmer_amd.library import seqio
from zotmer_amd.library.timing import Phase

READ_K = 25     # reads.reads() is built without K in capture.py:103, so reads.py:38's default applies


def bait_records(path):
    """[(name bytes, sequence bytes)] of the bait FASTA, as file.readFasta yields them (file.py:19-36)"""
    return [(nm.encode("latin-1"), seq) for nm, seq in seqio.fasta_records(path)]


def output_paths(prefix, name, paired, z):
    """ReadCache.__init__ (capture.py:27-44): '<P>/<name>.fastq', or '_1' / '_2' for paired reads; '.gz' with -z"""
    pfx, suff = os.fsencode(prefix), b".gz" if z else b""
    if paired:
        return [b"%s/%s_1.fastq%s" % (pfx, name, suff), b"%s/%s_2.fastq%s" % (pfx, name, suff)]
    return [b"%s/%s.fastq%s" % (pfx, name, suff)]


class _Reader:
    """One FASTQ input as device text batches of at most `batch` bytes that end at a line end.  Plain and gzip files are
    read by a zk_source ahead of the device; stdin and .bz2 are read (and decompressed) on the host and uploaded.
    fill() -> (device buffer, bytes in it, end of input reached); consume(cut) keeps the bytes after `cut` for the next
    batch (carried to the front of the other buffer) and, with `ahead`, starts reading the next batch behind them.  A
    context has one staging ring for its zk_sources, so only one request may be in flight at a time: the two mates of a
    pair are read one after the other (ahead=False), a single input is read ahead of the device."""

    def __init__(self, ctx, path, batch, ahead=True):
        self.ctx, self.path, self.B, self.ahead = ctx, path, int(batch), ahead
        self.native = path != "-" and not path.endswith(".bz2") and os.path.isfile(path)
        self.bufs = [ctx.empty(self.B + 64, np.uint8), ctx.empty(self.B + 64, np.uint8)]
        self.cur, self.carry, self.eof, self.n, self.ready = 0, 0, False, 0, False
        self.lines = None
        if self.native:
            self.src = ctx.source_open(path)
            if ahead:
                self.src.start(self.bufs[0], 0, self.B)
        else:
            self.src = seqio.open_binary(path)

    def fill(self):
        ctx, buf = self.ctx, self.bufs[self.cur]
        if not self.ready:
            if self.eof:
                got = 0
            elif self.native:
                if not self.ahead:
                    self.src.start(buf, self.carry, self.B - self.carry)
                with Phase(ctx, "wait for the reader"):
                    got, self.eof = self.src.finish()
            else:
                want = self.B - self.carry
                data = self.src.read(want)
                got = len(data)
                self.eof = got < want
                if got:
                    ctx._check(ctx.lib.zk_upload(ctx.h, buf.ptr + self.carry, data, got))
            self.n = self.carry + got
            if self.eof and self.n and buf.view(1, self.n - 1).to_host()[0] != 10:
                ctx._check(ctx.lib.zk_upload(ctx.h, buf.ptr + self.n, b"\n", 1))      # the last line counts without a terminator
                self.n += 1
            self.ready = True
        return buf, self.n, self.eof

    def consume(self, cut):
        ctx = self.ctx
        buf, nxt = self.bufs[self.cur], self.bufs[1 - self.cur]
        tail = self.n - cut
        if tail:
            ctx._check(ctx.lib.zk_copy(ctx.h, nxt.ptr, buf.ptr + cut, tail))
            ctx.sync()
        if self.native and self.ahead and not self.eof:
            self.src.start(nxt, tail, self.B - tail)          # the next batch streams in while this one is worked on
        self.carry, self.cur, self.ready = tail, 1 - self.cur, False

    def close(self):
        if self.src is not None and self.path != "-":
            self.src.close()
        self.src = None


class Sink:
    """The ReadCaches of all baits (capture.py:26-69): files are opened in append mode when a bait first has records
    (a bait without hits gets no file), each batch's span of a bait is appended (a gzip member of its own with -z),
    and end() prints one `<first path>: <reads>` line per bait in FASTA order."""

    def __init__(self, names, prefix, paired, z):
        self.paths = [output_paths(prefix, nm, paired, z) for nm in names]
        self.counts = [0] * len(names)
        self.z = z

    def write(self, mate, host_bytes, byte_spans):
        for b in np.nonzero(byte_spans[1:] > byte_spans[:-1])[0]:
            data = host_bytes[int(byte_spans[b]):int(byte_spans[b + 1])]
            with open(self.paths[b][mate], "ab") as f:
                f.write(gzip.compress(data.tobytes()) if self.z else data)

    def end(self, err=None):
        err = err or sys.stderr
        for paths, n in zip(self.paths, self.counts):
            err.write("%s: %d\n" % (os.fsdecode(paths[0]), n))


def capture_inputs(ctx, table, inputs, paired, sink, batch, verbose=False, veto=None):
    """reads.reads(inputs, paired=...) (reads.py:56-124): files in sequence, or in pairs (1,2), (3,4), ... with -p (a
    trailing odd file is ignored)"""
    step = 2 if paired else 1
    total = 0
    for i in range(0, len(inputs) - (step - 1), step):
        total += capture_files(ctx, table, inputs[i:i + step], sink, batch, verbose, veto)
    return total


def capture_files(ctx, table, paths, sink, batch, verbose=False, veto=None):
    """One input (or one pair of mates), batch by batch.  Both mates' batches must hold the same reads: each is cut after
    record r = min(complete records of either), by the device positions of their line ends, and the rest of each is
    carried into its next batch.  A pair ends with mate 1 (reads.py:95-98); if mate 2 ends first there is a warning
    (the reference meant to print it at reads.py:101) and the pair ends there.  Returns the number of reads."""
    readers = []
    n_reads = 0
    pairs_buf = out_buf = None
    try:
        for p in paths:
            readers.append(_Reader(ctx, p, batch, ahead=len(paths) == 1))
        while True:
            filled = [rd.fill() for rd in readers]
            recs = []
            for rd, (buf, n, eof) in zip(readers, filled):
                with Phase(ctx, "line ends", n):
                    rd.lines = ctx.line_ends(buf.view(n), out=_whole(rd.lines))
                recs.append(rd.lines.n // 4)
            r = min(recs)
            eofs = [f[2] for f in filled]
            done = eofs[0] and r == recs[0]
            short = (not done) and len(readers) == 2 and eofs[1] and r == recs[1] < recs[0]
            if r == 0 and not (done or short):
                raise IOError("%s: a record longer than the batch size (%d bytes); use a larger -m" % (paths[recs.index(0)], batch))
            cuts = [int(rd.lines.view(1, 4 * r - 1).to_host()[0]) + 1 if r else 0 for rd in readers]
            texts = [buf.view(cut) for (buf, _, _), cut in zip(filled, cuts)]
            lines = [rd.lines.view(4 * r) for rd in readers]
            if not (done or short):
                for rd, cut in zip(readers, cuts):
                    rd.consume(cut)
            if r:
                with Phase(ctx, "lookup + sort (%d reads)" % r):
                    pairs_buf = ctx.capture_hits(table, READ_K, texts[0], lines[0], r,
                                                 texts[1] if len(texts) == 2 else None, lines[1] if len(lines) == 2 else None,
                                                 veto=veto, out=_whole(pairs_buf))
                pairs = pairs_buf
                if pairs.n:
                    for mate in range(len(readers)):
                        with Phase(ctx, "gather", cuts[mate]):
                            out_buf, pair_spans, byte_spans = ctx.capture_gather(pairs, table.n_records, texts[mate], lines[mate],
                                                                                 out=_whole(out_buf))
                        with Phase(ctx, "download", out_buf.n):
                            host = out_buf.to_host()
                        with Phase(ctx, "file writes", out_buf.n):
                            sink.write(mate, host, byte_spans)
                    for b in np.nonzero(pair_spans[1:] > pair_spans[:-1])[0]:
                        sink.counts[b] += int(pair_spans[b + 1] - pair_spans[b])
                n_reads += r
                if verbose:
                    sys.stderr.write("%s: %d reads\n" % (" & ".join(os.path.basename(p) for p in paths), n_reads))
            if short:
                sys.stderr.write("warning: files had unequal length\n")
            if done or short:
                return n_reads
    finally:
        for rd in readers:
            rd.close()


def _whole(view):
    """the full allocation behind a view returned earlier (buffers are reused from batch to batch)"""
    if view is None:
        return None
    base = view
    while base._keep is not None and isinstance(base._keep, native.DeviceArray):
        base = base._keep
    return base


def build_table(ctx, records, K):
    """zk_bait_table of the bait sequences (capture.py:85-95)"""
    stream = b"".join(seq + b"\n" for _, seq in records)
    return ctx.bait_table(ctx.upload_stream(stream), K)
