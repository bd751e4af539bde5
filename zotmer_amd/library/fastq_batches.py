"""
FASTQ inputs as device text batches cut at record ends -- the reader under `zot capture` and `zot strand`.

A Reader streams one file onto the device in batches that end at a line end; record_batches walks one input, or the two
mates of a pair in lockstep, and hands out per batch the text of whole records and the positions of its line ends
(zk_line_ends): record r of a batch is lines 4r .. 4r+3, as file.readFastq groups them (zotmer/library/file.py:38-52).
"""
import os
import sys

import numpy as np

from zotmer_amd import native
from zotmer_amd.library import seqio
from zotmer_amd.library.timing import Phase


class Reader:
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


def whole(view):
    """the full allocation behind a view returned earlier (buffers are reused from batch to batch)"""
    if view is None:
        return None
    base = view
    while base._keep is not None and isinstance(base._keep, native.DeviceArray):
        base = base._keep
    return base


def record_batches(ctx, paths, batch, warn_unequal=True):
    """One input (or one pair of mates) as batches of whole records: yields (texts, lines, r, cuts) -- per mate the device
    text of the batch's r records (cuts[m] bytes) and its line ends.  Both mates' batches hold the same reads: each is cut
    after record r = min(complete records of either), by the device positions of their line ends, and the rest of each is
    carried into its next batch.  A trailing incomplete record is dropped (file.py:51-52).  The pair ends where the shorter
    mate ends; when that is mate 2 and warn_unequal is set, a warning goes to stderr.  The views are valid until the
    generator is resumed; close() it (or exhaust it) to close the files."""
    readers = []
    try:
        for p in paths:
            readers.append(Reader(ctx, p, batch, ahead=len(paths) == 1))
        while True:
            filled = [rd.fill() for rd in readers]
            recs = []
            for rd, (buf, n, eof) in zip(readers, filled):
                with Phase(ctx, "line ends", n):
                    rd.lines = ctx.line_ends(buf.view(n), out=whole(rd.lines))
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
                yield texts, lines, r, cuts
            if short and warn_unequal:
                sys.stderr.write("warning: files had unequal length\n")
            if done or short:
                return
    finally:
        for rd in readers:
            rd.close()
