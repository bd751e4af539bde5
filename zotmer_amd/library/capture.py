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
import contextlib
import gzip
import os
import sys

import numpy as np

from zotmer_amd.library import seqio
from zotmer_amd.library.fastq_batches import record_batches, whole
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
    """One input (or one pair of mates), batch by batch (fastq_batches.record_batches: both mates' batches hold the same
    reads).  A pair ends with mate 1 (reads.py:95-98); if mate 2 ends first there is a warning (the reference meant to print
    it at reads.py:101) and the pair ends there.  Returns the number of reads."""
    n_reads = 0
    pairs_buf = out_buf = None
    with contextlib.closing(record_batches(ctx, paths, batch)) as batches:
        for texts, lines, r, cuts in batches:
            with Phase(ctx, "lookup + sort (%d reads)" % r):
                pairs_buf = ctx.capture_hits(table, READ_K, texts[0], lines[0], r,
                                             texts[1] if len(texts) == 2 else None, lines[1] if len(lines) == 2 else None,
                                             veto=veto, out=whole(pairs_buf))
            pairs = pairs_buf
            if pairs.n:
                for mate in range(len(texts)):
                    with Phase(ctx, "gather", cuts[mate]):
                        out_buf, pair_spans, byte_spans = ctx.capture_gather(pairs, table.n_records, texts[mate], lines[mate],
                                                                             out=whole(out_buf))
                    with Phase(ctx, "download", out_buf.n):
                        host = out_buf.to_host()
                    with Phase(ctx, "file writes", out_buf.n):
                        sink.write(mate, host, byte_spans)
                for b in np.nonzero(pair_spans[1:] > pair_spans[:-1])[0]:
                    sink.counts[b] += int(pair_spans[b + 1] - pair_spans[b])
            n_reads += r
            if verbose:
                sys.stderr.write("%s: %d reads\n" % (" & ".join(os.path.basename(p) for p in paths), n_reads))
    return n_reads


def build_table(ctx, records, K):
    """zk_bait_table of the bait sequences (capture.py:85-95)"""
    stream = b"".join(seq + b"\n" for _, seq in records)
    return ctx.bait_table(ctx.upload_stream(stream), K)
