"""
`zot pulldown` on the device (zotmer/commands/pulldown.py): the read pairs of each bait in a ZIP archive, and the histogram
of the number of baits a pair hits.

The reference builds a dict from every bait 25-mer (both strands) to the baits holding it (pulldown.py:47-59) and a set of
the 25-mers of the -U sequences (pulldown.py:61-66), walks the forward 25-mers of both mates of every pair through them
(pulldown.py:77-99), appends the pair to a temp file per hit bait and mate, and at the end of a file pair writes the temp
files into the archive (pulldown.py:131-138).  Here both tables are bait tables on the device (library/capture.py), the
mates stream onto the device in batches cut at record ends (library/fastq_batches.py), and each batch is one
zk_pulldown_hits (the distinct (bait, pair) pairs, the histogram and the pushed-up count) and one zk_capture_gather per
mate; the host appends each bait's span to that bait's temp file and deflates the temp files into the archive when the
file pair ends.  The output does not depend on where the batches are cut.
"""
import contextlib
import os
import sys
import tempfile
import zipfile

import numpy as np

from zotmer_amd.library.fastq_batches import record_batches, whole
from zotmer_amd.library.timing import Phase

K = 25          # pulldown.py:45


def member_name(bait_name, path):
    """'<p>/<path>' with p = '/'.join(name.split()) (pulldown.py:134-137), as ZipFile.write stores an arcname: normalised
    (os.path.normpath), without a drive and without leading separators"""
    arc = "/".join(bait_name.split()) + "/" + path
    arc = os.path.normpath(os.path.splitdrive(arc)[1])
    seps = os.sep + (os.altsep or "")
    return arc.lstrip(seps).replace(os.sep, "/")


def name_clashes(names):
    """the bait names (str) that cannot have members of their own: [(name, why)] -- an empty name, or a name whose member
    path is that of an earlier bait ('a x' and 'a  x')"""
    bad, seen = [], {}
    for nm in names:
        p = "/".join(nm.split())
        if not p:
            bad.append((nm, "has no name"))
            continue
        key = member_name(nm, "x")
        if key in seen:
            bad.append((nm, "gives the same member path as %r" % seen[key]))
        else:
            seen[key] = nm
    return bad


class Archive:
    """The ZIP_DEFLATED archive and the temp files behind it.  Per file pair: begin(fn1, fn2); write(mate, bytes, spans)
    appends each bait's span of a batch to the temp file of that bait and mate; end() adds, for each bait in FASTA order
    that has pairs, the members '<p>/<fn1>' then '<p>/<fn2>', streamed from the temp files, and removes those.  The archive
    is opened once and holds the members of every file pair."""

    def __init__(self, path, names, tmpdir):
        self.names, self.tmpdir = names, tmpdir
        self.zip = zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED)
        self.fns, self.live = None, set()

    def _tmp(self, b, mate):
        return os.path.join(self.tmpdir, "%d_%d.fastq" % (b, mate + 1))

    def begin(self, fn1, fn2):
        self.fns, self.live = (fn1, fn2), set()

    def write(self, mate, host_bytes, byte_spans):
        for b in np.nonzero(byte_spans[1:] > byte_spans[:-1])[0]:
            b = int(b)
            with open(self._tmp(b, mate), "ab") as f:
                f.write(host_bytes[int(byte_spans[b]):int(byte_spans[b + 1])])
            self.live.add(b)

    def end(self):
        for b in sorted(self.live):
            for mate, fn in enumerate(self.fns):
                self.zip.write(self._tmp(b, mate), member_name(self.names[b], fn))
                os.remove(self._tmp(b, mate))
        self.live = set()

    def close(self):
        self.zip.close()


def pulldown_files(ctx, table, veto, paths, archive, batch, hist, verbose=False):
    """One pair of mate files, batch by batch; both files are read until either ends, silently (pulldown.py:33-40).
    hist (numpy u64[n_records + 1]) takes the batches' rows.  Returns (pairs read, pairs pushed up)."""
    n_reads = vetoed = 0
    pairs_buf = out_buf = None
    archive.begin(*paths)
    with contextlib.closing(record_batches(ctx, paths, batch, warn_unequal=False)) as batches:
        for texts, lines, r, cuts in batches:
            with Phase(ctx, "lookup + sort + tally (%d pairs)" % r):
                pairs_buf, h, nv = ctx.pulldown_hits(table, K, texts[0], lines[0], r, texts[1], lines[1], veto=veto, out=whole(pairs_buf))
            hist += h
            vetoed += nv
            if pairs_buf.n:
                for mate in range(2):
                    with Phase(ctx, "gather", cuts[mate]):
                        out_buf, _, byte_spans = ctx.capture_gather(pairs_buf, table.n_records, texts[mate], lines[mate], out=whole(out_buf))
                    with Phase(ctx, "download", out_buf.n):
                        host = out_buf.to_host()
                    with Phase(ctx, "temp writes", out_buf.n):
                        archive.write(mate, host, byte_spans)
            n_reads += r
            if verbose:
                sys.stderr.write("%s: %d pairs\n" % (" & ".join(os.path.basename(p) for p in paths), n_reads))
    with Phase(ctx, "deflate"):
        archive.end()
    return n_reads, vetoed


def pulldown(ctx, table, veto, names, inputs, output, batch, verbose=False, out=None):
    """All file pairs (inputs[0], inputs[1]), (inputs[2], inputs[3]), ... into the archive `output`; the rows
    '<n>\\t<pairs with n baits>' with a non-zero count, ascending, to `out` (stdout).  names: the baits' names (str) in FASTA
    order.  The temp files live in one temporary directory that is gone when this returns or raises.
    Returns (hist, pairs pushed up)."""
    assert len(inputs) % 2 == 0 and len(names) == table.n_records
    out = out or sys.stdout
    hist = np.zeros(table.n_records + 1, dtype=np.uint64)
    vetoed = 0
    with tempfile.TemporaryDirectory(prefix="zot_pulldown_") as tmpdir:
        archive = Archive(output, names, tmpdir)
        try:
            for i in range(0, len(inputs), 2):
                vetoed += pulldown_files(ctx, table, veto, inputs[i:i + 2], archive, batch, hist, verbose)[1]
        finally:
            archive.close()
    for n in np.nonzero(hist)[0]:
        out.write("%d\t%d\n" % (int(n), int(hist[n])))
    return hist, vetoed
