"""
Host side of `zot contigs` (zotmer/commands/contigs.py): per input, the links of every k-mer on the device
(zk_debruijn_links), the reference's ordered walk over them on the host (zk_contig_walk) and the FASTA text of the kept paths
on the device (zk_contig_render).  DESIGN.md section 6i says why the walk itself is not parallel.
"""
import sys

import numpy as np

MAX_KMERS = (1 << 32) - 2          # zk_debruijn_links: indices are 32 bits wide and 0xFFFFFFFF means "no link"


class TooManyKmers(Exception):
    pass


def min_length(K, l):
    """contigs.py:33-42: L = -l, or 2K; a negative L keeps everything"""
    return max(0, 2 * K if l is None else l)


def contigs_text(ctx, kmers, K, l=None):
    """ascending k-mers on the device -> the bytes the reference prints for them"""
    from zotmer_amd import native
    from zotmer_amd.library.timing import Phase
    if kmers.n > MAX_KMERS:
        raise TooManyKmers("%d k-mers; `zot contigs` indexes them with 32 bits, at most %d" % (kmers.n, MAX_KMERS))
    if kmers.n == 0:
        return b""
    with Phase(ctx, "contigs links", 16 * kmers.n):
        nx, rc = ctx.debruijn_links(kmers, K)
    with Phase(ctx, "contigs links to host", 8 * kmers.n):
        h_next, h_rc = nx.to_host(), rc.to_host()
    del nx, rc
    with Phase(ctx, "contigs walk"):
        nodes, offs = native.contig_walk(h_next, h_rc, K, min_length(K, l))
    if len(offs) == 1:
        return b""
    with Phase(ctx, "contigs nodes to device", 4 * len(nodes) + 8 * len(offs)):
        d_nodes, d_offs = ctx.upload(nodes, np.uint32), ctx.upload(offs, np.uint64)
    with Phase(ctx, "contigs render", 12 * len(nodes)):
        text = ctx.contig_render(kmers, K, d_nodes, d_offs)
    with Phase(ctx, "contigs text to host", text.n):
        return text.to_host().tobytes()


def run(ctx, inputs, l=None, out=None):
    """every input is read, linked, walked and printed, in order"""
    from zotmer_amd.library import vectors
    from zotmer_amd.library.container import KmerSet
    out = out or sys.stdout
    for fn in inputs:
        with KmerSet(fn, "r") as z:
            K = z.meta["K"]
            kmers = vectors.device_read_kmers(ctx, z)
        try:
            text = contigs_text(ctx, kmers, K, l)
        except TooManyKmers as e:
            sys.stderr.write("zot contigs: %s: %s\n" % (fn, e))
            raise SystemExit(1)
        del kmers
        out.write(text.decode("ascii"))
