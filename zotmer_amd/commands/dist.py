"""
Usage:
    zot dist [-M measure]... <k> <input>...

Options:
    -M measure  use "measure" for the distance between k-mer frequency sets.
                Use "-M list" to get a list of available measures.

The *.quant, *.ab and jensen.shannon measures compare k-mer spectra (the counts of the
<k>-mer prefixes) and need sets that carry counts.  They follow the reference's formulas,
with these differences:
  - counters are 64-bit: sums beyond 2^32 - 1 are computed, not refused;
  - spectra without a common k-mer give jaccard.ab = sorensen.ab = 1 (the limit; the
    reference divides by zero);
  - hellinger.quant of identical spectra is 0 (the reference takes the root of a rounding
    error, which fails when that is negative);
  - a set with no k-mers is an error (exit status 1).
With more than one process (torch.distributed.run) every rank holds a piece of each spectrum, and the
two floating-point sums behind hellinger.quant and jensen.shannon are added in another order: each
differs from the single-process sum by at most (n + 8) * 2^-52 * (the sum of its terms' magnitudes),
n = the number of shared k-mers.  Every other figure is computed in integers and is the same.
"""
# Drop-in for zotmer/commands/dist.py.  Set measures: per file Measure.prep (dist.py:43-49) = prefix projection +
# adjacent dedupe on the device (zk_project_dedupe); per pair dist.split (library/dist.py:241-265) = zk_split.
# Spectrum measures: per file Measure.prep in vector mode (dist.py:35-41) = the prefixes and the sums of their counts
# (zk_project_sum) instead of 4**K counters; per pair one merge pass (zk_spectrum_sums) gives the sums every vec=True
# branch of library/dist.py is a function of.  The closed forms stay on the host (library/measures.py).  Each file
# is decoded and uploaded once (the reference re-reads the right-hand file for every pair, dist.py:152-159).
import fnmatch
import sys

from zotmer_amd.library import engine, vectors
from zotmer_amd.library.container import KmerSet
from zotmer_amd.library.measures import MEASURES, SPECTRUM
from zotmer_amd.library.usage import Spec

_SPEC = Spec(options={"-M": "list"}, positionals=["<k>"], rest="<input>", rest_min=0)


class MismatchedK(Exception):       # zotmer/library/exceptions.py:31-38
    def __init__(self, k1, k2):
        self.k1, self.k2 = k1, k2

    def __str__(self):
        return "incompatible values of K: %d & %d" % (self.k1, self.k2)


def main(argv):
    opts = _SPEC.parse(argv[1:], __doc__)
    names = sorted(MEASURES)
    if "list" in opts["-M"]:                        # dist.py:97-104
        print("\n".join(m + "\t" + MEASURES[m][0] for m in names))
        return
    seen, bad = set(), False
    for pat in opts["-M"]:                          # dist.py:109-118
        hit = [m for m in names if fnmatch.fnmatch(m, pat)]
        if not hit:
            sys.stderr.write("warning: measure '%s' not found. Use -M list to see all measures.\n" % pat)
            bad = True
        seen.update(hit)
    ms = sorted(seen)
    if not ms or bad:                               # dist.py:122-123
        return
    vec = [m for m in ms if MEASURES[m][1]]
    need_set = len(vec) < len(ms)

    K = int(opts["<k>"])
    files = opts["<input>"]
    dist, world, rank = engine.distributed()        # one process per GPU under torch.distributed.run
    ctx = engine.context()
    if dist is not None:
        return _main_distributed(ctx, dist, K, files, ms)

    def prep(path):                                 # dist.py:29-49 -> (the set | None, the spectrum | None)
        with KmerSet(path, "r") as z:
            fK = z.meta["K"]
            if fK < K:
                raise MismatchedK(K, fK)
            if vec:                                 # files.readKmersAndCounts: a set without counts fails there too
                if "counts" not in z.toc:
                    raise SystemExit("zot dist: %s has no counts, which %s need%s" % (path, ", ".join(vec), "s" if len(vec) == 1 else ""))
                k, c = vectors.device_read_kmers_and_counts(ctx, z)
            else:
                k, c = vectors.device_read_kmers(ctx, z), None
        spec = engine.spectrum_prep(ctx, k, c, 2 * (fK - K)) if vec else None
        if spec is not None and spec[2] == 0:             # measures.EmptySpectrum, said with the file's name
            raise SystemExit("zot dist: %s holds no k-mers: it has no spectrum to compare" % path)
        return (engine.measure_prep(ctx, k, 2 * (fK - K)) if need_set else None), spec

    print("\t".join(["lhs.name", "rhs.name"] + ms))
    sets = {}
    for i in range(len(files)):
        for j in range(i + 1, len(files)):
            for f in (files[i], files[j]):
                if f not in sets:
                    sets[f] = prep(f)
            (xset, xspec), (yset, yspec) = sets[files[i]], sets[files[j]]
            abc = ctx.split(xset, yset) if need_set else None
            sums = ctx.spectrum_sums(xspec[0], xspec[1], xspec[2], yspec[0], yspec[1], yspec[2]) if vec else None
            vals = [SPECTRUM[m](sums) if MEASURES[m][1] else MEASURES[m][2](*abc) for m in ms]
            print("\t".join([files[i], files[j]] + ["%g" % v for v in vals]))


def _main_distributed(ctx, dist, K, files, ms):
    """Every rank decodes its own contiguous piece of each file (vectors.device_read_kmers_shard), the pieces of a pair
    are cut by one owner function and exchanged once, every rank splits what it owns, and (a, b, c) is all-reduced
    (zotmer_amd/parallel.py: Exchange.dist_pair).  The spectrum measures: every rank decodes its piece of the k-mers and the
    counts (vectors.device_read_kmers_and_counts_shard) and sums it under the prefixes; each file's spectrum is exchanged once,
    and one device call per row of the matrix compares what the rank owns (parallel.SpectrumDist).  Rank 0 prints."""
    import os
    import torch
    from zotmer_amd import parallel
    comm = parallel.make_comm(ctx, dist)
    ex = parallel.Exchange(ctx, dist, K, owner=os.environ.get("ZOT_OWNER", "range"), comm=comm)
    rank, world = comm.rank, comm.world

    vec = [m for m in ms if MEASURES[m][1]]
    need_set = len(vec) < len(ms)
    spectra = parallel.SpectrumDist(ex) if vec else None

    def prep(path):
        with KmerSet(path, "r") as z:
            fK = z.meta["K"]
            if fK < K:
                raise MismatchedK(K, fK)
            if vec:
                if "counts" not in z.toc:           # every rank reads the same table of contents: all of them stop here
                    raise SystemExit("zot dist: %s has no counts, which %s need%s" % (path, ", ".join(vec), "s" if len(vec) == 1 else ""))
                try:
                    t, c, n = vectors.device_read_kmers_and_counts_shard(ctx, z, rank, world, comm)
                except vectors.CodecError as e:
                    raise SystemExit("zot dist: %s is damaged: %s" % (path, e))
            else:
                k = vectors.device_read_kmers_shard(ctx, z, rank, world, comm)
                n = k.n
                t = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
                if n:
                    ctx._check(ctx.lib.zk_copy(ctx.h, t.data_ptr(), k.ptr, k.nbytes))
                    ctx.sync()
        spec = None
        if vec:                                     # this file's own shift: files of different K need no special case
            spec = spectra.prepare(t, c, n, 2 * (fK - K))
            if spectra.totals[spec] == 0:           # measures.EmptySpectrum; the total is global, so every rank leaves
                raise SystemExit("zot dist: %s holds no k-mers: it has no spectrum to compare" % path if rank == 0 else 1)
        return t, n, 2 * (fK - K), spec

    if rank == 0:
        print("\t".join(["lhs.name", "rhs.name"] + ms))
    sets = {}
    if len(files) > 1:
        for f in files:
            if f not in sets:
                sets[f] = prep(f)
    if vec and sets:                                # the spectra in the order of `files` (a file may be named twice)
        by_spec, totals = spectra.exchange_all(2 * K), spectra.totals
        spectra.pieces = [by_spec[sets[f][3]] for f in files]
        spectra.totals = [totals[sets[f][3]] for f in files]
    for i in range(len(files)):
        sums = spectra.row(i) if vec and sets else None
        for j in range(i + 1, len(files)):
            abc = None
            if need_set:
                (xt, nx, sx, _), (yt, ny, sy, _) = sets[files[i]], sets[files[j]]
                if sx != sy:                        # different file K: project each side on its own first
                    xt, nx = ex.ops.dedupe(xt, nx, sx)
                    yt, ny = ex.ops.dedupe(yt, ny, sy)
                    sx = 0
                abc, _ = ex.dist_pair(xt, nx, yt, ny, shift=sx)
            if rank == 0:
                vals = [SPECTRUM[m](sums[j - i - 1]) if MEASURES[m][1] else MEASURES[m][2](*abc) for m in ms]
                print("\t".join([files[i], files[j]] + ["%g" % v for v in vals]))


if __name__ == "__main__":
    main(["dist"] + sys.argv[1:])
