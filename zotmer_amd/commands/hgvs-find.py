"""
zot hgvs-find - search for known variants in read data.

Usage:
    zot hgvs-find [options] <index> <input>...

Options:
    -A ALPHA        alpha level for Kolmogorov-Smirnov test [default: 0.001] (accepted and ignored, as in the reference)
    -B BINFUNC      binning function to use [default: none] (accepted and ignored, as in the reference)
    -C MINCOV       minimum coverage to call an allele [default: 10]
    -D MAXHAM       maximum hamming distance to allow in flanks for calling an allele [default: 2]
    -F FORMAT       a format string for printing extra result statistics [default: rds,vaf]
    -k K            value of k to use (1..32) [default: 25]
    -m MEM          per-batch input size on the GPU (in MB); the output does not depend on it
    -o FILENMANE    write the output to the named file rather than stdout
    -s              single stranded k-mer extraction (accepted and ignored, as in the reference)
    -v              produce verbose output
    -V VAF          minimum vaf for calling an allele [default: 0.05]

Format Strings

Format strings control the fields that get included in the output.
The value is a comma separated list. The order of fields is fixed,
so the order in the format string is irrelevant.  The supported
fields are:

    binom           Score alleles against a binomial model for Hamming distances
    kmers           print the k-mers captured for each variant and their counts
    ks              Kolmogorov-Smirnov statistics
    rds             count the number of reads captured for each variant
    vaf             compute an approximate VAF

<index> is the file the reference's `zot hgvs-find -X` writes: a YAML list of dicts with the keys hgvs, lhsFlank, rhsFlank,
wtSeq and mutSeq (null for a variant whose mutant allele is not spelled out: insN, delinsN, insALU).  A JSON file of the
same shape is read without PyYAML (JSON is YAML, so the reference reads it too).  The inputs are FASTQ (plain, .gz, .bz2),
taken in pairs (1,2), (3,4), ....  A read pair counts for every variant whose bait (lhs + wt + rhs, and lhs + mut + rhs)
shares a k-mer with it, and all k-mers of the pair, both strands, are counted for that variant.  The wild-type and mutant
alleles are recovered from those counts -- through Hamming neighbours (fewer than -D mismatches) of the expected k-mers for
a variant that is spelled out, through de Bruijn paths between anchors in the flanks for an anonymous one -- and one line
is printed per variant: the call (null, wt, mut, wt/mut: coverage above -C, fewer than 4 mismatches, VAF above -V), the
reads captured, the number and the quantiles of the k-mer counts of at least -C, and each allele's least coverage,
mismatches and VAF.

Differences from the reference: indexing (-X, -T, -f, -g, -w, -W) is not implemented: indexes come from the reference's -X
or are written by hand; -c is not implemented: `zot pulldown` writes the read pairs per bait; FASTA read inputs are
refused; several processes (torch.distributed.run) are refused: one GPU for now; an odd number of inputs is refused (the
reference ignores a trailing one silently); when mate 2 ends before mate 1 the warning of `zot capture` is printed and the
pair ends there (the reference dies there); -F kmers prints in ascending (variant, k-mer) order (the reference prints in
dict order); where several bridged paths of one kind tie in coverage and mismatches, the one kept is the last in ascending
order of the anchors and of the k-mers a path is grown through (the reference's order is that of its dicts and sets);
-m is new.  Nothing touches the device before the arguments and the index are known to be good.
"""
# Drop-in for zotmer/commands/hgvs-find.py (scanning mode); the device path is zotmer_amd/library/hgvsfind.py.
import gzip
import os
import sys

from zotmer_amd.library import seqio
from zotmer_amd.library.usage import Spec

_INDEXING = ("-X", "-T", "-f", "-g", "-w", "-W")
_SPEC = Spec(options={"-A": True, "-B": True, "-C": True, "-D": True, "-F": True, "-k": True, "-m": True, "-o": True, "-s": False,
                      "-v": False, "-V": True, "-c": True, "-X": False, "-T": False, "-f": True, "-g": True, "-w": True, "-W": True},
             positionals=["<index>"], rest="<input>")


def _int(opts, name, default, lo=None, hi=None):
    v = opts[name]
    try:
        v = int(v) if v is not None else default
    except ValueError:
        _SPEC._die("option %s needs an integer" % name, __doc__)
    if (lo is not None and v < lo) or (hi is not None and v > hi):
        _SPEC._die("option %s out of range" % name, __doc__)
    return v


def _open_output(name):
    """outputFile (hgvs-find.py:62-65)"""
    if name is None or name == "-":
        return sys.stdout
    return gzip.open(name, "wt") if name.endswith(".gz") else open(name, "w")


def main(argv):
    opts = _SPEC.parse(argv[1:], __doc__)
    given = [o for o in _INDEXING if opts[o]]
    if given:
        _SPEC._die("zot hgvs-find: indexing (%s) is not implemented: indexes come from the reference's "
                   "`zot hgvs-find -X` or are written by hand" % ", ".join(given), __doc__)
    if opts["-c"] is not None:
        _SPEC._die("zot hgvs-find: -c is not implemented: `zot pulldown` writes the read pairs of every bait into a ZIP archive", __doc__)
    K = _int(opts, "-k", 25, 1, 32)
    D, Q = _int(opts, "-D", 2), _int(opts, "-C", 10)
    try:
        V = float(opts["-V"]) if opts["-V"] is not None else 0.05
    except ValueError:
        _SPEC._die("option -V needs a number", __doc__)
    if V != V:
        _SPEC._die("option -V needs a number", __doc__)
    mem = _int(opts, "-m", 0, 1) if opts["-m"] is not None else None
    fmt = set((opts["-F"] if opts["-F"] is not None else "rds,vaf").split(","))
    inputs = opts["<input>"]
    fasta = [p for p in inputs if seqio.is_fasta(p)]
    if fasta:
        _SPEC._die("zot hgvs-find reads FASTQ only: %s" % ", ".join(fasta), __doc__)
    if len(inputs) % 2:
        _SPEC._die("zot hgvs-find: paired reads need an even number of inputs", __doc__)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("zot hgvs-find: runs on a single GPU for now")

    # nothing touches the device before the arguments and the index are known to be good
    from zotmer_amd.library import hgvsfind
    try:
        items, variants = hgvsfind.read_index(opts["<index>"])
    except (hgvsfind.InputError, IOError) as e:
        sys.stderr.write("zot hgvs-find: %s\n" % e)
        raise SystemExit(1)
    from zotmer_amd.commands.capture import capture_batch_bytes
    from zotmer_amd.library import engine
    ctx = engine.context()
    batch = (mem << 20) if mem is not None else capture_batch_bytes(ctx)
    out = _open_output(opts["-o"])
    try:
        return hgvsfind.run(ctx, items, variants, inputs, K, D, Q, V, fmt, batch, out, verbose=opts["-v"])
    except hgvsfind.InputError as e:
        sys.stderr.write("zot hgvs-find: %s\n" % e)
        raise SystemExit(1)
    finally:
        if out is not sys.stdout:
            out.close()


if __name__ == "__main__":
    main(["hgvs-find"] + sys.argv[1:])
