"""
zot hgvs-index - index HGVS variants for `zot hgvs-find`, and test them for resolvability.

Usage:
    zot hgvs-index [options] <index> [<variant>...]
    zot hgvs-index -T [options] [<variant>...]

Options:
    -T              test variants for resolvability: print, per variant and allele, how many of its k-mers the
                    reference sequences hold how often (YAML on stdout); no index is written
    -f FILENAME     read more variants from a file (whitespace separated)
    -g PATH         directory of FASTA reference sequences [default: .]
    -k K            value of k to use (1..32) [default: 25]
    -n NAMES        text file with "accession  file-stem" per line: which file of -g holds an accession
    -w WIDTH        width of context for capture [default: 75]
    -W WIDTH        width of context for verification [default: 1024] (accepted and ignored, as in the reference)
    -m MEM          per-batch text size on the GPU (in MB) with -T; the output does not depend on it
    -v              produce verbose output

This is the indexing mode of the reference's hgvs-find (`zot hgvs-find -X [-T]`).  Each <variant> is a `g.` HGVS string
of one of ten kinds -- substitution, del, dup, ins, ins<length>, insALU, inv, delins, delins<length>, a repeat
`[count]` --, for instance chr7:g.140453136A>T.  The sequence of its accession is the first record of <-g>/<stem>.fa.gz,
else <stem>.fa, where the stem is what -n names for the accession and otherwise the accession itself.  The index is a YAML
list of dicts {hgvs, lhsFlank, rhsFlank, wtSeq, mutSeq}: the canonical spelling of the variant, -w bases on either side of
the range it replaces, the bases in that range, and what replaces them (null for ins<length>, delins<length>, insALU).
It is the <index> of `zot hgvs-find`.  A string that cannot be parsed is reported ("unable to parse ...") and skipped.

With -T every distinct variant gives two records, the wild-type and the mutant allele between K - 1 bases of either flank;
the k-mers of both strands of those records are looked up in the first record of every sequence file, on the GPU, and for
each k-mer x <= rc(x) the count c = count(x) + count(rc x) goes into the histogram {c: k-mers} of every record holding x.  A
variant is resolvable where its alleles have k-mers with c == 1 (wild type) and c == 0 (mutant).

Differences from the reference: a command of its own (`zot hgvs-find` keeps refusing -X, -T, -f, -g, -w, -W); the index
lists the variants grouped by accession in order of first appearance (the reference's order is that of a Python 2 dict,
which is undefined; under Python 3 it is this one); the reference maps the 24 RefSeq accessions of hg19 to chr1 .. chrY
through a table in its program text, here -n gives the mapping (new), and -T scans every *.fa.gz / *.fa of -g in name
order, or with -n exactly the files it names, where the reference scans those 24 files: the same counts when the directory
holds the 24 chromosomes; a missing sequence file, or one without a record, is refused (the reference dies, or silently
keeps the sequence of the accession before); .fa is read where there is no .fa.gz; in the scanned files a sequence line
must not begin or end with blanks other than its line break (they end a run of bases here; the reference strips them),
and a header is a '>' at the very start of a line; a variant string with a blank or a character outside ASCII is
refused; a palindromic k-mer counts twice, as in the reference; -m and -n are new; several processes
(torch.distributed.run) are refused: one GPU for now.  Nothing touches the device before the arguments are known to be
good, and indexing without -T does not touch it at all.
"""
# Drop-in for the indexing mode of zotmer/commands/hgvs-find.py:838-915; the work is zotmer_amd/library/hgvsindex.py.
import os
import sys

from zotmer_amd.library.usage import Spec

_SPEC = Spec(options={"-T": False, "-f": True, "-g": True, "-k": True, "-n": True, "-w": True, "-W": True, "-m": True, "-v": False},
             rest="<variant>", rest_min=0)


def _int(opts, name, default, lo=None, hi=None):
    v = opts[name]
    try:
        v = int(v) if v is not None else default
    except ValueError:
        _SPEC._die("option %s needs an integer" % name, __doc__)
    if (lo is not None and v < lo) or (hi is not None and v > hi):
        _SPEC._die("option %s out of range" % name, __doc__)
    return v


def main(argv):
    opts = _SPEC.parse(argv[1:], __doc__)
    words = list(opts["<variant>"])
    index = None
    if not opts["-T"]:
        if not words:
            _SPEC._die("wrong number of arguments", __doc__)
        index = words.pop(0)
    K = _int(opts, "-k", 25, 1, 32)
    W = _int(opts, "-w", 75, 0)
    _int(opts, "-W", 1024)
    mem = _int(opts, "-m", 0, 1) if opts["-m"] is not None else None
    home = opts["-g"] if opts["-g"] is not None else "."
    if not os.path.isdir(home):
        _SPEC._die("zot hgvs-index: %s is not a directory" % home, __doc__)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("zot hgvs-index: runs on a single GPU for now")

    from zotmer_amd.library import hgvsindex
    try:
        if opts["-f"] is not None:
            with open(opts["-f"]) as f:
                words += f.read().split()
        names = hgvsindex.read_names(opts["-n"]) if opts["-n"] is not None else None
        seqs = hgvsindex.Home(home, names)
        items, _ = hgvsindex.make_items(words, seqs, W)
        if not opts["-T"]:
            with open(index, "w") as f:
                f.write(hgvsindex.dump_yaml(items))
            return 0
        files = seqs.files()
    except (hgvsindex.InputError, IOError) as e:
        sys.stderr.write("zot hgvs-index: %s\n" % e)
        raise SystemExit(1)
    # nothing touches the device before the arguments and the variants are known to be good
    from zotmer_amd.library import engine
    ctx = engine.context()
    batch = (mem << 20) if mem is not None else hgvsindex.DEFAULT_BATCH
    try:
        return hgvsindex.run_test(ctx, items, K, files, batch, sys.stdout, verbose=opts["-v"])
    except (hgvsindex.InputError, IOError) as e:
        sys.stderr.write("zot hgvs-index: %s\n" % e)
        raise SystemExit(1)


if __name__ == "__main__":
    main(["hgvs-index"] + sys.argv[1:])
