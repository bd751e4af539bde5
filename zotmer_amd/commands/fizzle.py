"""
zot fizzle - exon groups, and so genes and gene pairs, hit by read pairs.

Usage:
    zot fizzle -P [options] <gene-list> <refgene> <bedfile>
    zot fizzle -X [options] <index> <must-have>
    zot fizzle -T [options] <index>
    zot fizzle [options] <index> <input>...

Options:
    -P              prepare a bed file
    -X              index exons
    -T              test the index for crosstalk
    -g PATH         directory of FASTA reference sequences [default: .]
    -k K            value of k to use (1..32) [default: 25]
    -M NUM          minimum number of reads to report gene group [default: 1]
    -m NUM          minimum number of reads to report exon group [default: 1]
    -R NUM          minimum number of k-mers/read to report gene group [default: 1]
    -r NUM          minimum number of k-mers/read to report exon group [default: 1]
    -t              when preparing the bedfile, read genes and transcripts, not just genes
    -Z MIN:MAX      minimum:maximum number of genes to report [default: 0:999999]
    -z MIN:MAX      minimum:maximum number of exons to report [default: 0:999999]
    -n NAMES        text file with "accession  file-stem" per line: which file of -g holds a chromosome
    -b MEM          per-batch input size on the GPU (in MB); the output does not depend on it
    -v              produce verbose output

-P reads a list of genes (with -t: of genes and transcripts) and a refGene table and writes <bedfile>: the exons of each gene
-- of all its transcripts, merged where they overlap or touch; with -t those of the listed transcripts as they stand --
numbered along the strand, as `chromosome start end gene/NN strand`.

-X cuts every exon of the BED file <must-have> from the first record of <-g>/<chromosome>.fa.gz (else .fa), reverse-complements
it on strand `-`, and writes <index>: one YAML document {chr, en, exon, gene, seq, st, strand} per exon, the chromosomes in
sorted order and the lines sorted within one.

The index maps every K-mer of the exons (forward strand of `seq` only) to the tuple of the exons that hold it.  -T prints, as
YAML, `aliasing-within`: the k-mers that two or more exons hold, and `aliasing-genomic`: the exons whose k-mers occur in the
chromosomes the index names, on either strand, another number of times than in the exon (counted on the GPU).

The scan takes FASTQ read pairs (<reads_1> <reads_2>, and more such pairs).  A pair gives two records: the k-mers of mate 1
with the reverse complements of mate 2's, and the other way round.  The tuples that a record's k-mers hit are joined where
they share an exon; a group answers with the exons common to all its tuples, and where no group has any, the tuples hit
least often are dropped until one does.  One line per distinct answer:

    numReads numKmers kmersPerRead ggNumReads ggNumKmers ggKmersPerRead numExons numGenes geneGroup exonGroup

the gg columns being the sums over the answers that name the same genes.  -v adds the hit statistics on stderr.

Differences from the reference: the reference's main enters an experiment (`if True:`) and dies there; this command implements
the path behind it.  The debugging print of recHits is dropped.  Rows are sorted by the bytes of exonGroup (the reference
walks a Python 2 dict).  -z tests the number of distinct exons of the row's own key (the reference tests a variable left over
from an earlier loop).  The hit histogram has as many bins as the longest pair needs (the reference has 1000 and dies beyond
that).  An index without documents is refused.  K outside 1..32 is refused.  FASTA read inputs are refused.  An odd number of
inputs is refused.  The reference maps the 24 RefSeq accessions of hg19 to chr1 .. chrY through a table in its program text;
here -n gives the mapping (new).  -b is new.  Several processes (torch.distributed.run) are refused: one GPU for now.  Nothing
touches the device before the arguments are known to be good, and -P and -X do not touch it at all.
"""
# Drop-in for zotmer/commands/fizzle.py; the work is zotmer_amd/library/fizzle.py.
import os
import sys

from zotmer_amd.library import seqio
from zotmer_amd.library.usage import Spec

_SPEC = Spec(options={"-P": False, "-X": False, "-T": False, "-t": False, "-v": False, "-g": True, "-k": True, "-M": True, "-m": True,
                      "-R": True, "-r": True, "-Z": True, "-z": True, "-n": True, "-b": True}, rest="<arg>", rest_min=1)


def _num(opts, name, default, kind=int, lo=None, hi=None):
    v = opts[name]
    try:
        v = kind(v) if v is not None else default
    except ValueError:
        _SPEC._die("option %s needs %s" % (name, "an integer" if kind is int else "a number"), __doc__)
    if (lo is not None and v < lo) or (hi is not None and v > hi):
        _SPEC._die("option %s out of range" % name, __doc__)
    return v


def _range(opts, name):
    v = opts[name] if opts[name] is not None else "0:999999"
    try:
        lo, hi = (int(w) for w in v.split(":"))
    except ValueError:
        _SPEC._die("option %s needs MIN:MAX" % name, __doc__)
    return lo, hi


def main(argv):
    opts = _SPEC.parse(argv[1:], __doc__)
    args = opts["<arg>"]
    if opts["-P"] + opts["-X"] + opts["-T"] > 1:
        _SPEC._die("one of -P, -X and -T at a time", __doc__)
    K = _num(opts, "-k", 25, int, 1, 32)
    mem = _num(opts, "-b", 0, int, 1) if opts["-b"] is not None else None
    from zotmer_amd.library import fizzle
    flt = fizzle.Filters(_num(opts, "-M", 1), _num(opts, "-m", 1), _num(opts, "-R", 1.0, float), _num(opts, "-r", 1.0, float),
                         _range(opts, "-Z"), _range(opts, "-z"))
    want = 3 if opts["-P"] else 2 if opts["-X"] else 1 if opts["-T"] else None
    if (want is not None and len(args) != want) or (want is None and len(args) < 2):
        _SPEC._die("wrong number of arguments", __doc__)
    home = opts["-g"] if opts["-g"] is not None else "."
    try:
        if opts["-P"]:
            return fizzle.run_prepare(args[0], args[1], args[2], opts["-t"])
        if not os.path.isdir(home):
            _SPEC._die("zot fizzle: %s is not a directory" % home, __doc__)
        from zotmer_amd.library import hgvsindex
        seqs = hgvsindex.Home(home, hgvsindex.read_names(opts["-n"]) if opts["-n"] is not None else None)
        if opts["-X"]:
            text = fizzle.dump_all(fizzle.index_items(args[1], seqs, verbose=opts["-v"]))
            with fizzle.open_text(args[0], "w") as f:
                f.write(text)
            return 0
        inputs = args[1:]
        if not opts["-T"]:
            fasta = [p for p in inputs if seqio.is_fasta(p)]
            if fasta:
                _SPEC._die("zot fizzle reads FASTQ only: %s" % ", ".join(fasta), __doc__)
            if len(inputs) % 2:
                _SPEC._die("zot fizzle reads pairs: an odd number of inputs", __doc__)
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("zot fizzle: runs on a single GPU for now")
        index = fizzle.ClassIndex(K, fizzle.load_index(args[0]))
        if opts["-T"]:
            for ch in sorted({itm["chr"] for itm in index.ref}):
                seqs.path(ch)
    except (fizzle.InputError, IOError) as e:
        sys.stderr.write("zot fizzle: %s\n" % e)
        raise SystemExit(1)
    # nothing touches the device before the arguments and the index are known to be good
    from zotmer_amd.library import engine
    ctx = engine.context()
    try:
        if opts["-T"]:
            batch = (mem << 20) if mem is not None else hgvsindex.DEFAULT_BATCH
            return fizzle.run_crosstalk(ctx, index, seqs, batch, sys.stdout, verbose=opts["-v"])
        from zotmer_amd.commands.capture import capture_batch_bytes
        batch = (mem << 20) if mem is not None else capture_batch_bytes(ctx)
        return fizzle.run_scan(ctx, index, inputs, batch, sys.stdout, flt, verbose=opts["-v"])
    except (fizzle.InputError, IOError) as e:
        sys.stderr.write("zot fizzle: %s\n" % e)
        raise SystemExit(1)


if __name__ == "__main__":
    main(["fizzle"] + sys.argv[1:])
