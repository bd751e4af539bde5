"""
zot spikein - simulate read pairs from zones of reference sequences, with variants spiked in.

Usage:
    zot spikein [options] <output-prefix> [<variant>...]

Options:
    -b BEDFILE      restrict sampling of reads to regions in the BED file
    -d DEVIATION    standard deviation of insert sizes (proportion of mean) [default: 0.1]
    -e RATE         error rate [default: 0.005]
    -f FILE         read variants from a file
    -g DIR          directory containing reference sequences [default: .]
    -I SIZE         insert size [default: 300]
    -l FILE         log file for introduced mutations (created empty, as in the reference)
    -L LENGTH       read length [default: 100]
    -m FILE         read a file containing <probability, variant> pairs, one per line to introduce stochastically
    -M PROB         accepted and ignored, as in the reference
    -n NAMES        text file with "accession  file-stem" per line: which file of -g holds an accession
    -N NUMBER       number of read pairs [default: 1000000]
    -S SEED         random number generator seed
    -B MB           size of the per-call output buffers on the GPU (in MB); the output does not depend on it
    -z              gzip the output
    -v              produce verbose progress messages
    -V VAF          variant allele frequency [default: 1.0]

Writes <output-prefix>_1.fastq and <output-prefix>_2.fastq (.gz with -z).  The zones are those of the BED file, or, without
-b, every sequence file of -g from its first base to its last.  Read pairs are spread over the zones in proportion to their
lengths; a pair is cut from the mutant allele of its zone -- the chromosome with the variants that overlap the zone applied
-- with probability -V, else from the wild type.  The fragment starts at u, drawn from the zone, and has fl bases, normal
around -I; mate 1 is its first -L bases and mate 2 its last, both on the fragment's strand; bases are replaced at rate -e.
The header of a record is `@<chrom>:<start>-<end> <name> <u> <fl> <strand> <errors>`, the errors `<position><base>><new base>`
joined by `;`.  With `zot hgvs-index` before and `zot hgvs-find` after, this is the reference's variant workflow.

Differences from the reference: the random numbers are a counter-based generator, every draw a function of the seed and the
pair's number (the reference uses Python's random, whose output differs between Python versions), and the fragment length
is a sum of twelve uniform draws, so it stays within 6 standard deviations of -I; without -S a seed is taken from the
operating system and printed under -v; chromosomes are taken in name order (the reference: the order of a Python 2 dict);
bases are upper-cased before they are complemented (the reference complements first, so a soft-masked base stays
uncomplemented on strand -); insALU is refused (the reference dies on it); a zone of which the variants leave nothing
(e0 < s0), and an allele shorter than twice the longest fragment, are refused with a message naming the zone (in the
reference an assertion fails); a string that is no variant is refused (the reference reports it and goes on); FASTQ only;
accessions are mapped to file stems by -n, not by a table of the 24 hg19 chromosomes, no `chr` is put in front of a name,
and without -b the zones are the files found under -g; a BED zone that is empty or starts below 0 is refused; -n and -B are
new; several processes (torch.distributed.run) are refused: one GPU for now.  Nothing touches the device before the
arguments, the BED file and the variants are known to be good.
"""
# Drop-in for zotmer/commands/spikein.py; the work is zotmer_amd/library/spikein.py.
import os
import sys

from zotmer_amd.library.usage import Spec

_SPEC = Spec(options={"-b": True, "-d": True, "-e": True, "-f": True, "-g": True, "-I": True, "-l": True, "-L": True, "-m": True,
                      "-M": True, "-n": True, "-N": True, "-S": True, "-B": True, "-z": False, "-v": False, "-V": True},
             positionals=["<output-prefix>"], rest="<variant>", rest_min=0)


def _num(opts, name, default, kind, lo=None, hi=None):
    v = opts[name]
    try:
        v = kind(v) if v is not None else default
    except ValueError:
        _SPEC._die("option %s needs %s" % (name, "an integer" if kind is int else "a number"), __doc__)
    if (lo is not None and v < lo) or (hi is not None and v > hi) or v != v:
        _SPEC._die("option %s out of range" % name, __doc__)
    return v


def main(argv):
    opts = _SPEC.parse(argv[1:], __doc__)
    I = _num(opts, "-I", 300, int, 1, (1 << 40) - 1)
    D = _num(opts, "-d", 0.1, float, 0.0)
    E = _num(opts, "-e", 0.005, float, 0.0, 1.0)
    L = _num(opts, "-L", 100, int, 1, 1 << 20)
    N = _num(opts, "-N", 1000000, int, 0, (1 << 40) - 1)
    V = _num(opts, "-V", 1.0, float, 0.0, 1.0)
    _num(opts, "-M", 0.0, float)
    mb = _num(opts, "-B", 0, int, 1) if opts["-B"] is not None else None
    seed = _num(opts, "-S", None, int)
    home = opts["-g"] if opts["-g"] is not None else "."
    if I * D * 65536 >= float(1 << 43):
        _SPEC._die("option -d out of range", __doc__)
    if not os.path.isdir(home):
        _SPEC._die("zot spikein: %s is not a directory" % home, __doc__)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        sys.stderr.write("zot spikein: runs on a single GPU for now\n")
        raise SystemExit(1)
    if seed is None:
        seed = int.from_bytes(os.urandom(8), "little")
        if opts["-v"]:
            sys.stderr.write("seed = %d\n" % seed)

    from zotmer_amd.library import hgvsindex, spikein
    try:
        names = hgvsindex.read_names(opts["-n"]) if opts["-n"] is not None else None
        plan = spikein.make_plan(dict(bed=opts["-b"], home=home, names=names, file=opts["-f"], pop=opts["-m"], seed=seed, L=L, I=I, D=D),
                                 opts["<variant>"])
    except (spikein.InputError, IOError) as e:
        sys.stderr.write("zot spikein: %s\n" % e)
        raise SystemExit(1)
    if opts["-v"]:
        sys.stderr.write("mean coverage = %g\n" % (float(N * L) / float(plan.cum[-1])))
    # nothing touches the device before the arguments, the BED file and the variants are known to be good
    from zotmer_amd.library import engine
    ctx = engine.context()
    try:
        if opts["-l"]:
            open(opts["-l"], "w").close()
        spikein.run(ctx, plan, N, V, E, opts["<output-prefix>"], z=opts["-z"], verbose=opts["-v"],
                    buffer_bytes=(mb << 20) if mb is not None else spikein.DEFAULT_BUFFER)
    except (spikein.InputError, IOError) as e:
        sys.stderr.write("zot spikein: %s\n" % e)
        raise SystemExit(1)
    return 0


if __name__ == "__main__":
    main(["spikein"] + sys.argv[1:])
