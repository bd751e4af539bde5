"""
zot alu-finder - find ALU insertion points

Usage:
    zot alu-finder [options] <regions> <input>...

Options:
    -k K            value of k to use (1..32) [default: 25]
    -g PATH         directory of FASTA reference sequences [default: .]
    -C INT          coverage cutoff value [default: 5]
    -L INT          Minimum length of spurs [default: 29]
    -m MEM          per-batch input size on the GPU (in MB); the output does not depend on it
    -r              produce raw spurs
    -S INT          Maximum distance to shift spurs [default: 5]
    -V FLOAT        minimum relative frequency for insertions [default: 0.05]
    -v              produce verbose output

<regions> is a BED file: chromosome, start, end, name; the zone `name` is bases start..end (1-based, inclusive) of the
first record of <PATH>/<chromosome>.fa (or .fa.gz).  The inputs are FASTQ (plain, .gz, .bz2, or - for stdin), taken in
pairs (1,2), (3,4), ....  Both orientations of both mates of every pair are placed on the zones by their k-mers: every
diagonal (zone, reference position - read position) that a k-mer of the read names gets all the read's k-mers piled up
at their places.  Counts below -C, or below -V of the counts that share all but the last base at that position, are
dropped.  From every reference k-mer that was seen, the paths through the pile-up that leave the reference are the
spurs; those of at least -L k-mers are printed as they are with -r, and otherwise shifted by up to -S bases along the
reference and joined, an `after` spur at p with a `before` spur at p + 1.

Differences from the reference: chromosome names are used as the BED file gives them (no hg19 <-> RefSeq renaming); a
BED line without a name, and a name on two chromosomes, are refused, and blank BED lines are skipped; FASTA read inputs
are refused; when mate 2 ends before mate 1 the warning is printed and the pair ends there (the reference dies there);
a trailing unpaired input is ignored, as in the reference; zones whose padded spans add up to 2^32 - 1 coordinates or
more are refused; a read longer than 65536 bases that hits a zone is refused; -m is new; with several processes
(torch.distributed.run) the command refuses: it runs on a single GPU.
"""
# Drop-in for zotmer/commands/alu-finder.py; the device path is zotmer_amd/library/alufinder.py.
import os
import sys

from zotmer_amd.library import seqio
from zotmer_amd.library.usage import Spec

_SPEC = Spec(options={"-k": True, "-g": True, "-C": True, "-L": True, "-m": True, "-r": False, "-S": True, "-V": True, "-v": False},
             positionals=["<regions>"], rest="<input>")


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
    K = _int(opts, "-k", 25, 1, 32)
    C, L, S = _int(opts, "-C", 5), _int(opts, "-L", 29), _int(opts, "-S", 5)
    try:
        V = float(opts["-V"]) if opts["-V"] is not None else 0.05
    except ValueError:
        _SPEC._die("option -V needs a number", __doc__)
    if V != V:
        _SPEC._die("option -V needs a number", __doc__)
    mem = _int(opts, "-m", 0, 1) if opts["-m"] is not None else None
    home = opts["-g"] if opts["-g"] is not None else "."
    inputs = opts["<input>"]
    fasta = [p for p in inputs if seqio.is_fasta(p)]
    if fasta:
        _SPEC._die("zot alu-finder reads FASTQ only: %s" % ", ".join(fasta), __doc__)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("zot alu-finder: runs on a single GPU for now")

    # nothing touches the device before the arguments, the regions and the reference are known to be good
    from zotmer_amd.library import alufinder
    try:
        zones = alufinder.load_zones(opts["<regions>"], home, K)
        alufinder.layout_of(zones)
    except (alufinder.InputError, IOError) as e:
        sys.stderr.write("zot alu-finder: %s\n" % e)
        raise SystemExit(1)
    from zotmer_amd.library import engine
    from zotmer_amd.commands.capture import capture_batch_bytes
    ctx = engine.context()
    batch = (mem << 20) if mem is not None else capture_batch_bytes(ctx)
    try:
        return alufinder.run(ctx, zones, inputs, C, L, S, V, opts["-r"], batch, sys.stdout, verbose=opts["-v"])
    except alufinder.InputError as e:
        sys.stderr.write("zot alu-finder: %s\n" % e)
        raise SystemExit(1)


if __name__ == "__main__":
    main(["alu-finder"] + sys.argv[1:])
