"""
zot scan - gene alleles in sets of k-mers

Usage:
    zot scan [-AX] <genes> <input>...

Options:
    -A          print all alleles (accepted and ignored, as in the reference)
    -X          create an index

`zot scan -X <genes> <input.fa>...` indexes the 27-mers of both strands of every FASTA record of at least 27 bases and
writes the index to <genes>.  `zot scan <genes> <input>...` reads the index and, for every k-mer set given, finds for
each k-mer of the index the k-mer of the set with the longest common prefix, places those on the positions of every
indexed sequence, joins overlapping positions into fragments, and prints for every sequence whose best fragment group is
not explained by chance one line

    <number> TAB <length> TAB <consensus length> TAB <KS distance> TAB <chi-square> TAB <log10 p> TAB <name> TAB <consensus>

with the three numbers in '%g' and the consensus in the 16-letter FASTA alphabet.  The search and the placement run on
the device (zk_lcp_resolve, zk_scan_place); the fragments and the statistics are computed on the host by the reference's
own formulas, its quirks included (the k-mer offered to a position is what the reference's two sequential passes leave,
not the nearest k-mer of the set; the linking of fragments works on ranks where k-mers were meant).

Differences from the reference:
  * an index whose K is not 27 is refused; the reference writes only K=27 and hard-codes 27 again in its consensus;
  * a k-mer set whose K differs from the index's is refused; the reference never looks and compares unrelated bits;
  * a k-mer set without k-mers is refused with a message; the reference dies with NameError;
  * where the chance of a match rounds to 1 -- sets of a handful of k-mers -- the command stops with a message that
    names the set; the reference dies with ValueError (math domain error);
  * -X without a single usable 27-mer is refused with a message; the reference dies with ZeroDivisionError;
  * a damaged index (k-mers out of order, offsets or positions outside their arrays) is refused when it is loaded;
  * dictionaries are walked in insertion order, as the reference does under Python 3; it matters only when two fragments
    of one sequence start with the same k-mer;
  * -A is accepted and ignored, as in the reference, which parses it and never reads it;
  * stderr carries the reference's lines (`loading...`, `done.`, `g = ...` per set with 12 significant digits, and under
    -X `warning: `name' skipped` for a record shorter than 27 bases);
  * with several processes (torch.distributed.run) the command refuses: it runs on a single GPU.
"""
# Drop-in for zotmer/commands/scan.py; the device path is csrc/lcp_scan.hip, the host side zotmer_amd/library/genescan.py.
import os
import sys

from zotmer_amd.library import genescan
from zotmer_amd.library.usage import Spec

_SPEC = Spec(options={"-A": False, "-X": False}, positionals=["<genes>"], rest="<input>")


def parse(argv):
    """docopt reads `-AX` as the two flags; Spec takes one option per argument"""
    args = []
    for a in argv:
        if len(a) > 2 and a[0] == "-" and a[1] != "-" and all(ch in "AX" for ch in a[1:]):
            args.extend("-" + ch for ch in a[1:])
        else:
            args.append(a)
    return _SPEC.parse(args, __doc__)


def main(argv):
    opts = parse(argv[1:])
    try:
        if opts["-X"]:
            genescan.build(opts["<genes>"], opts["<input>"])
            return 0
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("zot scan: runs on a single GPU for now")
        sys.stderr.write("loading...\n")
        meta, arrays = genescan.index_load(opts["<genes>"])
        genescan.check_samples(meta["K"], opts["<input>"])
        # nothing touches the device before the index and the sets are known to be good
        from zotmer_amd.library import engine
        genescan.run(engine.context(), meta, arrays, opts["<input>"])
    except genescan.ScanError as e:
        sys.stderr.write("zot scan: %s\n" % e)
        raise SystemExit(1)
    return 0


if __name__ == "__main__":
    main(["scan"] + sys.argv[1:])
