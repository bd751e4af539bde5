"""
Usage:
    zot mlst [-XK K] <alleles> <input>...

Determine which, out of a FASTA database of alleles exist in the
input set of k-mers.

Options:
    -X          Create an index
    -K K        If creating an index, use this value of K (default 27).

With -X the inputs are FASTA files and <alleles> is the index written from them; without it <alleles> is an index and
one line `input <TAB> record number <TAB> record name` is printed for every record all of whose k-mers (both strands)
are in the input set.  A record shorter than K has no k-mers and is printed for every input.  The index is the
reference's own file format: an index built by either program is read by the other.

Differences from the reference: an input whose K is not the index's is reported on stderr with the input's name and
both values of K, and the command ends with status 1 (the reference dies with a TypeError while formatting its
message); an index of more than 65 536 records keeps its record numbers as 32-bit words in a member `postings32`
with `U32` set in the meta, which the reference cannot read (and could not have built: its 16-bit array raises
OverflowError); -K outside 1 .. 32 is refused; with several processes (torch.distributed.run) the command refuses:
it runs on a single GPU.
"""
# Drop-in for zotmer/commands/mlst.py; the device path is zotmer_amd/library/mlst.py.
import os
import sys

from zotmer_amd.library import mlst
from zotmer_amd.library.usage import Spec

_SPEC = Spec(options={"-X": False, "-K": True}, positionals=["<alleles>"], rest="<input>")


def _split_flags(args):
    """`-XK 11`, as the usage line writes it: the flag -X followed by -K"""
    out = []
    for a in args:
        if a.startswith("-X") and len(a) > 2 and "--" not in out:
            out += ["-X", "-" + a[2:]]
        else:
            out.append(a)
    return out


def main(argv):
    opts = _SPEC.parse(_split_flags(argv[1:]), __doc__)
    K = mlst.DEFAULT_K
    if opts["-K"] is not None:
        try:
            K = int(opts["-K"])
        except ValueError:
            K = 0
        if not 1 <= K <= 32:
            _SPEC._die("zot mlst: -K must be a number from 1 to 32", __doc__)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("zot mlst: runs on a single GPU for now")
    idx = None
    if not opts["-X"]:
        try:
            idx = mlst.read_index_arrays(opts["<alleles>"])          # host only: the file is known to be an index first
        except IOError as e:
            sys.stderr.write("zot mlst: %s\n" % e)
            raise SystemExit(1)

    # nothing touches the device before the arguments are known to be good
    from zotmer_amd.library import engine, vectors
    from zotmer_amd.library.container import KmerSet
    ctx = engine.context()
    if opts["-X"]:
        table, names = mlst.build_index(ctx, K, opts["<input>"])
        mlst.write_index(opts["<alleles>"], table, names)
        return 0
    try:
        table, names, lens = mlst.upload_index(ctx, idx, opts["<alleles>"])      # once, whatever the number of inputs
    except mlst.BadIndex as e:
        sys.stderr.write("zot mlst: %s\n" % e)
        raise SystemExit(1)
    for inp in opts["<input>"]:
        with KmerSet(inp, "r") as z:
            K0 = z.meta["K"]
            if K0 != idx["K"]:
                sys.stderr.write('zot mlst: input "%s" has K = %d, the index %s has K = %d\n' % (inp, K0, opts["<alleles>"], idx["K"]))
                raise SystemExit(1)
            kmers = vectors.device_read_kmers(ctx, z)
        records = mlst.complete(ctx, table, lens, kmers)
        del kmers
        sys.stdout.write("".join(mlst.lines(inp, records, names)))
    return 0


if __name__ == "__main__":
    main(["mlst"] + sys.argv[1:])
