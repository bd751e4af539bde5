"""
zot strand - compute strand bias statistics

Usage:
    zot strand [options] <fastq>...

Options:
    -k K            k-mer size to use (1..31) [default: 25]
    -p P            sampling fraction [default: 0.1]
    -s              single ended reads only
    -a              also print the k-mers seen only on their greater strand
    -m MEM          per-batch input size on the GPU (in MB); the output does not depend on it
    -r REF          use reference to anchor strands (refused, see below)
    -v              produce verbose output

Inputs are FASTQ (plain, .gz, .bz2, or - for stdin), taken in pairs (1,2), (3,4), ...: mate 1 contributes its forward
k-mers, mate 2 the reverse complements of its k-mers, and a pair of files ends where the shorter one ends.  For the
sampled k-mers (those whose canonical form c = min(x, rc x) has (murmer(c, 17) & (4^K - 1)) <= int((4^K - 1) * P)) one
line `count <TAB> count` is printed per canonical k-mer: its count and its reverse complement's, the one with the larger
murmer(., 17) first.

As in the reference, a palindrome prints its count twice, and a k-mer seen only as the greater of {x, rc x} prints
nothing unless -a is given (then as a line with a zero); -v says on stderr how many of each there were.
Differences from the reference: the lines come in ascending canonical k-mer order (the reference prints in dict order);
-k accepts 1..31 (a key carries one strand bit; the reference disclaims K > 30); -s counts the forward k-mers of every
read of every file, which is the evident intent of the reference's branch (it cannot run: it never reads the file);
-r is refused (the reference draws random.random() per read pair there, so it has no defined output); -a and -m are
new; with several processes (torch.distributed.run) the command refuses: it runs on a single GPU.
"""
# Drop-in for zotmer/commands/strand.py; the device path is zotmer_amd/library/strand.py.
import os
import sys

from zotmer_amd.library.usage import Spec

_SPEC = Spec(options={"-k": True, "-p": True, "-s": False, "-a": False, "-m": True, "-r": True, "-v": False}, rest="<fastq>")


def _int(opts, name, default, lo, hi=None):
    v = opts[name]
    try:
        v = int(v) if v is not None else default
    except ValueError:
        _SPEC._die("option %s needs an integer" % name, __doc__)
    if v < lo or (hi is not None and v > hi):
        _SPEC._die("option %s out of range" % name, __doc__)
    return v


def main(argv):
    opts = _SPEC.parse(argv[1:], __doc__)
    if opts["-r"] is not None:
        _SPEC._die("zot strand: -r is not supported: the reference assigns each read pair to a strand by random.random(), "
                   "so its output is not defined", __doc__)
    if opts["-k"] is not None and opts["-k"].strip() == "32":
        _SPEC._die("zot strand: -k 32 is not supported: a key is 2K + 1 bits wide (1 <= K <= 31)", __doc__)
    K = _int(opts, "-k", 25, 1, 31)
    try:
        p = float(opts["-p"]) if opts["-p"] is not None else 0.1
    except ValueError:
        _SPEC._die("option -p needs a number", __doc__)
    if p != p:
        _SPEC._die("option -p needs a number", __doc__)
    mem = _int(opts, "-m", 0, 1) if opts["-m"] is not None else None
    single, orphans, verbose = opts["-s"], opts["-a"], opts["-v"]
    inputs = opts["<fastq>"]
    if not single and len(inputs) % 2:
        _SPEC._die("zot strand: paired reads need an even number of inputs (use -s for single ended reads)", __doc__)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("zot strand: runs on a single GPU for now")

    # nothing touches the device before the arguments are known to be good
    from zotmer_amd.library import engine, strand
    from zotmer_amd.commands.capture import capture_batch_bytes
    T = strand.threshold(K, p)
    if T is None:               # a negative P: (z & M) > T for every k-mer
        return 0
    ctx = engine.context()
    batch = (mem << 20) if mem is not None else capture_batch_bytes(ctx)
    table = strand.StrandTable(ctx, K, T)
    n_reads = strand.count_inputs(ctx, table, inputs, single, batch, verbose=verbose)
    keys, counts = table.result()
    st = strand.write_lines(ctx, keys, counts, K, orphans, sys.stdout)
    if verbose:
        sys.stderr.write("%d %s, %d sampled k-mer instances: %d lines, %d k-mers seen only on their greater strand (%s), %d palindromes\n"
                         % (n_reads, "reads" if single else "read pairs", table.windows, st.n_pairs, st.n_orphans,
                            "printed" if orphans else "not printed", st.n_palindromes))
    return 0


if __name__ == "__main__":
    main(["strand"] + sys.argv[1:])
