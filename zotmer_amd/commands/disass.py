"""
zot disass - "disassemble" contigs to produce some summary statistics

Usage:
    zot disass [options] <input>...

Options:
    -k K            value of k to use [default: 25]
    -c C            cutoff for distinguishing low and high frequency k-mers [default: 5]
    -p Prob         subsample k-mers with probability Prob [default: 1.0]
    -q Q            number of quantiles to compute [default: 10]
    -s              perform a single stranded analysis
    -S Seed         seed for subsampling [default: 17]
    -v              produce verbose output

Per FASTA file (plain, .gz or .bz2) a YAML document entry {file, contigs, global}: for every contig, and for the whole
file, the histogram of k-mer multiplicities as [count, frequency] pairs, its mean and median, the numbers of distinct
k-mers with a count below and from the cutoff, and the quantiles.  Without -s every window counts as itself and as
its reverse complement, two separate k-mers, each sampled by -p on its own (a k-mer is kept when its hash over
2^61 - 1 is below Prob: the hash has 64 bits, so 1.0 keeps about an eighth and 8 keeps all).  The median of an odd
number n of values is the reference's own: (cs[m] + cs[m+1]) / 2 with m = n // 2, the middle value and the one after it.

Differences from the reference:
  * quantiles walk the histogram in ascending count; the reference walks a dict, whose order is ascending under
    Python 3, and under Python 2 only while the count values do not collide in the hash table;
  * a contig or file with exactly one distinct k-mer has median = float(count); the reference dies with IndexError;
  * -q below 1 is refused (the reference divides by zero), as are -k outside 1 .. 32, a -p that is not a finite
    number, a -S outside 0 .. 2^64 - 1, and option values that are not numbers;
  * the YAML text is equal to the reference's as a loaded structure, not byte for byte: long flow lists are not
    wrapped at 80 columns;
  * -v is accepted and prints nothing more; with several processes (torch.distributed.run) the command refuses: it
    runs on a single GPU.
"""
# Drop-in for zotmer/commands/disass.py; the device path is zotmer_amd/library/disass.py.
import math
import os
import sys

from zotmer_amd.library import disass
from zotmer_amd.library.usage import Spec

_SPEC = Spec(options={"-k": True, "-c": True, "-p": True, "-q": True, "-s": False, "-S": True, "-v": False}, rest="<input>")


def _number(opts, name, default, kind, what):
    if opts[name] is None:
        return default
    try:
        return kind(opts[name])
    except ValueError:
        _SPEC._die("zot disass: %s must be %s" % (name, what), __doc__)


def parse(argv):
    """the options as numbers, refused where the reference would die or the device cannot follow"""
    opts = _SPEC.parse(argv, __doc__)
    D = disass.DEFAULTS
    K = _number(opts, "-k", D["K"], int, "a number from 1 to 32")
    C = _number(opts, "-c", D["C"], int, "a whole number")
    Q = _number(opts, "-q", D["Q"], int, "a whole number, 1 or more")
    S = _number(opts, "-S", D["S"], int, "a whole number")
    P = _number(opts, "-p", D["P"], float, "a finite number")
    if not 1 <= K <= 32:
        _SPEC._die("zot disass: -k must be a number from 1 to 32", __doc__)
    if Q < 1:
        _SPEC._die("zot disass: -q must be a whole number, 1 or more", __doc__)
    if not math.isfinite(P):
        _SPEC._die("zot disass: -p must be a finite number", __doc__)
    if not 0 <= S < 1 << 64:
        _SPEC._die("zot disass: -S must be a whole number below 2^64", __doc__)
    return dict(K=K, C=C, Q=Q, S=S, P=P, both=not opts["-s"], inputs=opts["<input>"])


def main(argv):
    o = parse(argv[1:])
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("zot disass: runs on a single GPU for now")

    # nothing touches the device before the arguments are known to be good
    from zotmer_amd.library import engine
    ctx = engine.context()
    res = []
    for fn in o["inputs"]:
        try:
            res.append(disass.file_result(ctx, fn, o["K"], o["C"], o["Q"], o["both"], o["S"], o["P"]))
        except disass.TooLarge as e:
            sys.stderr.write("zot disass: %s: %s\n" % (fn, e))
            raise SystemExit(1)
    sys.stdout.write(disass.dump_yaml(res))
    return 0


if __name__ == "__main__":
    main(["disass"] + sys.argv[1:])
