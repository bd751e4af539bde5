"""
zot vars - contexts in which a sample has a next base enriched over a reference k-mer set

Usage:
    zot vars -r ref <input>...

Options:
    -r ref      reference k-mers

The k-mers of a set are grouped by their first K-1 bases (the context).  For every context of an input, the counts of its
four next bases are compared with those of the same context in the reference set: with p = the reference's share of a
base, n = the input's count of the context and k = the input's count of the base, v = log Bin(p, n, X >= k) (0 where p is
0 or 1).  A context is printed when some v is below -10, as

    <context> TAB <the bases below -10, one letter of the 16-letter FASTA alphabet> TAB v(A) TAB v(C) TAB v(G) TAB v(T)

with the values in '%3.2g'.  The device reads both sets once and returns the few contexts that can print; the values are
then computed on the host by the reference's own formulas.

Differences from the reference:
  * a context of an input that the reference set does not have is skipped, and after the input's lines one line
    "zot vars: <file>: N of M contexts are not in the reference (first: <context>)" goes to stderr; the exit status stays
    0.  The reference dies there with AssertionError, after printing the lines before it;
  * without -r the command refuses with this usage text; the reference dies with AttributeError / NameError (its second
    mode was never finished);
  * a reference set whose K differs from the inputs' is refused; the reference never looks and compares unrelated bits;
  * the numeric columns equal the reference's as text on the same Python and C library.  Where the exact value is 0 they
    are amplified rounding noise (the reference itself prints values like 4.3e-10), so across machines a last printed
    digit may differ;
  * with several processes (torch.distributed.run) the command refuses: it runs on a single GPU.
"""
# Drop-in for zotmer/commands/vars.py; the device path is csrc/vars_scan.hip, the host side zotmer_amd/library/varscan.py.
import os
import sys

from zotmer_amd.library import varscan
from zotmer_amd.library.usage import Spec

_SPEC = Spec(options={"-r": True}, rest="<input>")


def parse(argv):
    opts = _SPEC.parse(argv, __doc__)
    if opts["-r"] is None:
        _SPEC._die("zot vars: -r ref is required", __doc__)
    return opts["-r"], opts["<input>"]


def main(argv):
    ref, inputs = parse(argv[1:])
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("zot vars: runs on a single GPU for now")
    try:
        K = varscan.read_k(inputs)
        kr = varscan.read_k([ref])
    except varscan.MismatchedK as e:
        sys.stderr.write("zot vars: mismatched K: %s\n" % e)
        raise SystemExit(1)
    if kr != K:
        sys.stderr.write("zot vars: the reference set %s has K=%d, the inputs have K=%d\n" % (ref, kr, K))
        raise SystemExit(1)

    # nothing touches the device before the arguments are known to be good
    from zotmer_amd.library import engine
    varscan.run(engine.context(), ref, inputs, K)
    return 0


if __name__ == "__main__":
    main(["vars"] + sys.argv[1:])
