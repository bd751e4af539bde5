"""
Usage:
    zot ksnp [(-H DIST|-L DIST)] <output> <ref>

Use the kSNP algorithm (and extensions) to find candidate SNPs in a set of reference k-mers.  With J = (K - 1) // 2 a
k-mer is read as a prefix of K - J - 1 bases, a middle base and a tail of J bases.  Without an option a k-mer is kept if
another k-mer of the set differs from it in the middle base only.  With -H or -L the k-mers of one prefix are joined
wherever two of them are at most DIST apart, and every connected cluster that holds two different middle bases is kept
whole.  The kept k-mers are written to <output> as a k-mer set without counts.  Counts in <ref> are ignored.

Options:
    -H DIST         Hamming based matching: at most DIST substituted bases between two k-mers of one prefix
    -L DIST         Levenshtein based matching: at most DIST edits (unit costs) between two k-mers of one prefix

Every pair of k-mers that share a prefix is compared once, on the device: the work is quadratic in the number of k-mers
of a prefix, as the reference's is, and no input is refused for it.  A low-complexity set at a small K can be one prefix.

Differences from the reference:
  * the reference's main dies with NameError (it calls writeKmers, which it does not import) before it writes anything.
    The file written here is the one it names: the `kmers` stream and the metadata K and kmers;
  * a DIST that is negative or not an integer is a usage error (the reference dies with ValueError, or keeps nothing);
  * a <ref> without k-mers gives the message of `zot dump` and exit status 1;
  * a <ref> of 2^32 - 1 k-mers or more is refused with a message: indices are 32 bits wide;
  * with several processes (torch.distributed.run) the command refuses: it runs on a single GPU.
"""
# Drop-in for zotmer/commands/ksnp.py; the device path is csrc/ksnp.hip, the host side zotmer_amd/library/ksnp.py.
import os
import sys

from zotmer_amd.library import ksnp
from zotmer_amd.library.usage import Spec

_SPEC = Spec(options={"-H": True, "-L": True}, positionals=["<output>", "<ref>"])


def parse(argv):
    """-> (mode, DIST, output, ref)"""
    opts = _SPEC.parse(argv, __doc__)
    if opts["-H"] is not None and opts["-L"] is not None:
        _SPEC._die("zot ksnp: -H and -L exclude each other", __doc__)
    mode, d = ksnp.DEFAULT, 0
    for o, m in (("-H", ksnp.HAMMING), ("-L", ksnp.LEVENSHTEIN)):
        if opts[o] is None:
            continue
        try:
            mode, d = m, int(opts[o])
        except ValueError:
            _SPEC._die("zot ksnp: %s DIST must be an integer, not %r" % (o, opts[o]), __doc__)
        if d < 0:
            _SPEC._die("zot ksnp: %s DIST must not be negative (%d)" % (o, d), __doc__)
    return mode, d, opts["<output>"], opts["<ref>"]


def main(argv):
    mode, d, out_path, ref = parse(argv[1:])
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("zot ksnp: runs on a single GPU for now")

    # nothing touches the device before the arguments and the input's metadata are known to be good
    def make_ctx():
        from zotmer_amd.library import engine
        return engine.context()
    ksnp.run(make_ctx, out_path, ref, mode, d)
    return 0


if __name__ == "__main__":
    main(["ksnp"] + sys.argv[1:])
