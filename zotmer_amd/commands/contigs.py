"""
Usage:
    zot contigs [-l LEN] <input>...

Perform a simple de Bruijn graph assembly of the input k-mers.  Only non-branching paths in the de Bruijn graph are
reported: no attempt is made to resolve branching at all.  For every input the k-mers are visited in ascending order;
from a k-mer not yet on a path the walk follows the only successor while there is exactly one and it is not on a path,
and every k-mer it passes also takes its reverse complement off the list of starts.  Each path of at least LEN bases is
printed as a FASTA record `>contig_<index of its first k-mer>`.  Counts in the inputs are ignored.

Options:
    -l LEN          minimum length of contig to report (default 2K)

The successor and reverse-complement searches of every k-mer and the text are computed on the device; the walk itself
depends on its order and runs once on the host.  The output equals the reference's byte for byte.

Differences from the reference:
  * a set that is not closed under reverse complement (after `zot sample`, for instance) has k-mers whose reverse
    complement lies above every k-mer of the set.  The reference marks index n there: IndexError when the number of
    k-mers is a multiple of 64, a slack bit with no effect otherwise.  Here the mark is dropped in both cases;
  * K < 5: the reference dies in its index over the set (a negative shift count); here the same definitions are applied;
  * an input of 2^32 - 1 k-mers or more is refused with a message: indices are 32 bits wide;
  * a LEN that is not an integer is a usage error (the reference dies with ValueError);
  * with several processes (torch.distributed.run) the command refuses: it runs on a single GPU.
"""
# Drop-in for zotmer/commands/contigs.py; the device path is csrc/debruijn.hip, the host side zotmer_amd/library/debruijn.py.
import os
import sys

from zotmer_amd.library import debruijn
from zotmer_amd.library.usage import Spec

_SPEC = Spec(options={"-l": True}, rest="<input>")


def parse(argv):
    opts = _SPEC.parse(argv, __doc__)
    l = None
    if opts["-l"] is not None:
        try:
            l = int(opts["-l"])
        except ValueError:
            _SPEC._die("zot contigs: -l LEN must be an integer, not %r" % opts["-l"], __doc__)
    return l, opts["<input>"]


def main(argv):
    l, inputs = parse(argv[1:])
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("zot contigs: runs on a single GPU for now")

    # nothing touches the device before the arguments are known to be good
    from zotmer_amd.library import engine
    debruijn.run(engine.context(), inputs, l)
    return 0


if __name__ == "__main__":
    main(["contigs"] + sys.argv[1:])
