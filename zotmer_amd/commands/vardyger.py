"""
zot vardyger - search for tandem duplications

Usage:
    zot vardyger [options] <sequences> <input>...

Options:
    -A              show anchors in reads (refused: see below)
    -a              report all detected duplications, not just in-frame ones.
    -b MEM          per-batch input size on the GPU (in MB); the output does not depend on it
    -k K            value of K to use - must be even. [default: 24]
    -m MIN          minimum k-mer coverage for reporting anchors [default: 10]
    -s              strict path validation
    -v              produce verbose output

<sequences> is a FASTA file of gene sequences; the inputs are FASTQ (plain, .gz, .bz2), single reads, taken file by
file.  A read counts for every sequence that holds one of its K-mers, of either strand, on its forward strand, and all
K-mers of both strands of the read are then counted for that sequence; K-mers counted at least 10 times stay.  With
J = K / 2, a tandem duplication of the bases pb .. pd - 1 shows as three K-mers: `left` = ab at pa = pb - J and `right` = cd
at pc = pd - J are K-mers of the sequence, and `mid` = cb, the first half of `right` followed by the second half of
`left`, spans the junction of the two copies.  One line is printed per sequence and placement with pc > pb, a != c, b != d
and `mid` and `right` among the K-mers that stayed:

    n  left  leftCov  mid  midCov  right  rightCov  len  vaf  hgvs

len = pc - pa, vaf = midCov / ((leftCov + rightCov) / 2), hgvs = <name>:c.<pb>_<pd - 1>dup.  Without -a only lengths
divisible by three are printed.  -s keeps a line only if the K-mers that stayed hold a path of len + 1 K-mers from `left`
to `mid` and one from `mid` to `right` (of several, the one with the largest summed coverage) whose K-mers J .. len - J
agree.  -m drops lines with a coverage below MIN.  A sequence whose own K-mers already look like a duplication gives
`warning: phantom dumplication: left-mid-right (len)` on stderr.  -v prints, on stderr, the reads taken per file and
one line per sequence with a `.` for every K-mer of it that stayed and an `X` for every one that did not.

Differences from the reference: the reference's main stops before its caller (it prints the coverage lines and debugging
traces on stdout, and continues with the next sequence); this is the caller behind that, without the traces.  Lines and
warnings come in ascending (sequence, c, b, d, a, pa, pc) order and n numbers them in that order; the reference's order
is that of its dicts and sets.  Of several paths with the same summed coverage -s takes the first in ascending order of
the K-mers they are grown through.  -A is refused (it keeps every captured read in memory to draw them).  FASTA read
inputs are refused.  Two sequences of one name are refused (the reference would print the last one's name for both).
An odd K prints `K must be even.` and returns, as in the reference; K outside 2..32 is refused.  With several processes
(torch.distributed.run) the command refuses: it runs on a single GPU.  -b is new.  Nothing touches the device before the
arguments and <sequences> are known to be good.
"""
# Drop-in for zotmer/commands/vardyger.py; the device path is zotmer_amd/library/vardyger.py.
import os
import sys

from zotmer_amd.library import seqio
from zotmer_amd.library.usage import Spec

_SPEC = Spec(options={"-A": False, "-a": False, "-b": True, "-k": True, "-m": True, "-s": False, "-v": False},
             positionals=["<sequences>"], rest="<input>")


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
    K = _int(opts, "-k", 24)
    if K & 1:
        sys.stderr.write("K must be even.\n")
        return
    if K < 2 or K > 32:
        _SPEC._die("option -k out of range", __doc__)
    min_cov = _int(opts, "-m", 10)
    mem = _int(opts, "-b", 0, 1) if opts["-b"] is not None else None
    if opts["-A"]:
        _SPEC._die("zot vardyger: -A is not implemented (it keeps every captured read in memory to draw them)", __doc__)
    inputs = opts["<input>"]
    fasta = [p for p in inputs if seqio.is_fasta(p)]
    if fasta:
        _SPEC._die("zot vardyger reads FASTQ only: %s" % ", ".join(fasta), __doc__)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("zot vardyger: runs on a single GPU for now")

    # nothing touches the device before the arguments and the sequences are known to be good
    from zotmer_amd.library import vardyger
    try:
        index = vardyger.load_index(opts["<sequences>"], K)
    except (vardyger.InputError, IOError) as e:
        sys.stderr.write("zot vardyger: %s\n" % e)
        raise SystemExit(1)
    from zotmer_amd.commands.capture import capture_batch_bytes
    from zotmer_amd.library import engine
    ctx = engine.context()
    batch = (mem << 20) if mem is not None else capture_batch_bytes(ctx)
    try:
        return vardyger.run(ctx, index, inputs, min_cov, opts["-a"], opts["-s"], batch, sys.stdout, verbose=opts["-v"])
    except vardyger.InputError as e:
        sys.stderr.write("zot vardyger: %s\n" % e)
        raise SystemExit(1)


if __name__ == "__main__":
    main(["vardyger"] + sys.argv[1:])
