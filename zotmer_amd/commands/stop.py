"""
zot stop - search for stop codons

Usage:
    zot stop [options] <input>...

Options:
    -k K            k-mer size (3..32) [default: 27]
    -r FILE         the transcripts (FASTA) the reads are placed on
    -S SEED         seed of the frame draw [default: 17]
    -m MEM          per-batch input size on the GPU (in MB); the output does not depend on it
    -v              produce verbose output

Every k-mer of the transcripts in FILE is indexed with its position, after a trailing run of five or more `A` has been
cut from each transcript.  The inputs are FASTQ (plain, .gz, .bz2, or - for stdin), single reads, taken in order.  Each
k-mer of a read, in either orientation, votes for the frames (transcript, offset, orientation) that its positions in the
index name; one frame is drawn with probability proportional to its votes, and the k-mers of that orientation that end,
in that frame, with TAA, TAG or TGA are counted for the transcript.  One line per transcript and counted k-mer:

    known|novel <k-mer> <count> <distance> <nearest> <transcript>

`known`: some transcript holds the k-mer at a position divisible by three (the reference tests the k-mer's first base,
not the stop's; so does this).  <distance> and <nearest>: the k-mer y of the transcript that is nearest to the counted
one, both shifted right by three bits (the reference's nearest3; <nearest> is y >> 3 rendered as K bases).

Differences from the reference: the reference's module dies on import (it needs zotmer/library/prot.py, which it does
not have); this follows its main.  The draw: the reference calls random.random() once per read that has a frame, after
random.seed(17), so a read's draw depends on the reads before it; here read number g (from 0, over all inputs) with n
votes draws the frame that holds vote floor(u n) of the votes ordered by (transcript name, offset, orientation), where
u = (rnd(SEED, 24, g) >> 11) / 2^53 comes from a counter-based generator -- the frame the reference's walk picks when
its random.random() returns u (but for a u within a few 2^-53 of a frame boundary, where its float sums round).
-S is new.  Lines are ordered by transcript name (as bytes) and then k-mer; the
reference's order is that of its dicts.  A tie for the nearest k-mer goes to the smallest; the reference's goes to the
order of its set.  Without -r the command refuses (the reference reads every input and prints nothing).  Two records of
one name are refused (the reference mixes them).  FASTA read inputs are refused.  K outside 3..32 is refused.
Transcripts that, with a margin of 8192 coordinates each, add up to 2^32 - 1 coordinates or more are refused.  A read
longer than 4096 bases that hits a transcript is refused.  -m is new.  With several processes (torch.distributed.run)
the command refuses: it runs on a single GPU.
"""
# Drop-in for zotmer/commands/stop.py; the device path is zotmer_amd/library/stopscan.py.
import os
import sys

from zotmer_amd.library import seqio
from zotmer_amd.library.usage import Spec

_SPEC = Spec(options={"-k": True, "-r": True, "-S": True, "-m": True, "-v": False}, rest="<input>")


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
    K = _int(opts, "-k", 27, 3, 32)
    seed = _int(opts, "-S", 17, 0, (1 << 64) - 1)
    mem = _int(opts, "-m", 0, 1) if opts["-m"] is not None else None
    if opts["-r"] is None:
        _SPEC._die("zot stop needs the transcripts: -r FILE", __doc__)
    inputs = opts["<input>"]
    fasta = [p for p in inputs if seqio.is_fasta(p)]
    if fasta:
        _SPEC._die("zot stop reads FASTQ only: %s" % ", ".join(fasta), __doc__)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("zot stop: runs on a single GPU for now")

    # nothing touches the device before the arguments and the index are known to be good
    from zotmer_amd.library import stopscan
    try:
        index = stopscan.load_index(opts["-r"], K)
        stopscan.layout_of(index)
    except (stopscan.InputError, IOError) as e:
        sys.stderr.write("zot stop: %s\n" % e)
        raise SystemExit(1)
    from zotmer_amd.library import engine
    from zotmer_amd.commands.capture import capture_batch_bytes
    ctx = engine.context()
    batch = (mem << 20) if mem is not None else capture_batch_bytes(ctx)
    try:
        return stopscan.run(ctx, index, inputs, seed, batch, sys.stdout, verbose=opts["-v"])
    except stopscan.InputError as e:
        sys.stderr.write("zot stop: %s\n" % e)
        raise SystemExit(1)


if __name__ == "__main__":
    main(["stop"] + sys.argv[1:])
