"""
zot pulldown - pull down the read pairs that share a k-mer with bait sequences

Usage:
    zot pulldown [options] <baits> <output> <input>...

Options:
    -p              treat the inputs as paired reads: (1,2), (3,4), ... (required)
    -U FASTA        sequences to "push up": a pair with a 25-mer of one of them (either strand) is left out
    -m MEM          per-batch input size on the GPU (in MB); the output does not depend on it
    -v              produce verbose output

Reads are FASTQ (plain, .gz, .bz2).  K is 25.  A pair hits every bait that shares a 25-mer (either strand of the bait,
forward strand of the mates) with one of its mates.  <output> is a ZIP archive (deflated): for each file pair and each bait,
in FASTA order, that was hit, the members <p>/<input 1> and <p>/<input 2> hold the pairs' records, where <p> is the bait's
name with its blanks turned into '/' and the input's path is normalised and loses leading separators, as ZipFile.write
stores it.  At the end one line `<n>\\t<pairs that hit n baits>` per n that occurred goes to stdout, ascending; pushed-up
pairs count in no line.  Both files of a pair are read until either ends.

Differences from the reference: -p is required and the inputs must come in pairs (the reference fails without -p, and on an
odd number of inputs); with several file pairs the archive holds the members of all of them, in input order (the reference
reopens the archive for every file pair, so that only the last one's members survive; with one file pair the result is the
reference's); baits whose names give the same member path ('a x' and 'a  x'), or a bait without a name, are refused (the
reference writes two members of one name); FASTA read inputs are refused, as in zot capture; -m is new; several processes
are refused (one GPU for now); the temp files live in one temporary directory that is gone at exit, on error as well.
"""
# Drop-in for zotmer/commands/pulldown.py; the device path is zotmer_amd/library/pulldown.py.
import os
import sys

from zotmer_amd.library import seqio
from zotmer_amd.library.usage import Spec

_SPEC = Spec(options={"-p": False, "-U": True, "-m": True, "-v": False}, positionals=["<baits>", "<output>"], rest="<input>")


def main(argv):
    opts = _SPEC.parse(argv[1:], __doc__)
    inputs = opts["<input>"]
    if not opts["-p"]:
        _SPEC._die("zot pulldown: single reads are not implemented (in the reference either): use -p", __doc__)
    if len(inputs) % 2:
        _SPEC._die("zot pulldown: paired reads need an even number of inputs", __doc__)
    mem = None
    if opts["-m"] is not None:
        try:
            mem = int(opts["-m"])
        except ValueError:
            _SPEC._die("option -m needs an integer", __doc__)
        if mem < 1:
            _SPEC._die("option -m out of range", __doc__)
    fasta = [p for p in inputs if seqio.is_fasta(p)]
    if fasta:
        _SPEC._die("zot pulldown reads FASTQ only: %s" % ", ".join(fasta), __doc__)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("zot pulldown: runs on a single GPU for now")

    # nothing touches the device before the arguments and the bait names are known to be good
    from zotmer_amd.library import capture, pulldown
    records = capture.bait_records(opts["<baits>"])
    names = [nm.decode("latin-1") for nm, _ in records]
    bad = pulldown.name_clashes(names)
    if bad:
        for nm, why in bad:
            sys.stderr.write("zot pulldown: bait %r %s\n" % (nm, why))
        raise SystemExit(1)
    up = capture.bait_records(opts["-U"]) if opts["-U"] is not None else []

    from zotmer_amd.commands.capture import capture_batch_bytes
    from zotmer_amd.library import engine
    ctx = engine.context()
    table = capture.build_table(ctx, records, pulldown.K)
    veto = capture.build_table(ctx, up, pulldown.K) if up else None
    batch = (mem << 20) if mem is not None else capture_batch_bytes(ctx)
    try:
        pulldown.pulldown(ctx, table, veto, names, inputs, opts["<output>"], batch, verbose=opts["-v"])
    finally:
        table.free()
        if veto is not None:
            veto.free()
    return 0


if __name__ == "__main__":
    main(["pulldown"] + sys.argv[1:])
