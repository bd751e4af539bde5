"""
zot capture - capture reads matching bait sequences

Usage:
    zot capture [options] <sequences> <input>...

Options:
    -b NUM          number of reads to buffer per bait sequence [default: 4096]
    -k K            value of K to use for the bait k-mers (1..32) [default: 24]
    -m MEM          per-batch input size on the GPU (in MB); the output does not depend on it
    -P PREFIX       prefix for output files [default: .]
    -p              treat inputs as paired reads
    -v              produce verbose output
    -z              produce compressed output

Reads are FASTQ (plain, .gz, .bz2, or - for stdin).  A read is captured by every bait that shares a k-mer with it and
is appended to <PREFIX>/<bait name>.fastq (or <name>_1.fastq and <name>_2.fastq with -p; .gz with -z).  A bait that
captures nothing gets no file.  At the end one line per bait, `<first file>: <reads>`, goes to stderr.

As in the reference, the read k-mers are forward 25-mers whatever -k says: with -k 24 a read hits a bait when one of
its 25-mers has the value of one of the bait's 24-mers (that is, 'A' followed by the bait 24-mer).
Differences from the reference: FASTA read inputs are refused (the reference fails at the first captured read); when
mate 2 ends before mate 1 the warning is printed and the pair ends there; baits with the same name share one file, each
batch's records written one bait after the other; -b does not change the output.
"""
# Drop-in for zotmer/commands/capture.py; the device path is zotmer_amd/library/capture.py.
import sys

from zotmer_amd.library import seqio
from zotmer_amd.library.usage import Spec

_SPEC = Spec(options={"-b": True, "-k": True, "-m": True, "-P": True, "-p": False, "-v": False, "-z": False},
             positionals=["<sequences>"], rest="<input>")


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
    K = _int(opts, "-k", 24, 1, 32)
    _int(opts, "-b", 4096, 1)                       # capture.py:75; only changes when the reference flushes
    mem = _int(opts, "-m", 0, 1) if opts["-m"] is not None else None
    prefix = opts["-P"] if opts["-P"] is not None else "."
    paired, verbose, z = opts["-p"], opts["-v"], opts["-z"]
    inputs = opts["<input>"]
    fasta = [p for p in inputs if seqio.is_fasta(p)]
    if fasta:
        _SPEC._die("zot capture reads FASTQ only: %s" % ", ".join(fasta), __doc__)

    # nothing touches the device before the arguments are known to be good
    from zotmer_amd.library import capture, engine
    records = capture.bait_records(opts["<sequences>"])
    if not records:
        return 0
    ctx = engine.context()
    table = capture.build_table(ctx, records, K)
    sink = capture.Sink([nm for nm, _ in records], prefix, paired, z)
    batch = (mem << 20) if mem is not None else capture_batch_bytes(ctx)
    try:
        capture.capture_inputs(ctx, table, inputs, paired, sink, batch, verbose=verbose)
    finally:
        table.free()
    sink.end()
    return 0


def capture_batch_bytes(ctx):
    """Default batch: 256 MiB of text per mate, less when device memory is short (two text buffers per mate, the line
    ends, the pairs and the gathered records: about 6 bytes per text byte and mate)."""
    free, _ = ctx.mem_info()
    return max(1 << 20, min(256 << 20, int(free * 0.5) // 12))


if __name__ == "__main__":
    main(["capture"] + sys.argv[1:])
