"""
Usage:
    zot spoligo [-l] [-d D] -p PROBES <input>...

Perform spoligotyping on sets of k-mers: for every probe of a panel, is it present in the set up to D substituted
bases?  A probe of at most K bases is present when some k-mer of the set starts with it; a longer one when every run
of K of its bases is.  One line `input <TAB> 0/1 per probe` is printed per input.

PROBES is a text file with an optional name and a probe on each line.  Lines starting with '#' are ignored; a probe
without a name is named by its number among the probe lines.

Options:
    -l          use long output format with one line per probe
    -d D        the largest Hamming distance accepted: 0, 1 or 2 [default: 2]
    -p PROBES   the name of a file containing probe sequences

Differences from the reference: -p is required (the reference's built-in panel of 43 MTB probes is not shipped; the
same probes given in a file print the reference's lines); -d is new (2 is the reference's constant); a probe with a
character other than AaCcGgTtUu is an error that names the probe (the reference dies with a TypeError); an input
with no k-mers prints all zeros; with several processes (torch.distributed.run) the command refuses: it runs on a
single GPU.
"""
# Drop-in for zotmer/commands/spoligo.py; the device path is zotmer_amd/library/spoligo.py.
import os
import sys

from zotmer_amd.library import spoligo
from zotmer_amd.library.usage import Spec

_SPEC = Spec(options={"-l": False, "-d": True, "-p": True}, rest="<input>")


def main(argv):
    opts = _SPEC.parse(argv[1:], __doc__)
    if opts["-p"] is None:
        _SPEC._die("zot spoligo: -p PROBES is required: the built-in MTB panel of the reference is not shipped.  PROBES is a "
                   "text file with one `[name] probe` per line; lines starting with '#' are ignored", __doc__)
    D = opts["-d"].strip() if opts["-d"] is not None else str(spoligo.MAX_D)
    if D not in ("0", "1", "2"):
        _SPEC._die("zot spoligo: -d must be 0, 1 or 2", __doc__)
    D = int(D)
    names, probes, bad = spoligo.read_probes(opts["-p"])
    if bad:
        raise SystemExit(1)         # spoligo.py:188-189, after the whole file
    wrong = spoligo.bad_probes(names, probes)
    if wrong:
        for nm, p in wrong:
            sys.stderr.write("zot spoligo: probe %s (%s) has a character other than AaCcGgTtUu\n" % (nm, p))
        raise SystemExit(1)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("zot spoligo: runs on a single GPU for now")

    # nothing touches the device before the arguments and the panel are known to be good
    from zotmer_amd.library import engine, vectors
    from zotmer_amd.library.container import KmerSet
    ctx = engine.context()
    panel = spoligo.Panel(names, probes)
    for inp in opts["<input>"]:
        with KmerSet(inp, "r") as z:
            K = z.meta["K"]
            kmers = vectors.device_read_kmers(ctx, z)
        present = panel.present(ctx, kmers, K, D)
        del kmers
        sys.stdout.write("".join(spoligo.lines(inp, names, present, opts["-l"])))
    return 0


if __name__ == "__main__":
    main(["spoligo"] + sys.argv[1:])
