"""
zot hgvs-gen - generate random variants over the zones of a BED file.

Usage:
    zot hgvs-gen [options] <regions>

Options:
    -D LENGTH       mean length for deletion events [default: 1.5]
    -I LENGTH       mean length for insertion events [default: 1.5]
    -U LENGTH       mean length for duplication events [default: 3.0]
    -g PATH         directory of reference sequences [default: .]
    -n NAMES        text file with "accession  file-stem" per line: which file of -g holds an accession
    -N NUMBER       number of HGVSg variants to generate [default: 1]
    -S SEED         set a random number seed
    -t TYPES        comma separated list of variant types [default: sub,del,ins,delins,dup]
    -T              produce output in a tabular form
    -o FILE         write the variants to FILE, not to the standard output
    -B MB           size of the per-call output buffer on the GPU (in MB); the output does not depend on it
    -v              produce progress messages
    -V              produce verbose output: a line `# <chrom> : <zone name>` whenever the zone name changes

Variant types: sub (substitution), del (deletion), ins (insertion), delins (deletion/insertion), dup (duplication), ani
(anonymous insertion, `ins<length>`), and (anonymous deletion/insertion, `delins<length>`).  Written as prob:type, a type is
drawn with the relative probability prob, 1.0 by default.

-N draws are spread over the zones in proportion to their lengths, both ends of a zone inclusive.  The variants come
chromosome by chromosome in name order, the zones of a chromosome in the order of their lines in the BED file.  A line is an
HGVSg string; with -T it is preceded by the accession, the 0-based half-open range the variant replaces, the length of what it
puts there, the wild-type bases and the mutant bases, separated by tabs.  The lengths are geometric with the means -D, -I and
-U; as in the reference a deletion or duplication of drawn length l covers p .. min(p + l, e), so l + 1 bases inside a zone.
The output feeds `zot hgvs-index`, and `zot spikein -f` / `-m`.

Differences from the reference: the random numbers are a counter-based generator, every draw a function of the seed and the
variant's number (the reference uses Python's random, whose output differs between Python versions); without -S a seed is
taken from the operating system and printed under -v; a geometric length is looked up in a table of 32-bit thresholds, so
lengths whose probability is below 2^-32 do not occur, and the means are limited to 1 .. about 4574 (a table of 65536
entries); a mean of exactly 1, at which the reference's geomvar raises (log1p(-1)), always gives the length 1; delins and
`and` draw their two lengths from the conditional law of the reference's rejection loop directly, and -D 1 with -I 1, where
every pair of lengths would be rejected, is refused when one of the two types can be drawn; a substitution tries 64 positions
and then takes the next base of ACGT round the zone, and a zone without one is refused (the reference loops forever); the
probabilities of a type named twice in -t add up; an unnamed zone is called None (the reference dies on it); chromosome names
are used as the BED file gives them, and accessions are mapped to file stems by -n, not by a table of the 24 hg19 chromosomes;
a zone that is empty, starts below 0 or ends at or beyond the end of its sequence is refused with a message (in the reference
an assertion fails); -n, -o and -B are new; -v prints counts, not a progress bar; several processes (torch.distributed.run)
are refused: one GPU for now. Nothing touches the device before the arguments, the BED file, the types and the sequence files
are known to be good.
"""
# Drop-in for zotmer/commands/hgvs-gen.py; the work is zotmer_amd/library/hgvsgen.py.
import os
import sys

from zotmer_amd.library.usage import Spec

_SPEC = Spec(options={"-D": True, "-I": True, "-U": True, "-g": True, "-n": True, "-N": True, "-S": True, "-t": True, "-T": False,
                      "-o": True, "-B": True, "-v": False, "-V": False},
             positionals=["<regions>"])


def _num(opts, name, default, kind, lo=None, hi=None):
    v = opts[name]
    try:
        v = kind(v) if v is not None else default
    except ValueError:
        _SPEC._die("option %s needs %s" % (name, "an integer" if kind is int else "a number"), __doc__)
    if v is not None and ((lo is not None and not v >= lo) or (hi is not None and not v <= hi)):
        _SPEC._die("option %s out of range" % name, __doc__)
    return v


class _Stdout:
    """the standard output as the binary file library/hgvsgen.py writes to"""

    def write(self, data):
        sys.stdout.write(bytes(data).decode("latin-1"))

    def flush(self):
        sys.stdout.flush()


def main(argv):
    opts = _SPEC.parse(argv[1:], __doc__)
    D = _num(opts, "-D", 1.5, float)
    I = _num(opts, "-I", 1.5, float)
    U = _num(opts, "-U", 3.0, float)
    N = _num(opts, "-N", 1, int, 0, (1 << 40) - 1)
    mb = _num(opts, "-B", 0, int, 1) if opts["-B"] is not None else None
    seed = _num(opts, "-S", None, int)
    home = opts["-g"] if opts["-g"] is not None else "."
    if not os.path.isdir(home):
        _SPEC._die("zot hgvs-gen: %s is not a directory" % home, __doc__)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        sys.stderr.write("zot hgvs-gen: runs on a single GPU for now\n")
        raise SystemExit(1)
    if seed is None:
        seed = int.from_bytes(os.urandom(8), "little")
        if opts["-v"]:
            sys.stderr.write("seed = %d\n" % seed)

    from zotmer_amd.library import hgvsgen, hgvsindex
    try:
        names = hgvsindex.read_names(opts["-n"]) if opts["-n"] is not None else None
        plan = hgvsgen.make_plan(dict(bed=opts["<regions>"], home=home, names=names, seed=seed,
                                      types=opts["-t"] if opts["-t"] is not None else hgvsgen.DEFAULT_TYPES, D=D, I=I, U=U))
    except (hgvsgen.InputError, IOError) as e:
        sys.stderr.write("zot hgvs-gen: %s\n" % e)
        raise SystemExit(1)
    # nothing touches the device before the arguments, the BED file, the types and the sequence files are known to be good
    from zotmer_amd.library import engine
    ctx = engine.context()
    out = open(opts["-o"], "wb") if opts["-o"] is not None else _Stdout()
    try:
        hgvsgen.run(ctx, plan, N, out, tab=opts["-T"], heads=opts["-V"], verbose=opts["-v"],
                    buffer_bytes=(mb << 20) if mb is not None else hgvsgen.DEFAULT_BUFFER)
        out.flush()
    except (hgvsgen.InputError, IOError) as e:
        sys.stderr.write("zot hgvs-gen: %s\n" % e)
        raise SystemExit(1)
    finally:
        if opts["-o"] is not None:
            out.close()
    return 0


if __name__ == "__main__":
    main(["hgvs-gen"] + sys.argv[1:])
