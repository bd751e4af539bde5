"""
`zot spoligo` on the device (zotmer/commands/spoligo.py): which probes of a panel are present in a k-mer set, up to D
substituted bases.

The reference enumerates the substitution neighbours of a probe window and searches the sorted set once per neighbour
(findApprox, spoligo.py:50-67: 2 776 searches for a 25-base window).  Its neighbourhoods are the values at Hamming
distance exactly 1 and exactly 2, so the answer is "the set holds a k-mer whose first J bases are within distance D of
the window", which zk_probe_scan (csrc/probe_scan.hip) tallies for every window of the panel in one pass over the set.
The host reads the probe file, cuts the windows from the text and turns the tallies into the reference's lines.
"""
import sys

# basics._nuc (basics.py:42): what basics.kmer accepts
NUC = {"A": 0, "a": 0, "C": 1, "c": 1, "G": 2, "g": 2, "T": 3, "t": 3, "U": 3, "u": 3}
MAX_D = 2                   # spoligo.py:73,81: the reference's constant


def encode(seq):
    """basics.kmer (basics.py:48-59) -> the 2-bit value, or None if a character is no base"""
    r = 0
    for ch in seq:
        b = NUC.get(ch)
        if b is None:
            return None
        r = (r << 2) | b
    return r


def read_probes(path, err=None):
    """the -p file as spoligo.py:166-189 reads it: a line whose first character is '#' is skipped; one token is a probe named
    by its ordinal among the probe lines, two are name and probe; anything else is reported as the reference reports it (with
    that ordinal, not the line number) -> (names, probes, bad).  The caller exits once the whole file is read."""
    err = err if err is not None else sys.stderr
    names, probes, bad = [], [], False
    with open(path) as f:
        i = 0
        for line in f:
            if line[0] == "#":
                continue
            i += 1
            t = line.split()
            if len(t) == 1:
                names.append(str(i))
                probes.append(t[0])
            elif len(t) == 2:
                names.append(t[0])
                probes.append(t[1])
            else:
                bad = True
                err.write("%s line %d, badly formatted.\n" % (path, i))
    return names, probes, bad


def bad_probes(names, probes):
    """[(name, probe)] of the probes basics.kmer has no value for"""
    return [(nm, p) for nm, p in zip(names, probes) if encode(p) is None]


def cut_windows(probe, K):
    """findProbe (spoligo.py:69-84): a probe of at most K bases is one window (J = its length); a longer one is every run
    of K of its bases, each of which must be present.  Cut from the text, so a probe may be longer than 32 bases.
    -> [(J, value)]"""
    Kp = len(probe)
    if Kp <= K:
        return [(Kp, encode(probe))]
    return [(K, encode(probe[i:i + K])) for i in range(1 + Kp - K)]


class Panel:
    """The probes of one file; the window list of a K is built once, whatever the number of inputs of that K."""

    def __init__(self, names, probes):
        self.names, self.probes = list(names), list(probes)
        self._plans = {}

    def plan(self, K):
        """-> (every window of the panel, [(first window, end) per probe])"""
        if K not in self._plans:
            windows, spans = [], []
            for p in self.probes:
                w = cut_windows(p, K)
                spans.append((len(windows), len(windows) + len(w)))
                windows += w
            self._plans[K] = (windows, spans)
        return self._plans[K]

    def present(self, ctx, kmers, K, D=MAX_D):
        """kmers: the ascending k-mers of a set on the device -> [bool per probe]"""
        windows, spans = self.plan(K)
        tallies = ctx.probe_scan(kmers, K, windows)
        hit = tallies[:, :D + 1].sum(axis=1) > 0
        return [bool(hit[a:b].all()) for a, b in spans]


def lines(inp, names, present, long_format):
    """spoligo.py:197-207"""
    res = ["1" if p else "0" for p in present]
    if long_format:
        return ["%s\t%s\t%s\n" % (inp, nm, r) for nm, r in zip(names, res)]
    return [inp + "\t" + "".join(res) + "\n"]
