"""The reference's own route through `zot disass` (zotmer/commands/disass.py:27-103, with basics.kmersList, basics.py:303-347,
basics.sub and basics.murmer, basics.py:191-259, and file.readFasta, file.py:19-36), restated in plain Python 3 over lists and
dictionaries: no numpy, nothing of the project under test.

One choice is made where Python 3 leaves one: summarize's histogram dict is filled from the sorted values, so its items come in
ascending count -- the order the quantile loop walks (under Python 2 it is the hash table's).  `single_ok` opts into the one
deviation the product documents: a dict of exactly one k-mer gives median = float(count) where disass.py:43 raises IndexError."""
from tests._mlst_restatement import NUC, read_fasta

MASK64 = (1 << 64) - 1


def murmer(x, s):
    """basics.murmer (basics.py:191-229)"""
    k = (x * 0x87c37b91114253d5) & MASK64
    k = ((k << 31) | (k >> 33)) & MASK64
    k = (k * 0x4cf5ad432745937f) & MASK64
    h = s ^ k
    h = ((h << 27) | (h >> 37)) & MASK64
    h = (h * 5 + 0x52dce729) & MASK64
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & MASK64
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & MASK64
    h ^= h >> 33
    return h


def sub(s, p, x):
    """basics.sub (basics.py:252-259)"""
    u = float(murmer(x, s)) / float(0x1FFFFFFFFFFFFFFF)
    return u < p


def kmers_list(K, seq, both):
    """basics.kmersList (basics.py:303-347): x, then with `both` its reverse complement, for every window of K bases AaCcGgTtUu"""
    out, x, xb, run = [], 0, 0, 0
    msk, s = (1 << (2 * K)) - 1, 2 * (K - 1)
    for ch in seq:
        b = NUC.get(ch)
        if b is None:
            x = xb = run = 0
            continue
        x = ((x << 2) | b) & msk
        xb = (xb >> 2) | ((3 - b) << s)
        run += 1
        if run >= K:
            out.append(x)
            if both:
                out.append(xb)
    return out


def summarize(xs, cut, Q, single_ok=False):
    """summarize (disass.py:27-64); xs: dict k-mer -> count"""
    res = {}
    h = {}
    cs = sorted(xs.values())
    for c in cs:
        h[c] = 1 + h.get(c, 0)

    res["histogram"] = [list(it) for it in sorted(h.items())]
    res["mean"] = float(sum(cs)) / float(max(1, len(cs)))
    res["median"] = 0
    if len(cs) > 0:
        if (len(cs) & 1) == 0:
            res["median"] = cs[len(cs) // 2]
        elif len(cs) == 1 and single_ok:
            res["median"] = float(cs[0])
        else:
            m = len(cs) // 2
            res["median"] = (cs[m] + cs[m + 1]) / 2.0

    res["low-count"] = 0
    res["high-count"] = 0

    t = float(sum(h.values()))
    q0 = t / Q
    q = q0
    quant = []
    cum = 0
    for (c, f) in h.items():
        if c < cut:
            res["low-count"] += f
        else:
            res["high-count"] += f
        while cum + f > q:
            quant.append(c)
            q += q0
        cum += f
    res["quantiles"] = quant
    return res


def contig_dicts(text, K, both, S, P):
    """disass.py:86-99 for one FASTA text -> ([(name, dict)], the file's dict)"""
    glob, out = {}, []
    for nm, seq in read_fasta(text):
        scaff = {}
        for x in kmers_list(K, seq, both):
            if sub(S, P, x):
                scaff[x] = 1 + scaff.get(x, 0)
        out.append((nm, scaff))
        for x, c in scaff.items():
            glob[x] = c + glob.get(x, 0)
    return out, glob


def disass(files, K=25, C=5, P=1.0, Q=10, S=17, both=True, single_ok=False):
    """main (disass.py:66-103); files: [(file name, FASTA text)] -> the structure that is dumped"""
    res = []
    for fn, text in files:
        contigs, glob = contig_dicts(text, K, both, S, P)
        fres = {"file": fn, "contigs": []}
        for nm, scaff in contigs:
            summary = summarize(scaff, C, Q, single_ok)
            summary["name"] = nm
            fres["contigs"].append(summary)
        fres["global"] = summarize(glob, C, Q, single_ok)
        res.append(fres)
    return res
