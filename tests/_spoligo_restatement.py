"""The reference's own route through `zot spoligo` (zotmer/commands/spoligo.py:26-84), restated in Python 3: the substitution
neighbours of a window are enumerated (neigh: every single substitution, sorted; for d = 2 the neighbours of the neighbours,
sorted, deduplicated, minus the window itself and minus its first neighbours) and the sorted set is searched once per
neighbour for an entry in [y << s, (y + 1) << s).  No Hamming distance is computed anywhere here: the device result is checked
against the reference's algorithm, not against its own formulation."""
import bisect

NUC = {"A": 0, "a": 0, "C": 1, "c": 1, "G": 2, "g": 2, "T": 3, "t": 3, "U": 3, "u": 3}


def kmer(seq):
    r = 0
    for ch in seq:
        r = (r << 2) | NUC[ch]
    return r


def _minus(xs, ys):
    """spoligo.diff: the sorted list xs without the members of the sorted list ys"""
    drop = set(ys)
    return [x for x in xs if x not in drop]


def neigh(K, x, d):
    if d == 0:
        return []
    xs = sorted(x ^ ((j + 1) << (2 * i)) for i in range(K) for j in range(3))
    if d == 1:
        return xs
    zs = []
    for y in xs:
        zs += neigh(K, y, d - 1)
    zs = sorted(set(zs))
    return _minus(_minus(zs, [x]), xs)


def _in_range(xs, y0, y1):
    """sparse.rank2(y0, y1) (library/sparse.py:77-91) gives r1 - r0 > 0: an entry of the sorted list in [y0, y1)"""
    r0 = bisect.bisect_left(xs, y0)
    return r0 < len(xs) and xs[r0] < y1


def find_approx(J, x, K, xs, D):
    assert J <= K
    s = 2 * (K - J)
    if _in_range(xs, x << s, (x + 1) << s):
        return True
    for d in range(1, D + 1):
        for y in neigh(J, x, d):
            if _in_range(xs, y << s, (y + 1) << s):
                return True
    return False


def find_probe(seq, K, xs, D=2):
    """findProbe on (len(seq), kmer(seq)): windows are taken from the low end of the value, the first absent one ends it"""
    Kp, x = len(seq), kmer(seq)
    if Kp <= K:
        return find_approx(Kp, x, K, xs, D)
    M = (1 << (2 * K)) - 1
    for _ in range(1 + Kp - K):
        if not find_approx(K, x & M, K, xs, D):
            return False
        x >>= 2
    return True


def spoligo(K, kmers, probes, D=2):
    """-> the 0/1 string of spoligo.py:197-207 for the probe sequences"""
    xs = sorted(kmers)
    return "".join("1" if find_probe(p, K, xs, D) else "0" for p in probes)
