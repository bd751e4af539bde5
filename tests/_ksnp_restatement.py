"""`zot ksnp` restated in plain Python 3, from the definitions (zotmer/commands/ksnp.py: ksnp, hamming, levenshtein).

With J = (K - 1) // 2, S = 2 (J + 1), T = 2 J a k-mer x has the prefix x >> S, the middle base (x >> T) & 3 and the tail
x & (4^J - 1).  The input is the ascending k-mer list of a set.

  default   x is kept iff another k-mer of the set has its prefix and its tail;
  -H d      inside every prefix group the pairs with ham(x, y) <= d are joined; a connected component is kept iff its members
            carry at least two different middle bases;
  -L d      the same with lev(K, x, y) <= d for x before y in the list, basics.lev's unit-cost recurrence (see lev below) -- the
            full (K + 1) x (K + 1) table, on purpose: the device compares the bases below the prefix only.

Every function returns the kept k-mers ascending.  tests/golden/k1_ksnp.json holds what the reference's generators yield."""

DEFAULT, HAMMING, LEVENSHTEIN = "default", "hamming", "levenshtein"


def geometry(K):
    J = (K - 1) // 2
    return J, 2 * (J + 1), 2 * J


def ham(x, y):
    z = x ^ y
    return bin((z | (z >> 1)) & 0x5555555555555555).count("1")


def bases(K, x):
    """the K bases of x, the LAST base first: the order basics.lev reads them in"""
    return [(x >> (2 * i)) & 3 for i in range(K)]


def lev(K, x, y):
    """basics.lev (basics.py:135-158).  Its table starts from a row of ZEROS, not from 0, 1, .. K: bases at the end of y may
    be left out for nothing, so this is the least edit distance between x and a leading part of y, it is not symmetric, and
    the callers pass the k-mer that comes first in the list as x."""
    a, b = bases(K, x), bases(K, y)
    row = [0] * (K + 1)
    for i in range(1, K + 1):
        new = [i] + [0] * K
        for j in range(1, K + 1):
            new[j] = min(row[j - 1] + (0 if a[i - 1] == b[j - 1] else 1), row[j] + 1, new[j - 1] + 1)
        row = new
    return row[K]


def groups(K, xs):
    """the k-mers by prefix, in the order of the list"""
    _, S, _ = geometry(K)
    out = {}
    for x in xs:
        out.setdefault(x >> S, []).append(x)
    return out


def flank(K, xs):
    J, S, _ = geometry(K)
    tail = (1 << (2 * J)) - 1
    seen = {}
    for x in xs:
        seen.setdefault((x >> S, x & tail), []).append(x)
    return sorted(x for members in seen.values() if len(members) > 1 for x in members)


class UnionFind:
    def __init__(self, n):
        self.parent = list(range(n))

    def find(self, i):
        root = i
        while self.parent[root] != root:
            root = self.parent[root]
        while self.parent[i] != root:
            self.parent[i], i = root, self.parent[i]
        return root

    def union(self, i, j):
        a, b = self.find(i), self.find(j)
        if a != b:
            self.parent[max(a, b)] = min(a, b)


def components(K, xs, near):
    """near(x, y) -> bool joins two k-mers of one group"""
    _, _, T = geometry(K)
    kept = []
    for members in groups(K, xs).values():
        u = UnionFind(len(members))
        for i in range(len(members)):
            for j in range(i + 1, len(members)):
                if near(members[i], members[j]):
                    u.union(i, j)
        middles = {}
        for i, x in enumerate(members):
            middles.setdefault(u.find(i), set()).add((x >> T) & 3)
        kept += [x for i, x in enumerate(members) if len(middles[u.find(i)]) >= 2]
    return sorted(kept)


def hamming(K, d, xs):
    return components(K, xs, lambda x, y: ham(x, y) <= d)


def levenshtein(K, d, xs):
    return components(K, xs, lambda x, y: lev(K, x, y) <= d)


def run(K, mode, d, xs):
    if mode == DEFAULT:
        return flank(K, xs)
    return (hamming if mode == HAMMING else levenshtein)(K, d, xs)
