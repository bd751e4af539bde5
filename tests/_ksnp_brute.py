"""`zot ksnp` a second time, by brute force in NumPy: per prefix group the whole distance matrix, then breadth-first components
over it.  Shares no code with tests/_ksnp_restatement.py (no union-find, no dicts of tails), and is fast enough for groups of a
few thousand k-mers, where the plain-Python restatement is not.  The edit distance is the full (K + 1) x (K + 1) recurrence over
all K bases, a row at a time for all pairs at once."""
import numpy as np

U = np.uint64


def geometry(K):
    J = (K - 1) // 2
    return J, 2 * (J + 1), 2 * J


def group_slices(K, xs):
    _, S, _ = geometry(K)
    p = xs >> U(S)
    cuts = np.flatnonzero(np.concatenate([[True], p[1:] != p[:-1], [True]]))
    return [(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]


def ham_matrix(g):
    z = g[:, None] ^ g[None, :]
    return np.bitwise_count((z | (z >> U(1))) & U(0x5555555555555555))


def lev_pairs(K, a, b):
    """basics.lev(K, a[p], b[p]) for all p: bases from the last one on, the first row of the table all zeros (bases at the end
    of b may be left out for nothing: not symmetric)"""
    sh = (2 * np.arange(K)).astype(np.uint64)
    A = ((a[None, :] >> sh[:, None]) & U(3)).astype(np.int8)          # [base, pair]
    B = ((b[None, :] >> sh[:, None]) & U(3)).astype(np.int8)
    ramp = np.arange(K + 1, dtype=np.int8)[:, None]
    row = np.zeros((K + 1, len(a)), dtype=np.int8)                    # row[j, p]: the cell of column j
    for i in range(1, K + 1):
        cost = (A[i - 1][None, :] != B).astype(np.int8)
        t = np.empty_like(row)
        t[0] = i
        t[1:] = np.minimum(row[:-1] + cost, row[1:] + 1)
        # new[j] = min over k <= j of t[k] + (j - k): the horizontal steps
        row = np.minimum.accumulate(t - ramp, axis=0) + ramp
    return row[K].astype(np.int16)


def lev_matrix(K, g, block=1 << 18):
    n = len(g)
    i, j = np.triu_indices(n, 1)
    m = np.zeros((n, n), dtype=np.int16)
    for s in range(0, len(i), block):
        m[i[s:s + block], j[s:s + block]] = lev_pairs(K, g[i[s:s + block]], g[j[s:s + block]])
    return m + m.T


def kept_of_group(K, g, near):
    """near: bool[n, n]"""
    _, _, T = geometry(K)
    mid = ((g >> U(T)) & U(3)).astype(np.int64)
    n = len(g)
    label = np.full(n, -1, dtype=np.int64)
    keep = np.zeros(n, dtype=bool)
    for s in range(n):
        if label[s] >= 0:
            continue
        seen = np.zeros(n, dtype=bool)
        seen[s] = True
        front = seen.copy()
        while front.any():
            nxt = near[front].any(axis=0) & ~seen
            seen |= nxt
            front = nxt
        label[seen] = s
        keep[seen] = len(np.unique(mid[seen])) >= 2
    return keep


def run(K, mode, d, xs):
    """mode: "default", "hamming" or "levenshtein" -> the kept k-mers, ascending (uint64)"""
    xs = np.asarray(xs, dtype=np.uint64)
    J, S, T = geometry(K)
    if mode == "default":
        hit = np.zeros(len(xs), dtype=bool)
        for b in (1, 2, 3):
            hit |= np.isin(xs ^ U(b << T), xs)
        return xs[hit]
    keep = np.zeros(len(xs), dtype=bool)
    for a, b in group_slices(K, xs):
        if b - a < 2:
            continue
        g = xs[a:b]
        dist = ham_matrix(g) if mode == "hamming" else lev_matrix(K, g)
        near = dist <= min(d, 1 << 14)
        np.fill_diagonal(near, False)
        keep[a:b] = kept_of_group(K, g, near)
    return xs[keep]
