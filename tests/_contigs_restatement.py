"""
`zot contigs` restated from its description, in Python 3 (written fresh; nothing here is derived from the reference's text):
the non-branching paths of the de Bruijn graph of an ascending k-mer list, walked greedily in index order.

    for i ascending, unless seen[i]:
        path = [i]; seen[i] = 1; x = S[i]
        while x has exactly one successor index j -- the entries of S in [y0, y0 + 3], y0 = (x << 2) & (4^K - 1):
            if seen[j]: stop
            path += [j]; seen[j] = 1; x = S[j]; seen[#{entries < rc(x)}] = 1
        print the path if len(path) + K - 1 >= L

The mark at #{entries < rc(x)} == n (a set that is not closed under reverse complement) is dropped: the reference sets a slack
bit of its bit vector there, or dies when n is a multiple of 64.
"""
import bisect

NO_LINK = 0xFFFFFFFF
DEAD_END, BRANCH, SEEN = "dead end", "branch", "seen"


def rc(K, x):
    y = 0
    for _ in range(K):
        y = (y << 2) | (3 - (x & 3))
        x >>= 2
    return y


def render(K, x):
    return "".join("ACGT"[(x >> (2 * (K - 1 - i))) & 3] for i in range(K))


def kmers_of(K, seq, both=True):
    """the ascending distinct k-mers of a sequence over ACGT (and of its reverse complement)"""
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    out = set()
    for i in range(len(seq) - K + 1):
        x = 0
        for ch in seq[i:i + K]:
            x = (x << 2) | code[ch]
        out.add(x)
        if both:
            out.add(rc(K, x))
    return sorted(out)


def links(K, xs):
    """-> (next, rank): next[i] = the index of the only successor of xs[i] or NO_LINK; rank[i] = the entries below rc(xs[i])"""
    m = (1 << (2 * K)) - 1
    nxt, rank = [], []
    for x in xs:
        y0 = (x << 2) & m
        a, b = bisect.bisect_left(xs, y0), bisect.bisect_right(xs, y0 + 3)
        nxt.append(a if b - a == 1 else NO_LINK)
        rank.append(bisect.bisect_left(xs, rc(K, x)))
    return nxt, rank


def successors(K, xs, x):
    m = (1 << (2 * K)) - 1
    y0 = (x << 2) & m
    return range(bisect.bisect_left(xs, y0), bisect.bisect_right(xs, y0 + 3))


def walk(K, xs, min_len, rc_marks=True, ends=None, dropped=None):
    """-> the kept paths as lists of indices, in start order.  ends (a list) takes, per kept path, why it stopped; dropped (a
    list) the nodes whose mark fell at n and was dropped."""
    n = len(xs)
    seen = [False] * n
    paths = []
    for i in range(n):
        if seen[i]:
            continue
        path = [i]
        seen[i] = True
        x = xs[i]
        while True:
            s = successors(K, xs, x)
            if len(s) != 1:
                why = DEAD_END if len(s) == 0 else BRANCH
                break
            j = s[0]
            if seen[j]:
                why = SEEN
                break
            path.append(j)
            seen[j] = True
            x = xs[j]
            if rc_marks:
                r = bisect.bisect_left(xs, rc(K, x))
                if r < n:
                    seen[r] = True
                elif dropped is not None:
                    dropped.append(j)
        if len(path) + K - 1 >= min_len:
            paths.append(path)
            if ends is not None:
                ends.append(why)
    return paths


def walk_links(nxt, rank, K, min_len):
    """the same walk on arbitrary link arrays (what zk_contig_walk is given) -> (nodes, offs)"""
    n = len(nxt)
    seen = [False] * n
    nodes, offs = [], []
    for i in range(n):
        if seen[i]:
            continue
        path = [i]
        seen[i] = True
        cur = i
        while nxt[cur] != NO_LINK and not seen[nxt[cur]]:
            cur = nxt[cur]
            path.append(cur)
            seen[cur] = True
            if rank[cur] < n:
                seen[rank[cur]] = True
        if len(path) + K - 1 >= min_len:
            offs.append(len(nodes))
            nodes += path
    offs.append(len(nodes))
    return nodes, offs


def text_of(K, xs, paths):
    out = []
    for p in paths:
        out.append(">contig_%d\n%s%s\n" % (p[0], render(K, xs[p[0]]), "".join("ACGT"[xs[j] & 3] for j in p[1:])))
    return "".join(out)


def stdout_text(K, xs, L=None, rc_marks=True, ends=None):
    return text_of(K, xs, walk(K, xs, 2 * K if L is None else L, rc_marks, ends))
