"""`zot scan` in plain Python, restated from the reference (zotmer/commands/scan.py with library/basics.py:115-170, 394-439,
misc.py:24-79, sparse.py:55-91 and stats.py:27-34, 77-93, 228-250, 273-283) for the tests: no product code is imported here.
tests/golden/make_golden_scan.py asserts that it reproduces the reference's index members and output lines.  The line numbers
are scan.py's unless a file is named."""
import bisect
import math

_SMALL = [math.log(math.factorial(n)) for n in range(25)]
_FAS = ['*', 'A', 'C', 'M', 'G', 'R', 'S', 'V', 'T', 'W', 'Y', 'H', 'K', 'D', 'B', 'N']
_NUC = {}
for _i, _cs in enumerate(("Aa", "Cc", "Gg", "TtUu")):
    for _c in _cs:
        _NUC[_c] = _i


# ---- basics.py ---------------------------------------------------------------------------------------------------------------

def lcp(K, x, y):
    """basics.py:160-170; ffs is the position of the highest set bit"""
    z = x ^ y
    if z == 0:
        return K
    return K - (1 + (z.bit_length() - 1) // 2)


def rc(K, x):
    """basics.py:115-121"""
    y = 0
    for _ in range(K):
        y = (y << 2) | (3 - (x & 3))
        x >>= 2
    return y


def kmers_with_pos(K, seq):
    """basics.py:394-439 with bothStrands"""
    z = len(seq)
    msk = (1 << (2 * K)) - 1
    s = 2 * (K - 1)
    i = j = x = xb = 0
    while i + K <= z:
        while i + j < z and j < K:
            b = _NUC.get(seq[i + j])
            if b is None:
                i += j + 1
                j = 0
                x = 0
                xb = 0
            else:
                x = (x << 2) | b
                xb = (xb >> 2) | ((3 - b) << s)
                j += 1
        if j == K:
            x &= msk
            yield (x, i + 1)
            yield (xb, -(i + 1))
            j -= 1
        i += 1


# ---- the index: lines 180-243 ------------------------------------------------------------------------------------------------

def index_build(records, K=27):
    """records = [(name, sequence str)] in file order -> (meta, S, T, U, V) as lists"""
    xs = []
    qacgt = [0, 0, 0, 0]
    N = 0
    for nm, seq in records:
        if len(seq) < K:
            continue
        for x, p in kmers_with_pos(K, seq):
            xs.append(x)
            qacgt[x & 3] += 1
            N += 1
    S = sorted(set(xs))
    qacgt = [float(c) / float(N) for c in qacgt]
    lens, nms, seqs = [], [], []
    tmp = [[] for _ in S]
    n = 0
    for nm, seq in records:
        if len(seq) < K:
            continue
        nms.append(nm)
        seqs.append(seq)
        lens.append(len(seq))
        for x, p in kmers_with_pos(K, seq):
            tmp[bisect.bisect_left(S, x)].append((n, p))
        n += 1
    T, U, V = [], [], []
    t = 0
    for nps in tmp:
        T.append(t)
        t += len(nps)
        for n_, p in nps:
            U.append(n_)
            V.append(p)
    T.append(t)
    meta = {"K": K, "lens": lens, "qacgt": qacgt, "nms": nms, "seqs": seqs}
    return meta, S, T, U, V


# ---- resolveAll: lines 95-120 ------------------------------------------------------------------------------------------------

def resolve_all(K, S, X, passes=2):
    """-> (L, Y); passes=1 stops after the first loop (for the builders' conditions)"""
    Z = len(S)
    L = [0] * Z
    Y = [0] * Z
    i = 0
    for x in X:
        while i < Z and S[i] <= x:
            l = lcp(K, x, S[i])
            if l > L[i]:
                L[i] = l
                Y[i] = x
            i += 1
    while i < Z:
        l = lcp(K, x, S[i])          # x: the last element of X (NameError when X is empty)
        if l > L[i]:
            L[i] = l
            Y[i] = x
        i += 1
    if passes == 1:
        return L, Y
    for i in range(1, Z):
        x = Y[i - 1]
        l = lcp(K, x, S[i])
        if l > L[i]:
            L[i] = l
            Y[i] = x
    return L, Y


def best_of_neighbours(K, S, X):
    """what resolveAll is NOT: the longer lcp with the predecessor and the successor of S[i] in X"""
    out = []
    for s in S:
        j = bisect.bisect_left(X, s)
        out.append(max([lcp(K, X[q], s) for q in (j - 1, j) if 0 <= q < len(X)]))
    return out


# ---- the placement: lines 281-304 --------------------------------------------------------------------------------------------

def place(K, L, Y, T, U, V, slots):
    """slots[n] = lens[n] - K + 1 -> (P, Q, cnt) as lists per record"""
    cnt = [[0] * (K + 1) for _ in slots]
    P = [[0] * w for w in slots]
    Q = [[0] * w for w in slots]
    for i in range(len(T) - 1):
        for j in range(T[i], T[i + 1]):
            n = U[j]
            p = V[j]
            y = Y[i]
            l = L[i]
            cnt[n][l] += 1
            if p > 0:
                p -= 1
            else:
                p = -(p + 1)
                y = rc(K, y)
            if l > Q[n][p]:
                Q[n][p] = l
                P[n][p] = y
    return P, Q, cnt


# ---- the per-record stage: lines 122-175, 306-449 ----------------------------------------------------------------------------

class UnionFind:
    """misc.py:24-79"""

    def __init__(self):
        self.parent = {}
        self.rank = {}

    def find(self, x):
        if x not in self.parent:
            self.parent[x] = x
            self.rank[x] = 0
            return x
        xp = self.parent[x]
        if xp != x:
            self.parent[x] = self.find(xp)
        return self.parent[x]

    def union(self, x, y):
        xr = self.find(x)
        yr = self.find(y)
        if xr == yr:
            return
        if self.rank[xr] < self.rank[yr]:
            self.parent[xr] = yr
        elif self.rank[xr] > self.rank[yr]:
            self.parent[yr] = xr
        else:
            self.parent[yr] = xr
            self.rank[xr] += 1


def ham(x, y):
    """basics.py:123-133"""
    z = x ^ y
    return bin((z | (z >> 1)) & 0x5555555555555555).count("1")


def succ(K, X, x):
    """lines 122-127; sparse.rank2 (sparse.py:77-91) = two lower bounds"""
    m = (1 << (2 * K)) - 1
    y0 = (x << 2) & m
    y1 = y0 + 4
    return range(bisect.bisect_left(X, y0), bisect.bisect_left(X, y1))


def null(g, s, j):
    if j == 0:
        return 0.0
    return math.exp(s * math.log1p(-math.pow(g, j)))


def log_fac(n):
    if n < len(_SMALL):
        return _SMALL[n]
    return n * math.log(n) - n + math.log(n * (1 + 4 * n * (1 + 2 * n))) / 6.0 + math.log(math.pi) / 2.0


def log_add(a, b):
    x = max(a, b)
    y = min(a, b)
    w = y - x
    return x + math.log1p(math.exp(w))


def log1mexp(a):
    if -a < 0.6931472:
        return math.log(-math.expm1(a))
    else:
        return math.log1p(-math.exp(a))


def log_gamma_p_int(n, x):
    if x < n:
        lx = math.log(x)
        w = 0
        v = log_fac(n)
        s = w - v
        j = 1
        while True:
            w += lx
            v += math.log(j + n)
            u = log_add(s, w - v)
            if s == u:
                break
            s = u
            j += 1
        return n * lx + s - x
    else:
        lx = math.log(x)
        s = 0
        v = 0
        for k in range(1, n):
            v += math.log(k)
            t = k * lx - v
            u = log_add(t, s)
            s = u
        w = min(s - x, -1e-200)
        return log1mexp(w)


def chi2(n, x):
    d = int(math.ceil(n / 2.0))
    c2 = x / 2.0
    return log_gamma_p_int(d, c2)


def counts2cdf(xs):
    n = max(1, sum(xs))
    t = 0
    ys = []
    for x in [float(x) / n for x in xs]:
        ys.append(t)
        t += x
    return ys


def ks_distance2(l, r):
    dl = 0
    dr = 0
    for x, y in zip(l, r):
        dl = max(dl, x - y)
        dr = max(dr, y - x)
    return dl, dr


def record_stage(K, meta, sacgt, X, P, Q, cnt, events=None):
    """lines 276-278 and 306-449 for one sample -> the stdout lines.  events (a dict) collects which branches ran."""
    lens, nms = meta["lens"], meta["nms"]
    M = len(X)
    g = sum([qp * sp for (qp, sp) in zip(meta["qacgt"], sacgt)])
    nm = [null(g, M, j) for j in range(0, K + 1)]
    out = []
    ev = events if events is not None else {}
    for i in range(len(nms)):
        qc = math.log(K * 0.05 / float(lens[i] - K + 1) / 2)
        m = (1 << (2 * K - 2)) - 1
        py = 0
        u = UnionFind()
        for j in range(lens[i] - K + 1):
            x = P[i][j]
            y = x >> 2
            if j > 0:
                d = ham(py, y)
                if d == 0:
                    u.union(j - 1, j)
            py = x & m

        udx = {}
        for j in range(lens[i] - K + 1):
            v = u.find(j)
            if v not in udx:
                udx[v] = []
            udx[v].append(j)

        idxLhs = {}
        kx = []
        for (jx, js) in udx.items():
            q = 0
            for j in js:
                q += math.log1p(-nm[Q[i][j]])
            if q > math.log(0.05 / len(js)):
                continue
            kx.append((-len(js), jx))
            idxLhs[P[i][js[0]]] = jx
        kx.sort()
        if len(kx) > 1:
            ev["fragments>1"] = ev.get("fragments>1", 0) + 1

        links = {}
        for (_, jx) in kx:
            jR = udx[jx][-1]
            if jR == lens[i] - K + 1:
                continue
            x = P[i][jR]
            xs = []
            lnk = None
            for k in range(100):
                ys = succ(K, X, x)
                if len(ys) != 1:
                    break
                x = ys[0]
                if x in idxLhs:
                    lnk = idxLhs[x]
                    break
                xs.append(x)
            if lnk is not None:
                links[jx] = xs
                u.union(jx, lnk)
                ev["link"] = ev.get("link", 0) + 1

        vdx = {}
        for j in [jx for (_, jx) in kx]:
            v = u.find(j)
            if v not in vdx:
                vdx[v] = []
            vdx[v].append(j)

        res = []
        for (jxx, jxs) in vdx.items():
            fs = [(udx[jx][0], jx) for jx in jxs]
            fs.sort()
            sxs = []
            for fj in range(len(fs)):
                (_, jx) = fs[fj]
                beg = udx[jx][0]
                end = udx[jx][-1] + 1
                if fj == 0:
                    for j in range(beg):
                        sxs.append((0, 0))
                xs = links.get(jx, None)
                for j in range(beg, end):
                    x = P[i][j]
                    l = Q[i][j]
                    sxs.append((x, l))
                if xs:
                    for x in xs:
                        sxs.append((x, 27))
                else:
                    if fj < len(fs) - 1:
                        nxt = fs[fj + 1][0]
                    else:
                        nxt = lens[i] - K + 1
                    for j in range(end, nxt):
                        sxs.append((0, 0))
            seq = [[0, 0, 0, 0] for j in range(len(sxs) + K - 1)]
            for j in range(len(sxs)):
                (x, l) = sxs[j]
                p = math.log1p(-nm[l])
                for k in range(K):
                    seq[j + K - k - 1][x & 3] += p
                    x >>= 2
            ax = []
            p = None
            inf = False
            for j in range(len(seq)):
                b = 0
                for k in range(4):
                    if seq[j][k] < qc:
                        b |= 1 << k
                ax.append(_FAS[b])
                ssj = sum(seq[j])
                if p is None:
                    p = ssj
                else:
                    p = log_add(p, ssj)
                if ssj > -1e-300:
                    inf = True
            dst = counts2cdf(cnt[i])
            (_, kd) = ks_distance2(dst, nm)
            df = math.ceil(len(seq) / float(K))
            if inf:
                q = 1e300
                pv = 0.0
            else:
                q = 2 * math.exp(p)
                pv = chi2(df, q)
            res.append((pv, q, kd, ''.join(ax)))

        if len(res) == 0:
            ev["no line"] = ev.get("no line", 0) + 1
            continue
        res.sort()
        if res[0][0] < -2:
            pv = res[0][0] / math.log(10)
            c2 = res[0][1]
            kd = res[0][2]
            a = res[0][3]
            out.append('%d\t%d\t%d\t%g\t%g\t%g\t%s\t%s' % (i, lens[i], len(a), kd, c2, pv, nms[i], a))
            ev["line"] = ev.get("line", 0) + 1
        else:
            ev["no line"] = ev.get("no line", 0) + 1
    return out


def scan_lines(records, samples, K=27, events=None):
    """the whole command: records as for index_build, samples = [(acgt, ascending k-mers)] -> the lines per sample"""
    meta, S, T, U, V = index_build(records, K)
    slots = [n - K + 1 for n in meta["lens"]]
    out = []
    for sacgt, X in samples:
        L, Y = resolve_all(K, S, X)
        P, Q, cnt = place(K, L, Y, T, U, V, slots)
        out.append(record_stage(K, meta, sacgt, X, P, Q, cnt, events))
    return out
