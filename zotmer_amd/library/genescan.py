"""
Host side of `zot scan` (zotmer/commands/scan.py): the gene index (-X), its loading, the per-sample driver around
zk_lcp_resolve / zk_scan_place, and the per-record stage.

The per-record stage (scan.py:306-449) is a RESTATEMENT by necessity, like jstats.py and varscan.py: the printed columns are
'%g' of sums of logs and the consensus letters compare such sums with a threshold, so the same operations run in the same
order in Python floats.  Two things of the reference are kept on purpose: dictionaries are walked in insertion order (the
converted reference under Python 3), and the linking step's `x = ys[0]` puts a RANK of the sample where a k-mer was, which
every later step then works on.  The reference's `lev` is never called and has no counterpart here.
"""
import json
import math
import sys

import numpy as np

from zotmer_amd.library.jstats import log_add, log_fac

K_INDEX = 27                        # scan.py:181; :395 hard-codes it again
MEMBERS = (("S", "<u8"), ("T", "<u4"), ("U", "<u4"), ("V", "<i4"))
FASTA = "*ACMGRSVTWYHKDBN"          # basics.py:69-86: bit j of the index = base j
_CODE = np.full(256, 4, dtype=np.uint8)
for _b, _cs in enumerate(("Aa", "Cc", "Gg", "TtUu")):
    for _c in _cs:
        _CODE[ord(_c)] = _b


class ScanError(Exception):
    """an input that `zot scan` refuses, with the message for stderr"""


# ---- the index (scan.py:180-243) ---------------------------------------------------------------------------------------------

def windows_with_pos(K, seq):
    """basics.kmersWithPos(K, seq, True) (basics.py:394-439) as arrays in the order it yields: (x, p) and (rc x, -p) for every
    window without a byte outside AaCcGgTtUu, p = the 1-based start"""
    codes = _CODE[np.frombuffer(seq, dtype=np.uint8)].astype(np.uint64)
    n = len(codes) - K + 1
    if n <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.int64)
    bad = np.concatenate(([0], np.cumsum(codes == 4)))
    ok = (bad[K:] - bad[:-K]) == 0
    x = np.zeros(n, np.uint64)
    xb = np.zeros(n, np.uint64)
    for j in range(K):
        c = codes[j:j + n] & np.uint64(3)
        x |= c << np.uint64(2 * (K - 1 - j))
        xb |= (np.uint64(3) - c) << np.uint64(2 * j)
    pos = np.nonzero(ok)[0].astype(np.int64) + 1
    xs = np.empty(2 * len(pos), np.uint64)
    ps = np.empty(2 * len(pos), np.int64)
    xs[0::2], xs[1::2] = x[ok], xb[ok]
    ps[0::2], ps[1::2] = pos, -pos
    return xs, ps


def index_build(records, K=K_INDEX, warn=None):
    """records = (name, sequence bytes) in file order -> (meta dict, {member: array}): S the ascending distinct k-mers of both
    strands of every record of at least K bases; T, U, V the CSR lists of (record, signed position) per k-mer in the order
    met (file, record, position, forward before reverse)"""
    xs, ns, ps, lens, nms, seqs = [], [], [], [], [], []
    for nm, seq in records:
        if len(seq) < K:
            if warn is not None:
                warn.write("warning: `%s' skipped\n" % (nm,))          # scan.py:206
            continue
        x, p = windows_with_pos(K, seq)
        xs.append(x)
        ps.append(p)
        ns.append(np.full(len(x), len(nms), np.uint32))
        nms.append(nm)
        seqs.append(seq.decode("latin-1"))
        lens.append(len(seq))
    x = np.concatenate(xs) if xs else np.zeros(0, np.uint64)
    N = len(x)
    if N == 0:
        raise ScanError("no k-mers: no record of at least %d bases without other letters (the reference divides by zero here)" % K)
    if N >= 1 << 32:
        raise ScanError("%d k-mer positions: the index's offsets are 32 bits wide" % N)
    counts = np.bincount((x & np.uint64(3)).astype(np.int64), minlength=4)
    qacgt = [float(int(c)) / float(N) for c in counts]          # scan.py:195
    S, rank = np.unique(x, return_inverse=True)
    order = np.argsort(rank, kind="stable")
    T = np.zeros(len(S) + 1, np.uint32)
    T[1:] = np.cumsum(np.bincount(rank, minlength=len(S)))
    meta = {"K": K, "lens": lens, "qacgt": qacgt, "nms": nms, "seqs": seqs}
    arrays = {"S": S.astype("<u8"), "T": T.astype("<u4"), "U": np.concatenate(ns)[order].astype("<u4"),
              "V": np.concatenate(ps)[order].astype("<i4")}
    return meta, arrays


def index_write(path, meta, arrays):
    """the casket of scan.py:229-241: __meta__ first, then S, T, U, V as the bytes of native arrays"""
    from zotmer_amd.library.container import Container
    with Container(path, "w") as z:
        z.add("__meta__", json.dumps(meta).encode())
        for nm, dt in MEMBERS:
            z.add(nm, np.ascontiguousarray(arrays[nm], dtype=dt).tobytes())


def index_load(path):
    """-> (meta, arrays), checked: everything zk_scan_place relies on is refused here with a message"""
    from zotmer_amd.library.container import Container
    with Container(path, "r") as z:
        try:
            meta = json.loads(z.read("__meta__").decode())
            arrays = {nm: np.frombuffer(z.read(nm), dtype=dt) for nm, dt in MEMBERS}
        except KeyError as e:
            raise ScanError("%s: no member %s: not an index of `zot scan -X`" % (path, e))
    for f in ("K", "lens", "qacgt", "nms", "seqs"):
        if f not in meta:
            raise ScanError("%s: the index's meta data has no %r" % (path, f))
    K = meta["K"]
    if K != K_INDEX:
        raise ScanError("%s: the index has K=%r; only K=%d is supported (the reference's consensus hard-codes it)" % (path, K, K_INDEX))
    S, T, U, V = (arrays[nm] for nm, _ in MEMBERS)
    lens = np.asarray(meta["lens"], dtype=np.int64)
    ok = (len(meta["nms"]) == len(lens) and len(meta["qacgt"]) == 4 and len(T) == len(S) + 1 and len(U) == len(V)
          and (len(S) < 2 or bool(np.all(S[1:] > S[:-1]))) and (len(S) == 0 or int(S[-1]) >> (2 * K) == 0)
          and int(T[0]) == 0 and int(T[-1]) == len(U) and bool(np.all(T[1:] >= T[:-1])) and bool(np.all(lens >= K)))
    if ok and len(U):
        slots = lens - K + 1
        ok = bool(np.all(U < len(lens))) and bool(np.all(V != 0)) and bool(np.all(np.abs(V.astype(np.int64)) <= slots[np.minimum(U, len(lens) - 1)]))
    if not ok:
        raise ScanError("%s: the index is damaged (k-mers out of order, offsets that do not ascend to the number of entries, or an "
                        "entry outside its record)" % path)
    return meta, arrays


class DeviceIndex:
    """the index's arrays on the device, once for all samples"""

    def __init__(self, ctx, meta, arrays):
        self.ctx, self.meta, self.K = ctx, meta, meta["K"]
        self.lens = [int(v) for v in meta["lens"]]
        off = np.zeros(len(self.lens) + 1, np.uint64)
        off[1:] = np.cumsum(np.asarray(self.lens, dtype=np.int64) - self.K + 1)
        self.rec_off, self.n_slots = off, int(off[-1])
        self.S, self.T, self.U, self.V = (ctx.upload(np.ascontiguousarray(arrays[nm])) for nm, _ in MEMBERS)
        self.d_off = ctx.upload(off)

    def place(self, X):
        """sample k-mers on the device -> (P, Q, cnt) on the host: scan.py:266-304"""
        from zotmer_amd.library.timing import Phase
        ctx = self.ctx
        with Phase(ctx, "scan resolve", 8 * (self.S.n + X.n)):
            L, Y = ctx.lcp_resolve(self.S, X, self.K)
        with Phase(ctx, "scan place", 8 * self.U.n + 9 * self.n_slots):
            P, Q, cnt = ctx.scan_place(L, Y, self.T, self.U, self.V, self.d_off, self.n_slots, self.K)
        return P.to_host(), Q.to_host(), cnt.to_host().reshape(len(self.lens), self.K + 1)


# ---- the per-record stage (scan.py:122-175, 306-449) -------------------------------------------------------------------------

class UnionFind:
    """misc.unionfind (misc.py:24-79): the labels it returns depend on the order of the calls, and the stage sorts by them"""

    def __init__(self):
        self.parent, self.rank = {}, {}

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
        xr, yr = self.find(x), self.find(y)
        if xr == yr:
            return
        if self.rank[xr] < self.rank[yr]:
            self.parent[xr] = yr
        elif self.rank[xr] > self.rank[yr]:
            self.parent[yr] = xr
        else:
            self.parent[yr] = xr
            self.rank[xr] += 1


def null(g, s, j):
    """scan.py:129-132"""
    if j == 0:
        return 0.0
    return math.exp(s * math.log1p(-math.pow(g, j)))


def log1mexp(a):
    """stats.py:27-34"""
    if -a < 0.6931472:
        return math.log(-math.expm1(a))
    return math.log1p(-math.exp(a))


def log_gamma_p_int(n, x):
    """scan.py:137-163"""
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
    lx = math.log(x)
    s = 0
    v = 0
    for k in range(1, n):
        v += math.log(k)
        t = k * lx - v
        s = log_add(t, s)
    w = min(s - x, -1e-200)
    return log1mexp(w)


def chi2(n, x):
    """scan.py:165-168"""
    return log_gamma_p_int(int(math.ceil(n / 2.0)), x / 2.0)


def succ(K, X, x):
    """scan.py:122-127 over sparse.rank2 (sparse.py:55-91): the ranks in X of the k-mers that follow x"""
    y0 = (x << 2) & ((1 << (2 * K)) - 1)
    return range(int(np.searchsorted(X, np.uint64(y0), side="left")), int(np.searchsorted(X, np.uint64(min(y0 + 4, (1 << 64) - 1)), side="left")))


def ks_right(cnt, nm):
    """the second of stats.ksDistance2(counts2cdf(cnt), nm) (stats.py:228-250, 273-283)"""
    n = max(1, sum(cnt))
    t = 0
    dr = 0
    for c, y in zip(cnt, nm):
        dr = max(dr, y - t)
        t += float(c) / n
    return dr


def call_record(K, i, length, name, P, Q, cnt, nm, X):
    """one record (scan.py:306-449): P, Q its slots as Python ints, cnt its K + 1 counts, nm the null distribution, X the
    sample's k-mers (ascending, numpy) -> the line the reference prints, or None"""
    W = length - K + 1
    qc = math.log(K * 0.05 / float(W) / 2)

    # positions whose consecutive k-mers overlap by K - 1 bases
    m = (1 << (2 * K - 2)) - 1
    py = 0
    u = UnionFind()
    for j in range(W):
        x = P[j]
        if j > 0 and py == x >> 2:          # ham(py, y) == 0
            u.union(j - 1, j)
        py = x & m
    udx = {}
    for j in range(W):
        udx.setdefault(u.find(j), []).append(j)

    # the fragments that chance does not explain, longest first, by their left k-mer
    idx_lhs = {}
    kx = []
    for jx, js in udx.items():
        q = 0
        for j in js:
            q += math.log1p(-nm[Q[j]])
        if q > math.log(0.05 / len(js)):
            continue
        kx.append((-len(js), jx))
        idx_lhs[P[js[0]]] = jx
    kx.sort()

    # the attempt to link fragments through the sample; from the first step on x is a rank, as in the reference
    links = {}
    for _, jx in kx:
        x = P[udx[jx][-1]]
        xs = []
        lnk = None
        for _k in range(100):
            ys = succ(K, X, x)
            if len(ys) != 1:
                break
            x = ys[0]
            if x in idx_lhs:
                lnk = idx_lhs[x]
                break
            xs.append(x)
        if lnk is not None:
            links[jx] = xs
            u.union(jx, lnk)

    vdx = {}
    for _, jx in kx:
        vdx.setdefault(u.find(jx), []).append(jx)

    res = []
    for jxs in vdx.values():
        fs = sorted((udx[jx][0], jx) for jx in jxs)
        sxs = []
        for fj, (_, jx) in enumerate(fs):
            beg, end = udx[jx][0], udx[jx][-1] + 1
            if fj == 0:
                sxs.extend([(0, 0)] * beg)
            xs = links.get(jx, None)
            for j in range(beg, end):
                sxs.append((P[j], Q[j]))
            if xs:
                for x in xs:
                    sxs.append((x, 27))
            else:
                nxt = fs[fj + 1][0] if fj < len(fs) - 1 else W
                sxs.extend([(0, 0)] * (nxt - end))
        # Per base and letter, the sum of log1p(-nm[l]) over the k-mers that put that letter there.  The reference adds k-mer by
        # k-mer (j ascending, then k); a cell gets at most one term from each k, and for one cell k ascends with j, so adding
        # the K columns one after the other gives every cell its terms in the reference's order: the same doubles.
        n = len(sxs)
        xs_all = np.array([x for x, _ in sxs], dtype=np.uint64)
        ps = np.array([math.log1p(-nm[l]) for _, l in sxs], dtype=np.float64)
        seq = np.zeros((n + K - 1, 4), dtype=np.float64)
        at = np.arange(n)
        for k in range(K):
            seq[at + (K - 1 - k), ((xs_all >> np.uint64(2 * k)) & np.uint64(3)).astype(np.intp)] += ps
        letters = ((seq < qc) * np.array([1, 2, 4, 8])).sum(axis=1)
        ax = [FASTA[b] for b in letters.tolist()]
        p = None
        inf = False
        for ssj in (((seq[:, 0] + seq[:, 1]) + seq[:, 2]) + seq[:, 3]).tolist():          # sum(seq[j]): 0 + a + c + g + t
            p = ssj if p is None else log_add(p, ssj)
            if ssj > -1e-300:
                inf = True
        kd = ks_right(cnt, nm)
        df = math.ceil((n + K - 1) / float(K))
        if inf:
            q, pv = 1e300, 0.0
        else:
            q = 2 * math.exp(p)
            pv = chi2(df, q)
        res.append((pv, q, kd, "".join(ax)))

    if not res:
        return None
    res.sort()
    if not res[0][0] < -2:
        return None
    pv, c2, kd, a = res[0]
    return "%d\t%d\t%d\t%g\t%g\t%g\t%s\t%s" % (i, length, len(a), kd, c2, pv / math.log(10), name, a)


def sample_lines(meta, sacgt, P, Q, cnt, rec_off, X, sample_name, err=None):
    """everything after the placement for one sample (scan.py:276-278, 306-449) -> the lines"""
    K, lens, nms = meta["K"], meta["lens"], meta["nms"]
    M = len(X)
    g = sum([qp * sp for qp, sp in zip(meta["qacgt"], sacgt)])
    if err is not None:
        err.write("g = %.12g\n" % g)          # scan.py:277: Python 2's str(float)
    nm = [null(g, M, j) for j in range(0, K + 1)]
    P, Q = P.tolist(), Q.tolist()
    lines = []
    for i in range(len(nms)):
        a, b = int(rec_off[i]), int(rec_off[i + 1])
        try:
            ln = call_record(K, i, lens[i], nms[i], P[a:b], Q[a:b], cnt[i].tolist(), nm, X)
        except ValueError:
            # log1p(-1.0): the chance of some match length rounds to 1 (the reference dies here too); a handful of k-mers only
            raise ScanError("%s: with %d k-mers the chance of a match rounds to 1 and its complement has no logarithm (record %s); "
                            "the sample is too small to scan" % (sample_name, M, nms[i]))
        if ln is not None:
            lines.append(ln)
    return lines


# ---- the two modes -------------------------------------------------------------------------------------------------------------

def build(genes, inputs, err=None):
    """zot scan -X <genes> <input>...  (scan.py:180-243)"""
    from zotmer_amd.library import seqio
    err = err or sys.stderr
    meta, arrays = index_build(((nm, seq) for fn in inputs for nm, seq in seqio.fasta_records(fn)), warn=err)
    index_write(genes, meta, arrays)


def check_samples(K, inputs):
    """the refusals that need no device: a set of another K, a set without k-mers"""
    from zotmer_amd.library.container import KmerSet
    for fn in inputs:
        with KmerSet(fn, "r") as z:
            if z.meta["K"] != K:
                raise ScanError("%s has K=%r, the index K=%d" % (fn, z.meta["K"], K))
            if z.member_size("kmers") == 0:
                raise ScanError("%s holds no k-mers (the reference dies here with NameError)" % fn)


def run(ctx, meta, arrays, inputs, out=None, err=None):
    """zot scan <genes> <input>... after index_load (scan.py:263-449): the index stays on the device; every sample is read,
    resolved, placed and called"""
    from zotmer_amd.library import vectors
    from zotmer_amd.library.container import KmerSet
    from zotmer_amd.library.timing import Phase
    out = out or sys.stdout
    err = err or sys.stderr
    index = DeviceIndex(ctx, meta, arrays)
    err.write("done.\n")
    for fn in inputs:
        with KmerSet(fn, "r") as z:
            sacgt = z.meta["acgt"]
            X = vectors.device_read_kmers(ctx, z)
        P, Q, cnt = index.place(X)
        with Phase(ctx, "scan records", 9 * index.n_slots):
            lines = sample_lines(meta, sacgt, P, Q, cnt, index.rec_off, X.to_host(), fn, err)
        for ln in lines:
            out.write(ln + "\n")
        out.flush()
