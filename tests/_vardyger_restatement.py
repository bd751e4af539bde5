"""A literal Python 3 restatement of the caller of zotmer/commands/vardyger.py -- the index (lines 289-334), the read loop
(338-354), the threshold (359-362), the coverage line (371-376), findDup, pairs, nearest, offset and positions (66-133), the
filters and the row (420-506) -- with basics.kmersList / kmersWithPosList / ham / render, file.readFasta / readFastq and
debruijn.Interpolator as they are written.  The reference's main `continue`s at line 401, in front of lines 403-506; this is
what runs with the trace loop of lines 395-401 taken out.  Dicts and sets are walked in Python 3's order, which is not the
reference's (Python 2): the order of the rows and warnings is not the reference's own either, so callers compare them sorted.
Written from the reference's text and from nothing of the product, which it checks."""
import io

M1 = 0x5555555555555555
_NUC = {"A": 0, "a": 0, "C": 1, "c": 1, "G": 2, "g": 2, "T": 3, "t": 3, "U": 3, "u": 3}


def ham(x, y):
    """basics.ham (basics.py:123-133)"""
    z = x ^ y
    return bin((z | (z >> 1)) & M1).count("1")


def render(k, x):
    """basics.render (basics.py:61-67)"""
    r = []
    for _ in range(k):
        r.append("ACGT"[x & 3])
        x >>= 2
    return "".join(r[::-1])


def _walk(k, seq, both):
    """the loop of basics.kmersList / kmersWithPosList (basics.py:320-347, 414-439): (x, rc x, i + 1) per window"""
    z = len(seq)
    msk = (1 << (2 * k)) - 1
    s = 2 * (k - 1)
    i = j = x = xb = 0
    while i + k <= z:
        while i + j < z and j < k:
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
        if j == k:
            x &= msk
            yield x, xb, i + 1
            j -= 1
        i += 1


def kmers_list(k, seq, both=False):
    res = []
    for x, xb, _ in _walk(k, seq, both):
        res.append(x)
        if both:
            res.append(xb)
    return res


def kmers_with_pos_list(k, seq):
    return [(x, p) for x, _, p in _walk(k, seq, False)]


def read_fasta(text):
    """file.readFasta (file.py:19-36)"""
    nm, seq = None, []
    for l in io.StringIO(text, newline="\n"):
        l = l.strip()
        if len(l) and l[0] == ">":
            if nm is not None:
                yield nm, "".join(seq)
            nm, seq = l[1:].strip(), []
        else:
            seq.append(l)
    if nm is not None:
        yield nm, "".join(seq)


def read_fastq(text):
    """file.readFastq (file.py:38-52; a trailing incomplete group is dropped: `grp == 4` is never true) -> the sequence lines"""
    grp = []
    for l in io.StringIO(text, newline="\n"):
        grp.append(l.strip())
        if len(grp) == 4:
            yield grp[1]
            grp = []


# ---- vardyger.py:66-133 ------------------------------------------------------------------------------------------------------------
def pairs(xs, ys):
    for i in range(len(xs)):
        for j in range(len(ys)):
            if xs[i] != ys[j]:
                yield (xs[i], ys[j])


def find_dup(refFst, refLst, xFst, xLst):
    cs = set(xFst.keys()) & set(refFst.keys())
    Ws = set(refLst.keys())
    for c in cs:
        ys = xFst[c]
        Ys = set(ys)
        ds = sorted(Ys & set(refFst[c]))
        bs = sorted(Ys & Ws)
        for (b, d) in pairs(bs, ds):
            for a in refLst[b]:
                if a == c:
                    continue
                yield (a, b, c, d)


def nearest(m, xs, y):
    dMin = m
    posMin = []
    for (x, p) in xs.items():
        d = ham(x, y)
        if d > dMin:
            continue
        if d < dMin:
            dMin = d
            posMin = []
        posMin += p
    return posMin


def offset(xs, ys, d):
    for x in xs:
        for y in ys:
            if x + d == y:
                yield (x, y)


def positions(posIdx, J, a, b, c, d):
    D = 1
    pas = nearest(D, posIdx, a)
    pbs = nearest(D, posIdx, b)
    pabs = list(offset(pas, pbs, J))
    pcs = nearest(D, posIdx, c)
    pds = nearest(D, posIdx, d)
    pcds = list(offset(pcs, pds, J))
    res = None
    for (pa, pb) in pabs:
        for (pc, pd) in pcds:
            if pc <= pb:
                continue
            if res is None:
                res = []
            res.append((pa, pb, pc, pd))
    return res


# ---- debruijn.py:77-128, 164-176 ---------------------------------------------------------------------------------------------------
class Interpolator(object):
    def __init__(self, K, xs):
        self.K = K
        self.M = (1 << (2 * K)) - 1
        self.S = 2 * (K - 1)
        self.xs = xs
        self.tied = False          # (not the reference's: two paths shared the largest sum, and the dict order chose)

    def succ(self, x):
        y0 = (x << 2) & self.M
        for i in range(4):
            y = y0 + i
            if y in self.xs:
                yield y

    def pred(self, x):
        y0 = x >> 2
        for i in range(4):
            y = y0 + (i << self.S)
            if y in self.xs:
                yield y

    def path(self, xb, xe, n):
        fwd = {xb: [[xb]]}
        rev = {xe: [[xe]]}
        i = 1
        while i <= n:
            if i == n:
                for x in set(fwd.keys()) & set(rev.keys()):
                    for fst in fwd[x]:
                        for snd in rev[x]:
                            yield fst + snd[1:]
            if (i & 1) == 0:
                nextFwd = {}
                for (x, ps) in fwd.items():
                    for y in self.succ(x):
                        if y not in nextFwd:
                            nextFwd[y] = []
                        for p in ps:
                            nextFwd[y].append(p + [y])
                fwd = nextFwd
            else:
                nextRev = {}
                for (x, ps) in rev.items():
                    for y in self.pred(x):
                        if y not in nextRev:
                            nextRev[y] = []
                        for p in ps:
                            nextRev[y].append([y] + p)
                rev = nextRev
            i += 1

    def interpolate(self, xb, xe, n):
        sMax = 0
        pMax = None
        for p in self.path(xb, xe, n):
            s = 0
            for x in p:
                s += self.xs[x]
            if s > sMax:
                sMax = s
                pMax = p
                self.tied = False
            elif s == sMax and p != pMax:
                self.tied = True
        return pMax


def interpolate(K, xs, xb, xe, n, ties=None):
    I = Interpolator(K, xs)
    p = I.interpolate(xb, xe, n)
    if ties is not None and I.tied:
        ties.append((xb, xe, n))
    return p


# ---- main --------------------------------------------------------------------------------------------------------------------------
class Index(object):
    """vardyger.py:282-334"""

    def __init__(self, K, records):
        self.K = K
        J = self.J = K // 2
        S = self.S = 2 * (K - J)
        Mj = self.Mj = (1 << (2 * J)) - 1
        self.names, self.seqs, self.bait, self.wtFst, self.wtLst, self.posIdx, self.warnings = [], {}, {}, [], [], [], []
        for (nm, seq) in records:
            n = len(self.names)
            self.names.append(nm)
            self.seqs[nm] = seq
            wf = {}
            wl = {}
            for x in kmers_list(K, seq, False):
                if x not in self.bait:
                    self.bait[x] = set([])
                self.bait[x].add(n)
                y0 = x >> S
                y1 = x & Mj
                if y0 not in wf:
                    wf[y0] = set([])
                wf[y0].add(y1)
                if y1 not in wl:
                    wl[y1] = set([])
                wl[y1].add(y0)
            self.wtFst.append(wf)
            self.wtLst.append(wl)
            px = {}
            for (x, p) in kmers_with_pos_list(J, seq):
                if x not in px:
                    px[x] = []
                px[x].append(p)
            self.posIdx.append(px)
            for (a, b, c, d) in find_dup(wf, wl, wf, wl):
                pps = positions(px, J, a, b, c, d)
                if pps is None:
                    continue
                for pp in pps:
                    ab = a << S | b
                    cb = c << S | b
                    cd = c << S | d
                    dd = pp[2] - pp[0]
                    self.warnings.append("warning: phantom dumplication: %s-%s-%s (%d)" % (render(K, ab), render(K, cb), render(K, cd), dd))


def count_reads(index, reads):
    """vardyger.py:338-354 -> X"""
    X = [{} for _ in index.names]
    for rd in reads:
        xs = kmers_list(index.K, rd, True)
        hits = set([])
        for x in xs:
            if x in index.bait:
                hits |= index.bait[x]
        for n in hits:
            for x in xs:
                if x not in X[n]:
                    X[n][x] = 0
                X[n][x] += 1
    return X


def call(index, X, minCov=10, report_all=False, strict=False, ties=None):
    """vardyger.py:356-506 without lines 377-401 -> (the coverage lines, the rows as tuples of the printed fields without n)"""
    K, J, S, Mj = index.K, index.J, index.S, index.Mj
    cover, rows = [], []
    for n in range(len(index.names)):
        xs = {}
        for (x, c) in X[n].items():
            if c >= 10:
                xs[x] = c
        seq = index.seqs[index.names[n]]
        xx = []
        for x in kmers_list(K, seq, False):
            if x in xs:
                xx.append(".")
            else:
                xx.append("X")
        cover.append("".join(xx))
        fst = {}
        lst = {}
        for (x, c) in xs.items():
            y0 = x >> S
            y1 = x & Mj
            if y0 not in fst:
                fst[y0] = []
            fst[y0].append(y1)
            if y1 not in lst:
                lst[y1] = []
            lst[y1].append(y0)
        for (a, b, c, d) in find_dup(index.wtFst[n], index.wtLst[n], fst, lst):
            pps = positions(index.posIdx[n], J, a, b, c, d)
            if pps is None:
                continue
            for pp in pps:
                ab = a << S | b
                cb = c << S | b
                cd = c << S | d
                dd = pp[2] - pp[0]
                if not report_all and dd % 3 != 0:
                    continue
                if strict:
                    fstPath = interpolate(K, xs, ab, cb, dd + 1, ties)
                    sndPath = interpolate(K, xs, cb, cd, dd + 1, ties)
                    if fstPath is None:
                        continue
                    if sndPath is None:
                        continue
                    if fstPath[J:-J] != sndPath[J:-J]:
                        continue
                pa, pb, pc, pd = pp
                cab = xs.get(ab, 0)
                ccb = xs.get(cb, 0)
                ccd = xs.get(cd, 0)
                if cab < minCov:
                    continue
                if ccb < minCov:
                    continue
                if ccd < minCov:
                    continue
                m = (cab + ccd) / 2.0
                w = ccb / m
                hgvs = "%s:c.%d_%ddup" % (index.names[n], pb, pd - 1)
                rows.append((n, a, b, c, d, pa, pc, "%s\t%d\t%s\t%d\t%s\t%d\t%d\t%g\t%s" % (render(K, ab), cab, render(K, cb), ccb, render(K, cd),
                                                                                       ccd, dd, w, hgvs)))
    return cover, rows


HEADER = "n\tleft\tleftCov\tmid\tmidCov\tright\trightCov\tlen\tvaf\thgvs"


def ordered(rows):
    """the rows in the product's order: ascending (sequence, c, b, d, a, pa, pc) -> the lines without n"""
    return [r[7] for r in sorted(rows, key=lambda r: (r[0], r[3], r[2], r[4], r[1], r[5], r[6]))]


def candidates(index, n, xs):
    """findDup + positions for record n against the counted k-mers xs (a dict: the k-mers that stayed) -> the set of
    (a, b, c, d, pa, pc): what zk_dup_join computes"""
    K, J, S, Mj = index.K, index.J, index.S, index.Mj
    fst, lst = {}, {}
    for x in xs:
        fst.setdefault(x >> S, []).append(x & Mj)
        lst.setdefault(x & Mj, []).append(x >> S)
    out = []
    for (a, b, c, d) in find_dup(index.wtFst[n], index.wtLst[n], fst, lst):
        pps = positions(index.posIdx[n], J, a, b, c, d)
        if pps is None:
            continue
        for pp in pps:
            out.append((a, b, c, d, pp[0], pp[2]))
    return out
