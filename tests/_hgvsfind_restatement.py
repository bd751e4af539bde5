"""A plain-Python restatement of `zot hgvs-find` in scanning mode (zotmer/commands/hgvs-find.py:917-1131 with
library/{capture,debruijn,stats,basics,file,reads}.py), written from the reference's semantics for the tests: the fixtures of
tests/golden/h1_hgvsfind.json must come out of it, and the device path must agree with it.  Dicts and sets all the way, a pass
over a bait's whole k-mer dict per path position: small inputs only.

Where the reference walks a dict or a set the order is fixed here: candidates ascend, and paths are extended in ascending
k-mer order.  The outcome depends on it only where several bridged paths of one kind tie."""
import math
import re

from tests._capture_restatement import fastq_records, kmers

M1 = 0x5555555555555555


def rc(K, x):
    y = 0
    for _ in range(K):
        y = (y << 2) | (3 - (x & 3))
        x >>= 2
    return y


def ham(x, y):
    """basics.ham: a base that differs in one bit or in both is one mismatch"""
    z = x ^ y
    return bin((z | (z >> 1)) & M1).count("1")


def render(K, x):
    return "".join("ACGT"[(x >> (2 * (K - 1 - i))) & 3] for i in range(K))


def render_path(K, xs):
    return render(K, xs[0]) + "".join("ACGT"[x & 3] for x in xs[1:]) if xs else ""


# ---- the variants --------------------------------------------------------------------------------------------------------
_POS = r"([^:]+):g\.([0-9]+)(?:_([0-9]+))?"
_KINDS = [("sub", r"([ACGT])>([ACGT])"), ("del", r"del([ACGT]+)?"), ("dup", r"dup([ACGT]+)?"), ("ins", r"ins([ACGT]+)"),
          ("insN", r"ins([0-9]+)"), ("insALU", r"insALU"), ("inv", r"inv([ACGT]+)?"), ("delins", r"delins([ACGT]+)"),
          ("delinsN", r"delins([0-9]+)"), ("repeat", r"(?:[ACGT]+)?\[([0-9]+)\]")]


def variant(h):
    """-> (kind, size as hgvs.py's size() gives it, anonymous), or None when hgvs.makeHGVS would not take the string"""
    for kind, tail in _KINDS:
        m = re.match(_POS + tail + "$", h)
        if not m:
            continue
        p0, p1 = int(m.group(2)), m.group(3)
        if kind == "sub":
            return None if p1 else (kind, 1, False)
        if kind in ("ins", "insN", "insALU", "inv") and p1 is None:
            return None
        span = (int(p1) if p1 else p0) - p0 + 1
        size = {"del": 0, "dup": 2 * span, "inv": span, "insALU": None}.get(kind, 0)
        if kind in ("ins", "delins"):
            size = len(m.group(4))
        elif kind in ("insN", "delinsN"):
            size = int(m.group(4))
        elif kind == "repeat":
            size = int(m.group(4)) * span
        return kind, size, kind in ("insN", "delinsN")
    return None


# ---- step 2: the capture ---------------------------------------------------------------------------------------------------
def baits(K, index):
    """{k-mer of either strand of a bait: [bait numbers]} (hgvs-find.py:941-956, capture.py:18-30)"""
    idx = {}
    for n, itm in enumerate(index):
        b = itm["lhsFlank"] + itm["wtSeq"] + itm["rhsFlank"]
        if itm["mutSeq"] is not None:
            b += "N" + itm["lhsFlank"] + itm["mutSeq"] + itm["rhsFlank"]
        for x in kmers(K, b, True):
            idx.setdefault(x, set()).add(n)
    return idx


def capture(K, index, inputs):
    """capture.addReadPairAndKmers over the file pairs (inputs[0], inputs[1]), ... -> (capKmers: one {k-mer: count} per bait,
    capReadCounts)"""
    idx = baits(K, index)
    cap, nreads = [dict() for _ in index], [0] * len(index)
    for i in range(0, len(inputs) - 1, 2):
        r1, r2 = fastq_records(inputs[i]), fastq_records(inputs[i + 1])
        for a, b in zip(r1, r2):
            xs = kmers(K, a[1], True) + kmers(K, b[1], True)
            ns = set()
            for x in xs:
                ns |= idx.get(x, set())
            for n in ns:
                nreads[n] += 1
                for x in xs:
                    cap[n][x] = cap[n].get(x, 0) + 1
    return cap, nreads


# ---- step 4: definite alleles ----------------------------------------------------------------------------------------------
def get_mask(K, i, L):
    """fixed_path_finder.get_mask (debruijn.py:349-362), exactly as written there"""
    M = (1 << (2 * K)) - 1
    lhs = (1 << (2 * (i + 1))) - 1 if i < K else M
    j = i - (L - K + 1)
    rhs = M if j < 0 else ((1 << (2 * (j + 1))) - 1) ^ M
    return lhs & rhs


def intersect(K, xs, ys):
    """debruijn_intersection: the xs with a successor in ys, the ys with a predecessor in xs"""
    m = (1 << (2 * (K - 1))) - 1
    tails, heads = {x & m for x in xs}, {y >> 2 for y in ys}
    both = tails & heads
    return [x for x in xs if (x & m) in both], [y for y in ys if (y >> 2) in both]


def fixed_path(K, D, mx, xs):
    L = len(xs)
    Y = []
    for i, x in enumerate(xs):
        m = get_mask(K, i, L)
        ys = sorted(y for y in mx if (y & m) == (x & m) and ham(x, y) < D)
        if not ys:
            return None
        Y.append(ys)
    done = False
    while not done:
        done = True
        for j in range(1, L):
            vs, ws = intersect(K, Y[j - 1], Y[j])
            if not vs or not ws:
                return None
            if len(vs) != len(Y[j - 1]):
                Y[j - 1], done = vs, False
            if len(ws) != len(Y[j]):
                Y[j], done = ws, False
    return Y


def consensus(K, ys, mx):
    """the base-wise majority weighted by counts (the lowest base wins a tie), and the smallest winning weight"""
    r, c = 0, None
    for i in range(K):
        w = [0, 0, 0, 0]
        for y in ys:
            w[(y >> (2 * i)) & 3] += mx[y]
        b = max(range(4), key=lambda q: (w[q], -q))
        r |= b << (2 * i)
        c = w[b] if c is None else min(c, w[b])
    return r, c


def definite(K, D, lhs, mid, rhs, mx):
    """findFairlySimpleAllele -> an allele dict, or None"""
    allele = lhs[-(K - 1):] + mid + rhs[:K - 1]
    xs = kmers(K, allele, False)
    Y = fixed_path(K, D, mx, xs)
    if Y is None:
        return None
    path, cov = zip(*[consensus(K, ys, mx) for ys in Y]) if Y else ((), ())
    return {"path": list(path), "covMin": min(cov), "lhsPos": 0, "rhsPos": 0, "allele": render_path(K, list(path))}


# ---- step 5: bridged alleles -----------------------------------------------------------------------------------------------
def follows(K, x, y):
    return (x & ((1 << (2 * (K - 1))) - 1)) == (y >> 2)


def anchors(K, seq, mx, is_lhs, D):
    """findAnchors (hgvs-find.py:517-583) -> sorted [(k-mer, distance from the variant)]"""
    xps = [(x, p) for p, x in enumerate(window_positions(K, seq))]
    xps = [(x, p) for x, p in xps if x is not None]
    xc = max([mx.get(x, 0) for x, _ in xps] + [0])
    if xc == 0:
        return []
    t = int(math.exp(math.log(xc) - 1.5))
    strong = sorted(y for y, c in mx.items() if c >= t)
    zs = {}
    for x, p in xps:
        zs[p] = set(y for y in strong if ham(x, y) <= D) if mx.get(x, 0) >= t and x in mx else set()
    res = set()
    order = xps if is_lhs else xps[::-1]
    step = -1 if is_lhs else 1
    for x, p in order:
        for s in sorted(zs.get(p, ())):
            res.add((s, p))
            for u in zs.get(p + step, ()):
                if (follows(K, u, s) if is_lhs else follows(K, s, u)):
                    res.discard((u, p + step))
    if is_lhs:
        last = len(seq) - K
        return sorted((x, last - p) for x, p in res)
    return sorted(res)


def window_positions(K, seq):
    """the k-mer at every start of seq, None where the window holds a byte outside AaCcGgTtUu (kmersWithPosList, 0-based)"""
    out = []
    for i in range(len(seq) - K + 1):
        xs = kmers(K, seq[i:i + K], False)
        out.append(xs[0] if xs else None)
    return out


def paths(K, mx, xb, xe, n):
    """Interpolator.path for an exact length n (debruijn.py:98-128): every path of n k-mers of mx from xb to xe, grown from both
    ends in turn; candidates are extended in ascending k-mer order"""
    M, S = (1 << (2 * K)) - 1, 2 * (K - 1)
    fwd, rev = {xb: [[xb]]}, {xe: [[xe]]}
    i = 1
    while i <= n:
        if i == n:
            for x in sorted(set(fwd) & set(rev)):
                for a in fwd[x]:
                    for b in rev[x]:
                        yield a + b[1:]
        if i & 1 == 0:
            nxt = {}
            for x in sorted(fwd):
                for y in (((x << 2) & M) + q for q in range(4)):
                    if y in mx:
                        nxt.setdefault(y, []).extend(p + [y] for p in fwd[x])
            fwd = nxt
        else:
            nxt = {}
            for x in sorted(rev):
                for y in ((x >> 2) + (q << S) for q in range(4)):
                    if y in mx:
                        nxt.setdefault(y, []).extend([y] + p for p in rev[x])
            rev = nxt
        i += 1


def bridge(K, mx, lx, lxp, rx, rxp, z):
    """findAllele"""
    for pth in paths(K, mx, lx, rx, z + lxp + rxp + 1 + K):
        seq = render_path(K, pth)[lxp + K:-(rxp + K)]
        yield {"allele": seq, "covMin": min(mx[x] for x in pth[lxp + 1:-(rxp + 1)]), "path": pth[1:-1], "lhsPos": lxp, "rhsPos": rxp}


def bridging(K, D, mx, lhs, rhs, wt, mut, wtZ, mutZ):
    """AlleleFinder.bridgingAlleles -> [(kind, allele dict)] in the order the reference's loops give"""
    out = []
    max_bridge = 4 * K
    for lx, lxp in anchors(K, lhs, mx, True, D):
        for rx, rxp in anchors(K, rhs, mx, False, D):
            if wtZ == mutZ:
                if wtZ > max_bridge:
                    continue
                for a in bridge(K, mx, lx, lxp, rx, rxp, wtZ):
                    if a["allele"] == wt:
                        out.append(("wt", a))
                    elif mut is None or a["allele"] == mut:
                        out.append(("mut", a))
            else:
                if wtZ > max_bridge:
                    continue
                for a in bridge(K, mx, lx, lxp, rx, rxp, wtZ):
                    if a["allele"] == wt:
                        out.append(("wt", a))
                if mutZ > max_bridge:
                    continue
                for a in bridge(K, mx, lx, lxp, rx, rxp, mutZ):
                    if mut is None or a["allele"] == mut:
                        out.append(("mut", a))
    return out


# ---- step 6: scores and the table -------------------------------------------------------------------------------------------
def log_fac(n):
    """stats.logFac: the logarithm of the exact factorial below 25, Ramanujan's formula from there"""
    if n < 25:
        return math.log(math.factorial(n))
    return n * math.log(n) - n + math.log(n * (1 + 4 * n * (1 + 2 * n))) / 6.0 + math.log(math.pi) / 2.0


def log_choose(n, k):
    return 0 if k == 0 or k == n else log_fac(n) - (log_fac(n - k) + log_fac(k))


def log_add(a, b):
    x, y = max(a, b), min(a, b)
    return x + math.log1p(math.exp(y - x))


def log_bin_eq(p, n, k):
    return log_choose(n, k) + math.log(p) * k + math.log1p(-p) * (n - k)


def log_bin_le(p, n, k):
    v = log_bin_eq(p, n, k)
    for j in range(1, k + 1):
        v = log_add(v, log_bin_eq(p, n, k - j))
    return v


def pdf2cdf(xs):
    t, ys = 0, []
    for x in xs:
        ys.append(t)
        t += x
    return ys


class Scorer:
    def __init__(self, K):
        self.K = K
        self.null_cdf = pdf2cdf([math.exp(log_bin_eq(0.25, K, j)) for j in range(K + 1)])
        self.bin_model = [1 - math.exp(log_bin_le(0.25, K, d)) for d in range(K + 1)]

    def score(self, res, lhs, seq, rhs):
        K = self.K
        xs = res["path"]
        r = [0] * (K + 1)
        lp, rp = K - 1 + res["lhsPos"], K - 1 + res["rhsPos"]
        if seq is None:
            allele = lhs[-lp:] + len(res["allele"]) * "N" + rhs[:rp]
            r[0] += len(xs)
        else:
            allele = lhs[-lp:] + seq + rhs[:rp]
            for x, y in zip(xs, kmers(K, allele, False)):
                r[ham(x, y)] += 1
        n = max(1, sum(r))
        cdf = pdf2cdf([float(x) / n for x in r])
        res["ksDist"] = max([0] + [x - y for x, y in zip(cdf, self.null_cdf)])
        got = render_path(K, xs)
        res["hamming"] = sum(1 for i in range(len(allele)) if allele[i] != got[i] and allele[i] != "N" and got[i] != "N")
        p = 1.0
        for d in range(K + 1):
            p *= math.pow(self.bin_model[d], r[d])
        res["binom"] = 1.0 - p


def better(a, b):
    if a["covMin"] != b["covMin"]:
        return a["covMin"] > b["covMin"]
    return a["hamming"] <= b["hamming"]


def best(scorer, alleles, lhs, seq, rhs):
    res = {"covMin": 0, "binom": 1.0, "ksDist": 0.0, "hamming": 0, "path": []}
    for a in alleles:
        scorer.score(a, lhs, seq, rhs)
        if better(a, res):
            res = a
    return res


def median(mx, path):
    xs = sorted(mx.get(x, 0) for x in path) or [0]
    return xs[len(xs) // 2]


def find(index, inputs, K=25, D=2, Q=10, V=0.05, F="rds,vaf"):
    """the text hgvs-find prints for an index (the list of dicts) and FASTQ texts"""
    fmt = set(F.split(","))
    cap, nreads = capture(K, index, inputs)
    scorer = Scorer(K)
    lines, header = [], False
    for n, itm in enumerate(index):
        kind, size, anon = variant(itm["hgvs"])
        mx = cap[n]
        if "kmers" in fmt:
            lines += ["%d\t%s\t%d" % (n, render(K, x), c) for x, c in sorted(mx.items())]
        lhs, rhs, wt, mut = itm["lhsFlank"], itm["rhsFlank"], itm["wtSeq"], itm["mutSeq"]
        cs = sorted(c for c in mx.values() if c >= Q)
        nk = len(cs)
        cs = cs or [0]
        q10, q50, q90 = cs[len(cs) // 10], cs[5 * len(cs) // 10], cs[9 * len(cs) // 10]
        alleles = {"wt": [], "mut": []}
        if not anon:
            for t, seq in (("wt", wt), ("mut", mut)):
                a = definite(K, D, lhs, seq, rhs, mx) if seq is not None else None
                if a is not None:
                    alleles[t].append(a)
        else:
            for t, a in bridging(K, D, mx, lhs, rhs, wt, mut, len(wt), size):
                alleles[t].append(a)
        w = best(scorer, alleles["wt"], lhs, wt, rhs)
        m = best(scorer, alleles["mut"], lhs, mut, rhs)
        wmed, mmed = median(mx, w["path"]), median(mx, m["path"])
        tot = max(1.0, float(wmed + mmed), float(q90))
        wvaf, mvaf = wmed / tot, mmed / tot
        call = 1 * (w["covMin"] > Q and w["hamming"] < 4 and wvaf > V) + 2 * (m["covMin"] > Q and m["hamming"] < 4 and mvaf > V)
        cols = [("n", "%d", n), ("res", "%s", ["null", "wt", "mut", "wt/mut"][call])]
        if "rds" in fmt:
            cols.append(("numReads", "%d", nreads[n]))
        cols += [("numKmers", "%d", nk), ("covQ10", "%d", q10), ("covQ50", "%d", q50), ("covQ90", "%d", q90),
                 ("wtMin", "%d", w["covMin"]), ("mutMin", "%d", m["covMin"]), ("wtHam", "%d", w["hamming"]), ("mutHam", "%d", m["hamming"])]
        if "ks" in fmt:
            cols += [("wtD", "%g", w["ksDist"]), ("mutD", "%g", m["ksDist"])]
        if "binom" in fmt:
            cols += [("wtQ", "%g", w["binom"]), ("mutQ", "%g", m["binom"])]
        if "vaf" in fmt:
            cols += [("wtVaf", "%g", wvaf), ("mutVaf", "%g", mvaf)]
        cols.append(("hgvs", "%s", itm["hgvs"]))
        if not header:
            lines.append("\t".join(c[0] for c in cols))
            header = True
        lines.append("\t".join(c[1] % c[2] for c in cols))
    return "".join(l + "\n" for l in lines)


def options(words):
    """the command's option words -> the keyword arguments of find()"""
    names = {"-k": ("K", int), "-D": ("D", int), "-C": ("Q", int), "-V": ("V", float), "-F": ("F", str)}
    return {names[words[i]][0]: names[words[i]][1](words[i + 1]) for i in range(0, len(words), 2)}
