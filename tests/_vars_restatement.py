"""`zot vars -r` in plain Python, restated from the reference (zotmer/commands/vars.py:33-46, 85-119 with library/stats.py:77-92,
121-128, 214-226 and basics.py:60-90) for the tests: no product code is imported here.  tests/golden/make_golden_vars.py asserts
that it reproduces the reference's output as text."""
import math

_SMALL = [math.log(math.factorial(n)) for n in range(25)]
_FAS = ['*', 'A', 'C', 'M', 'G', 'R', 'S', 'V', 'T', 'W', 'Y', 'H', 'K', 'D', 'B', 'N']


def log_fac(n):
    if n < len(_SMALL):
        return _SMALL[n]
    return n * math.log(n) - n + math.log(n * (1 + 4 * n * (1 + 2 * n))) / 6.0 + math.log(math.pi) / 2.0


def log_add(a, b):
    x = max(a, b)
    y = min(a, b)
    w = y - x
    return x + math.log1p(math.exp(w))


def log_choose(n, k):
    if k == 0 or k == n:
        return 0
    return log_fac(n) - (log_fac(n - k) + log_fac(k))


def log_bin_eq(p, n, k):
    lp = math.log(p)
    l1mp = math.log1p(-p)
    return log_choose(n, k) + lp * k + l1mp * (n - k)


def log_bin_ge(p, n, k):
    lp = math.log(p)
    l1mp = math.log1p(-p)
    v = log_choose(n, k) + lp * k + l1mp * (n - k)
    for j in range(k + 1, n + 1):
        w = log_choose(n, j) + lp * j + l1mp * (n - j)
        v = log_add(v, w)
    return v


def render(k, x):
    r = []
    for i in range(k):
        r.append("ACGT"[x & 3])
        x >>= 2
    return ''.join(r[::-1])


def groups(pairs):
    """[(context, [(k-mer, count)])] of an ascending list"""
    out = []
    for x, c in pairs:
        if not out or out[-1][0] != x >> 2:
            out.append((x >> 2, []))
        out[-1][1].append((x, c))
    return out


def group_values(ref_grp, sam_grp):
    """one joined group -> (b, [v0..v3], sx, gx)"""
    gt = float(sum(c for _, c in ref_grp))
    gx = [0, 0, 0, 0]
    for x, c in ref_grp:
        gx[x & 3] = c
    st = sum(c for _, c in sam_grp)
    sx = [0, 0, 0, 0]
    for x, c in sam_grp:
        sx[x & 3] = c
    b, vs = 0, []
    for j in range(4):
        p = float(gx[j]) / gt
        v = 0.0
        if 0.0 < p and p < 1.0:
            v = log_bin_ge(p, st, sx[j])
            if v < -10:
                b |= 1 << j
        vs.append(v)
    return b, vs, sx, gx


def line(K, ctx, b, vs):
    return '%s\t%s\t%s' % (render(K - 1, ctx), _FAS[b], '\t'.join('%3.2g' % (v,) for v in vs))


def stdout_lines(K, ref, sample, skip_missing=False, values=None):
    """the lines of one input; a context that the reference lacks is an AssertionError as in the reference (vars.py:96-97),
    or skipped.  values: a list that takes (context, b, vs, sx, gx) of every joined group."""
    by_ctx = dict(groups(ref))
    out = []
    for ctx, grp in groups(sample):
        if ctx not in by_ctx:
            assert skip_missing, "context %d is not in the reference" % ctx
            continue
        b, vs, sx, gx = group_values(by_ctx[ctx], grp)
        if values is not None:
            values.append((ctx, b, vs, sx, gx))
        if b > 0:
            out.append(line(K, ctx, b, vs))
    return out


def noise(K, ref, samples):
    """the largest |v| of a lane whose sample count is 0: its tail probability is 1, so v is rounding noise"""
    worst = 0.0
    for _, pairs in samples:
        vals = []
        stdout_lines(K, ref, pairs, values=vals)
        for _, _, vs, sx, _ in vals:
            worst = max([worst] + [abs(v) for v, k in zip(vs, sx) if k == 0])
    return worst
