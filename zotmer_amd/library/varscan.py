"""
Host side of `zot vars -r`: the reference's binomial tail in its own order of operations, the guard that zk_vars_scan
puts around its first term, the evaluation of the rows the device hands back, and the loop over the inputs.

Like jstats.py this file restates its source by necessity (zotmer/library/stats.py:77-92, 121-128, 214-226 and
zotmer/commands/vars.py:98-117): the numeric columns are printed with '%3.2g' and where the exact value is 0 they are
rounding noise, so the text depends on the order of the floating-point operations.
"""
import math
import sys

from zotmer_amd.library.jstats import log_add, log_choose

THRESHOLD = -10.0                   # vars.py:113
GUARD_UNIT = 2.0 ** -47             # VS_GUARD_UNIT (csrc/vars_scan.hip)
FASTA = "*ACMGRSVTWYHKDBN"          # basics.py:69-86: bit j of the index = base j


def first_term(p, n, k):
    """logBinEq(p, n, k), the term logBinGe starts from (stats.py:220-222)"""
    lp = math.log(p)
    l1mp = math.log1p(-p)
    return log_choose(n, k) + lp * k + l1mp * (n - k)


def log_bin_ge(p, n, k):
    """log Bin(p, n, X >= k)  (stats.py:214-226)"""
    lp = math.log(p)
    l1mp = math.log1p(-p)
    v = log_choose(n, k) + lp * k + l1mp * (n - k)
    for j in range(k + 1, n + 1):
        w = log_choose(n, j) + lp * j + l1mp * (n - j)
        v = log_add(v, w)
    return v


def _mag_fac(m):
    return 64.0 if m < 25 else m * math.log(m) + m + 64.0


def guard(n, k, p):
    """G of include/zotk.h: a bound on the difference between two double-precision evaluations of first_term(p, n, k) that
    differ only in their log / log1p (each within 4 ulp) -- 2^-47 times the sum of the magnitudes of the terms added up"""
    s = k * abs(math.log(p)) + (n - k) * abs(math.log1p(-p))
    if 0 < k < n:
        s += _mag_fac(n) + _mag_fac(n - k) + _mag_fac(k)
    return s * GUARD_UNIT


def candidate(sx_j, st, gx_j, gt, threshold=THRESHOLD, guards=1.0):
    """the device's predicate for one base, on the host's own first term (tests bracket the device with guards = 0 and 2)"""
    if not 0 < gx_j < gt or not sx_j * gt > st * gx_j:
        return False
    p = float(gx_j) / float(gt)
    if not 0.0 < p < 1.0:
        return False
    return first_term(p, st, sx_j) < threshold + guards * guard(st, sx_j, p)


def render(J, x):
    """basics.render (basics.py:60-66)"""
    return "".join("ACGT"[(x >> (2 * (J - 1 - i))) & 3] for i in range(J))


def eval_row(sx, gx, threshold=THRESHOLD):
    """one joined group -> (b, [v0, v1, v2, v3])  (vars.py:98-115)"""
    gt = float(sum(gx))
    st = sum(sx)
    b = 0
    vs = []
    for j in range(4):
        p = float(gx[j]) / gt
        v = 0.0
        if 0.0 < p and p < 1.0:
            v = log_bin_ge(p, st, sx[j])
            if v < threshold:
                b |= 1 << j
        vs.append(v)
    return b, vs


def format_row(J, ctx, b, vs):
    """vars.py:115-117"""
    return "%s\t%s\t%s" % (render(J, ctx), FASTA[b], "\t".join("%3.2g" % (v,) for v in vs))


def lines_of_rows(K, ctxs, rows):
    """the device's rows (contexts; 8 counts each) -> the lines the reference prints for them"""
    out = []
    for c, r in zip(ctxs, rows):
        r = [int(x) for x in r]
        b, vs = eval_row(r[0:4], r[4:8])
        if b > 0:
            out.append(format_row(K - 1, int(c), b, vs))
    return out


class MismatchedK(Exception):
    pass


def read_k(paths):
    """vars.getK (vars.py:22-31)"""
    from zotmer_amd.library.container import KmerSet
    K = None
    for fn in paths:
        with KmerSet(fn, "r") as z:
            k0 = z.meta["K"]
            if K is None:
                K = k0
            elif K != k0:
                raise MismatchedK("%s has K=%d, the inputs before it K=%d" % (fn, k0, K))
    return K


def run(ctx, ref_path, inputs, K, out=None, err=None):
    """the reference set stays on the device; every input is read, scanned and printed"""
    from zotmer_amd.library import vectors
    from zotmer_amd.library.container import KmerSet
    from zotmer_amd.library.timing import Phase
    out = out or sys.stdout
    err = err or sys.stderr
    with KmerSet(ref_path, "r") as z:
        rk, rc = vectors.device_read_kmers_and_counts(ctx, z)
    for fn in inputs:
        with KmerSet(fn, "r") as z:
            sk, sc = vectors.device_read_kmers_and_counts(ctx, z)
        with Phase(ctx, "vars scan", 16 * (rk.n + sk.n)):
            ctxs, rows, st = ctx.vars_scan(rk, rc, sk, sc, K, THRESHOLD)
        with Phase(ctx, "vars rows", 72 * st.n_rows):
            lines = lines_of_rows(K, ctxs.to_host(), rows.to_host().reshape(-1, 8))
        for ln in lines:
            out.write(ln + "\n")
        if st.n_missing:
            err.write("zot vars: %s: %d of %d contexts are not in the reference (first: %s)\n"
                      % (fn, st.n_missing, st.n_groups, render(K - 1, st.first_missing)))
