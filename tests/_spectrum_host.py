"""Host-side specification of the spectrum measures of `zot dist`, for the tests: the spectrum of a golden set with numpy, and the
sums zk_spectrum_sums returns in Python integers and math.fsum (one correctly rounded sum of the same terms)."""
import math

import numpy as np

from tests import _golden as G


def host_project_sum(kmers, counts, shift):
    """numpy's statement of zk_project_sum -> (prefixes u64 ascending, sums u64, total int)"""
    k = np.asarray(kmers, dtype=np.uint64) >> np.uint64(shift)
    u, inv = np.unique(k, return_inverse=True)
    s = np.zeros(len(u), dtype=np.uint64)
    np.add.at(s, inv, np.asarray(counts).astype(np.uint64))
    return u, s, sum(int(c) for c in np.asarray(counts))


def golden_spectrum(name, K, parity=None):
    """(prefixes, sums, total) of a golden set at <k> = K; parity: only the prefixes with that lowest bit (the disjoint case)"""
    info, km, ct, _, _ = G.load_case(name)
    u, s, _ = host_project_sum(km, ct, 2 * (info["K"] - K))
    if parity is not None:
        keep = (u & np.uint64(1)) == np.uint64(parity)
        u, s = u[keep], s[keep]
    return u, s, sum(int(v) for v in s)


def host_spectrum_sums(xk, xs, yk, ys):
    """dict of the sums (the keys of native.Context.spectrum_sums) + js_abs = sum of |Jensen-Shannon term| and sqrt_abs = S_sqrt,
    the scales of the rounding error of the two doubles.  The terms are written as library/dist.py:90,138-139 writes them."""
    xd = {int(k): int(v) for k, v in zip(xk, xs)}
    cx, cy = sum(xd.values()), sum(int(v) for v in ys)
    fx, fy = float(cx), float(cy)
    out = dict(cx=cx, cy=cy, n_shared=0, S_min=0, X_shared=0, Y_shared=0, S_xy=0)
    roots, js = [], []
    for k, y in zip(yk, ys):
        x, y = xd.get(int(k), 0), int(y)
        if x == 0 or y == 0:
            continue
        out["n_shared"] += 1
        out["S_min"] += min(x, y)
        out["X_shared"] += x
        out["Y_shared"] += y
        out["S_xy"] += x * y
        roots.append(math.sqrt(x * y))
        js.append(x / fx * math.log(2 * fy * x / (fy * x + fx * y)))
        js.append(y / fy * math.log(2 * fx * y / (fx * y + fy * x)))
    out["S_sqrt"], out["S_js"] = math.fsum(roots), math.fsum(js)
    out["sqrt_abs"], out["js_abs"] = out["S_sqrt"], math.fsum(abs(t) for t in js)
    return out
