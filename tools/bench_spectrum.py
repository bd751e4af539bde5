#!/usr/bin/env python3
"""The two kernels behind the spectrum measures of `zot dist` at BASELINE config 3's size on one MI355X (run on the GPU box).

Two counted sets of N = 100 M 50-bit keys, about half of each shared (zk_synth_keys walks one pool, the second set starts half
a set later; zk_synth_counts gives geometric 64-bit counts):
  zk_project_sum    at shift 0 (a copy and a widen) and shift 10        algorithmic bytes: 8 n + 16 n read, 16 per prefix written
  zk_spectrum_sums  on the two lists                                     16 per entry read
and as yardsticks on the same arrays zk_split (8 per entry read) and zk_union_sum with 64-bit counts (16 per entry read, 16
per entry of the union written).  Every figure: one warm-up call, then `reps` calls timed on the host around a call that ends
in a stream synchronise; min / median / max are printed, GB/s from the median.

--golden adds, per measure, the largest |device value - reference value| over the cases of tests/golden/g11_dist_spectrum.json.

--row measures something else instead, zk_spectrum_sums_row against the per-pair entry (row_mode below): each figure min / median /
max of `reps` rounds after a warm-up, the two sides alternated.

Usage: tools/bench_spectrum.py [--scale F] [--reps R] [--golden | --row] [--out FILE]      prints one JSON object
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zotmer_amd import native          # noqa: E402
from zotmer_amd.library import measures          # noqa: E402


def timed(ctx, f, reps):
    r = f()
    ctx.sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        ctx.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(ms_min=min(ts), ms_median=statistics.median(ts), ms_max=max(ts)), r


def rate(rec, nbytes):
    rec["algorithmic_bytes"] = int(nbytes)
    rec["GBps"] = nbytes / (rec["ms_median"] * 1e-3) / 1e9
    return rec


def golden_differences(ctx):
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, "g11_dist_spectrum.json")) as f:
        cases = json.load(f)
    worst = {}
    for c in cases:
        spec = []
        for name, par in zip((c["lhs"], c["rhs"]), c.get("prefix_parity", [None, None])):
            with open(os.path.join(gold, name + ".json")) as f:
                fK = json.load(f)["K"]
            z = np.load(os.path.join(gold, name + ".npz"))
            km, ct = z["kmers"], z["counts"]
            if par is not None:
                keep = ((km >> np.uint64(2 * (fK - c["k"]))) & np.uint64(1)) == np.uint64(par)
                km, ct = km[keep], ct[keep]
            spec.append(ctx.project_sum(ctx.upload(km), ctx.upload(ct.astype(np.uint64)), 2 * (fK - c["k"])))
        s = ctx.spectrum_sums(spec[0][0], spec[0][1], spec[0][2], spec[1][0], spec[1][1], spec[1][2])
        for m, want in c["values"].items():
            d = abs(measures.SPECTRUM[m](s) - float.fromhex(want["hex"]))
            worst[m] = max(worst.get(m, 0.0), d)
    return dict(cases=len(cases), max_abs_difference=worst)


def alternated(ctx, fs, reps):
    """{name: min / median / max ms} of the calls fs[name], one warm-up each, then `reps` rounds that time each of them in turn"""
    for f in fs.values():
        f()
    ctx.sync()
    ts = {name: [] for name in fs}
    for _ in range(reps):
        for name, f in fs.items():
            t0 = time.perf_counter()
            f()
            ctx.sync()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    return {name: dict(ms_min=min(v), ms_median=statistics.median(v), ms_max=max(v)) for name, v in ts.items()}


def row_mode(ctx, a):
    """zk_spectrum_sums_row against the per-pair entry it does not replace:
      (a) 63 spectra of 65 536 entries (every prefix of <k> = 8 present) against a 64th: one row call, and 63 zk_spectrum_sums calls
      (b) two lists of N = 100 M entries, m = 1: the row call and the existing entry"""
    out = {"reps": a.reps}
    rng = np.random.default_rng(30)
    n, m = 65536, 63
    keys = ctx.upload(np.arange(n, dtype=np.uint64))
    specs = []
    for _ in range(m + 1):
        s = rng.integers(1, 4000, size=n, dtype=np.uint64)
        specs.append((keys, ctx.upload(s), int(s.sum())))
    x, ys = specs[0], specs[1:]
    res = alternated(ctx, {"row_call": lambda: ctx.spectrum_sums_row(x, ys),
                           "pair_calls": lambda: [ctx.spectrum_sums(x[0], x[1], x[2], y[0], y[1], y[2]) for y in ys]}, a.reps)
    row, pairs = ctx.spectrum_sums_row(x, ys), [ctx.spectrum_sums(x[0], x[1], x[2], y[0], y[1], y[2]) for y in ys]
    assert all(r[f] == p[f] for r, p in zip(row, pairs) for f in ("n_shared", "S_min", "X_shared", "Y_shared", "S_xy"))
    spread = max(v["ms_max"] - v["ms_min"] for v in res.values())
    res.update(m=m, entries_per_spectrum=n, spread_ms=spread,
               row_beats_pairs_by_more_than_the_spread=bool(res["pair_calls"]["ms_median"] - res["row_call"]["ms_median"] > spread))
    out["a_63_spectra_of_65536"] = res
    del specs, x, ys
    N = int(100_000_000 * a.scale)
    ak, ac = ctx.synth_set(11, 0, N, 50)
    bk, bc = ctx.synth_set(11, N // 2, N, 50)
    cx, cy = ctx.project_sum(ak, ac, 40)[2], ctx.project_sum(bk, bc, 40)[2]
    res = alternated(ctx, {"row_call": lambda: ctx.spectrum_sums_row((ak, ac, cx), [(bk, bc, cy)]),
                           "pair_call": lambda: ctx.spectrum_sums(ak, ac, cx, bk, bc, cy)}, a.reps)
    r, p = ctx.spectrum_sums_row((ak, ac, cx), [(bk, bc, cy)])[0], ctx.spectrum_sums(ak, ac, cx, bk, bc, cy)
    assert all(r[f] == p[f] for f in ("n_shared", "S_min", "X_shared", "Y_shared", "S_xy"))
    spread = max(v["ms_max"] - v["ms_min"] for v in res.values())
    for v in (res["row_call"], res["pair_call"]):
        rate(v, 16 * (ak.n + bk.n))
    res.update(nA=ak.n, nB=bk.n, spread_ms=spread,
               row_costs_no_more_than_pair_plus_spread=bool(res["row_call"]["ms_median"] <= res["pair_call"]["ms_median"] + spread))
    out["b_two_lists_m1"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--golden", action="store_true")
    ap.add_argument("--row", action="store_true", help="zk_spectrum_sums_row against zk_spectrum_sums (a row of 63, and m = 1 at full size)")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.row:
        with native.Context(0) as ctx:
            out = row_mode(ctx, a)
        text = json.dumps(out, indent=1, sort_keys=True)
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return
    N = int(100_000_000 * a.scale)
    out = {"n_per_set": N, "reps": a.reps}
    with native.Context(0) as ctx:
        ak, ac = ctx.synth_set(11, 0, N, 50)
        bk, bc = ctx.synth_set(11, N // 2, N, 50)
        out["nA"], out["nB"] = ak.n, bk.n
        n2 = ak.n + bk.n
        t, abc = timed(ctx, lambda: ctx.split(ak, bk), a.reps)
        out["split"] = rate(t, 8 * n2)
        out["shared"] = abc[0]
        ok, oc = ctx.empty(n2, np.uint64), ctx.empty(n2, np.uint64)
        t, r = timed(ctx, lambda: ctx.union_sum(ak, ac, bk, bc, out=(ok, oc)), a.reps)
        out["union_sum_u64"] = rate(t, 16 * n2 + 16 * r[0].n)
        out["union_sum_u64"]["read_only_GBps"] = 16 * n2 / (t["ms_median"] * 1e-3) / 1e9
        del ok, oc, r
        for sh in (0, 10):
            t, r = timed(ctx, lambda: ctx.project_sum(ak, ac, sh), a.reps)
            out["project_sum_shift%d" % sh] = rate(t, 8 * ak.n + 16 * ak.n + 16 * r[0].n)
            out["project_sum_shift%d" % sh]["prefixes"] = r[0].n
            del r
        cx, cy = ctx.project_sum(ak, ac, 40)[2], ctx.project_sum(bk, bc, 40)[2]
        t, s = timed(ctx, lambda: ctx.spectrum_sums(ak, ac, cx, bk, bc, cy), a.reps)
        out["spectrum_sums"] = rate(t, 16 * n2)
        assert s["n_shared"] == abc[0], (s["n_shared"], abc)
        out["spectrum_sums"]["values"] = {m: f(s) for m, f in sorted(measures.SPECTRUM.items())}
        spread = out["union_sum_u64"]["ms_max"] - out["union_sum_u64"]["ms_min"]
        out["sums_no_slower_than_union_sum"] = bool(out["spectrum_sums"]["ms_median"] <= out["union_sum_u64"]["ms_median"] + spread)
        if a.golden:
            out["golden"] = golden_differences(ctx)
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
