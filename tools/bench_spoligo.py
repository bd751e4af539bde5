#!/usr/bin/env python3
"""zk_probe_scan, the kernel behind `zot spoligo`, at BASELINE config 3's size on one MI355X (run on the GPU box).

One set of N = 100 M ascending 50-bit keys (K = 25; zk_synth_keys) and panels of W = 1, 43 and 430 windows of J = 25 bases
(random 25-mers; every tenth window is a k-mer of the set with one base substituted, so that the tallies are not all zero):
  zk_probe_scan     algorithmic bytes: 8 per key and call, whatever W
and as the yardstick in the same run zk_split of the set against a second one of the same size (8 per entry read).  Every
figure: one warm-up call, then `reps` calls timed on the host around a call that ends in a stream synchronise; min / median /
max are printed, GB/s from the median.  The slope between W = 43 and W = 430 is the cost of one (key, window) test.

The CPU figure is the restatement of the reference's route (tests/_spoligo_restatement.py: neighbour enumeration and one
binary search per neighbour) on the 43-window panel and the first 200 000 keys of the set, on one core.

Usage: tools/bench_spoligo.py [--scale F] [--reps R] [--out FILE]      prints one JSON object
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
from tests import _spoligo_restatement as R          # noqa: E402

K = J = 25


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


def panel(rng, W, some_kmers):
    out = []
    for w in range(W):
        if w % 10 == 0:
            v = int(some_kmers[rng.integers(0, len(some_kmers))]) ^ (int(rng.integers(1, 4)) << (2 * int(rng.integers(0, J))))
        else:
            v = int(rng.integers(0, 1 << 50))
        out.append((J, v))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    N = int(100_000_000 * a.scale)
    out = {"n_keys_asked": N, "reps": a.reps, "K": K, "J": J}
    rng = np.random.default_rng(43)
    with native.Context(0) as ctx:
        ak, _ = ctx.synth_set(11, 0, N, 50, counts=False)
        bk, _ = ctx.synth_set(11, N // 2, N, 50, counts=False)
        out["n"], out["n_other"] = ak.n, bk.n
        head = ak.to_host(min(ak.n, 200_000))
        t, abc = timed(ctx, lambda: ctx.split(ak, bk), a.reps)
        out["split"] = rate(t, 8 * (ak.n + bk.n))
        panels = {W: panel(rng, W, head) for W in (1, 43, 430)}
        for W, windows in panels.items():
            t, tallies = timed(ctx, lambda: ctx.probe_scan(ak, K, windows), a.reps)
            rec = rate(t, 8 * ak.n)
            rec["windows"] = W
            rec["tallies_d0_d1_d2"] = [int(v) for v in tallies.sum(axis=0)]
            rec["windows_present"] = int((tallies.sum(axis=1) > 0).sum())
            rec["ns_per_key_window"] = t["ms_median"] * 1e6 / (ak.n * W)
            out["probe_scan_W%d" % W] = rec
        p1, p43, p430 = (out["probe_scan_W%d" % W] for W in (1, 43, 430))
        out["slope_ns_per_key_window"] = (p430["ms_median"] - p43["ms_median"]) * 1e6 / (ak.n * (430 - 43))
        out["W1_rate_over_split_rate"] = p1["GBps"] / out["split"]["GBps"]
        out["W1_within_15_percent_of_split"] = bool(p1["GBps"] >= 0.85 * out["split"]["GBps"])
        # linear in W once compute-bound: the time per window at 430 against the slope
        out["W430_ms_over_slope_times_W"] = p430["ms_median"] * 1e6 / (ak.n * 430) / out["slope_ns_per_key_window"]
        # the reference's route on one CPU core, same panel, a small set; the device must agree with it
        xs = [int(x) for x in head]
        seqs = ["".join("ACGT"[(v >> (2 * (J - 1 - i))) & 3] for i in range(J)) for _, v in panels[43]]
        t0 = time.perf_counter()
        want = R.spoligo(K, xs, seqs)
        dt = time.perf_counter() - t0
        got = ctx.probe_scan(ctx.upload(head), K, panels[43])
        assert "".join("1" if r.sum() else "0" for r in got) == want
        out["cpu_restatement"] = dict(keys=len(xs), probes=len(seqs), seconds=dt, probes_per_s=len(seqs) / dt, present=want.count("1"))
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
