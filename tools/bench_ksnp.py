#!/usr/bin/env python3
"""`zot ksnp` on one MI355X (run on the GPU box): the pair pass, the default pass, the entries and the command.

Two sets, made on the host from zotmer_amd/synth.py's genome (base g = rnd(seed, 1, g) & 3) of `--genome` bases and a copy of it
in which about 1 % of the bases are substituted (position g when the low 32 bits of rnd(seed, 30, g) are below frac32(0.01), by
(base + 1 + rnd(seed, 31, g) % 3) & 3): the distinct K-mers of both, forward strand.
  k25   K = 25: the prefix is 12 bases, nearly every group is one k-mer or a k-mer and its SNP variants;
  k13   K = 13: the prefix is 6 bases, 4096 groups of about a thousand k-mers each.
Per set the group-size histogram and the number of pair tests sum s (s - 1) / 2 are stated (NumPy, on the host): the work of
-H and -L is the pair tests, not the bytes.

Per set and mode (default, -H 1, -H 2, -L 1, -L 2), one warm-up call and `--reps` timed ones, min / median / max:
  entry        the whole zk_ksnp_* call into a buffer with room, host clock around a call that ends in a stream synchronise
  pair pass    the ZK_PROF_KSNP_PAIRS records of the call summed (zk_profile: HIP events around the pair kernels), and the pair
               tests per second from the median
  default pass the ZK_PROF_KSNP_FLANK record, and GB/s of list read (8 B per k-mer) from the median
and once, with --e2e DIR, the command on a set file (ZOT_TIMING=2).
CPU baseline: the plain-Python restatement (tests/_ksnp_restatement.py) on one core on the first groups of the set (a leading
part of the first group where that alone is too much), up to `--cpu-pairs` pair tests, a hundredth of that for -L; its time
per pair test scaled to the set's pair tests (the default mode: per k-mer).

Usage: tools/bench_ksnp.py [--genome G] [--reps R] [--cpu-pairs P] [--e2e DIR] [--out FILE]      prints one JSON object
"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("ZOT_TIMING", "2")          # library/timing.py reads it at import
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from zotmer_amd import native, synth          # noqa: E402
from bench_vars import run_command          # noqa: E402
from tests import _ksnp_restatement as R          # noqa: E402

MODES = (("default", None, 0), ("H1", native.KSNP_HAMMING, 1), ("H2", native.KSNP_HAMMING, 2), ("L1", native.KSNP_LEVENSHTEIN, 1),
         ("L2", native.KSNP_LEVENSHTEIN, 2))
U = np.uint64


def kmers_of(codes, K):
    x = np.zeros(len(codes) - K + 1, dtype=np.uint64)
    for j in range(K):
        x = (x << U(2)) | codes[j:j + len(x)]
    return x


def make_set(seed, G, K):
    g = np.arange(G, dtype=np.uint64)
    base = synth.rnd(seed, 1, g) & U(3)
    hit = (synth.rnd(seed, 30, g) & U(0xFFFFFFFF)) < U(synth.frac32(0.01))
    copy = np.where(hit, (base + U(1) + synth.rnd(seed, 31, g) % U(3)) & U(3), base)
    return np.unique(np.concatenate([kmers_of(base, K), kmers_of(copy, K)])), int(hit.sum())


def group_sizes(K, xs):
    S = 2 * ((K - 1) // 2 + 1)
    p = xs >> U(S)
    cuts = np.flatnonzero(np.concatenate([[True], p[1:] != p[:-1], [True]]))
    return np.diff(cuts)


def histogram(sizes):
    """groups by size class: 1, 2, 3-4, 5-8, ... (the upper bound of each class) -> {bound: groups}"""
    bound = np.where(sizes <= 1, 1, 1 << np.ceil(np.log2(np.maximum(sizes, 1))).astype(np.int64))
    v, c = np.unique(bound, return_counts=True)
    return {str(int(a)): int(b) for a, b in zip(v, c)}


def spread(ts):
    return dict(ms_min=min(ts), ms_median=statistics.median(ts), ms_max=max(ts))


def bench_set(ctx, K, xs, reps, cpu_pairs):
    sizes = group_sizes(K, xs)
    pairs = int((sizes.astype(np.int64) * (sizes.astype(np.int64) - 1) // 2).sum())
    rec = dict(K=K, n=int(len(xs)), groups=int(len(sizes)), largest_group=int(sizes.max()), pair_tests=pairs, group_histogram=histogram(sizes))
    d = ctx.upload(xs)
    out = ctx.empty(d.n, np.uint64)
    for name, metric, dist in MODES:
        entry, kernel = [], []
        tag = "ksnp_flank" if metric is None else "ksnp_pairs"
        for r in range(reps + 1):
            ctx.profile(True)
            ctx.sync()
            t0 = time.perf_counter()
            n, fit = ctx.ksnp_into(d, K, out, metric, dist)
            ctx.sync()
            dt = (time.perf_counter() - t0) * 1e3
            p = ctx.profile_read()
            ctx.profile(False)
            assert fit
            if r:          # the first call is the warm-up
                entry.append(dt)
                kernel.append(p[tag]["ms"])
        m = dict(kept=int(n), entry=spread(entry), launches=int(p[tag]["launches"]))
        if metric is None:
            m["default_pass"] = dict(spread(kernel), GBps_list_read=8 * len(xs) / (statistics.median(kernel) * 1e-3) / 1e9)
        else:
            m["pair_pass"] = dict(spread(kernel), pair_tests_per_s=pairs / (statistics.median(kernel) * 1e-3))
        rec[name] = m
    # the restatement on one core, on the first groups of the set (a leading part of the first group where that alone is too much)
    def piece_of(budget):
        cum = np.cumsum(sizes.astype(np.int64) * (sizes.astype(np.int64) - 1) // 2)
        g = int(np.searchsorted(cum, budget, side="right"))
        m = int(np.cumsum(sizes)[g - 1]) if g else min(int(sizes[0]), max(2, int((2 * budget) ** 0.5)))
        piece = xs[:m]
        ps = group_sizes(K, piece).astype(np.int64)
        return piece.tolist(), int((ps * (ps - 1) // 2).sum())

    cpu = {}
    for name, mode, dist, budget in (("default", R.DEFAULT, 0, cpu_pairs), ("H1", R.HAMMING, 1, cpu_pairs),
                                     ("L1", R.LEVENSHTEIN, 1, max(cpu_pairs // 100, 1))):
        piece, piece_pairs = piece_of(budget)
        t0 = time.perf_counter()
        R.run(K, mode, dist, piece)
        dt = time.perf_counter() - t0
        cpu[name] = dict(seconds=dt, kmers=len(piece), pair_tests=piece_pairs)
        if mode == R.DEFAULT:
            cpu[name]["scaled_to_the_set_s"] = dt * len(xs) / max(len(piece), 1)          # linear in the k-mers
        elif piece_pairs:
            cpu[name]["us_per_pair_test"] = dt * 1e6 / piece_pairs
            cpu[name]["scaled_to_the_set_s"] = dt * pairs / piece_pairs
    rec["cpu_restatement_one_core"] = cpu
    return rec, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-pairs", type=int, default=200_000)
    ap.add_argument("--e2e")
    ap.add_argument("--out")
    a = ap.parse_args()
    out = {"reps": a.reps, "genome": a.genome, "warm_up_calls": 1}

    def emit():
        text = json.dumps(out, indent=1, sort_keys=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return text

    from zotmer_amd.library import engine
    ctx = engine.context()
    for K in (25, 13):
        xs, subs = make_set(synth.DEFAULT_SEED, a.genome, K)
        rec, d = bench_set(ctx, K, xs, a.reps, a.cpu_pairs)
        rec["substituted_bases"] = subs
        if a.e2e:
            from zotmer_amd.library import ksnp
            os.makedirs(a.e2e, exist_ok=True)
            path, res = os.path.join(a.e2e, "set.k%d" % K), os.path.join(a.e2e, "out.k%d" % K)
            ksnp.write_set(path, K, ctx=ctx, kmers_dev=d)
            rec["command"] = {"set_bytes": os.path.getsize(path)}
            for name, opt in (("default", []), ("H1", ["-H", "1"]), ("L2", ["-L", "2"])):
                dt, _, phases, other = run_command(["ksnp"] + opt + [res, path])
                rec["command"][name] = dict(seconds=dt, phases_ms=phases, stderr=other[:4], out_bytes=os.path.getsize(res))
            os.remove(path)
            os.remove(res)
        del d
        out["k%d" % K] = rec
        emit()
    print(emit())
    engine.close()


if __name__ == "__main__":
    main()
