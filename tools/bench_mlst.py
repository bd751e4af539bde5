#!/usr/bin/env python3
"""zk_bait_tally, the kernel behind `zot mlst`, and the two ways to its table, on one MI355X (run on the GPU box).

A synthetic scheme at K = 27: 7 loci x 1 000 alleles x 450 bases, each allele its locus's base sequence with about 1 % of its
bases substituted.  The sample: 10 M ascending 54-bit keys (zk_synth_keys), merged with all k-mers of one allele per locus.
  zk_bait_table_build         from the records' base stream
  zk_bait_table_from_arrays   from the built table's arrays (the device-side check, three copies, the directory)
  zk_bait_tally               algorithmic bytes: 8 per set entry; the number of adds is recorded beside it
and as the yardstick in the same run zk_split of the sample against a second set of the same size (8 per entry read).  Every
figure: one warm-up call, then `reps` calls timed on the host around a call that ends in a stream synchronise; min / median /
max are printed, GB/s from the median.

The CPU figure is the restatement of the reference's loop (tests/_mlst_restatement.py: mlst.py:45-54 over the index as lists,
one binary search per k-mer) on the first `--cpu-fraction` of the sample plus the planted alleles' k-mers, on one core; the
device must call the same records.

Usage: tools/bench_mlst.py [--scale F] [--reps R] [--cpu-fraction F] [--label TEXT] [--out FILE]      prints one JSON object
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
from tests import _mlst_restatement as R          # noqa: E402

K, LOCI, ALLELES, BASES, SUB = 27, 7, 1000, 450, 0.01


def timed(ctx, f, reps):
    r = f()
    ctx.sync()
    ts = []
    for _ in range(reps):
        del r
        t0 = time.perf_counter()
        r = f()
        ctx.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(ms_min=min(ts), ms_median=statistics.median(ts), ms_max=max(ts)), r


def rate(rec, nbytes):
    rec["algorithmic_bytes"] = int(nbytes)
    rec["GBps"] = nbytes / (rec["ms_median"] * 1e-3) / 1e9
    return rec


def scheme(rng):
    """the records' base stream (one '\\n' per record) as a uint8 array, record = locus * ALLELES + allele"""
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    recs = np.empty((LOCI * ALLELES, BASES + 1), dtype=np.uint8)
    recs[:, BASES] = 10
    for l in range(LOCI):
        base = rng.integers(0, 4, size=BASES)
        al = np.tile(base, (ALLELES, 1))
        sub = rng.random((ALLELES, BASES)) < SUB
        al[sub] = (al[sub] + rng.integers(1, 4, size=int(sub.sum()))) & 3
        recs[l * ALLELES:(l + 1) * ALLELES, :BASES] = acgt[al]
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-fraction", type=float, default=0.02)
    ap.add_argument("--label", default="")
    ap.add_argument("--out")
    a = ap.parse_args()
    N = int(10_000_000 * a.scale)
    out = {"label": a.label, "lib": os.path.basename(native.LIB_PATH), "n_keys_asked": N, "reps": a.reps, "K": K,
           "scheme": dict(loci=LOCI, alleles=ALLELES, bases=BASES, substituted=SUB)}
    rng = np.random.default_rng(27)
    recs = scheme(rng)
    planted = [l * ALLELES + int(rng.integers(0, ALLELES)) for l in range(LOCI)]
    with native.Context(0) as ctx:
        stream = ctx.upload_stream(recs.reshape(-1))
        t, table = timed(ctx, lambda: ctx.bait_table(stream, K), a.reps)
        out["table_build"] = rate(t, stream.n)
        out["table"] = dict(n_keys=table.n_keys, n_ids=table.n_ids, n_records=table.n_records)
        keys, offs, ids = table.arrays()
        t, again = timed(ctx, lambda: ctx.bait_table_from_arrays(K, keys, offs, ids, table.n_records), a.reps)
        out["table_from_arrays"] = rate(t, 8 * keys.n + 4 * offs.n + 4 * ids.n)
        lens = ctx.bait_record_sizes(table).to_host()
        assert np.array_equal(ctx.bait_record_sizes(again).to_host(), lens)
        del again
        # the sample: synthetic keys merged with every k-mer of one allele per locus
        small = ctx.bait_table(ctx.upload_stream(recs[planted].reshape(-1)), K)
        own = small.arrays()[0].to_host()
        ak, _ = ctx.synth_set(11, 0, N, 2 * K, counts=False)
        bk, _ = ctx.synth_set(11, N // 2, N, 2 * K, counts=False)
        sample_host = np.union1d(ak.to_host(), own)
        sample = ctx.upload(sample_host)
        out["n"], out["n_other"], out["n_planted_kmers"] = sample.n, bk.n, len(own)
        t, abc = timed(ctx, lambda: ctx.split(sample, bk), a.reps)
        out["split"] = rate(t, 8 * (sample.n + bk.n))
        hits = ctx.empty(table.n_records, np.uint32)
        t, _ = timed(ctx, lambda: ctx.bait_tally(table, sample, out=hits), a.reps)
        h = hits.to_host()
        rec = rate(t, 8 * sample.n)
        rec["adds"] = int(h.sum())
        rec["ns_per_add"] = t["ms_median"] * 1e6 / max(rec["adds"], 1)
        called = np.nonzero(h == lens)[0].tolist()
        rec["records_called"] = len(called)
        assert sorted(planted) == [c for c in called if c in set(planted)] and np.array_equal(h, ctx.bait_tally(table, sample).to_host())
        out["tally"] = rec
        out["tally_rate_over_split_rate"] = rec["GBps"] / out["split"]["GBps"]
        # the same table with every key in the set: n_ids adds
        t, _ = timed(ctx, lambda: ctx.bait_tally(table, keys, out=hits), a.reps)
        rec = rate(t, 8 * keys.n)
        rec["adds"] = int(hits.to_host().sum())
        rec["ns_per_add"] = t["ms_median"] * 1e6 / max(rec["adds"], 1)
        assert rec["adds"] == table.n_ids
        out["tally_every_key"] = rec
        if a.cpu_fraction > 0:
            # the reference's loop on one CPU core for a fraction of the sample; the device must call the same records
            part = np.union1d(sample_host[:int(len(sample_host) * a.cpu_fraction)], own)
            idx = dict(K=K, lens=lens.tolist(), S=keys.to_host().tolist(), T=offs.to_host().tolist(), U=ids.to_host().tolist())
            xs = part.tolist()
            t0 = time.perf_counter()
            want = R.complete(idx, xs)
            dt = time.perf_counter() - t0
            got = np.nonzero(ctx.bait_tally(table, ctx.upload(part)).to_host() == lens)[0].tolist()
            assert got == want and set(planted) <= set(want)
            out["cpu_restatement"] = dict(fraction=a.cpu_fraction, entries=len(xs), seconds=dt, entries_per_s=len(xs) / dt, records_called=len(want))
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
