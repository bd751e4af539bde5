#!/usr/bin/env python3
"""A / B of the two forms of pass 0 on the headline stream (config 2 of bench.py: 50 M x 150 bp, K = 25), alternated in ONE process
so that both run on the same box: ZK_TUNE_STREAM_PASS 1 (one 1024-thread workgroup per CU, 128-byte units) and 2 (two 512-thread
workgroups per CU, 64-byte units).  Per alternation: the HIP-event time of the pass (`pass_stream`), of the histogram kernel that
cuts the ranges for it (`hist_stream`) and of the whole kmerize call, and whether the two forms left the same table (order-free
checksums).  usage: p0_wide_ab.py [alternations=5] [reads=50e6] [out.json]"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zotmer_amd import native, synth

alts = int(sys.argv[1]) if len(sys.argv) > 1 else 5
reads = int(float(sys.argv[2])) if len(sys.argv) > 2 else None
out_path = sys.argv[3] if len(sys.argv) > 3 else None
cfg = synth.CONFIGS["config2"]
R, L, K = reads or cfg["reads"], cfg["L"], cfg["K"]
ctx = native.Context(0)
d = ctx.synth_reads(synth.DEFAULT_SEED, 0, R, L, genome=cfg["genome"], sub_thr=synth.frac32(cfg["sub"]), n_thr=synth.frac32(cfg["n"]))
cap = min(int(2 * (min(cfg["genome"], R * L) + R * L * cfg["sub"] * 22) * 1.25) + (1 << 20), 2 * R * (L + 1))
outs = (ctx.empty(cap, np.uint64), ctx.empty(cap, np.uint32))
runs = {1: [], 2: []}
sums = {}
for v in (1, 2):          # warm-up of both forms
    ctx.tune(stream_pass=v)
    ctx.kmerize(d, K, out=outs)
ctx.sync()
for i in range(alts):
    for v in ((1, 2) if i % 2 == 0 else (2, 1)):
        ctx.tune(stream_pass=v)
        ctx.profile(True)
        t0 = time.perf_counter()
        k, c, st = ctx.kmerize(d, K, out=outs)
        ctx.sync()
        dt = time.perf_counter() - t0
        prof = ctx.profile_read()
        ctx.profile(False)
        runs[v].append(dict(pass_stream_ms=prof.get("pass_stream", {}).get("ms"), hist_stream_ms=prof.get("hist_stream", {}).get("ms"),
                            kmerize_ms=round(dt * 1e3, 2)))
        if i == 0:
            sums[v] = (int(k.n), list(ctx.checksum(k, c)) if hasattr(ctx, "checksum") else None)
ctx.tune(stream_pass=1)


def stat(v, key):
    x = [r[key] for r in runs[v] if r[key] is not None]
    return dict(min=round(min(x), 3), median=round(float(np.median(x)), 3), max=round(max(x), 3)) if x else None


res = {"reads": R, "K": K, "alternations": alts, "same_table": sums.get(1) == sums.get(2),
       "variant1_wide": {k: stat(1, k) for k in ("pass_stream_ms", "hist_stream_ms", "kmerize_ms")},
       "variant2_512": {k: stat(2, k) for k in ("pass_stream_ms", "hist_stream_ms", "kmerize_ms")},
       "runs": {str(v): r for v, r in runs.items()}}
p1, p2 = res["variant1_wide"]["pass_stream_ms"], res["variant2_512"]["pass_stream_ms"]
if p1 and p2:
    res["pass0_speedup_median"] = round(p2["median"] / p1["median"], 3)
line = json.dumps(res)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
ctx.close()
