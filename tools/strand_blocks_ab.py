#!/usr/bin/env python3
"""A / B of the two strand rebuilds on the headline stream (config 2 of bench.py: 50 M x 150 bp, K = 25), alternated in ONE process
so that both run on the same box: two values of ZK_TUNE_STRAND_BLOCKS, by default 1 (block by block, strand_blocks.hip) and 0 (the
mirror sort over 26 bits and the merge-path union); `1,2`: the route with the unsorted dedupe and the persistent union against the
route before them (sorted blocks, one union workgroup per block).  Per alternation: the HIP-event times of the block dedupe (`rle`)
and of the tail -- the copy that writes the mirror words (`select`), the passes over them (`pass_packed`), the union (`union_sum`) --
and of the whole kmerize call, and whether the two left the same table (order-free checksums).  `skew`: every T that follows CAA in a read becomes A (the same on every copy of a stretch of the genome, so
the reads still repeat their k-mers): 9-base prefixes far from uniform -- blocks of the A-rich prefixes several times the mean, the
case where blocks are declined and cut into sub-tiles by value.
usage: strand_blocks_ab.py [alternations=5] [reads=50e6] [out.json] [skew|plain] [values=1,0]"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zotmer_amd import native, synth

alts = int(sys.argv[1]) if len(sys.argv) > 1 else 5
reads = int(float(sys.argv[2])) if len(sys.argv) > 2 else None
out_path = sys.argv[3] if len(sys.argv) > 3 else None
skew = len(sys.argv) > 4 and sys.argv[4] == "skew"
VA, VB = (int(x) for x in (sys.argv[5] if len(sys.argv) > 5 else "1,0").split(","))
cfg = synth.CONFIGS["config2"]
R, L, K = reads or cfg["reads"], cfg["L"], cfg["K"]
ctx = native.Context(0)
d = ctx.synth_reads(synth.DEFAULT_SEED, 0, R, L, genome=cfg["genome"], sub_thr=synth.frac32(cfg["sub"]), n_thr=synth.frac32(cfg["n"]))
if skew:
    h = d.to_host()
    A, C, T = ord("A"), ord("C"), ord("T")
    step = 1 << 28
    for s0 in range(((len(h) - 1) // step) * step, -1, -step):          # back to front: the three bases before a chunk are still as read
        lo = max(s0, 3)
        e = min(s0 + step, len(h))
        m = (h[lo - 3:e - 3] == C) & (h[lo - 2:e - 2] == A) & (h[lo - 1:e - 1] == A) & (h[lo:e] == T)
        h[lo:e][m] = A
    del d
    d = ctx.upload_stream(h)
    del h
cap = min(int(2 * (min(cfg["genome"], R * L) + R * L * cfg["sub"] * 22) * 1.25) + (1 << 20), 2 * R * (L + 1))
outs = (ctx.empty(cap, np.uint64), ctx.empty(cap, np.uint32))
TAIL = ("select", "pass_packed", "union_sum")
runs = {VA: [], VB: []}
sums = {}
for v in (VA, VB):          # warm-up of both forms
    ctx.tune(strand_blocks=v)
    ctx.kmerize(d, K, out=outs)
ctx.sync()
for i in range(alts):
    for v in ((VA, VB) if i % 2 == 0 else (VB, VA)):
        ctx.tune(strand_blocks=v)
        ctx.profile(True)
        t0 = time.perf_counter()
        k, c, st = ctx.kmerize(d, K, out=outs)
        ctx.sync()
        dt = time.perf_counter() - t0
        prof = ctx.profile_read()
        ctx.profile(False)
        tail = {t: prof.get(t, {}).get("ms") for t in TAIL}
        dd = prof.get("rle", {}).get("ms")
        runs[v].append(dict(tail_ms=round(sum(x for x in tail.values() if x), 3), dedupe_tail_ms=round((dd or 0) + sum(x for x in tail.values() if x), 3),
                            rle_ms=dd, kmerize_ms=round(dt * 1e3, 2),
                            union_records=prof.get("union_sum", {}).get("launches"), pass_packed_launches=prof.get("pass_packed", {}).get("launches"),
                            **{t + "_ms": x for t, x in tail.items()}))
        if i == 0:
            sums[v] = (int(k.n), int(st.n_canonical), list(ctx.checksum(k, c)))
ctx.tune(strand_blocks=1)


def stat(v, key):
    x = [r[key] for r in runs[v] if r[key] is not None]
    return dict(min=round(min(x), 3), median=round(float(np.median(x)), 3), max=round(max(x), 3)) if x else None


KEYS = ("dedupe_tail_ms", "tail_ms", "rle_ms", "kmerize_ms") + tuple(t + "_ms" for t in TAIL)
res = {"reads": R, "K": K, "skew": skew, "alternations": alts, "same_table": sums.get(VA) == sums.get(VB), "tables": {str(v): s for v, s in sums.items()},
       "strand_blocks_%d" % VA: {k: stat(VA, k) for k in KEYS},
       "strand_blocks_%d" % VB: {k: stat(VB, k) for k in KEYS},
       "runs": {str(v): r for v, r in runs.items()}}
line = json.dumps(res)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
ctx.close()
