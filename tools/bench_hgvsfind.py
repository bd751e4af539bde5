#!/usr/bin/env python3
"""`zot hgvs-find` on synthetic read pairs (run on the GPU box): R pairs x 150 bp written as tools/bench_pulldown.py writes them,
and a panel of V substitutions (every 50th entry an anonymous insertion instead) with flanks of 75 bases cut from the same
100 Mb genome.  Records:

  * the phases of the whole scan (library/hgvsfind.run with its stats): lookup, emission, sort and count, host merge, path
    scan, host allele work -- one warm-up, then `--reps` repetitions, wall time of each phase (min / median / max);
  * zk_capture_hits alone against zk_capture_hits + zk_capture_kmers on one device batch that holds every pair, alternated
    in one process, one warm-up and `--reps` repetitions each;
  * the zk_profile records of one emission: the emit kernel's time, the bytes it wrote and their rate against the HBM peak.

    python3 tools/bench_hgvsfind.py [--pairs R] [--variants V] [--out profiles/<round>/hgvsfind.json]
"""
import argparse, io, json, os, shutil, statistics, sys, time
os.environ.setdefault("ZOT_TIMING", "0")          # no phase lines (bench_pulldown would ask for them): the stats of the scan are the record
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_capture as bc
import bench_pulldown as bp
from zotmer_amd.library import capture, engine, fastq_batches, hgvsfind

PHASES = ("lookup_seconds", "emission_seconds", "count_seconds", "merge_seconds", "path_scan_seconds", "allele_seconds")


def panel(V, seed):
    rng = np.random.default_rng(seed)
    items = []
    for i, p in enumerate(sorted(int(x) for x in rng.integers(1000, bc.GENOME - 1000, V))):
        s = bc.genome_slice(p - 75, 151).decode()
        lhs, wt, rhs = s[:75], s[75], s[76:]
        if i % 50 == 49:
            items.append({"hgvs": "syn:g.%d_%dins12" % (p, p + 1), "lhsFlank": lhs, "rhsFlank": wt + rhs, "wtSeq": "", "mutSeq": None})
        else:
            alt = "ACGT"[("ACGT".index(wt) + 1 + i % 3) % 4]
            items.append({"hgvs": "syn:g.%d%s>%s" % (p + 1, wt, alt), "lhsFlank": lhs, "rhsFlank": rhs, "wtSeq": wt, "mutSeq": alt})
    return items


def spread(ts):
    return {"min_ms": min(ts) * 1e3, "median_ms": statistics.median(ts) * 1e3, "max_ms": max(ts) * 1e3}


def scan_phases(ctx, items, variants, fq, batch, reps):
    runs, text = [], None
    for rep in range(reps + 1):                        # rep 0 warms the page cache, the allocator and the workspace
        out, st = io.StringIO(), hgvsfind.new_stats()
        ctx.sync()
        t0 = time.perf_counter()
        hgvsfind.run(ctx, items, variants, fq, 25, 2, 10, 0.05, {"rds", "vaf"}, batch, out, stats=st)
        st["wall_seconds"] = time.perf_counter() - t0
        assert text is None or text == out.getvalue()
        text = out.getvalue()
        if rep:
            runs.append(st)
    res = {name[:-8]: spread([r[name] for r in runs]) for name in PHASES + ("wall_seconds",)}
    res["counts"] = {k: runs[-1][k] for k in ("read_pairs", "batches", "slices", "entries", "distinct_entries", "path_windows", "path_matches",
                                               "anchor_windows")}
    calls = [l.split("\t")[1] for l in text.splitlines()[1:]]
    res["calls"] = {c: calls.count(c) for c in sorted(set(calls))}
    med = {name: res[name[:-8]]["median_ms"] for name in PHASES}
    res["largest_phase"] = max(med, key=med.get)[:-8]
    return res


def entries_ab(ctx, table, fq, R, reps):
    size = max(os.path.getsize(p) for p in fq)
    batches = fastq_batches.record_batches(ctx, fq, size + 4096, warn_unequal=False)
    texts, lines, r, cuts = next(batches)
    assert r == R
    buf = ctx.empty(4 * r + 1024, np.uint64)
    t = {"capture_hits": [], "capture_hits_and_kmers": []}
    out = None
    for rep in range(reps + 1):
        for name in t:
            ctx.sync()
            t0 = time.perf_counter()
            pairs = ctx.capture_hits(table, 25, texts[0], lines[0], r, texts[1], lines[1], out=buf)
            if name != "capture_hits":
                ob, ok = ctx.capture_kmers(pairs, texts[0], lines[0], r, 25, texts[1], lines[1], out=out)
                out = (fastq_batches.whole(ob), fastq_batches.whole(ok))
            dt = time.perf_counter() - t0
            if rep:
                t[name].append(dt)
    ctx.profile(True)
    ob, ok = ctx.capture_kmers(pairs, texts[0], lines[0], r, 25, texts[1], lines[1], out=out)
    prof = ctx.profile_read()
    ctx.profile(False)
    batches.close()
    k = prof["capture_kmers"]
    res = {"pairs_of_reads": r, "text_bytes": cuts, "bait_pairs": pairs.n, "entries": ob.n, "repetitions": reps,
           "capture_hits": spread(t["capture_hits"]), "capture_hits_and_kmers": spread(t["capture_hits_and_kmers"]),
           "emit_kernel": {"ms": k["ms"], "bytes_written": k["bytes"], "bytes_per_s": k["bytes"] / (k["ms"] * 1e-3),
                           "share_of_hbm_peak_8e12": k["bytes"] / (k["ms"] * 1e-3) / bc.PEAK}}
    res["kmers_over_hits_median"] = res["capture_hits_and_kmers"]["median_ms"] / res["capture_hits"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=float, default=2e6)
    ap.add_argument("--variants", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tmp", default="/tmp/zot_hgvsfind_bench")
    a = ap.parse_args()
    R = int(a.pairs)
    shutil.rmtree(a.tmp, ignore_errors=True)
    os.makedirs(a.tmp)
    fq = [os.path.join(a.tmp, "r_%d.fastq" % (m + 1)) for m in range(2)]
    for m in range(2):
        bp.write_mate(fq[m], R, m * R)
    items = panel(a.variants, 13)
    items, variants = hgvsfind.parse_index(json.dumps(items))
    res = {"pairs": R, "read_length": bc.L, "fastq_bytes": [os.path.getsize(p) for p in fq], "variants": len(items),
           "anonymous_variants": sum(v.anonymous() for v in variants)}
    ctx = engine.context()
    from zotmer_amd.commands.capture import capture_batch_bytes
    res["scan"] = scan_phases(ctx, items, variants, fq, capture_batch_bytes(ctx), a.reps)
    print("scan", json.dumps(res["scan"]), flush=True)
    table = capture.build_table(ctx, [(itm["hgvs"].encode(), hgvsfind.bait_of(itm).encode()) for itm in items], 25)
    res["entries"] = entries_ab(ctx, table, fq, R, a.reps)
    table.free()
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    shutil.rmtree(a.tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
