#!/usr/bin/env python3
"""`zot pulldown` on synthetic read pairs (run on the GPU box): R pairs x 150 bp written the way tools/bench_capture.py writes
its reads (mate 2 continues the generator's read numbers after mate 1), one bait panel (1000 baits x 5 kb) and one -U panel
(50 x 2 kb) cut from the same 100 Mb genome.  Records:

  * zk_pulldown_hits against zk_capture_hits on the same device batch with the same two tables, alternated in one process:
    one warm-up, then `--reps` repetitions each, wall time of the whole call (min / median / max), and the zk_profile records
    of one pulldown pass (the lookup, the sort passes, the tally and the histogram);
  * the command end to end, cold and warm, with the ZOT_TIMING=2 phases of the warm run summed by name.

    python3 tools/bench_pulldown.py [--pairs R] [--out profiles/<round>/pulldown.json]
"""
import argparse, json, os, shutil, statistics, sys, time
os.environ.setdefault("ZOT_TIMING", "2")          # library/timing.py reads it at import
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_capture as bc
from zotmer_amd import synth
from zotmer_amd.library import capture, engine, fastq_batches

L = bc.L


def write_mate(path, R, first):
    ctx = engine.context()
    with open(path, "wb") as f:
        step = 1_000_000
        for a in range(0, R, step):
            m = min(step, R - a)
            seq = ctx.synth_reads(synth.DEFAULT_SEED, first + a, m, L, genome=bc.GENOME, sub_thr=synth.frac32(0.005),
                                  n_thr=synth.frac32(0.0005)).to_host().reshape(m, L + 1)
            rec = np.empty((m, 13 + (L + 1) + 2 + (L + 1)), dtype=np.uint8)
            rec[:, 0] = ord("@"); rec[:, 1] = ord("r")
            rec[:, 2:12] = np.frombuffer("".join(np.char.zfill(np.arange(a, a + m).astype(str), 10)).encode(), np.uint8).reshape(m, 10)
            rec[:, 12] = ord("\n")
            rec[:, 13:14 + L] = seq
            rec[:, 14 + L] = ord("+"); rec[:, 15 + L] = ord("\n")
            rec[:, 16 + L:16 + 2 * L] = ord("I"); rec[:, 16 + 2 * L] = ord("\n")
            f.write(rec.tobytes())


def spread(ts):
    return {"min_ms": min(ts) * 1e3, "median_ms": statistics.median(ts) * 1e3, "max_ms": max(ts) * 1e3}


def kernels_ab(ctx, table, veto, paths, R, reps):
    """both entries on one batch that holds every pair"""
    size = max(os.path.getsize(p) for p in paths)
    batches = fastq_batches.record_batches(ctx, paths, size + 4096, warn_unequal=False)
    texts, lines, r, cuts = next(batches)
    assert r == R
    args = (table, 25, texts[0], lines[0], r, texts[1], lines[1])
    buf = ctx.empty(4 * r + 1024, np.uint64)
    t = {"capture_hits": [], "pulldown_hits": []}
    n = {}
    for rep in range(reps + 1):                    # rep 0 warms both (and sizes the workspace)
        for name in ("capture_hits", "pulldown_hits"):
            ctx.sync()
            t0 = time.perf_counter()
            got = getattr(ctx, name)(*args, veto=veto, out=buf)
            dt = time.perf_counter() - t0
            if rep:
                t[name].append(dt)
            n[name] = got.n if name == "capture_hits" else got[0].n
    assert n["capture_hits"] == n["pulldown_hits"]
    ctx.profile(True)
    pairs, hist, vetoed = ctx.pulldown_hits(*args, veto=veto, out=buf)
    prof = ctx.profile_read()
    ctx.profile(False)
    batches.close()
    res = {"pairs_of_reads": r, "text_bytes": cuts, "bait_pairs": pairs.n, "vetoed": vetoed, "rows": {int(i): int(hist[i]) for i in np.nonzero(hist)[0]},
           "repetitions": reps, "capture_hits": spread(t["capture_hits"]), "pulldown_hits": spread(t["pulldown_hits"]),
           "profile_of_one_pulldown_pass": prof}
    res["pulldown_over_capture_median"] = res["pulldown_hits"]["median_ms"] / res["capture_hits"]["median_ms"]
    res["extra_bytes_read_by_the_two_passes"] = 8 * pairs.n + 5 * r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=float, default=2e6)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tmp", default="/tmp/zot_pulldown_bench")
    a = ap.parse_args()
    R = int(a.pairs)
    shutil.rmtree(a.tmp, ignore_errors=True)
    os.makedirs(a.tmp)
    fq = [os.path.join(a.tmp, "r_%d.fastq" % (m + 1)) for m in range(2)]
    for m in range(2):
        write_mate(fq[m], R, m * R)
    fa, up = os.path.join(a.tmp, "baits.fa"), os.path.join(a.tmp, "up.fa")
    bc.write_panel(fa, 1000, 5000, 7)
    bc.write_panel(up, 50, 2000, 11)
    res = {"pairs": R, "read_length": L, "fastq_bytes": [os.path.getsize(p) for p in fq], "panel": "1000 x 5 kb", "pushup_panel": "50 x 2 kb"}
    ctx = engine.context()
    table = capture.build_table(ctx, capture.bait_records(fa), 25)
    veto = capture.build_table(ctx, capture.bait_records(up), 25)
    res["entries"] = kernels_ab(ctx, table, veto, fq, R, a.reps)
    table.free()
    veto.free()
    print("entries", json.dumps(res["entries"]), flush=True)
    out = os.path.join(a.tmp, "out.zip")
    runs = []
    for rep in range(2):                              # the first run warms the page cache and the allocator
        saved = os.dup(1)
        null = os.open(os.devnull, os.O_WRONLY)
        sys.stdout.flush()
        os.dup2(null, 1)
        try:
            dt, phases, _ = bc.run("pulldown", "-p", "-U", up, fa, out, fq[0], fq[1])
        finally:
            sys.stdout.flush()
            os.dup2(saved, 1)
            os.close(saved)
            os.close(null)
        runs.append(dt)
    res["command"] = {"wall_s_cold": runs[0], "wall_s_warm": runs[1], "pairs_per_s_warm": R / runs[1], "phases_ms_warm": phases,
                      "archive_bytes": os.path.getsize(out)}
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    shutil.rmtree(a.tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
