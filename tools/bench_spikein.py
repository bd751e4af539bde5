#!/usr/bin/env python3
"""`zot spikein` on a synthetic genome (run on the GPU box).  One chromosome of `--bases` uniform bases (zotmer_amd/synth.py), a
BED file of `--zones` zones of 2000 bases spread over it, a substitution in every 50th zone, default options.

  1. zk_spike_pairs on `--pairs` pairs in one call: the zk_profile records of the write pass (algorithmic bytes = the two texts
     written) and of the size pass with its two scans, one warm-up and `--reps` repetitions.
  2. the command end to end (library/spikein.run behind its argument checks) into a temporary directory, split into kernel
     calls, D2H and file writing, plain and with -z (the -z run on a quarter of the pairs: it is bounded by deflate).
  3. the restatement of tests/_spikein_restatement.py on one core, per pair, scaled to `--pairs`: the CPU figure (the reference
     itself does not run on the GPU box).

    python3 tools/bench_spikein.py [--pairs N] [--zones Z] [--out profiles/<round>/spikein.json]
"""
import argparse, json, os, shutil, statistics, sys, tempfile, time
os.environ.setdefault("ZOT_TIMING", "0")
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zotmer_amd import synth
from zotmer_amd.library import engine, spikein

HBM_PEAK = 8.0e12
ZONE = 2000


def spread(ts):
    return {"min_ms": min(ts), "median_ms": statistics.median(ts), "max_ms": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--zones", type=int, default=1000)
    ap.add_argument("--bases", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    seed, L, I, D, E, V = synth.DEFAULT_SEED, 100, 300, 0.1, 0.005, 1.0
    res = {"pairs": a.pairs, "zones": a.zones, "bases": a.bases, "L": L, "I": I, "D": D, "E": E, "V": V, "repetitions": a.reps}
    tmp = tempfile.mkdtemp(dir=a.tmp)
    try:
        seq = synth.reads_matrix(seed, 0, 1, a.bases).reshape(-1).tobytes().decode()
        with open(os.path.join(tmp, "chr1.fa"), "w") as f:
            f.write(">chr1\n" + seq + "\n")
        step = (a.bases - 2 * ZONE) // a.zones
        starts = [1000 + i * step for i in range(a.zones)]
        with open(os.path.join(tmp, "zones.bed"), "w") as f:
            f.write("".join("chr1\t%d\t%d\tz%d\n" % (s, s + ZONE - 1, i) for i, s in enumerate(starts)))
        variants = []
        for s in starts[::50]:
            c = seq[s + 999]
            variants.append("chr1:g.%d%s>%s" % (s + 1000, c, "ACGT"[("ACGT".index(c) + 1) & 3]))
        t0 = time.perf_counter()
        plan = spikein.make_plan(dict(bed=os.path.join(tmp, "zones.bed"), home=tmp, names=None, file=None, pop=None, seed=seed, L=L, I=I, D=D),
                                 variants)
        res["plan_s"] = time.perf_counter() - t0
        ctx = engine.context()

        # 1. the kernels
        t0 = time.perf_counter()
        counts = spikein.zone_counts(ctx, plan, a.pairs)
        res["zone_counts_s"] = time.perf_counter() - t0
        assert int(counts.sum()) == a.pairs
        dev = [ctx.upload(x) for x in plan.tables(counts)]
        res["window_text_bytes"] = dev[0].n
        scal = (seed, L, I, plan.sd_q, synth.frac32(V), synth.frac32(E))
        nb, fit = ctx.spike_pairs_into(*dev, *scal, 0, a.pairs, ctx.empty(0, np.uint8), ctx.empty(0, np.uint8))
        assert not fit
        outs = (ctx.empty(nb[0], np.uint8), ctx.empty(nb[1], np.uint8))
        tw, ts, walls = [], [], []
        for rep in range(a.reps + 1):
            ctx.profile(True)
            t0 = time.perf_counter()
            got, fit = ctx.spike_pairs_into(*dev, *scal, 0, a.pairs, *outs)
            wall = time.perf_counter() - t0
            p = ctx.profile_read()
            ctx.profile(False)
            assert fit and got == nb and p["spike_pairs"]["bytes"] == sum(nb)
            if rep:
                tw.append(p["spike_pairs"]["ms"]); ts.append(p["spike_size"]["ms"]); walls.append(wall * 1e3)
        w, s = spread(tw), spread(ts)
        res["spike_pairs"] = {"bytes_written": sum(nb), "write_pass": w, "size_pass_and_scans": s, "call_wall": spread(walls),
                              "write_pass_GB_per_s": sum(nb) / w["median_ms"] / 1e6,
                              "write_pass_fraction_of_hbm_peak": sum(nb) / (w["median_ms"] * 1e-3) / HBM_PEAK,
                              "size_and_scan_share_of_kernel_time": s["median_ms"] / (s["median_ms"] + w["median_ms"])}
        print("spike_pairs", json.dumps(res["spike_pairs"]), flush=True)
        head = outs[0].to_host(4096).tobytes().decode("latin-1")

        # 3. the restatement on one core
        sys.path.insert(0, ROOT)
        from tests import _spikein_restatement as R
        n_small = 2000
        ch, zone, wt, mut = plan.zones[0]
        zs = [(spikein.head_prefix(ch, zone), n_small, [(wt.flat(), wt.s0, wt.e0), (mut.flat(), mut.s0, mut.e0)])]
        t0 = time.perf_counter()
        R.record_list(seed, L, I, plan.sd_q, synth.frac32(V), synth.frac32(E), zs)
        t = time.perf_counter() - t0
        res["python_single_core"] = {"pairs": n_small, "seconds": t, "microseconds_per_pair": t / n_small * 1e6,
                                     "scaled_to_the_pairs_seconds": t / n_small * a.pairs}
        res["python_over_kernels"] = res["python_single_core"]["scaled_to_the_pairs_seconds"] / ((s["median_ms"] + w["median_ms"]) * 1e-3)
        del outs

        # 2. the command end to end
        if not a.skip_e2e:
            runs = {}
            for name, z, n in (("plain", False, a.pairs), ("warm", False, a.pairs), ("gzip", True, a.pairs // 4)):
                stats = spikein.new_stats()
                t0 = time.perf_counter()
                spikein.run(ctx, plan, n, V, E, os.path.join(tmp, name), z=z, stats=stats)
                runs[name] = dict(stats, wall_s=time.perf_counter() - t0,
                                  file_bytes=sum(os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp) if f.startswith(name + "_")))
                print(name, json.dumps(runs[name]), flush=True)
            with open(os.path.join(tmp, "plain_1.fastq"), "rb") as f:
                assert f.read(4096).decode("latin-1") == head
            res["end_to_end"] = runs
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
