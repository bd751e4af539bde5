#!/usr/bin/env python3
"""`zot hgvs-gen` on a synthetic genome (run on the GPU box).  One chromosome of `--bases` uniform bases (zotmer_amd/synth.py), a
BED file of `--zones` zones of 2000 bases spread over it, `--variants` variants at the default types and means.

  1. the two entries, in the batches the library cuts (hgvsgen.DRAW_BATCH variants a call): the zk_profile records of the draw
     pass with its scan, of the fill pass, of the size pass with its scan and of the write pass, summed over the batches of a
     run; the write pass in both forms that were tried -- tiles put together in LDS and stored 16 bytes wide, and every line
     written in place by its thread (ZK_HGVS_DIRECT) -- plain and -T, the forms alternated batch by batch; one warm-up run and
     `--reps` repetitions.  Algorithmic bytes of a write pass = 56 per row + the text written.
  2. the command end to end (library/hgvsgen.run behind its argument checks) into a file of a temporary directory, split into
     the zone tally, draw calls, render calls, D2H and file writing, plain and -T.
  3. the restatement of tests/_hgvsgen_restatement.py on one core on a slice, scaled to `--variants`: the CPU figure (the
     reference itself does not run on the GPU box).

    python3 tools/bench_hgvsgen.py [--variants N] [--zones Z] [--out profiles/<round>/hgvsgen.json]
"""
import argparse, json, os, shutil, statistics, sys, tempfile, time
os.environ.setdefault("ZOT_TIMING", "0")
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zotmer_amd import synth
from zotmer_amd.library import engine, hgvsgen, spikein

HBM_PEAK = 8.0e12
ZONE = 2000
FORMS = (("plain_lds", 0), ("plain_direct", 4), ("tab_lds", 1), ("tab_direct", 5))


def spread(ts):
    return {"min_ms": min(ts), "median_ms": statistics.median(ts), "max_ms": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=10000000)
    ap.add_argument("--zones", type=int, default=1000)
    ap.add_argument("--bases", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    seed, N = synth.DEFAULT_SEED, a.variants
    res = {"variants": N, "zones": a.zones, "bases": a.bases, "types": hgvsgen.DEFAULT_TYPES, "D": 1.5, "I": 1.5, "U": 3.0, "repetitions": a.reps,
           "draw_batch": hgvsgen.DRAW_BATCH}
    tmp = tempfile.mkdtemp(dir=a.tmp)
    try:
        seq = synth.reads_matrix(seed, 0, 1, a.bases).reshape(-1).tobytes().decode()
        with open(os.path.join(tmp, "chr1.fa"), "w") as f:
            f.write(">chr1\n" + seq + "\n")
        step = (a.bases - 2 * ZONE) // a.zones
        starts = [1000 + i * step for i in range(a.zones)]
        bed = "".join("chr1\t%d\t%d\tz%d\n" % (s, s + ZONE - 1, i) for i, s in enumerate(starts))
        with open(os.path.join(tmp, "zones.bed"), "w") as f:
            f.write(bed)
        t0 = time.perf_counter()
        plan = hgvsgen.make_plan(dict(bed=os.path.join(tmp, "zones.bed"), home=tmp, names=None, seed=seed, types=hgvsgen.DEFAULT_TYPES,
                                      D=1.5, I=1.5, U=3.0))
        res["plan_s"] = time.perf_counter() - t0
        ctx = engine.context()

        # 1. the kernels
        t0 = time.perf_counter()
        counts = spikein.zone_counts(ctx, plan, N)
        res["zone_counts_s"] = time.perf_counter() - t0
        assert int(counts.sum()) == N
        text, zones, first, accs, acc_offs, names, name_offs = (ctx.upload(x) for x in plan.device_tables(counts))
        geom_n = [len(t) for t in plan.tables]
        geom = ctx.upload(np.asarray(sum(plan.tables, []), dtype=np.uint64))
        RW, B = ctx.HGVS_ROW_WORDS, min(hgvsgen.DRAW_BATCH, N)
        rows, pool = ctx.empty(RW * B, np.uint64), ctx.empty(4 * B + 64, np.uint8)
        out = ctx.empty(160 * B + 4096, np.uint8)
        keys = ["draw", "fill"] + [k + "_" + f for f, _ in FORMS for k in ("size", "write")]
        runs = {k: [] for k in keys}
        written, pool_bytes, walls = {}, 0, []
        for rep in range(a.reps + 1):
            ms = dict.fromkeys(keys, 0.0)
            by = dict.fromkeys([f for f, _ in FORMS], 0)
            pool_bytes = 0
            t_run = time.perf_counter()
            for lo in range(0, N, B):
                n = min(B, N - lo)
                ctx.profile(True)
                got, fit = ctx.hgvs_draw_into(text, zones, first, plan.thr, geom, geom_n, plan.mix, seed, lo, n, rows, pool)
                p = ctx.profile_read()
                ctx.profile(False)
                assert fit and got[0] == n
                pool_bytes += got[1]
                ms["draw"] += p["hgvs_draw"]["ms"]; ms["fill"] += p["hgvs_fill"]["ms"]
                rv, pv = rows.view(RW * n), pool.view(got[1])
                for form, flags in FORMS:
                    ctx.profile(True)
                    nb, fit = ctx.hgvs_render_into(rv, pv, text, zones, accs, acc_offs, names, name_offs, first, lo, flags, out)
                    p = ctx.profile_read()
                    ctx.profile(False)
                    assert fit and p["hgvs_render"]["bytes"] == 56 * n + nb
                    ms["size_" + form] += p["hgvs_size"]["ms"]; ms["write_" + form] += p["hgvs_render"]["ms"]
                    by[form] += nb
            walls.append((time.perf_counter() - t_run) * 1e3)
            assert by["plain_lds"] == by["plain_direct"] and by["tab_lds"] == by["tab_direct"]
            written = by
            if rep:
                for k in keys:
                    runs[k].append(ms[k])
        k = {name: spread(ts) for name, ts in runs.items()}
        res["kernels"] = dict(k, pool_bytes=pool_bytes, text_bytes={"plain": written["plain_lds"], "tab": written["tab_lds"]},
                              all_forms_wall=spread(walls[1:]), window_text_bytes=text.n)
        for form, _ in FORMS:
            w = k["write_" + form]["median_ms"]
            nb = written[form]
            res["kernels"]["write_" + form].update(text_GB_per_s=nb / w / 1e6, algorithmic_GB_per_s=(56 * N + nb) / w / 1e6,
                                                   fraction_of_hbm_peak=(56 * N + nb) / (w * 1e-3) / HBM_PEAK)
        res["kernels"]["lds_over_direct"] = {"plain": k["write_plain_lds"]["median_ms"] / k["write_plain_direct"]["median_ms"],
                                             "tab": k["write_tab_lds"]["median_ms"] / k["write_tab_direct"]["median_ms"]}
        print("kernels", json.dumps(res["kernels"]), flush=True)
        del out, rows, pool

        # 3. the restatement on one core
        from tests import _hgvsgen_restatement as R
        n_small = 20000
        t0 = time.perf_counter()
        small = R.command(bed, {"chr1": seq}, seed, n_small, R.Params(), tab=True)
        t = time.perf_counter() - t0
        res["python_single_core"] = {"variants": n_small, "seconds": t, "microseconds_per_variant": t / n_small * 1e6,
                                     "scaled_to_the_variants_seconds": t / n_small * N, "form": "-T"}
        dev_ms = k["draw"]["median_ms"] + k["fill"]["median_ms"] + k["size_tab_lds"]["median_ms"] + k["write_tab_lds"]["median_ms"]
        res["python_over_kernels"] = res["python_single_core"]["scaled_to_the_variants_seconds"] / (dev_ms * 1e-3)

        # 2. the command end to end
        if not a.skip_e2e:
            e2e = {}
            for name, tab in (("plain", False), ("plain_warm", False), ("tab", True)):
                stats = hgvsgen.new_stats()
                path = os.path.join(tmp, name + ".txt")
                t0 = time.perf_counter()
                with open(path, "wb") as f:
                    hgvsgen.run(ctx, plan, N, f, tab=tab, stats=stats)
                e2e[name] = dict(stats, wall_s=time.perf_counter() - t0, file_bytes=os.path.getsize(path))
                print(name, json.dumps(e2e[name]), flush=True)
            stats = hgvsgen.new_stats()
            with open(os.path.join(tmp, "small.txt"), "wb") as f:
                hgvsgen.run(ctx, plan, n_small, f, tab=True, stats=stats)
            with open(os.path.join(tmp, "small.txt")) as f:
                assert f.read() == small                    # the device and the restatement agree on the slice
            res["end_to_end"] = e2e
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
