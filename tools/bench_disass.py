#!/usr/bin/env python3
"""`zot disass` on an assembly-like input (run on the GPU box): the first G bases of the counter-based generator's genome cut
into contigs one after the other, once into a few long contigs and once into about 10^5 short ones, at K = 25 and both strands.
Per input:
  zk_contig_spectra        the whole device path of a batch, per stream byte and per window
  zk_kmerize               the yardstick for it on the same base stream (same binary): one sort of the same keys without a
                           payload, no second sort
  zk_count_spectrum        the file's histogram from the batch's counted key list
  zk_project_sum, shift 0  the yardstick for the run and reduce kernels, on the counted key list (arrays of the size the run
                           kernels read)
each (outputs preallocated): two warm-up calls, then `reps` calls timed on the host around a call that ends in a stream synchronise; min / median / max.
Then the command end to end on the FASTA file, twice (the second run warm), with the ZOT_TIMING=2 phases summed by name, and
the reference's loop (tests/_disass_restatement.py, one CPU core) over the first contigs.  -p 8 keeps every k-mer (the hash over
2^61 - 1 is below 8), so the spectra are those of all k-mers; the default -p 1.0 keeps an eighth.

    python3 tools/bench_disass.py [--bases G] [--reps R] [--out profiles/<round>/disass.json]
"""
import argparse, json, os, shutil, statistics, sys, time
os.environ.setdefault("ZOT_TIMING", "2")          # library/timing.py reads it at import
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_capture import genome_slice, run          # noqa: E402
from zotmer_amd import native                         # noqa: E402
from zotmer_amd.library import engine                 # noqa: E402

K, P = 25, 8.0


def timed(ctx, fn, reps):
    for _ in range(2):          # the first call sizes the workspace, the second runs in it
        r = fn()
        ctx.sync()
    ts = []
    for _ in range(reps):
        del r
        t0 = time.perf_counter()
        r = fn()
        ctx.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": min(ts), "median_ms": statistics.median(ts), "max_ms": max(ts)}, r


def write_fasta(path, G, n):
    """contig i = bases [i * G // n, (i + 1) * G // n) of the genome -> the base stream of the same records"""
    cuts = [i * G // n for i in range(n + 1)]
    g = genome_slice(0, G)
    with open(path, "wb") as f:
        for i in range(n):
            f.write(b">contig_%d\n%s\n" % (i, g[cuts[i]:cuts[i + 1]]))
    return b"".join(g[cuts[i]:cuts[i + 1]] + b"\n" for i in range(n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=float, default=20e6)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-bases", type=float, default=200e3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tmp", default="/tmp/zot_disass_bench")
    a = ap.parse_args()
    G = int(a.bases)
    shutil.rmtree(a.tmp, ignore_errors=True)
    os.makedirs(a.tmp)
    res = {"bases": G, "K": K, "p": P, "both_strands": True, "reps": a.reps, "lib": os.path.basename(native.LIB_PATH), "inputs": {}}
    ctx = engine.context()

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1, sort_keys=True)
                f.write("\n")

    for name, n in (("long_20_contigs", 20), ("short_1e5_contigs", 100_000)):
        fa = os.path.join(a.tmp, name + ".fa")
        stream_host = write_fasta(fa, G, n)
        d = ctx.upload_stream(stream_host)
        rec = {"contigs": n, "stream_bytes": d.n}
        bufs = (ctx.empty(d.n // 4, np.uint64), ctx.empty(d.n // 4, np.uint64), ctx.empty(d.n, np.uint64), ctx.empty(d.n, np.uint32))
        t, (words, freq, keys, counts, st) = timed(ctx, lambda: ctx.contig_spectra(d, K, True, 17, P, out=bufs), a.reps)
        rec.update(n_windows=int(st.n_windows), n_keys=int(st.n_keys), n_bins=int(st.n_bins))
        t["G_windows_per_s"] = st.n_windows / (t["median_ms"] * 1e-3) / 1e9
        t["stream_GB_per_s"] = d.n / (t["median_ms"] * 1e-3) / 1e9
        rec["zk_contig_spectra"] = t
        kbufs = (ctx.empty(2 * d.n, np.uint64), ctx.empty(2 * d.n, np.uint32))
        t, (kk, kc, _) = timed(ctx, lambda: ctx.kmerize(d, K, out=kbufs), a.reps)
        t["G_windows_per_s"] = st.n_windows / (t["median_ms"] * 1e-3) / 1e9
        rec["zk_kmerize"] = t
        rec["contig_spectra_over_kmerize"] = rec["zk_contig_spectra"]["median_ms"] / t["median_ms"]
        del kk, kc, kbufs
        t, glob = timed(ctx, lambda: ctx.count_spectrum(keys, counts, K, True, 17, P), a.reps)
        t["algorithmic_bytes"] = 12 * keys.n
        rec["zk_count_spectrum"] = t
        rec["global_bins"] = len(glob)
        t, _ = timed(ctx, lambda: ctx.project_sum(keys, counts, 0), a.reps)
        t["algorithmic_bytes"] = (12 + 16) * keys.n
        rec["zk_project_sum_shift0"] = t
        for v in (rec["zk_count_spectrum"], rec["zk_project_sum_shift0"]):
            v["GB_per_s_median"] = v["algorithmic_bytes"] / (v["median_ms"] * 1e-3) / 1e9
        rec["count_spectrum_over_project_sum"] = rec["zk_count_spectrum"]["median_ms"] / rec["zk_project_sum_shift0"]["median_ms"]
        del d, words, freq, keys, counts, bufs
        # the command end to end
        sink = os.path.join(a.tmp, "out.yaml")
        walls = []
        for rep in range(2):
            saved = os.dup(1)
            fd = os.open(sink, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
            sys.stdout.flush()
            os.dup2(fd, 1)
            try:
                dt, phases, _ = run("disass", "-k", K, "-p", repr(P), fa)
            finally:
                sys.stdout.flush()
                os.dup2(saved, 1)
                os.close(saved)
                os.close(fd)
            walls.append(dt)
        rec["command"] = {"wall_s_cold": walls[0], "wall_s_warm": walls[1], "phases_ms_warm": phases, "output_bytes": os.path.getsize(sink),
                          "device_phases_ms_warm": sum(phases.values())}
        res["inputs"][name] = rec
        print(name, json.dumps(rec), flush=True)
        save()
    # the reference's loop on one CPU core over the first bases of the short contigs
    from tests import _disass_restatement as R
    m = int(a.cpu_bases)
    text = "".join(">c%d\n%s\n" % (i, genome_slice(i * 200, 200).decode()) for i in range(m // 200))
    t0 = time.perf_counter()
    R.disass([("slice.fa", text)], K=K, P=P)
    dt = time.perf_counter() - t0
    res["restatement_one_core"] = {"bases": m, "contigs": m // 200, "seconds": dt, "bases_per_s": m / dt}
    print(json.dumps(res, indent=1, sort_keys=True))
    save()
    shutil.rmtree(a.tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
