#!/usr/bin/env python3
"""The stages of `zot contigs` at BASELINE config 3's size on one MI355X (run on the GPU box).

Two sets:
  random     N = 100 M draws of 32-bit keys (K = 16: about 98.8 M distinct keys; zk_synth_keys walks one pool).  2.3 % of all
             16-mers: most k-mers have no successor, nearly every node is a path of its own;
  genome     the k-mers (K = 25, both strands) of error-free 150-base reads over a synthetic genome (zk_synth_reads +
             zk_kmerize): the graph of an assembly, long non-branching paths.
Per set:
  zk_debruijn_links   algorithmic bytes: 8 read + 8 written per k-mer; the successor and the rank kernels' own times (HIP
                      events) beside it.  Yardstick: zk_split of the array with itself (8 per entry read, twice)
  the copy of the links to the host
  zk_contig_walk      host, ms and ns per node, at the default -l and at -l 1 (everything kept)
  zk_contig_render    at -l 1: bytes written
Every device figure: two warm-up calls, then `reps` calls timed on the host around a call that ends in a stream synchronise;
min / median / max are printed, GB/s from the median.
--e2e writes the genome set as a set file and runs the command on it with ZOT_TIMING=2.

Usage: tools/bench_contigs.py [--scale F] [--reps R] [--e2e DIR] [--out FILE]      prints one JSON object
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
from bench_vars import rate, run_command, timed          # noqa: E402


def host_timed(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(ms_min=min(ts), ms_median=statistics.median(ts), ms_max=max(ts)), r


def stages(ctx, kmers, K, reps):
    n = kmers.n
    rec = {"n": n, "K": K}
    t, _ = timed(ctx, lambda: ctx.split(kmers, kmers), reps)
    rec["split_with_itself"] = rate(t, 16 * n)
    nx, rc = ctx.empty(n, np.uint32), ctx.empty(n, np.uint32)
    t, _ = timed(ctx, lambda: ctx.debruijn_links(kmers, K, out=(nx, rc)), reps)
    rec["links"] = rate(t, 16 * n)
    rec["links"]["ratio_to_split"] = t["ms_median"] / rec["split_with_itself"]["ms_median"]
    ctx.profile(True)
    ctx.debruijn_links(kmers, K, out=(nx, rc))
    ctx.sync()
    p = ctx.profile_read()
    ctx.profile(False)
    rec["links"]["next_kernel_ms"] = p["links"]["ms"] / p["links"]["launches"]
    rec["links"]["rc_kernel_ms"] = p["links_rc"]["ms"] / p["links_rc"]["launches"]
    t, (h_next, h_rc) = host_timed(lambda: (nx.to_host(), rc.to_host()), 3)
    rec["links_to_host"] = rate(t, 8 * n)
    rec["linked_share"] = float((h_next != native.NO_LINK).mean())
    del nx, rc
    for name, ml in (("walk_default_l", 2 * K), ("walk_l_1", 1)):
        t, (nodes, offs) = host_timed(lambda: native.contig_walk(h_next, h_rc, K, ml), 3)
        t.update(ns_per_node=t["ms_median"] * 1e6 / n, nodes_kept=int(len(nodes)), contigs=int(len(offs) - 1),
                 longest=int(np.diff(offs).max()) if len(offs) > 1 else 0)
        rec[name] = t
    d_nodes, d_offs = ctx.upload(nodes, np.uint32), ctx.upload(offs, np.uint64)
    out = ctx.empty(len(nodes) + (len(offs) - 1) * (K + 19), np.uint8)
    t, text = timed(ctx, lambda: ctx.contig_render(kmers, K, d_nodes, d_offs, out=out), reps)
    rec["render_l_1"] = rate(t, 12 * len(nodes) + 16 * (len(offs) - 1) + text.n)
    rec["render_l_1"]["bytes_written"] = text.n
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--e2e")
    ap.add_argument("--out")
    a = ap.parse_args()
    out = {"reps": a.reps, "scale": a.scale}

    def emit():
        text = json.dumps(out, indent=1, sort_keys=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return text

    from zotmer_amd.library import engine
    ctx = engine.context()
    k, _ = ctx.synth_set(11, 0, int(100_000_000 * a.scale), 32, counts=False)
    out["random"] = stages(ctx, k, 16, a.reps)
    del k
    emit()
    reads, genome = int(4_000_000 * a.scale), int(40_000_000 * a.scale)
    d = ctx.synth_reads(synth.DEFAULT_SEED, 0, reads, 150, genome=genome, sub_thr=0, n_thr=0)
    gk, gc, _ = ctx.kmerize(d, 25)
    del d
    gk, gc = ctx.copy_of(gk), ctx.widen(gc)
    out["genome"] = dict(stages(ctx, gk, 25, a.reps), reads=reads, genome=genome)
    emit()
    if a.e2e:
        from zotmer_amd.library import vectors
        from zotmer_amd.library.container import KmerSet
        os.makedirs(a.e2e, exist_ok=True)
        path = os.path.join(a.e2e, "genome.k25")
        with KmerSet(path, "w") as z:
            vectors.device_write_kmers_and_counts(ctx, z, gk, gc)
            z.meta.update({"K": 25, "kmers": "kmers", "counts": "counts"})
        dt, lines, phases, other = run_command(["contigs", path])
        out["command"] = dict(seconds=dt, lines=lines, phases_ms=phases, stderr=other[:4], set_bytes=os.path.getsize(path))
        os.remove(path)
    print(emit())
    engine.close()


if __name__ == "__main__":
    main()
