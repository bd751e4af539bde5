#!/usr/bin/env python3
"""`zot scan` on a synthetic gene index (run on the GPU box): G records x LEN bases of zotmer_amd/synth.py's uniform sequences
indexed as `zot scan -X` does, and a sample that holds every record with substitutions at rate SUB plus R background reads,
k-merized on the device.  Records:

  * zk_lcp_resolve, zk_scan_place (with the read-back of P, Q and cnt) and the per-record host stage, each on its own: one
    warm-up and `--reps` repetitions of the two device stages (min / median / max), one run of the host stage;
  * the single-core restatement of the reference's resolveAll (scan.py:95-120) in plain Python on the same two lists, once,
    and that its L and Y equal the device's;
  * the zk_profile records of one resolve and one placement;
  * zk_lcp_resolve on the degenerate input of include/zotk.h -- a sample of two elements around an index of `--degenerate`
    k-mers that all begin with A -- where a walk without the stepping over tiles would be quadratic.

    python3 tools/bench_scan.py [--genes G] [--length LEN] [--background R] [--out profiles/<round>/scan.json]
"""
import argparse, io, json, os, statistics, sys, time
os.environ.setdefault("ZOT_TIMING", "0")
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zotmer_amd import synth
from zotmer_amd.library import engine, genescan

K = genescan.K_INDEX


def spread(ts):
    return {"min_ms": min(ts) * 1e3, "median_ms": statistics.median(ts) * 1e3, "max_ms": max(ts) * 1e3}


def lcp(x, y):
    z = x ^ y
    return K if z == 0 else K - (1 + (z.bit_length() - 1) // 2)


def resolve_all_cpu(S, X):
    """scan.py:95-120 on Python lists"""
    Z = len(S)
    L, Y = [0] * Z, [0] * Z
    i = 0
    for x in X:
        while i < Z and S[i] <= x:
            l = lcp(x, S[i])
            if l > L[i]:
                L[i], Y[i] = l, x
            i += 1
    while i < Z:
        l = lcp(x, S[i])
        if l > L[i]:
            L[i], Y[i] = l, x
        i += 1
    changed = 0
    for i in range(1, Z):
        x = Y[i - 1]
        l = lcp(x, S[i])
        if l > L[i]:
            L[i], Y[i] = l, x
            changed += 1
    return L, Y, changed


def timed(ctx, fn, reps):
    ts, r = [], None
    for rep in range(reps + 1):          # rep 0 warms the workspace
        ctx.sync()
        t0 = time.perf_counter()
        r = fn()
        ctx.sync()
        if rep:
            ts.append(time.perf_counter() - t0)
    return spread(ts), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=300)
    ap.add_argument("--length", type=int, default=1000)
    ap.add_argument("--background", type=int, default=20000, help="background reads of 150 bases in the sample")
    ap.add_argument("--sub", type=float, default=0.005)
    ap.add_argument("--degenerate", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    seed = synth.DEFAULT_SEED
    genes = synth.reads_matrix(seed, 0, a.genes, a.length)
    t0 = time.perf_counter()
    meta, arrays = genescan.index_build([("gene_%d" % i, bytes(r)) for i, r in enumerate(genes)])
    t_index = time.perf_counter() - t0
    res = {"K": K, "genes": a.genes, "gene_length": a.length, "index_kmers": len(arrays["S"]), "index_entries": len(arrays["U"]),
           "index_build_host_ms": t_index * 1e3, "substitution_rate": a.sub, "background_reads": a.background, "repetitions": a.reps}

    # the sample: every gene with substitutions, and background reads; k-merized on the device
    idx = np.arange(genes.size, dtype=np.uint64).reshape(genes.shape)
    hit = (synth.rnd(seed, 11, idx) & np.uint64(0xFFFFFFFF)) < np.uint64(synth.frac32(a.sub))
    code = np.searchsorted(np.frombuffer(b"ACGT", np.uint8), genes).astype(np.uint64)
    alt = (code + np.uint64(1) + synth.rnd(seed, 12, idx) % np.uint64(3)) & np.uint64(3)
    sample = np.where(hit, np.frombuffer(b"ACGT", np.uint8)[alt.astype(np.intp)], genes)
    rows = np.full((a.genes, a.length + 1), ord("\n"), np.uint8)
    rows[:, :a.length] = sample
    stream = np.concatenate((rows.reshape(-1), synth.base_stream(seed, 1 << 20, a.background, 150)))
    ctx = engine.context()
    X, _, st = ctx.kmerize(ctx.upload_stream(stream), K)
    X = ctx.copy_of(X)
    tot = float(sum(list(st.acgt)))
    sacgt = [c / tot for c in list(st.acgt)]
    res["sample_kmers"] = X.n

    index = genescan.DeviceIndex(ctx, meta, arrays)
    res["resolve"], (L, Y) = timed(ctx, lambda: ctx.lcp_resolve(index.S, X, K), a.reps)
    res["place"], (P, Q, cnt) = timed(ctx, lambda: tuple(v.to_host() for v in ctx.scan_place(L, Y, index.T, index.U, index.V, index.d_off,
                                                                                             index.n_slots, K)), a.reps)
    ctx.profile(True)
    ctx.lcp_resolve(index.S, X, K)
    ctx.scan_place(L, Y, index.T, index.U, index.V, index.d_off, index.n_slots, K)
    prof = ctx.profile_read()
    ctx.profile(False)
    res["kernels"] = {k: prof[k] for k in ("lcp_resolve", "scan_place")}
    print("device", json.dumps({k: res[k] for k in ("index_kmers", "sample_kmers", "resolve", "place", "kernels")}), flush=True)

    Xh = X.to_host()
    t0 = time.perf_counter()
    lines = genescan.sample_lines(meta, sacgt, P, Q, cnt.reshape(a.genes, K + 1), index.rec_off, Xh, "sample", io.StringIO())
    res["host_stage_ms"] = (time.perf_counter() - t0) * 1e3
    res["lines"] = len(lines)

    Sl, Xl = arrays["S"].tolist(), Xh.tolist()
    t0 = time.perf_counter()
    Lc, Yc, changed = resolve_all_cpu(Sl, Xl)
    res["resolve_all_python_single_core_ms"] = (time.perf_counter() - t0) * 1e3
    assert Lc == L.to_host().tolist() and Yc == Y.to_host().tolist(), "the device and the restatement of resolveAll differ"
    Ld = np.array(Lc)
    res["entries_changed_by_pass_2"] = changed
    res["L_histogram"] = {str(int(v)): int(c) for v, c in zip(*np.unique(Ld, return_counts=True))}
    res["python_over_device_resolve"] = res["resolve_all_python_single_core_ms"] / res["resolve"]["median_ms"]

    # the degenerate input: everything begins with A, pass 1 leaves (0, 0), the carried 0 matches the leading A's
    n = a.degenerate
    Sd = ctx.upload(np.arange(1, n + 1, dtype=np.uint64) * np.uint64(3))
    Xd = ctx.upload(np.array([0, (3 << (2 * K - 2)) | 5], dtype=np.uint64))
    res["degenerate"] = {"index_kmers": n, "sample_kmers": 2}
    res["degenerate"]["resolve"], (Ld_, Yd_) = timed(ctx, lambda: ctx.lcp_resolve(Sd, Xd, K), a.reps)
    assert not Yd_.to_host().any() and int(Ld_.to_host()[1:].min()) >= K - 11
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
