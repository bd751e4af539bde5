#!/usr/bin/env python3
"""The kernel behind `zot vars -r` at BASELINE config 3's size on one MI355X (run on the GPU box).

A reference list of N = 100 M draws of 32-bit keys (K = 16: about 98.8 M distinct keys, 3.4 % of their groups hold 2 or more
bases; zk_synth_keys walks one pool, zk_synth_counts gives geometric 64-bit counts of mean 8) against three samples:
  same       the reference's own keys and counts: every base sits exactly on its expectation, no row      (the join alone)
  redrawn    the reference's keys, the counts drawn again with another seed: rows are rare
  missing    the walk started N / 100 later with redrawn counts: about 1 % of the sample's contexts are not in the reference
  zk_vars_scan      algorithmic bytes: 16 per entry of both lists read, 72 per row written
and as yardsticks on the same arrays zk_split (8 per entry read) and zk_union_sum with 64-bit counts (16 per entry read, 16
per entry of the union written).  Every figure: two warm-up calls, then `reps` calls timed on the host around a call that ends
in a stream synchronise; min / median / max are printed, GB/s from the median.  The kernel's own time (HIP events) is beside it.

Per mix the share of candidate bases that the exact tail does not flag, on the first `--rows` rows (host evaluation).
--e2e writes the reference and the `redrawn` sample as set files and runs the command on them with ZOT_TIMING=2.

Usage: tools/bench_vars.py [--scale F] [--reps R] [--rows M] [--e2e DIR] [--out FILE]      prints one JSON object
"""
import argparse
import io
import json
import os
import re
import statistics
import sys
import tempfile
import time

os.environ.setdefault("ZOT_TIMING", "2")          # library/timing.py reads it at import
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zotmer_amd import native          # noqa: E402
from zotmer_amd.library import varscan          # noqa: E402

K, KEY_BITS = 16, 32


def timed(ctx, f, reps):
    for _ in range(2):
        r = f()
        ctx.sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        ctx.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(ms_min=min(ts), ms_median=statistics.median(ts), ms_max=max(ts)), r


def rate(rec, nbytes):
    rec["algorithmic_bytes"] = int(nbytes)
    rec["GBps"] = nbytes / (rec["ms_median"] * 1e-3) / 1e9
    return rec


def predicate_share(ctxs, rows, limit):
    """of the candidate bases of the first `limit` rows: how many the exact tail flags"""
    r = rows.to_host(8 * min(limit, ctxs.n)).reshape(-1, 8).tolist()
    cand = flagged = printed = 0
    for row in r:
        sx, gx = row[:4], row[4:]
        b, _ = varscan.eval_row(sx, gx)
        printed += b > 0
        st, gt = sum(sx), sum(gx)
        for j in range(4):
            cand += varscan.candidate(sx[j], st, gx[j], gt, guards=1.0)
            flagged += (b >> j) & 1
    return dict(rows_evaluated=len(r), rows_printed=printed, candidate_bases=cand, flagged_bases=flagged,
                candidates_not_flagged_share=(cand - flagged) / cand if cand else 0.0)


def run_command(argv):
    """-> (seconds, lines of stdout, the [engine] phase lines of ZOT_TIMING=2 summed by phase name, in ms, other stderr lines)"""
    from contextlib import redirect_stdout
    from zotmer_amd import cli
    t0 = time.perf_counter()
    buf = io.StringIO()
    err = tempfile.TemporaryFile(mode="w+")
    saved = os.dup(2)
    os.dup2(err.fileno(), 2)
    try:
        with redirect_stdout(buf):
            cli.main_inner(argv)
    finally:
        sys.stderr.flush()
        os.dup2(saved, 2)
        os.close(saved)
    dt = time.perf_counter() - t0
    err.seek(0)
    phases, other = {}, []
    for line in err.read().splitlines():
        m = re.match(r"\s*\[engine\] (.+?)\s+([\d.]+) ms", line)
        if m:
            phases[m.group(1)] = phases.get(m.group(1), 0.0) + float(m.group(2))
        else:
            other.append(line)
    return dt, buf.getvalue().count("\n"), phases, other


def write_set(ctx, path, k, c):
    from zotmer_amd.library import vectors
    from zotmer_amd.library.container import KmerSet
    with KmerSet(path, "w") as z:
        vectors.device_write_kmers_and_counts(ctx, z, k, c)
        z.meta.update({"K": K, "kmers": "kmers", "counts": "counts"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--e2e")
    ap.add_argument("--out")
    a = ap.parse_args()
    N = int(100_000_000 * a.scale)
    out = {"draws_per_list": N, "reps": a.reps, "K": K}

    def emit():
        text = json.dumps(out, indent=1, sort_keys=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return text

    from zotmer_amd.library import engine
    ctx = engine.context()
    rk, rc = ctx.synth_set(11, 0, N, KEY_BITS)
    out["n_ref"] = rk.n
    samples = {}
    samples["same"] = (rk, rc)
    c2 = ctx.empty(rk.n, np.uint64)
    ctx._check(ctx.lib.zk_synth_counts(ctx.h, 12, rk.ptr, rk.n, c2.ptr))
    samples["redrawn"] = (rk, c2)
    mk, _ = ctx.synth_set(11, N // 100, N, KEY_BITS, counts=False)
    mc = ctx.empty(mk.n, np.uint64)
    ctx._check(ctx.lib.zk_synth_counts(ctx.h, 12, mk.ptr, mk.n, mc.ptr))
    samples["missing"] = (mk, mc)
    n2 = 2 * rk.n
    t, abc = timed(ctx, lambda: ctx.split(rk, samples["missing"][0]), a.reps)
    out["split"] = rate(t, 8 * (rk.n + samples["missing"][0].n))
    ok, oc = ctx.empty(n2, np.uint64), ctx.empty(n2, np.uint64)
    t, r = timed(ctx, lambda: ctx.union_sum(rk, rc, samples["missing"][0], samples["missing"][1], out=(ok, oc)), a.reps)
    out["union_sum_u64"] = rate(t, 16 * (rk.n + samples["missing"][0].n) + 16 * r[0].n)
    del ok, oc, r
    emit()
    for name, (sk, sc) in samples.items():
        t, r = timed(ctx, lambda: ctx.vars_scan(rk, rc, sk, sc, K, cap_rows=1 << 22), a.reps)
        ctxs, rows, st = r
        rec = rate(t, 16 * (rk.n + sk.n) + 72 * st.n_rows)
        rec.update(n_sam=sk.n, n_groups=st.n_groups, n_missing=st.n_missing, n_mixed=st.n_mixed, n_rows=st.n_rows,
                   mixed_share=st.n_mixed / max(1, st.n_groups - st.n_missing))
        ctx.profile(True)
        ctx.vars_scan(rk, rc, sk, sc, K, cap_rows=1 << 22)
        ctx.sync()
        p = ctx.profile_read().get("vars_scan")
        ctx.profile(False)
        if p:
            rec["join_kernel_ms"] = p["ms"] / p["launches"]
        rec["predicate"] = predicate_share(ctxs, rows, a.rows)
        out["vars_scan_" + name] = rec
        del ctxs, rows, r
        emit()
    u = out["union_sum_u64"]
    out["scan_no_slower_than_union_sum"] = bool(out["vars_scan_missing"]["ms_median"] <= u["ms_median"] + (u["ms_max"] - u["ms_min"]))
    if a.e2e:
        os.makedirs(a.e2e, exist_ok=True)
        ref, sam = os.path.join(a.e2e, "ref.k16"), os.path.join(a.e2e, "sam.k16")
        write_set(ctx, ref, rk, rc)
        write_set(ctx, sam, *samples["redrawn"])
        dt, lines, phases, other = run_command(["vars", "-r", ref, sam])
        out["command"] = dict(seconds=dt, lines=lines, phases_ms=phases, stderr=other[:4],
                              set_bytes=[os.path.getsize(ref), os.path.getsize(sam)])
        os.remove(ref)
        os.remove(sam)
    print(emit())
    engine.close()


if __name__ == "__main__":
    main()
