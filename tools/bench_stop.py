#!/usr/bin/env python3
"""`zot stop` on a synthetic transcriptome (run on the GPU box): T transcripts of 2 to 4 kb of random bases, R reads x 150 bp cut
from them in either orientation with 1 % substituted bases.  Records:

  kernels      zk_profile's records (device events) of zk_stop_frames (the pick kernel, the emit kernel) beside zk_anchor_pileup's
               lookup-and-emit kernel on the same reads and the same table, `--kernel-reads` of them in one batch: two warm-ups,
               then `--reps` alternated repetitions, every one listed, medians, and the ratio of the medians.  Both kernels look
               every window of both orientations up (dependent random 8-byte reads); the pile-up then writes 12 B per
               (diagonal, window), the stop kernel bisects only where a read has several frames and writes 16 B per read.
  nearest      zk_stop_nearest on the command's counted list: entries, pair tests (entries x distinct k-mers of their
               transcripts), `--reps` repetitions after a warm-up, the median and pair tests per second
  command      wall time of the library's own path (the index, the table, the batches, the nearest pass, the lines): one warm
               run, then three timed, every one listed with its stages, the median
  reference    the single-core time of the CPU restatement (tests/_stop_restatement.py) on the first `--cpu-reads` reads, scaled

    python3 tools/bench_stop.py [--reads R] [--transcripts T] [--out profiles/<round>/stop.json]
"""
import argparse
import io
import json
import os
import shutil
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                     # noqa: E402
from zotmer_amd.library import alufinder, engine, stopscan             # noqa: E402

K, L, SEED = 27, 150, 17
T0 = time.perf_counter()


def note(msg):
    sys.stderr.write("[%7.1f s] %s\n" % (time.perf_counter() - T0, msg))
    sys.stderr.flush()


def transcripts(T, rng):
    lens = rng.integers(2000, 4001, size=T)
    return [rng.integers(0, 4, size=int(n), dtype=np.uint8) for n in lens]


def write_inputs(tmp, T, R, rng):
    """tx.fa and reads.fastq -> (paths, bytes of the FASTQ)"""
    tx = transcripts(T, rng)
    letters = np.frombuffer(b"ACGT", np.uint8)
    fa = os.path.join(tmp, "tx.fa")
    with open(fa, "wb") as f:
        for i, codes in enumerate(tx):
            f.write(b">tx%05d\n" % i + letters[codes].tobytes() + b"\n")
    flat = np.concatenate(tx)
    starts = np.concatenate(([0], np.cumsum([len(c) for c in tx])))[:-1]
    lens = np.array([len(c) for c in tx])
    fq = os.path.join(tmp, "reads.fastq")
    with open(fq, "wb") as f:
        step = 500_000
        for a in range(0, R, step):
            m = min(step, R - a)
            t = rng.integers(0, T, size=m)
            p = (rng.random(m) * (lens[t] - L + 1)).astype(np.int64) + starts[t]
            codes = flat[p[:, None] + np.arange(L)[None, :]]
            sub = rng.random((m, L)) < 0.01
            codes = np.where(sub, (codes + rng.integers(1, 4, size=(m, L), dtype=np.uint8)) & 3, codes).astype(np.uint8)
            rev = rng.random(m) < 0.5
            codes[rev] = 3 - codes[rev][:, ::-1]
            rec = np.empty((m, 13 + (L + 1) + 2 + (L + 1)), dtype=np.uint8)
            rec[:, 0] = ord("@"); rec[:, 1] = ord("r")
            rec[:, 2:12] = np.frombuffer("".join(np.char.zfill(np.arange(a, a + m).astype(str), 10)).encode(), np.uint8).reshape(m, 10)
            rec[:, 12] = ord("\n")
            rec[:, 13:13 + L] = letters[codes]
            rec[:, 13 + L] = ord("\n")
            rec[:, 14 + L] = ord("+"); rec[:, 15 + L] = ord("\n")
            rec[:, 16 + L:16 + 2 * L] = ord("I"); rec[:, 16 + 2 * L] = ord("\n")
            f.write(rec.tobytes())
    return fa, fq, os.path.getsize(fq)


def head_text(path, n_records):
    out = []
    with open(path) as f:
        for _ in range(4 * n_records):
            out.append(f.readline())
    return "".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=2e6)
    ap.add_argument("--transcripts", type=int, default=1000)
    ap.add_argument("--kernel-reads", type=int, default=500_000)
    ap.add_argument("--cpu-reads", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tmp", default="/tmp/zot_stop_bench")
    a = ap.parse_args()
    R, T = int(a.reads), a.transcripts
    shutil.rmtree(a.tmp, ignore_errors=True)
    os.makedirs(a.tmp)
    rng = np.random.default_rng(24)
    fa, fq, fq_bytes = write_inputs(a.tmp, T, R, rng)
    note("inputs written")
    ctx = engine.context()
    out = dict(reads=R, transcripts=T, K=K, read_length=L, seed=SEED, fastq_bytes=fq_bytes, substitutions=0.01)

    # ---- the two lookup kernels on the same reads and the same table -------------------------------------------------------------
    index = stopscan.load_index(fa, K)
    layout = stopscan.layout_of(index)
    table = stopscan.anchor_table(ctx, index, layout)
    starts = ctx.upload(stopscan.starts_of(layout))
    n = min(a.kernel_reads, R)
    text = ctx.upload(np.frombuffer(head_text(fq, n).encode(), dtype=np.uint8))
    lines = ctx.line_ends(text)
    bufs_s = bufs_p = None
    rec = dict(stop_frames=[], stop_emit=[], pileup=[])
    for rep in range(2 + a.reps):
        ctx.profile(True)
        tx, km = ctx.stop_frames(table, starts, text, lines, n, K, layout.pad, SEED, 0, out=bufs_s)
        ps = ctx.profile_read()
        ctx.profile(True)
        pc, pk = ctx.anchor_pileup(table, text, lines, n, K, layout.pad, out=bufs_p)
        pp = ctx.profile_read()
        ctx.profile(False)
        bufs_s, bufs_p = (alufinder.whole(tx), alufinder.whole(km)), (alufinder.whole(pc), alufinder.whole(pk))
        if rep >= 2:
            rec["stop_frames"].append(ps["stop_frames"]["ms"])
            rec["stop_emit"].append(ps["stop_emit"]["ms"])
            rec["pileup"].append(pp["pileup"]["ms"])
    med = {k: statistics.median(v) for k, v in rec.items()}
    windows = 2 * n * (L - K + 1)
    out["kernels"] = dict(reads=n, lookups=windows, stops=tx.n, pileup_pairs=pc.n, ms=rec, median_ms=med,
                          stop_frames_over_pileup=med["stop_frames"] / med["pileup"],
                          stop_frames_and_emit_over_pileup=(med["stop_frames"] + med["stop_emit"]) / med["pileup"],
                          G_lookups_per_s=dict(stop_frames=windows / (med["stop_frames"] * 1e-3) / 1e9, pileup=windows / (med["pileup"] * 1e-3) / 1e9),
                          text_bytes=ps["stop_frames"]["bytes"] - 16 * n,
                          stop_frames_text_GBps=(ps["stop_frames"]["bytes"] - 16 * n) / (med["stop_frames"] * 1e-3) / 1e9)
    note("kernels measured")
    del text, lines, bufs_s, bufs_p, tx, km, pc, pk
    table.free()

    # ---- the command ----------------------------------------------------------------------------------------------------------------
    from zotmer_amd.commands.capture import capture_batch_bytes
    batch = capture_batch_bytes(ctx)
    out["batch_bytes"] = batch

    def command():
        stats = {}
        t0 = time.perf_counter()
        idx = stopscan.load_index(fa, K)
        t1 = time.perf_counter()
        sink = io.StringIO()
        stopscan.run(ctx, idx, [fq], SEED, batch, sink, stats=stats)
        stats.update(seconds=time.perf_counter() - t0, index_seconds=t1 - t0, lines_printed=sink.getvalue().count("\n"))
        return stats

    command()                                     # warm: the workspace, the file cache
    note("command warm")
    runs = [command() for _ in range(3)]
    note("command timed")
    runs.sort(key=lambda s: s["seconds"])
    out["command"] = dict(runs=runs, median=runs[1], fastq_MBps=fq_bytes / runs[1]["seconds"] / 1e6)

    # ---- zk_stop_nearest on the command's counted list -------------------------------------------------------------------------------
    pile = alufinder.Pileup()
    table = stopscan.anchor_table(ctx, index, layout)
    stopscan.scan_inputs(ctx, table, ctx.upload(stopscan.starts_of(layout)), K, layout.pad, SEED, [fq], batch, pile)
    table.free()
    ctx_tx, ctx_k, _ = pile.result()
    tk, offs = index.transcript_kmers()
    d_tx, d_k, d_tk, d_offs, d_known = ctx.upload(ctx_tx, np.uint32), ctx.upload(ctx_k, np.uint64), ctx.upload(tk), ctx.upload(offs), \
        ctx.upload(index.known_stops())
    pairs = int(np.sum((offs[1:] - offs[:-1])[ctx_tx.astype(np.int64)]))
    ms = []
    for rep in range(1 + a.reps):
        ctx.profile(True)
        ctx.stop_nearest(d_tx, d_k, K, d_tk, d_offs, d_known)
        p = ctx.profile_read()
        ctx.profile(False)
        if rep >= 1:
            ms.append(p["stop_nearest"]["ms"])
    m = statistics.median(ms)
    out["nearest"] = dict(entries=len(ctx_tx), pair_tests=pairs, ms=ms, median_ms=m, G_pair_tests_per_s=pairs / (m * 1e-3) / 1e9)

    note("nearest measured")
    # ---- the restatement on one core ---------------------------------------------------------------------------------------------------
    from tests import _stop_restatement as REF
    nc = min(a.cpu_reads, R)
    t0 = time.perf_counter()
    ref = REF.Index(K, REF.read_fasta(open(fa).read()))
    t1 = time.perf_counter()
    res = REF.count_stops(ref, REF.read_fastq(head_text(fq, nc)), SEED)
    t2 = time.perf_counter()
    rows = REF.rows(ref, res)
    t3 = time.perf_counter()
    note("restatement timed")
    lines_all = runs[1]["lines"]
    scaled = (t1 - t0) + (t2 - t1) * R / nc + (t3 - t2) * lines_all / max(len(rows), 1)
    out["reference_one_core"] = dict(reads=nc, index_seconds=t1 - t0, reads_seconds=t2 - t1, nearest_seconds=t3 - t2, lines=len(rows),
                                     seconds_scaled=scaled, scaling="reads by R / reads, the nearest loop by lines / lines")
    out["speedup_over_one_core"] = scaled / runs[1]["seconds"]
    text = json.dumps(out, indent=1, sort_keys=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    shutil.rmtree(a.tmp, ignore_errors=True)
    engine.close()


if __name__ == "__main__":
    main()
