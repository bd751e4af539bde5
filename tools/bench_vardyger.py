#!/usr/bin/env python3
"""`zot vardyger` on a synthetic gene panel (run on the GPU box): T sequences of 2 to 4 kb of random bases (the panel of
tools/bench_stop.py), one in ten with a tandem duplication of 30 to 90 bases spiked into the genome its reads come from, R
single reads x 150 bp cut from those genomes in either orientation with 1 % substituted bases, K = 24.  Records:

  join         zk_profile's records (device events) of zk_dup_join on the command's merged counted list and the panel's
               occurrence table: the cover pass and the join (count pass + emit pass) separately; two warm-ups, then `--reps`
               repetitions, every one listed, medians.  Beside it the closed form in NumPy on the host (searchsorted over the same
               arrays; best of three) and the literal restatement of findDup + positions in Python on one core, on the first
               `--cpu-sequences` sequences, scaled by sequences.
  capture      zk_capture_hits and zk_capture_kmers on single reads: `--kernel-reads` reads in one batch, the same repetitions
  command      wall time of the library's own path, with its stages (lookup, emission, count, merge, join, -s, formatting): one
               warm run, then three timed, every one listed, the median

    python3 tools/bench_vardyger.py [--reads R] [--sequences T] [--out profiles/<round>/vardyger.json]
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
from zotmer_amd.library import capture, engine, hgvsfind, vardyger     # noqa: E402
from zotmer_amd.library.alufinder import Pileup                        # noqa: E402

K, L = 24, 150
T0 = time.perf_counter()
LETTERS = np.frombuffer(b"ACGT", np.uint8)


def note(msg):
    sys.stderr.write("[%7.1f s] %s\n" % (time.perf_counter() - T0, msg))
    sys.stderr.flush()


def write_inputs(tmp, T, R, rng):
    """genes.fa and reads.fastq -> (paths, bytes of the FASTQ, duplications spiked)"""
    lens = rng.integers(2000, 4001, size=T)
    genes = [rng.integers(0, 4, size=int(n), dtype=np.uint8) for n in lens]
    genomes, spiked = [], 0
    for i, g in enumerate(genes):
        if i % 10 == 3:
            u = 3 * int(rng.integers(10, 31))
            at = int(rng.integers(200, len(g) - 200 - u))
            g = np.concatenate((g[:at + u], g[at:at + u], g[at + u:]))
            spiked += 1
        genomes.append(g)
    fa = os.path.join(tmp, "genes.fa")
    with open(fa, "wb") as f:
        for i, codes in enumerate(genes):
            f.write(b">gene%05d\n" % i + LETTERS[codes].tobytes() + b"\n")
    flat = np.concatenate(genomes)
    glen = np.array([len(c) for c in genomes])
    starts = np.concatenate(([0], np.cumsum(glen)))[:-1]
    fq = os.path.join(tmp, "reads.fastq")
    with open(fq, "wb") as f:
        step = 500_000
        for a in range(0, R, step):
            m = min(step, R - a)
            t = rng.integers(0, T, size=m)
            p = (rng.random(m) * (glen[t] - L + 1)).astype(np.int64) + starts[t]
            codes = flat[p[:, None] + np.arange(L)[None, :]]
            sub = rng.random((m, L)) < 0.01
            codes = np.where(sub, (codes + rng.integers(1, 4, size=(m, L), dtype=np.uint8)) & 3, codes).astype(np.uint8)
            rev = rng.random(m) < 0.5
            codes[rev] = 3 - codes[rev][:, ::-1]
            rec = np.empty((m, 13 + (L + 1) + 2 + (L + 1)), dtype=np.uint8)
            rec[:, 0] = ord("@"); rec[:, 1] = ord("r")
            rec[:, 2:12] = np.frombuffer("".join(np.char.zfill(np.arange(a, a + m).astype(str), 10)).encode(), np.uint8).reshape(m, 10)
            rec[:, 12] = ord("\n")
            rec[:, 13:13 + L] = LETTERS[codes]
            rec[:, 13 + L] = ord("\n")
            rec[:, 14 + L] = ord("+"); rec[:, 15 + L] = ord("\n")
            rec[:, 16 + L:16 + 2 * L] = ord("I"); rec[:, 16 + 2 * L] = ord("\n")
            f.write(rec.tobytes())
    return fa, fq, os.path.getsize(fq), spiked


def head_text(path, n_records):
    out = []
    with open(path) as f:
        for _ in range(4 * n_records):
            out.append(f.readline())
    return "".join(out)


def numpy_join(index, baits, kmers, counts, min_count):
    """the closed form on the host: (cover, rows as (e, i, j) arrays in the entry's order).  K <= 24 and fewer than 2^16
    sequences: (sequence, k-mer) and (sequence, half) each pack into one word."""
    Kb = np.uint64(index.K)
    lst = (baits.astype(np.uint64) << np.uint64(48)) | kmers
    occ = (index.rseq.astype(np.uint64) << np.uint64(48)) | index.rkmer
    at = np.minimum(np.searchsorted(lst, occ), max(len(lst) - 1, 0))
    cover = np.where(lst[at] == occ, counts[at], 0) if len(lst) else np.zeros(len(occ), counts.dtype)
    live = np.nonzero(counts >= min_count)[0]
    c, b = kmers[live] >> Kb, kmers[live] & np.uint64((1 << index.K) - 1)
    seq = baits[live].astype(np.uint64) << np.uint64(48)
    by = index.by_second.astype(np.int64)
    second_key = (index.rseq[by].astype(np.uint64) << np.uint64(48)) | index.second[by]
    first_key = (index.rseq.astype(np.uint64) << np.uint64(48)) | index.first
    i0, i1 = np.searchsorted(second_key, seq | b, "left"), np.searchsorted(second_key, seq | b, "right")
    j0, j1 = np.searchsorted(first_key, seq | c, "left"), np.searchsorted(first_key, seq | c, "right")
    ni, nj = i1 - i0, j1 - j0
    has = np.nonzero((ni > 0) & (nj > 0))[0]
    prod = ni[has] * nj[has]
    which = np.repeat(np.arange(len(has)), prod)
    p = np.arange(int(prod.sum())) - np.repeat(np.cumsum(prod) - prod, prod)
    ii, jj = p // nj[has][which], p % nj[has][which]
    e = live[has][which]
    i = by[i0[has][which] + ii]
    j = j0[has][which] + jj
    keep = (index.first[i] != kmers[e] >> Kb) & (index.rkmer[j] != kmers[e]) & (cover[j] >= min_count) & \
        (index.rpos[j].astype(np.int64) > index.rpos[i].astype(np.int64) + index.J)
    return cover, e[keep], i[keep], j[keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=2e6)
    ap.add_argument("--sequences", type=int, default=1000)
    ap.add_argument("--kernel-reads", type=int, default=500_000)
    ap.add_argument("--cpu-sequences", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tmp", default="/tmp/zot_vardyger_bench")
    a = ap.parse_args()
    R, T = int(a.reads), a.sequences
    shutil.rmtree(a.tmp, ignore_errors=True)
    os.makedirs(a.tmp)
    rng = np.random.default_rng(27)
    fa, fq, fq_bytes, spiked = write_inputs(a.tmp, T, R, rng)
    note("inputs written")
    ctx = engine.context()
    out = dict(reads=R, sequences=T, K=K, read_length=L, fastq_bytes=fq_bytes, substitutions=0.01, duplications=spiked,
               wave_pairs_bound=64)

    # ---- the command ----------------------------------------------------------------------------------------------------------------
    from zotmer_amd.commands.capture import capture_batch_bytes
    batch = capture_batch_bytes(ctx)
    out["batch_bytes"] = batch

    def command(strict):
        stats = vardyger.new_stats()
        t0 = time.perf_counter()
        idx = vardyger.load_index(fa, K)
        t1 = time.perf_counter()
        sink = io.StringIO()
        vardyger.run(ctx, idx, [fq], 10, False, strict, batch, sink, err=io.StringIO(), stats=stats)
        stats.update(seconds=time.perf_counter() - t0, index_seconds=t1 - t0, lines_printed=sink.getvalue().count("\n"))
        return stats

    command(False)                                # warm: the workspace, the file cache
    note("command warm")
    runs = [command(False) for _ in range(3)]
    runs.sort(key=lambda s: s["seconds"])
    strict = command(True)
    note("command timed")
    out["command"] = dict(runs=runs, median=runs[1], fastq_MBps=fq_bytes / runs[1]["seconds"] / 1e6, with_strict=strict)

    # ---- single reads through the two capture kernels ------------------------------------------------------------------------------------
    index = vardyger.load_index(fa, K)
    table = capture.build_table(ctx, [(nm.encode(), seq.encode()) for nm, seq in zip(index.names, index.seqs)], K)
    n = min(a.kernel_reads, R)
    text = ctx.upload(np.frombuffer(head_text(fq, n).encode(), dtype=np.uint8))
    lines = ctx.line_ends(text)
    rec = dict(capture_hits=[], capture_kmers=[])
    pairs_buf = bufs = None
    for rep in range(2 + a.reps):
        ctx.profile(True)
        pairs_buf = ctx.capture_hits(table, K, text, lines, n, out=hgvsfind.whole(pairs_buf))
        take = min(pairs_buf.n, (1 << 25) // (2 * (L - K + 1)))
        ob, ok = ctx.capture_kmers(pairs_buf.view(take), text, lines, n, K, out=bufs)
        p = ctx.profile_read()
        ctx.profile(False)
        bufs = (hgvsfind.whole(ob), hgvsfind.whole(ok))
        if rep >= 2:
            rec["capture_hits"].append(p["capture_hits"]["ms"])
            rec["capture_kmers"].append(p["capture_kmers"]["ms"])
    med = {k: statistics.median(v) for k, v in rec.items()}
    out["capture_single_reads"] = dict(reads=n, pairs=pairs_buf.n, pairs_emitted=take, entries=ob.n, ms=rec, median_ms=med,
                                       G_lookups_per_s=n * (L - K + 1) / (med["capture_hits"] * 1e-3) / 1e9,
                                       G_entries_per_s=ob.n / (med["capture_kmers"] * 1e-3) / 1e9)
    note("capture kernels measured")
    del text, lines, pairs_buf, bufs, ob, ok

    # ---- zk_dup_join on the command's merged list -------------------------------------------------------------------------------------------
    pile = Pileup()
    vardyger.capture_inputs(ctx, table, K, [fq], batch, vardyger.EMIT_BUDGET, pile, np.zeros(T, np.int64), vardyger.new_stats())
    table.free()
    baits, kmers, counts = pile.result()
    dev = vardyger.DeviceIndex(ctx, index)
    d_list = (ctx.upload(baits.astype(np.uint32)), ctx.upload(kmers), ctx.upload(counts.astype(np.uint32)))
    rec = dict(dup_cover=[], dup_join=[])
    bufs = tuple(ctx.empty(1 << 16, np.uint32) for _ in range(3))
    for rep in range(2 + a.reps):
        ctx.profile(True)
        cover, e, i, j = ctx.dup_join(*d_list, *dev.arrays, K, vardyger.THRESHOLD, out=bufs)
        p = ctx.profile_read()
        ctx.profile(False)
        if rep >= 2:
            rec["dup_cover"].append(p["dup_cover"]["ms"])
            rec["dup_join"].append(p["dup_join"]["ms"])
    med = {k: statistics.median(v) for k, v in rec.items()}
    live = int((counts >= vardyger.THRESHOLD).sum())
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        h_cover, he, hi, hj = numpy_join(index, baits, kmers, counts, vardyger.THRESHOLD)
        host.append(time.perf_counter() - t0)
    same = np.array_equal(h_cover.astype(np.uint32), cover) and sorted(zip(he.tolist(), hi.tolist(), hj.tolist())) == sorted(zip(e.tolist(), i.tolist(), j.tolist()))
    out["join"] = dict(entries=len(baits), entries_at_threshold=live, occurrences=index.m, rows=len(e), ms=rec, median_ms=med,
                       M_entries_per_s=len(baits) / (med["dup_join"] * 1e-3) / 1e6, M_occurrences_per_s=index.m / (med["dup_cover"] * 1e-3) / 1e6,
                       numpy_closed_form_seconds=host, numpy_closed_form_best_ms=min(host) * 1e3, numpy_agrees=bool(same),
                       device_over_numpy=min(host) * 1e3 / (med["dup_cover"] + med["dup_join"]))
    note("join measured")

    # ---- the literal restatement on one core -----------------------------------------------------------------------------------------------
    from tests import _vardyger_restatement as REF
    nc = min(a.cpu_sequences, T)
    records = list(zip(index.names[:nc], index.seqs[:nc]))
    t0 = time.perf_counter()
    ref = REF.Index(K, records)
    t1 = time.perf_counter()
    offs = np.searchsorted(baits, np.arange(nc + 1))
    rows = 0
    for s in range(nc):
        lo, hi = int(offs[s]), int(offs[s + 1])
        keep = counts[lo:hi] >= vardyger.THRESHOLD
        rows += len(REF.candidates(ref, s, dict(zip(kmers[lo:hi][keep].tolist(), counts[lo:hi][keep].tolist()))))
    t2 = time.perf_counter()
    out["reference_one_core"] = dict(sequences=nc, index_and_phantom_seconds=t1 - t0, find_dup_positions_seconds=t2 - t1, rows=rows,
                                     seconds_scaled=(t2 - t0) * T / nc, scaling="by sequences: T / sequences")
    out["join_speedup_over_one_core"] = out["reference_one_core"]["seconds_scaled"] * 1e3 / (med["dup_cover"] + med["dup_join"])
    note("restatement timed")
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
