#!/usr/bin/env python3
"""`zot fizzle` on a synthetic exome (run on the GPU box): G genes of 10 exons of 150 to 250 random bases, one gene in twenty a
paralog of another (its exons copied with 2 % of the bases changed: tuples of two exons), R read pairs of 2 x 150 cut from
fragments of 400 bases of the transcripts, either way round, with 1 % substituted bases; 3 % of the pairs are fusions (mate 1 from
one gene, mate 2 from another).  K = 25.  Records:

  kernels      zk_profile's records (device events) of zk_fizzle_votes (the lookup-and-count kernel; the pass after the decision)
               beside zk_capture_hits' window lookup on the same pairs and the same table, `--kernel-pairs` of them in one batch:
               two warm-ups, then `--reps` alternated repetitions, every one listed, medians, and the ratios of the medians.  The
               new kernel looks every window up twice (as the k-mer and as its reverse complement: the table has a strand),
               capture once: the yardstick is twice capture's time.
  command      wall time of the library's own path (the class index, the table, the batches, the grouped host stage, the
               lines): one warm run, then three timed, every one listed with its stages, the median
  reference    the single-core time of the CPU restatement (tests/_fizzle_restatement.py) on the first `--cpu-pairs` pairs, scaled

    python3 tools/bench_fizzle.py [--pairs R] [--genes G] [--out profiles/<round>/fizzle.json]
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
from zotmer_amd.library import engine, fizzle                          # noqa: E402
from zotmer_amd.library.fastq_batches import whole                     # noqa: E402

K, L, FRAG = 25, 150, 400
T0 = time.perf_counter()
LETTERS = np.frombuffer(b"ACGT", np.uint8)


def note(msg):
    sys.stderr.write("[%7.1f s] %s\n" % (time.perf_counter() - T0, msg))
    sys.stderr.flush()


def make_genes(G, rng):
    """[[exon codes]] per gene"""
    genes = []
    for g in range(G):
        if g % 20 == 19:
            src = genes[int(rng.integers(0, g))]
            genes.append([np.where(rng.random(len(e)) < 0.02, (e + rng.integers(1, 4, size=len(e), dtype=np.uint8)) & 3, e).astype(np.uint8) for e in src])
        else:
            genes.append([rng.integers(0, 4, size=int(n), dtype=np.uint8) for n in rng.integers(150, 251, size=10)])
    return genes


def write_fastq(path, codes, first):
    m = len(codes)
    rec = np.empty((m, 13 + (L + 1) + 2 + (L + 1)), dtype=np.uint8)
    rec[:, 0] = ord("@"); rec[:, 1] = ord("r")
    rec[:, 2:12] = np.frombuffer("".join(np.char.zfill(np.arange(first, first + m).astype(str), 10)).encode(), np.uint8).reshape(m, 10)
    rec[:, 12] = ord("\n")
    rec[:, 13:13 + L] = LETTERS[codes]
    rec[:, 13 + L] = ord("\n")
    rec[:, 14 + L] = ord("+"); rec[:, 15 + L] = ord("\n")
    rec[:, 16 + L:16 + 2 * L] = ord("I"); rec[:, 16 + 2 * L] = ord("\n")
    path.write(rec.tobytes())


def write_inputs(tmp, genes, R, rng):
    tx = [np.concatenate(g) for g in genes]
    flat = np.concatenate(tx)
    lens = np.array([len(t) for t in tx])
    starts = np.concatenate(([0], np.cumsum(lens)))[:-1]
    p1, p2 = os.path.join(tmp, "reads_1.fastq"), os.path.join(tmp, "reads_2.fastq")
    with open(p1, "wb") as f1, open(p2, "wb") as f2:
        step = 500_000
        for a in range(0, R, step):
            m = min(step, R - a)
            t = rng.integers(0, len(tx), size=m)
            p = (rng.random(m) * (lens[t] - FRAG + 1)).astype(np.int64) + starts[t]
            t2 = np.where(rng.random(m) < 0.03, rng.integers(0, len(tx), size=m), t)
            q = np.where(t2 == t, p + FRAG - L, (rng.random(m) * (lens[t2] - L + 1)).astype(np.int64) + starts[t2])
            m1 = flat[p[:, None] + np.arange(L)[None, :]]
            m2 = 3 - flat[q[:, None] + np.arange(L)[None, :]][:, ::-1]
            for codes in (m1, m2):
                sub = rng.random((m, L)) < 0.01
                codes[...] = np.where(sub, (codes + rng.integers(1, 4, size=(m, L), dtype=np.uint8)) & 3, codes)
            flip = rng.random(m) < 0.5
            m1, m2 = np.where(flip[:, None], m2, m1).astype(np.uint8), np.where(flip[:, None], m1, m2).astype(np.uint8)
            write_fastq(f1, m1, a)
            write_fastq(f2, m2, a)
    return p1, p2, os.path.getsize(p1) + os.path.getsize(p2)


def head_text(path, n_records):
    out = []
    with open(path) as f:
        for _ in range(4 * n_records):
            out.append(f.readline())
    return "".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=float, default=2e6)
    ap.add_argument("--genes", type=int, default=1000)
    ap.add_argument("--kernel-pairs", type=int, default=500_000)
    ap.add_argument("--cpu-pairs", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tmp", default="/tmp/zot_fizzle_bench")
    a = ap.parse_args()
    R, G = int(a.pairs), a.genes
    shutil.rmtree(a.tmp, ignore_errors=True)
    os.makedirs(a.tmp)
    rng = np.random.default_rng(25)
    genes = make_genes(G, rng)
    ref = [dict(gene="G%04d" % g, exon="%02d" % (i + 1), chr="c", st="0", en="0", strand="+", seq=LETTERS[e].tobytes().decode())
           for g, exons in enumerate(genes) for i, e in enumerate(exons)]
    p1, p2, fq_bytes = write_inputs(a.tmp, genes, R, rng)
    note("inputs written")
    ctx = engine.context()
    t0 = time.perf_counter()
    index = fizzle.ClassIndex(K, ref)
    index_seconds = time.perf_counter() - t0
    out = dict(pairs=R, genes=G, exons=len(ref), K=K, read_length=L, fragment=FRAG, substitutions=0.01, fusions=0.03, fastq_bytes=fq_bytes,
               keys=len(index.keys), classes=len(index.tuples), classes_of_two_or_more=sum(len(t) > 1 for t in index.tuples),
               class_index_seconds=index_seconds, fizzle_classes_in_lds=512)

    # ---- the two lookup kernels on the same pairs and the same table -------------------------------------------------------------
    table = index.table(ctx)
    n = min(a.kernel_pairs, R)
    texts = [ctx.upload(np.frombuffer(head_text(p, n).encode(), dtype=np.uint8)) for p in (p1, p2)]
    lines = [ctx.line_ends(t) for t in texts]
    single = ctx.upload(np.zeros(2 * len(index.tuples), dtype=np.uint64))
    hist = ctx.upload(np.zeros(4096, dtype=np.uint64))
    bufs = cap_buf = None
    rec = dict(fizzle_count=[], fizzle_emit=[], capture_hits=[])
    for rep in range(2 + a.reps):
        ctx.profile(True)
        r_, c_, k_ = ctx.fizzle_votes(table, K, texts[0], lines[0], texts[1], lines[1], n, single, hist, out=bufs)
        pf = ctx.profile_read()
        ctx.profile(True)
        hits = ctx.capture_hits(table, K, texts[0], lines[0], n, texts[1], lines[1], out=cap_buf)
        pc = ctx.profile_read()
        ctx.profile(False)
        bufs, cap_buf = (whole(r_), whole(c_), whole(k_)), whole(hits)
        if rep >= 2:
            rec["fizzle_count"].append(pf["fizzle_count"]["ms"])
            rec["fizzle_emit"].append(pf["fizzle_emit"]["ms"])
            rec["capture_hits"].append(pc["capture_hits"]["ms"])
    med = {k: statistics.median(v) for k, v in rec.items()}
    windows = 2 * n * (L - K + 1)
    both = med["fizzle_count"] + med["fizzle_emit"]
    out["kernels"] = dict(pairs=n, windows=windows, lookups=dict(fizzle=2 * windows, capture=windows), entries=r_.n,
                          multi_class_records=int(len(np.unique(r_.to_host()))), capture_pairs=hits.n, ms=rec, median_ms=med,
                          both_passes_ms=both, both_passes_over_capture=both / med["capture_hits"],
                          count_pass_over_capture=med["fizzle_count"] / med["capture_hits"], yardstick="2 x capture, a quarter over it allowed: 2.5",
                          G_lookups_per_s=dict(fizzle_count=2 * windows / (med["fizzle_count"] * 1e-3) / 1e9,
                                               capture_hits=windows / (med["capture_hits"] * 1e-3) / 1e9),
                          profile_records=dict(fizzle=pf, capture=pc))
    note("kernels measured")
    del texts, lines, bufs, cap_buf, r_, c_, k_, hits
    table.free()

    # ---- the command ----------------------------------------------------------------------------------------------------------------
    from zotmer_amd.commands.capture import capture_batch_bytes
    batch = capture_batch_bytes(ctx)
    out["batch_bytes"] = batch

    def command():
        stats = fizzle.new_stats()
        t0 = time.perf_counter()
        idx = fizzle.ClassIndex(K, ref)
        t1 = time.perf_counter()
        sink = io.StringIO()
        fizzle.run_scan(ctx, idx, [p1, p2], batch, sink, stats=stats)
        stats.update(seconds=time.perf_counter() - t0, index_seconds=t1 - t0, lines_printed=sink.getvalue().count("\n"))
        stats["ingest_and_rest_seconds"] = stats["scan_seconds"] - stats["kernel_seconds"] - stats["d2h_seconds"] - stats["group_seconds"]
        stats["slow_share_of_group"] = stats["slow_seconds"] / stats["group_seconds"] if stats["group_seconds"] else 0.0
        return stats, sink.getvalue()

    command()                                     # warm: the workspace, the file cache
    note("command warm")
    runs = [command() for _ in range(3)]
    note("command timed")
    table_text = runs[0][1]
    runs = sorted((r[0] for r in runs), key=lambda s: s["seconds"])
    out["command"] = dict(runs=runs, median=runs[1], fastq_MBps=fq_bytes / runs[1]["seconds"] / 1e6)

    # ---- the restatement on one core ---------------------------------------------------------------------------------------------------
    from tests import _fizzle_restatement as REF
    nc = min(a.cpu_pairs, R)
    t0 = time.perf_counter()
    idx, _ = REF.tuple_index(K, ref)
    t1 = time.perf_counter()
    pairs = list(zip(REF.read_fastq(head_text(p1, nc)), REF.read_fastq(head_text(p2, nc))))
    acc, hit_counts, rn = REF.scan(K, idx, pairs)
    t2 = time.perf_counter()
    note("restatement timed")
    scaled = (t1 - t0) + (t2 - t1) * R / nc
    out["reference_one_core"] = dict(pairs=nc, index_seconds=t1 - t0, pairs_seconds=t2 - t1, seconds_scaled=scaled,
                                     scaling="the index once, the pairs by R / pairs")
    out["speedup_over_one_core"] = scaled / runs[1]["seconds"]
    if nc == R:
        out["table_equals_restatement"] = table_text == "".join(l + "\n" for l in REF.table(ref, acc))
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
