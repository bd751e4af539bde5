#!/usr/bin/env python3
"""`zot alu-finder` end to end on a synthetic panel (run on the GPU box): Z zones of 1 kb at random places of a G-base genome
of the counter-based generator (zotmer_amd/synth.py), R read pairs x 150 bp drawn over that genome (0.5 % substitutions,
mate 2 a second draw of reads), so that about Z kb / G of the reads lie on a zone.  Records:

  kernels      zk_profile's records of one pass over the reads through the library: the lookup-and-emit kernel (ZK_PROF_PILEUP;
               bytes = the text read + 12 per pair written) with its achieved bytes/s beside the 6.29 TB/s a float4 copy reaches
               on this chip, the gather and the cut of zk_pileup_count (ZK_PROF_PILEUP_CUT) and its sort passes
  command      warm wall time of the command's own path (the zones, the table, the batches, the decode, the report), the host
               merge's seconds and share of it, and the other host stages
  reference    the single-core time of the CPU restatement (tests/_alufinder_restatement.py) on the first `--cpu-pairs` pairs,
               scaled to R pairs

    python3 tools/bench_alufinder.py [--pairs R] [--zones Z] [--genome G] [--out profiles/<round>/alufinder.json]
"""
import argparse
import io
import json
import os
import shutil
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                     # noqa: E402
from zotmer_amd import synth                                           # noqa: E402
from zotmer_amd.library import alufinder, engine                       # noqa: E402

K, L, ZONE = 25, 150, 1000
HBM_COPY_TBPS = 6.29


def genome_text(G):
    b = synth.rnd(synth.DEFAULT_SEED, 1, np.arange(G, dtype=np.uint64)) & np.uint64(3)
    return np.frombuffer(b"ACGT", np.uint8)[b.astype(np.intp)].tobytes()


def write_fastq(ctx, path, first, R, G):
    with open(path, "wb") as f:
        step = 1_000_000
        for a in range(first, first + R, step):
            m = min(step, first + R - a)
            seq = ctx.synth_reads(synth.DEFAULT_SEED, a, m, L, genome=G, sub_thr=synth.frac32(0.005), n_thr=synth.frac32(0.0005))
            seq = seq.to_host().reshape(m, L + 1)
            rec = np.empty((m, 13 + (L + 1) + 2 + (L + 1)), dtype=np.uint8)
            rec[:, 0] = ord("@"); rec[:, 1] = ord("r")
            rec[:, 2:12] = np.frombuffer("".join(np.char.zfill(np.arange(a, a + m).astype(str), 10)).encode(), np.uint8).reshape(m, 10)
            rec[:, 12] = ord("\n")
            rec[:, 13:14 + L] = seq
            rec[:, 14 + L] = ord("+"); rec[:, 15 + L] = ord("\n")
            rec[:, 16 + L:16 + 2 * L] = ord("I"); rec[:, 16 + 2 * L] = ord("\n")
            f.write(rec.tobytes())


def head_text(path, n_records):
    out = []
    with open(path) as f:
        for _ in range(4 * n_records):
            out.append(f.readline())
    return "".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=float, default=2e6)
    ap.add_argument("--zones", type=int, default=100)
    ap.add_argument("--genome", type=float, default=2e6)
    ap.add_argument("--cpu-pairs", type=int, default=20000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tmp", default="/tmp/zot_alufinder_bench")
    a = ap.parse_args()
    R, G = int(a.pairs), int(a.genome)
    shutil.rmtree(a.tmp, ignore_errors=True)
    os.makedirs(a.tmp)
    ctx = engine.context()
    genome = genome_text(G)
    with open(os.path.join(a.tmp, "chrS.fa"), "wb") as f:
        f.write(b">chrS\n" + genome + b"\n")
    rng = np.random.default_rng(16)
    starts = np.sort(rng.choice(G // ZONE - 1, a.zones, replace=False)) * ZONE + 1
    bed_text = "".join("chrS\t%d\t%d\tzone%03d\n" % (s, s + ZONE - 1, i) for i, s in enumerate(starts.tolist()))
    bed = os.path.join(a.tmp, "zones.bed")
    with open(bed, "w") as f:
        f.write(bed_text)
    m1, m2 = os.path.join(a.tmp, "m1.fastq"), os.path.join(a.tmp, "m2.fastq")
    write_fastq(ctx, m1, 0, R, G)
    write_fastq(ctx, m2, R, R, G)
    text_bytes = os.path.getsize(m1) + os.path.getsize(m2)
    out = dict(pairs=R, zones=a.zones, zone_bases=ZONE, genome=G, K=K, read_length=L, fastq_bytes=text_bytes)

    from zotmer_amd.commands.capture import capture_batch_bytes
    batch = capture_batch_bytes(ctx)
    out["batch_bytes"] = batch

    def command(stats):
        t0 = time.perf_counter()
        zones = alufinder.load_zones(bed, a.tmp, K)
        t1 = time.perf_counter()
        sink = io.StringIO()
        alufinder.run(ctx, zones, [m1, m2], 5, 29, 5, 0.05, False, batch, sink, stats=stats)
        stats.update(seconds=time.perf_counter() - t0, zones_seconds=t1 - t0, lines=sink.getvalue().count("\n"))
        return stats

    command({})                                   # warm: the workspace, the file cache
    ctx.profile(True)
    st = command({})
    prof = ctx.profile_read()
    ctx.profile(False)
    out["kernels"] = prof
    if "pileup" in prof:
        p = prof["pileup"]
        p["GBps"] = p["bytes"] / (p["ms"] * 1e-3) / 1e9
        p["share_of_hbm_copy_rate"] = p["GBps"] / (HBM_COPY_TBPS * 1e3)
        p["G_windows_per_s"] = 2 * R * (L - K + 1) / (p["ms"] * 1e-3) / 1e9
    st = command({})                              # the timed run, without the profile's events
    st["merge_share"] = st["merge_seconds"] / st["seconds"]
    st["fastq_MBps"] = text_bytes / st["seconds"] / 1e6
    out["command"] = st

    sys.path.insert(0, ROOT)
    from tests import _alufinder_restatement as REF
    n = min(a.cpu_pairs, R)
    case = dict(k=K, C=5, L=29, S=5, V=0.05, raw=False, bed=bed_text, genomes={"chrS": genome.decode()},
                inputs=[head_text(m1, n), head_text(m2, n)])
    t0 = time.perf_counter()
    idx = REF.build_index(K, case["bed"], case["genomes"])
    t1 = time.perf_counter()
    acc = REF.pile_up(K, idx[1], case["inputs"])
    t2 = time.perf_counter()
    REF.report(K, REF.filter_acc(acc, case["V"], case["C"]), idx[0], idx[2], case["L"], case["S"], case["raw"])
    t3 = time.perf_counter()
    out["reference_one_core"] = dict(pairs=n, index_seconds=t1 - t0, pile_up_seconds=t2 - t1, filter_report_seconds=t3 - t2,
                                     pile_up_seconds_scaled=(t2 - t1) * R / n,
                                     seconds_scaled=(t1 - t0) + (t2 - t1) * R / n + (t3 - t2))
    out["speedup_over_one_core"] = out["reference_one_core"]["seconds_scaled"] / st["seconds"]
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
