#!/usr/bin/env python3
"""`zot hgvs-index -T` on synthetic text (run on the GPU box).  The text is zotmer_amd/synth.py's uniform base sequence as
60-column lines; the table holds the alleles of `--variants` substitutions placed in it (wt and mut records of 2 K - 1 bases).

  1. zk_sequence_tally on `--bases` bases in one call: the zk_profile record of the tile kernel (algorithmic bytes = the text
     bytes), one warm-up and `--reps` repetitions; beside it the single-core Python restatement of the reference's loop
     (hgvs-find.py:884-891) on 2^20 bases, scaled.
  2. zk_capture_hits on the same bases cut as 150-base reads (synth's uniform mode indexes bases by position, so the two texts
     spell the same sequence), looked up in the same table: the existing kernel with the same lookup per window.  The line
     table names each read's bytes as the second line of a record.
  3. `zot hgvs-index -T` end to end over 24 gzip files of that text: wall time, the time spent waiting for the reader
     (inflation and copies that the kernel did not hide) and the time in the tally calls; and the same files inflated by one
     zk_source alone, which is the floor.

    python3 tools/bench_hgvsindex.py [--bases N] [--variants V] [--out profiles/<round>/hgvs_index.json]
"""
import argparse, gzip, io, json, os, shutil, statistics, sys, tempfile, time
os.environ.setdefault("ZOT_TIMING", "0")
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zotmer_amd import synth
from zotmer_amd.library import engine, hgvsindex

K, COLS, READ = 25, 60, 150
HBM_PEAK = 8.0e12


def spread(ts):
    return {"min_ms": min(ts), "median_ms": statistics.median(ts), "max_ms": max(ts)}


def profiled(ctx, tag, fn, reps):
    """one warm-up, then `reps` calls, each its own zk_profile record -> (spread of the kernel's ms, its bytes, fn's last result)"""
    ts, nbytes, r = [], 0, None
    for rep in range(reps + 1):
        ctx.profile(True)
        r = fn()
        p = ctx.profile_read()[tag]
        ctx.profile(False)
        if rep:
            ts.append(p["ms"])
            nbytes = p["bytes"]
    return spread(ts), nbytes, r


def python_tally(seq, want):
    """the reference's loop on one core: basics.kmers over the joined sequence, a dict bumped"""
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    counts = dict.fromkeys(want, 0)
    msk, x, run = (1 << (2 * K)) - 1, 0, 0
    for ch in seq:
        b = code.get(ch)
        if b is None:
            x = run = 0
            continue
        x = ((x << 2) | b) & msk
        run += 1
        if run >= K and x in counts:
            counts[x] += 1
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=1 << 30)
    ap.add_argument("--variants", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    seed = synth.DEFAULT_SEED
    n_lines, n_reads = a.bases // COLS, a.bases // READ
    res = {"K": K, "bases": n_lines * COLS, "columns": COLS, "variants": a.variants, "repetitions": a.reps}
    ctx = engine.context()

    # the table: substitutions spread over the first 2^22 bases
    head = synth.reads_matrix(seed, 0, (1 << 22) // COLS, COLS).reshape(-1).tobytes().decode()
    pos = (synth.rnd(seed, 21, np.arange(a.variants, dtype=np.uint64)) % np.uint64(len(head) - 4 * K)).astype(np.int64) + 2 * K
    recs = []
    for p in pos.tolist():
        wt = head[p - (K - 1):p + K]
        recs += [wt, wt[:K - 1] + "ACGT"[("ACGT".index(wt[K - 1]) + 1) & 3] + wt[K:]]
    table = ctx.bait_table(ctx.upload_stream("".join(r + "\n" for r in recs).encode()), K)
    res["table_keys"] = table.n_keys

    # 1. the tally kernel
    text = ctx.synth_reads(seed, 0, n_lines, COLS)
    counts = ctx.upload(np.zeros(table.n_keys, dtype=np.uint64))
    sp, nbytes, (st, nw, gt) = profiled(ctx, "seq_tally", lambda: ctx.sequence_tally(table, text, (0, 0), counts), a.reps)
    assert nbytes == text.n and nw == n_lines * COLS - K + 1 and gt == text.n
    hits = counts.to_host()
    assert int(hits.sum()) % (a.reps + 1) == 0
    hits //= np.uint64(a.reps + 1)
    res["sequence_tally"] = dict(sp, text_bytes=text.n, windows=nw, hits=int(hits.sum()), GB_per_s=text.n / sp["median_ms"] / 1e6,
                                 fraction_of_hbm_peak=text.n / (sp["median_ms"] * 1e-3) / HBM_PEAK)
    print("sequence_tally", json.dumps(res["sequence_tally"]), flush=True)
    small = synth.reads_matrix(seed, 0, (1 << 20) // COLS, COLS).reshape(-1).tobytes().decode()
    keys = [int(x) for x in table.arrays()[0].to_host()]
    t0 = time.perf_counter()
    got = python_tally(small, keys)
    t = time.perf_counter() - t0
    res["python_single_core"] = {"bases": len(small), "seconds": t, "scaled_to_the_text_seconds": t * res["bases"] / len(small)}
    check = ctx.upload(np.zeros(table.n_keys, dtype=np.uint64))
    ctx.sequence_tally(table, text, (0, 0), check, n=(len(small) // COLS) * (COLS + 1))
    assert check.to_host().tolist() == [got[x] for x in keys], "the device and the Python loop differ"
    res["python_over_device"] = res["python_single_core"]["scaled_to_the_text_seconds"] / (sp["median_ms"] * 1e-3)

    # 2. zk_capture_hits on the same bases as 150-base reads
    reads = ctx.synth_reads(seed, 0, n_reads, READ)
    ends = np.arange(n_reads, dtype=np.uint64) * np.uint64(READ + 1) + np.uint64(READ)
    lines = np.empty((n_reads, 4), dtype=np.uint64)
    lines[:, 0] = ends - np.uint64(READ + 1)            # the '\n' before the read (read 0: 2^64 - 1, + 1 = 0)
    lines[:, 1] = lines[:, 2] = lines[:, 3] = ends
    d_lines = ctx.upload(lines.reshape(-1))
    buf = ctx.empty(4 * a.variants * 64 + (1 << 20), np.uint64)
    sp2, nb2, pairs = profiled(ctx, "capture_hits", lambda: ctx.capture_hits(table, K, reads, d_lines, n_reads, out=buf), a.reps)
    res["capture_hits"] = dict(sp2, text_bytes=reads.n, reads=n_reads, pairs=pairs.n, GB_per_s=reads.n / sp2["median_ms"] / 1e6,
                               fraction_of_hbm_peak=reads.n / (sp2["median_ms"] * 1e-3) / HBM_PEAK)
    res["tally_bytes_per_s_over_capture_hits"] = res["sequence_tally"]["GB_per_s"] / res["capture_hits"]["GB_per_s"]
    print("capture_hits", json.dumps(res["capture_hits"]), flush=True)
    del reads, d_lines, buf, lines

    # 3. the command's -T over 24 gzip files of the text
    if not a.skip_e2e:
        tmp = tempfile.mkdtemp(dir=a.tmp)
        try:
            host = text.to_host()
            per = (n_lines // 24) * (COLS + 1)
            t0 = time.perf_counter()
            for i in range(24):
                with open(os.path.join(tmp, "chr%02d.fa.gz" % i), "wb") as f:
                    f.write(gzip.compress(b">chr%02d\n" % i + host[i * per:(i + 1) * per].tobytes(), 1))
            res["write_gzip_s"] = time.perf_counter() - t0
            del host
            gz = sum(os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp))
            items = [{"hgvs": "v%d" % i, "lhsFlank": recs[2 * i][:K - 1], "rhsFlank": recs[2 * i][K:], "wtSeq": recs[2 * i][K - 1],
                      "mutSeq": recs[2 * i + 1][K - 1]} for i in range(a.variants)]
            files = hgvsindex.Home(tmp).files()
            runs = []
            for rep in range(2):
                stats, out = hgvsindex.new_stats(), io.StringIO()
                t0 = time.perf_counter()
                hgvsindex.run_test(ctx, items, K, files, hgvsindex.DEFAULT_BATCH, out, stats=stats)
                runs.append(dict(stats, wall_s=time.perf_counter() - t0))
            assert stats["windows"] == 24 * (per // (COLS + 1) * COLS - K + 1)
            # the floor: the same files through a zk_source alone
            bufs = [ctx.empty(hgvsindex.DEFAULT_BATCH, np.uint8), ctx.empty(hgvsindex.DEFAULT_BATCH, np.uint8)]
            t0 = time.perf_counter()
            got = 0
            for path in files:
                src = ctx.source_open(path)
                eof, cur = False, 0
                while not eof:
                    src.start(bufs[cur], 0, hgvsindex.DEFAULT_BATCH)
                    n, eof = src.finish()
                    got += n
                    cur = 1 - cur
                src.close()
            t_src = time.perf_counter() - t0
            res["end_to_end"] = {"files": 24, "gzip_bytes": gz, "text_bytes": got, "batch_bytes": hgvsindex.DEFAULT_BATCH, "runs": runs,
                                 "source_alone_s": t_src, "source_alone_GB_per_s": got / t_src / 1e9,
                                 "warm_wall_over_source_alone": runs[1]["wall_s"] / t_src}
            print("end_to_end", json.dumps(res["end_to_end"]), flush=True)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
