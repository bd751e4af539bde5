#!/usr/bin/env python3
"""`zot strand` end to end on synthetic read pairs (run on the GPU box): R pairs x 150 bp written the way
tools/bench_capture.py writes its reads (the counter-based generator's 100 Mb genome; mate 2 is a second draw of reads), at
-p 0.1 and -p 1.0.  Records, per P: warm end-to-end wall time, the ZOT_TIMING=2 phases summed by name, zk_strand_keys in
G windows/s (HIP events around the launches), and -- on the final table of that run -- zk_strand_pairs and zk_format_pairs
in GB/s against zk_project_sum at shift 0 on the same arrays (host clock around calls that end in a stream synchronise).
Last, the reference algorithm's rate (tests/_strand_restatement.py, one CPU core) over a slice.

    python3 tools/bench_strand.py [--pairs R] [--out profiles/<round>/strand.json]
"""
import argparse, json, os, shutil, statistics, sys, time
os.environ.setdefault("ZOT_TIMING", "2")          # library/timing.py reads it at import
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_capture import L, run, write_fastq as write_reads          # noqa: E402
from zotmer_amd import synth                                           # noqa: E402
from zotmer_amd.library import engine, strand                          # noqa: E402

K = 25


def write_pair(tmp, R):
    """mate 1 = reads [0, R) of the generator, mate 2 = reads [R, 2R): bench_capture.write_fastq writes reads [0, n), so mate 2
    is cut from a file of 2R reads"""
    f1, f2, both = (os.path.join(tmp, n) for n in ("m1.fastq", "m2.fastq", "both.fastq"))
    write_reads(both, 2 * R)
    size = os.path.getsize(both)
    assert size % (2 * R) == 0
    half = size // 2
    with open(both, "rb") as src:
        for path, n in ((f1, half), (f2, half)):
            with open(path, "wb") as dst:
                left = n
                while left:
                    buf = src.read(min(left, 64 << 20))
                    dst.write(buf)
                    left -= len(buf)
    os.remove(both)
    return f1, f2


def timed(ctx, fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": min(ts), "median_ms": statistics.median(ts), "max_ms": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=float, default=20e6)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tmp", default="/tmp/zot_strand_bench")
    ap.add_argument("--p", default="0.1,1.0")
    a = ap.parse_args()
    R = int(a.pairs)
    shutil.rmtree(a.tmp, ignore_errors=True)
    os.makedirs(a.tmp)
    t0 = time.perf_counter()
    f1, f2 = write_pair(a.tmp, R)
    res = {"pairs": R, "read_length": L, "K": K, "fastq_bytes": os.path.getsize(f1) + os.path.getsize(f2),
           "write_fastq_s": time.perf_counter() - t0, "runs": {}}
    ctx = engine.context()
    windows = 2 * R * (L - K + 1)
    sink = os.path.join(a.tmp, "lines.txt")

    def save():
        if a.out:
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    for p in [float(v) for v in a.p.split(",")]:
        runs = []
        for rep in range(2):                          # the first run warms the page cache and the allocator
            ctx.profile(True)
            saved = os.dup(1)
            fd = os.open(sink, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
            sys.stdout.flush()
            os.dup2(fd, 1)
            try:
                dt, phases, text = run("strand", "-k", K, "-p", repr(p), "-v", f1, f2)
            finally:
                sys.stdout.flush()
                os.dup2(saved, 1)
                os.close(saved)
                os.close(fd)
            prof = ctx.profile_read()
            ctx.profile(False)
            runs.append(dt)
        keys_ms = prof.get("strand_keys", {}).get("ms", 0.0)
        device = sum(v for k, v in phases.items() if not k.startswith(("wait for the reader", "print")))
        rec = {"wall_s_cold": runs[0], "wall_s_warm": runs[1], "pairs_per_s_warm": R / runs[1],
               "fastq_GB_per_s_warm": res["fastq_bytes"] / runs[1] / 1e9, "phases_ms": phases,
               "device_phases_ms": device, "reader_wait_ms": phases.get("wait for the reader", 0.0),
               "summary": [l for l in text.splitlines() if "sampled k-mer instances" in l][-1:],
               "output_bytes": os.path.getsize(sink),
               "strand_keys_kernel": {"launches": prof.get("strand_keys", {}).get("launches", 0), "ms": keys_ms,
                                      "keys_written": prof.get("strand_keys", {}).get("bytes", 0) // 8,
                                      "G_windows_per_s": windows / (keys_ms / 1e3) / 1e9 if keys_ms else None}}
        res["runs"]["p=%g" % p] = rec
        print("p=%g" % p, json.dumps(rec), flush=True)
        save()
        # the final table once more through the library, for the two kernels behind the output and their yardstick
        table = strand.StrandTable(ctx, K, strand.threshold(K, p))
        strand.count_inputs(ctx, table, [f1, f2], False, 256 << 20)
        keys, counts = table.result()
        n, cb = keys.n, counts.dtype.itemsize
        a_, b_, st = ctx.strand_pairs(keys, counts, K)
        out = ctx.format_pairs(a_, b_)
        kern = {"entries": n, "count_bits": 8 * cb, "lines": int(st.n_pairs), "text_bytes": out.n}
        kern["zk_strand_pairs"] = timed(ctx, lambda: ctx.strand_pairs(keys, counts, K))
        kern["zk_strand_pairs"]["algorithmic_bytes"] = (16 + cb) * n + 16 * int(st.n_pairs)
        kern["zk_format_pairs"] = timed(ctx, lambda: ctx.format_pairs(a_, b_, out=out))
        kern["zk_format_pairs"]["algorithmic_bytes"] = 48 * a_.n + out.n        # 16 read + 8 written, 8 + 16 read, the text
        kern["zk_project_sum_shift0"] = timed(ctx, lambda: ctx.project_sum(keys, counts, 0))
        kern["zk_project_sum_shift0"]["algorithmic_bytes"] = (16 + cb) * n + 16 * n
        for v in kern.values():
            if isinstance(v, dict):
                v["GB_per_s_median"] = v["algorithmic_bytes"] / (v["median_ms"] / 1e3) / 1e9
        rec["kernels_on_final_table"] = kern
        print("p=%g kernels" % p, json.dumps(kern), flush=True)
        del table, keys, counts, a_, b_, out
        save()
    # the reference's algorithm on one CPU core over a slice of the same pairs
    from tests import _strand_restatement as RS
    texts = []
    for f in (f1, f2):
        with open(f, "rb") as fh:
            texts.append(b"".join(fh.readline() for _ in range(4 * 5000)).decode())
    t0 = time.perf_counter()
    RS.strand(K, 0.1, texts)
    dt = time.perf_counter() - t0
    res["restatement_one_core"] = {"pairs": 5000, "p": 0.1, "seconds": dt, "pairs_per_s": 5000 / dt}
    print(json.dumps(res, indent=1))
    save()
    shutil.rmtree(a.tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
