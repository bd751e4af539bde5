#!/usr/bin/env python3
"""`zot capture` end to end on a synthetic FASTQ (run on the GPU box): R reads x 150 bp written the way tools/bench_e2e.py
writes them (from the counter-based generator's 100 Mb genome), against two bait panels cut from the same genome: a small
one (200 baits x 2 kb) and a large one (20 Mb: 2000 baits x 10 kb).  Records, per panel: warm end-to-end wall time, the
ZOT_TIMING=2 phases summed by name, the lookup kernel (zk_capture_hits) in G windows/s and as a fraction of 8 TB/s over the
bytes it must read, and the reference algorithm's rate (tests/_capture_restatement.py, one CPU core) over a slice.

    python3 tools/bench_capture.py [--reads R] [--out profiles/<round>/capture.json]
"""
import argparse, io, json, os, re, shutil, sys, tempfile, time
os.environ.setdefault("ZOT_TIMING", "2")          # library/timing.py reads it at import
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zotmer_amd import cli, synth
from zotmer_amd.library import engine

L, GENOME, PEAK = 150, 100_000_000, 8e12


def write_fastq(path, R):
    ctx = engine.context()
    with open(path, "wb") as f:
        step = 2_000_000
        for a in range(0, R, step):
            m = min(step, R - a)
            seq = ctx.synth_reads(synth.DEFAULT_SEED, a, m, L, genome=GENOME, sub_thr=synth.frac32(0.005),
                                  n_thr=synth.frac32(0.0005)).to_host().reshape(m, L + 1)
            rec = np.empty((m, 13 + (L + 1) + 2 + (L + 1)), dtype=np.uint8)
            rec[:, 0] = ord("@"); rec[:, 1] = ord("r")
            rec[:, 2:12] = np.frombuffer("".join(np.char.zfill(np.arange(a, a + m).astype(str), 10)).encode(), np.uint8).reshape(m, 10)
            rec[:, 12] = ord("\n")
            rec[:, 13:14 + L] = seq
            rec[:, 14 + L] = ord("+"); rec[:, 15 + L] = ord("\n")
            rec[:, 16 + L:16 + 2 * L] = ord("I"); rec[:, 16 + 2 * L] = ord("\n")
            f.write(rec.tobytes())


def genome_slice(p, n):
    return np.frombuffer(b"ACGT", np.uint8)[(synth.rnd(synth.DEFAULT_SEED, 1, np.arange(p, p + n, dtype=np.uint64)) & np.uint64(3)).astype(np.intp)].tobytes()


def write_panel(path, n, size, seed):
    rng = np.random.default_rng(seed)
    with open(path, "wb") as f:
        for i, p in enumerate(rng.integers(0, GENOME - size, n)):
            f.write(b">bait%d\n%s\n" % (i, genome_slice(int(p), size)))


def run(*argv):
    """-> (seconds, the [engine] phase lines summed by name in ms, stderr text)"""
    err = tempfile.TemporaryFile(mode="w+")
    saved = os.dup(2)
    os.dup2(err.fileno(), 2)
    t0 = time.perf_counter()
    try:
        cli.main_inner([str(a) for a in argv])
    finally:
        sys.stderr.flush()
        os.dup2(saved, 2)
        os.close(saved)
    dt = time.perf_counter() - t0
    err.seek(0)
    text = err.read()
    phases = {}
    for line in text.splitlines():
        m = re.match(r"\s*\[engine\] (.+?)\s+([\d.]+) ms", line)
        if m:
            name = re.sub(r"\d+", "N", m.group(1))
            phases[name] = phases.get(name, 0.0) + float(m.group(2))
    return dt, phases, text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=50e6)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tmp", default="/tmp/zot_capture_bench")
    a = ap.parse_args()
    R = int(a.reads)
    shutil.rmtree(a.tmp, ignore_errors=True)
    os.makedirs(a.tmp)
    fq = os.path.join(a.tmp, "reads.fastq")
    t0 = time.perf_counter()
    write_fastq(fq, R)
    res = {"reads": R, "read_length": L, "fastq_bytes": os.path.getsize(fq), "write_fastq_s": time.perf_counter() - t0, "panels": {}}
    ctx = engine.context()
    for name, n, size in (("small_200x2kb", 200, 2000), ("large_20Mb", 2000, 10000)):
        fa = os.path.join(a.tmp, name + ".fa")
        write_panel(fa, n, size, 7)
        out = os.path.join(a.tmp, "out_" + name)
        runs = []
        for rep in range(2):                          # the first run warms the page cache and the allocator
            shutil.rmtree(out, ignore_errors=True)
            os.makedirs(out)
            ctx.profile(True)
            dt, phases, text = run("capture", "-k", 25, "-P", out, fa, fq)
            prof = ctx.profile_read().get("capture_hits", {})
            ctx.profile(False)
            runs.append(dt)
        counts = [int(l.rsplit(": ", 1)[1]) for l in text.splitlines() if re.search(r"\.fastq: \d+$", l)]
        windows = R * (L - 25 + 1)
        must_read = R * L + 8 * windows               # the sequence bytes, and one directory line probe (2 x u32) per window
        ms = prof.get("ms", 0.0)
        res["panels"][name] = {
            "baits": n, "bait_bases": n * size, "wall_s_cold": runs[0], "wall_s_warm": runs[1],
            "reads_per_s_warm": R / runs[1], "fastq_GB_per_s_warm": res["fastq_bytes"] / runs[1] / 1e9,
            "phases_ms": phases, "pairs": sum(counts),
            "lookup_kernel": {"launches": prof.get("launches", 0), "ms": ms,
                              "G_windows_per_s": windows / (ms / 1e3) / 1e9 if ms else None,
                              "bytes_it_must_read": must_read,
                              "fraction_of_8TBps": (must_read / (ms / 1e3)) / PEAK if ms else None},
        }
        print(name, json.dumps(res["panels"][name]), flush=True)
    # the reference's algorithm on one CPU core over a slice of the same reads, small panel
    sys.path.insert(0, ROOT)
    from tests import _capture_restatement as RS
    with open(fq, "rb") as f:
        head = b"".join(f.readline() for _ in range(4 * 20000)).decode()
    baits = open(os.path.join(a.tmp, "small_200x2kb.fa")).read()
    t0 = time.perf_counter()
    RS.capture(baits, [head], 25)
    dt = time.perf_counter() - t0
    res["restatement_one_core"] = {"reads": 20000, "seconds": dt, "reads_per_s": 20000 / dt,
                                   "note": "includes building the bait dict for the 200 x 2 kb panel"}
    g = res["panels"]["small_200x2kb"]["reads_per_s_warm"]
    res["speedup_vs_restatement_small_panel"] = g / res["restatement_one_core"]["reads_per_s"]
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    shutil.rmtree(a.tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
