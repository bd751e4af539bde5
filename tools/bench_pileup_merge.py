#!/usr/bin/env python3
"""zk_pileup_merge on the lists of `zot vardyger` (run on the GPU box): the workload of tools/bench_vardyger.py -- T sequences,
R single reads x 150 bp, K = 24 -- is captured once, every slice's counted list kept on the device as zk_pileup_count left it,
and the lists are then merged one after the other into an accumulated list, as alufinder.DevicePileup does.  Records:

  steps        per merge: the lengths of the accumulated list (A), of the batch list (B) and of their union, zk_profile's record
               (device events around the partition, the count pass, the scan and the emit pass; the read-back of the union's length
               between the passes is inside it) -- two warm sequences, then `--reps`, every one listed, the median, and the
               algorithmic GB/s of the median (12 B per input for the count pass, 20 per A element, 16 per B element, 20 per output)
  union_sum    zk_union_sum on u64 lists of the same lengths and the same overlap, 64-bit counts: the keys are the lists'
               own (bait << 48 | k-mer), which K = 24 and fewer than 2^16 sequences fit into one word.  The only yardstick the
               library has for a merge; its record is the merge kernel's alone (16 B per input, 16 per output)
  last_step    the two beside each other for the merge of the last batch list into everything before it
  commands     (--commands FILE ...) the figures of tools/bench_vardyger.py and tools/bench_hgvsfind.py, run at the parent
               commit and at this one on the same machine in the same session, as `name=path` of their JSON outputs: seconds and
               merge_seconds of each

    python3 tools/bench_pileup_merge.py [--reads R] [--sequences T] [--commands vardyger_parent=a.json ...] [--out profiles/<round>/pileup_merge.json]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np                                                     # noqa: E402
import bench_vardyger as bv                                            # noqa: E402
from zotmer_amd import native                                          # noqa: E402
from zotmer_amd.library import capture, engine, vardyger               # noqa: E402

K = bv.K


class Keeper:
    """stands where a pileup does and keeps every counted list on the device"""

    def __init__(self):
        self.lists = []

    def add_device(self, oc, ok, cnt):
        if oc.n:
            self.lists.append((oc, ok, cnt))


def command_figures(specs):
    out = {}
    for spec in specs:
        name, path = spec.split("=", 1)
        d = json.load(open(path))
        if "command" in d:                       # bench_vardyger
            m = d["command"]["median"]
            out[name] = dict(seconds=m["seconds"], merge_seconds=m["merge_seconds"], count_seconds=m["count_seconds"], reads=d["reads"],
                             distinct_entries=m["distinct_entries"], merges=m.get("merges"))
        else:                                    # bench_hgvsfind
            s = d["scan"]
            out[name] = dict(seconds=s["wall"]["median_ms"] / 1e3, merge_seconds=s["merge"]["median_ms"] / 1e3,
                             count_seconds=s["count"]["median_ms"] / 1e3, pairs=d["pairs"], distinct_entries=s["counts"]["distinct_entries"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=2e6)
    ap.add_argument("--sequences", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--commands", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    ap.add_argument("--tmp", default="/tmp/zot_pileup_merge_bench")
    a = ap.parse_args()
    R, T = int(a.reads), a.sequences
    shutil.rmtree(a.tmp, ignore_errors=True)
    os.makedirs(a.tmp)
    fa, fq, fq_bytes, _ = bv.write_inputs(a.tmp, T, R, np.random.default_rng(27))
    bv.note("inputs written")
    ctx = engine.context()
    from zotmer_amd.commands.capture import capture_batch_bytes
    index = vardyger.load_index(fa, K)
    table = capture.build_table(ctx, [(nm.encode(), seq.encode()) for nm, seq in zip(index.names, index.seqs)], K)
    keep = Keeper()
    stats = vardyger.new_stats()
    t0 = time.perf_counter()
    vardyger.capture_inputs(ctx, table, K, [fq], capture_batch_bytes(ctx), vardyger.EMIT_BUDGET, keep, np.zeros(T, np.int64), stats)
    table.free()
    out = dict(reads=R, sequences=T, K=K, fastq_bytes=fq_bytes, lists=len(keep.lists), pairs=sum(l[0].n for l in keep.lists),
               capture_seconds=time.perf_counter() - t0, count_seconds=stats["count_seconds"], tile=native.PILEUP_MERGE_TILE)
    bv.note("%d lists captured" % len(keep.lists))

    # ---- the merges of a run, one after the other ------------------------------------------------------------------------------------
    lists = keep.lists
    cap = sum(l[0].n for l in lists)
    bufs = [tuple(ctx.empty(cap, dt) for dt in (np.uint32, np.uint64, np.uint64)) for _ in range(2)]
    steps = [dict(na=None, nb=l[0].n, ms=[]) for l in lists[1:]]
    for rep in range(2 + a.reps):
        cur, n = 0, lists[0][0].n
        ctx._check(ctx.lib.zk_copy(ctx.h, bufs[0][0].ptr, lists[0][0].ptr, 4 * n))
        ctx._check(ctx.lib.zk_copy(ctx.h, bufs[0][1].ptr, lists[0][1].ptr, 8 * n))
        ctx._check(ctx.lib.zk_widen_counts(ctx.h, lists[0][2].ptr, bufs[0][2].ptr, n))
        ctx.sync()
        for st, b in zip(steps, lists[1:]):
            ctx.profile(True)
            m, fit = ctx.pileup_merge_into(tuple(x.view(n) for x in bufs[cur]), b, bufs[1 - cur])
            p = ctx.profile_read()["pileup_merge"]
            ctx.profile(False)
            assert fit
            st.update(na=n, m=m, bytes=p["bytes"])
            if rep >= 2:
                st["ms"].append(p["ms"])
            cur, n = 1 - cur, m
    for st in steps:
        st["median_ms"] = statistics.median(st["ms"])
        st["GBps"] = st["bytes"] / (st["median_ms"] * 1e-3) / 1e9
    out["steps"] = steps
    out["merges_of_a_run_ms"] = sum(st["median_ms"] for st in steps)
    out["distinct_pairs"] = n
    bv.note("merges measured")

    # ---- zk_union_sum on one-word keys of the same lengths and overlap -------------------------------------------------------------------
    word = lambda l: (l[0].to_host().astype(np.uint64) << np.uint64(48)) | l[1].to_host()
    assert T < (1 << 16) and 2 * K <= 48
    acc_k = ctx.upload(word(lists[0]))
    acc_c = ctx.widen(lists[0][2])
    union = []
    for i, b in enumerate(lists[1:]):
        bk, bc = ctx.upload(word(b)), ctx.widen(b[2])
        rec = dict(na=acc_k.n, nb=bk.n, ms=[])
        last = i == len(lists) - 2
        for rep in range((2 + a.reps) if last or i == 0 else 1):
            ctx.profile(True)
            ok, oc = ctx.union_sum(acc_k, acc_c, bk, bc)
            p = ctx.profile_read()["union_sum"]
            ctx.profile(False)
            if rep >= 2 or not (last or i == 0):
                rec["ms"].append(p["ms"])
            rec.update(m=ok.n, bytes=p["bytes"], launches=p["launches"])
        rec["median_ms"] = statistics.median(rec["ms"])
        rec["GBps"] = rec["bytes"] / (rec["median_ms"] * 1e-3) / 1e9
        union.append(rec)
        assert rec["m"] == steps[i]["m"] and rec["na"] == steps[i]["na"]
        acc_k, acc_c = ok, oc
    out["union_sum"] = union
    if steps:
        out["last_step"] = dict(na=steps[-1]["na"], nb=steps[-1]["nb"], m=steps[-1]["m"], pileup_merge_ms=steps[-1]["median_ms"],
                                pileup_merge_GBps=steps[-1]["GBps"], union_sum_ms=union[-1]["median_ms"], union_sum_GBps=union[-1]["GBps"],
                                pileup_merge_bytes_per_input=steps[-1]["bytes"] / (steps[-1]["na"] + steps[-1]["nb"]),
                                union_sum_bytes_per_input=union[-1]["bytes"] / (union[-1]["na"] + union[-1]["nb"]))
    # the merged list is the host's
    got = tuple(x.view(n).to_host() for x in bufs[cur])
    from zotmer_amd.library.alufinder import Pileup
    host = Pileup()
    t0 = time.perf_counter()
    for l in lists:
        host.add_device(*l)
    want = host.result()
    out["host_pileup_seconds"] = time.perf_counter() - t0
    out["host_merge_seconds"] = host.merge_seconds
    out["agrees_with_host_pileup"] = bool(all(np.array_equal(g, w) for g, w in zip(got, want)))
    bv.note("host pileup timed")
    if a.commands:
        out["commands"] = command_figures(a.commands)
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
