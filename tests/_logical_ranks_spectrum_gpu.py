"""Run by tests/test_gpu_dist_spectrum_sharded.py in its own process (torch first, as the commands do under torch.distributed.run).

The spectrum measures of `zot dist` over 8 LOGICAL ranks on ONE device: eight threads, each with its own zk_ctx, run
parallel.SpectrumDist with GpuOps (zk_project_sum, zk_add_u64, zk_lower_bound, zk_hash_partition, zk_merge_n,
zk_spectrum_sums_row on the device) over the thread transport of tests/_logical_ranks_gpu.py, every library call under that
script's one lock.  Counted sets position-sharded over the ranks: three synthetic sets of K = 25, a set of 3 k-mers (five ranks
hold nothing of it) and a set of K = 20, at <k> = 25 (the files' own K: shift 0; without the K = 20 set), 12 and 1 (four
prefixes over eight ranks: chains, and ranks the seam rule leaves empty).  Against ONE context's zk_project_sum and
zk_spectrum_sums on the whole sets: the owned pieces together are the whole spectrum (keys and sums exact), the global integers
exact, the two doubles within (n_shared + 8) * 2**-52 * sum |term| of math.fsum over the host's terms, for both owners.
"""
import os
import sys
import threading

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.argv = sys.argv[:1]                              # _logical_ranks_gpu reads its scale from the command line
from tests import _logical_ranks_gpu as L            # noqa: E402
from tests import _spectrum_host as H                # noqa: E402
from zotmer_amd import native, parallel, synth       # noqa: E402

W = L.W
KS = (25, 12, 1)
INTS = ("cx", "cy", "n_shared", "S_min", "X_shared", "Y_shared", "S_xy")


def make_sets():
    """[(K, k-mers, counts)]"""
    sets = []
    for s in range(3):
        a = synth.config4_set_args(s, 0.0004)
        k = synth.set_keys(a["seed"], a["first"], a["count"], a["key_bits"], mul=a["mul"], add=a["add"], mod=a["mod"])
        sets.append((25, k, synth.set_counts(a["seed"], k)))
    sets.append((25, sets[0][1][[5, 9000, 17000]].copy(), np.array([3, 1, 4], dtype=np.uint64)))
    k20, c20, _ = H.host_project_sum(sets[1][1][::2], sets[1][2][::2], 10)
    sets.append((20, k20, c20))
    return sets


def files_at(sets, kk):
    return [s for s in sets if s[0] >= kk]


def dev_tensor(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64).copy()).cuda() if len(a) else torch.empty(1, dtype=torch.int64, device="cuda")


def worker(rank, owner, sets, results):
    try:
        ctx = native.Context(0)
        comm = L.ThreadComm(rank)
        out = {}
        for kk in KS:
            ex = parallel.Exchange(ctx, None, kk, owner=owner, seed=11, comm=comm)
            sp = parallel.SpectrumDist(ex)
            shards = []
            for fK, km, ct in files_at(sets, kk):
                ck, cc = np.array_split(km, W)[rank], np.array_split(ct, W)[rank]
                sp.prepare(dev_tensor(ck), dev_tensor(cc), len(ck), 2 * (fK - kk))
                shards.append(sp.local[-1][2])
            pieces = sp.exchange_all(2 * kk)
            host = []
            for kt, st, n in pieces:
                with L._device_lock:
                    torch.cuda.synchronize()
                    host.append((kt[:n].cpu().numpy().view(np.uint64).copy(), st[:n].cpu().numpy().view(np.uint64).copy()))
            out[kk] = dict(pieces=host, kept=shards, totals=list(sp.totals), rows=[sp.row(i) for i in range(len(pieces))])
        results[rank] = out
        ctx.close()
    except BaseException as e:          # noqa: BLE001
        import traceback
        L.ThreadComm.shared["err"].append("rank %d: %s" % (rank, traceback.format_exc()))
        try:
            L.ThreadComm.shared["bar"].abort()
        except Exception:               # noqa: BLE001
            pass
        raise e


def reference(sets):
    """one context on the whole sets -> {kk: ([(keys, sums, total)], {(i, j): dict})}, and the host's bound terms"""
    ref = {}
    with native.Context(0) as ctx:
        for kk in KS:
            spec = []
            for fK, km, ct in files_at(sets, kk):
                k, s, total = ctx.project_sum(ctx.upload(km), ctx.upload(ct), 2 * (fK - kk))
                spec.append((k, s, total))
            pairs = {}
            for i in range(len(spec)):
                for j in range(i + 1, len(spec)):
                    pairs[(i, j)] = ctx.spectrum_sums(spec[i][0], spec[i][1], spec[i][2], spec[j][0], spec[j][1], spec[j][2])
            ref[kk] = [(k.to_host(), s.to_host(), t) for k, s, t in spec], pairs
    return ref


def main():
    sets = make_sets()
    ref = reference(sets)
    L._serialise_library_calls()
    for owner in ("range", "hash"):
        L.ThreadComm.setup()
        results = [None] * W
        th = [threading.Thread(target=worker, args=(r, owner, sets, results)) for r in range(W)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        errs = L.ThreadComm.shared["err"]
        if errs:
            root = [e for e in errs if "BrokenBarrierError" not in e] or errs
            print("SPECTRUM-RANKS-FAILED", owner, "\n" + "\n".join(root[:2]), flush=True)
            sys.exit(1)
        note = []
        for kk in KS:
            spec, pairs = ref[kk]
            owned = [0] * W
            for f, (wk, ws, wt) in enumerate(spec):
                ks = np.concatenate([r[kk]["pieces"][f][0] for r in results])
                ss = np.concatenate([r[kk]["pieces"][f][1] for r in results])
                if owner == "hash":
                    order = np.argsort(ks, kind="stable")
                    ks, ss = ks[order], ss[order]
                assert np.array_equal(ks, wk) and np.array_equal(ss, ws), (owner, kk, f, "the owned pieces are not the whole spectrum")
                assert all(r[kk]["totals"][f] == wt for r in results), (owner, kk, f)
                # after the seam rule the ranks' own lists already add up to the spectrum's length: no key is held twice
                assert sum(r[kk]["kept"][f] for r in results) == len(wk), (owner, kk, f)
                for q, r in enumerate(results):
                    owned[q] += len(r[kk]["pieces"][f][0])
            if kk == 1:
                assert all(len(wk) <= 4 for wk, _, _ in spec)
                assert any(r[1]["kept"][0] == 0 for r in results), "no rank was left empty by the seam rule"
            assert sum(1 for r in results if r[kk]["kept"][3] == 0) >= 5          # the set of 3 k-mers
            if owner == "range" and sum(owned) > 64 * W * len(spec):
                assert max(owned) <= 1.2 * sum(owned) / W, (kk, owned)
            for (i, j), pair in pairs.items():
                want = H.host_spectrum_sums(spec[i][0], spec[i][1], spec[j][0], spec[j][1])
                eps = (want["n_shared"] + 8) * 2.0 ** -52
                got = results[0][kk]["rows"][i][j - i - 1]
                assert all(r[kk]["rows"][i][j - i - 1] == got for r in results), (owner, kk, i, j)
                assert [got[f] for f in INTS] == [want[f] for f in INTS] == [pair[f] for f in INTS], (owner, kk, i, j, got, pair)
                print("%s k %d (%d, %d): n_shared %d S_sqrt %.17g (fsum %.17g, tol %.3g) S_js %.17g (fsum %.17g, tol %.3g)" % (
                    owner, kk, i, j, want["n_shared"], got["S_sqrt"], want["S_sqrt"], eps * want["sqrt_abs"], got["S_js"], want["S_js"],
                    eps * want["js_abs"]))
                assert abs(got["S_sqrt"] - want["S_sqrt"]) <= eps * want["sqrt_abs"], (owner, kk, i, j)
                assert abs(got["S_js"] - want["S_js"]) <= eps * want["js_abs"], (owner, kk, i, j)
            note.append((kk, owned))
        print("SPECTRUM-RANKS-OK", owner, note)


if __name__ == "__main__":
    main()
