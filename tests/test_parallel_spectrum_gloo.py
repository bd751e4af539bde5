"""
The counted exchange of the multi-process `zot dist` (zotmer_amd/parallel.py: SpectrumDist, seam_verdict; library/vectors.py:
device_read_kmers_and_counts_shard, count_shard_moves) under the gloo backend on CPU tensors, worlds 2 and 3, both owners.  The
data-path arithmetic is numpy and the host forms of tests/_spectrum_host.py here (on the GPU it is libzotk); the results are
compared with the host forms over the whole sets.  The two doubles: two summation orders of n terms differ by at most
(n + 8) * 2**-52 * sum |term|, n = n_shared (the form of tests/golden/make_golden_dist_spectrum.py).
"""
import math
import os
import pickle

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import _golden as G
from tests import _spectrum_host as H
from tests.test_parallel_gloo import NumpyOps, _free_port, _init
from zotmer_amd import parallel
from zotmer_amd.library import vectors
from zotmer_amd.library.container import KmerSet

INTS = ("cx", "cy", "n_shared", "S_min", "X_shared", "Y_shared", "S_xy")


def u64(t, n, off=0):
    return t[off:off + n].numpy().view(np.uint64)


def tensor(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64).copy()) if len(a) else torch.empty(1, dtype=torch.int64)


class SpectrumNumpyOps(NumpyOps):
    """the operations SpectrumDist adds to parallel.GpuOps, with numpy"""

    def project_sum(self, k, c, n, shift):
        u, s, total = H.host_project_sum(u64(k, n), u64(c, n), shift)
        return tensor(u), tensor(s), len(u), total

    def peek(self, t, i):
        return int(u64(t, 1, i)[0])

    def add_at(self, sums_t, i, value):
        sums_t[i:i + 1].numpy().view(np.uint64)[0] += np.uint64(value)

    def spectrum_row(self, x, ys):
        out = []
        for yk, ys_, ny, cy in ys:
            d = H.host_spectrum_sums(u64(x[0], x[2]), u64(x[1], x[2]), u64(yk, ny), u64(ys_, ny))
            # the Jensen-Shannon terms take the GLOBAL totals: restated with them (the host form uses the sums of what it is given)
            fx, fy = float(x[3]), float(cy)
            xd = {int(k): int(v) for k, v in zip(u64(x[0], x[2]), u64(x[1], x[2]))}
            js = []
            for k, y in zip(u64(yk, ny), u64(ys_, ny)):
                a, b = xd.get(int(k), 0), int(y)
                if a and b:
                    js.append(a / fx * math.log(2 * fy * a / (fy * a + fx * b)))
                    js.append(b / fy * math.log(2 * fx * b / (fx * b + fy * a)))
            d["S_js"] = float(sum(js))          # a plain left-to-right sum: an order of its own, as on the device
            d["cx"], d["cy"] = x[3], cy
            out.append(d)
        return out


def the_sets():
    """three counted sets: two golden ones of K = 25 and one of K = 24 (a different file K)"""
    out = []
    for name in ("g4_part0", "g4_part1", "g3_kmerize_genome_k24"):
        info, km, ct, _, _ = G.load_case(name)
        out.append((info["K"], km, ct.astype(np.uint64)))
    return out


def _spectrum_worker(rank, world, port, outdir, owner, k):
    _init(rank, world, port)
    try:
        ex = parallel.Exchange(None, dist, k, ops=SpectrumNumpyOps(), owner=owner, seed=5)
        sp = parallel.SpectrumDist(ex)
        for fK, km, ct in the_sets():
            ck, cc = np.array_split(km, world)[rank], np.array_split(ct, world)[rank]
            sp.prepare(tensor(ck), tensor(cc), len(ck), 2 * (fK - k))
        pieces = sp.exchange_all(2 * k)
        rows = [sp.row(i) for i in range(len(pieces))]
        with open(os.path.join(outdir, "s%d.pkl" % rank), "wb") as f:
            pickle.dump(dict(pieces=[(u64(a, n).copy(), u64(b, n).copy()) for a, b, n in pieces], rows=rows, totals=sp.totals), f)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,owner,k", [(2, "range", 8), (3, "range", 1), (3, "hash", 6), (2, "hash", 12)])
def test_spectrum_dist_gloo(tmp_path, world, owner, k):
    mp.spawn(_spectrum_worker, args=(world, _free_port(), str(tmp_path), owner, k), nprocs=world, join=True)
    got = [pickle.load(open(str(tmp_path / ("s%d.pkl" % r)), "rb")) for r in range(world)]
    whole = [H.host_project_sum(km, ct, 2 * (fK - k)) for fK, km, ct in the_sets()]
    for f, (wk, ws, wt) in enumerate(whole):
        ks = np.concatenate([g["pieces"][f][0] for g in got])
        ss = np.concatenate([g["pieces"][f][1] for g in got])
        if owner == "hash":
            order = np.argsort(ks, kind="stable")
            ks, ss = ks[order], ss[order]
        assert np.array_equal(ks, wk) and np.array_equal(ss, ws), f          # the owned pieces ARE the whole spectrum
        assert all(g["totals"][f] == wt for g in got)
    for i in range(len(whole)):
        for p, j in enumerate(range(i + 1, len(whole))):
            want = H.host_spectrum_sums(whole[i][0], whole[i][1], whole[j][0], whole[j][1])
            eps = (want["n_shared"] + 8) * 2.0 ** -52
            for g in got:
                d = g["rows"][i][p]
                assert [d[f] for f in INTS] == [want[f] for f in INTS]
                assert abs(d["S_sqrt"] - want["S_sqrt"]) <= eps * want["sqrt_abs"]
                assert abs(d["S_js"] - want["S_js"]) <= eps * want["js_abs"]
            assert all(g["rows"][i][p] == got[0]["rows"][i][p] for g in got)          # every rank holds the same global dict
    assert all(g["rows"][-1] == [] for g in got)


# ---- the seam rule on hand-made tables -------------------------------------------------------------------------------------------

def apply_seams(lists):
    """lists[r] = [(key, sum)] -> what every rank keeps, by seam_verdict"""
    table = [(len(l), l[0][0], l[0][1], l[-1][0]) if l else (0, 0, 0, 0) for l in lists]
    out = []
    for r, l in enumerate(lists):
        drop, add = parallel.seam_verdict(table, r)
        l = [list(e) for e in l]
        if add:
            l[-1][1] += add
        out.append([tuple(e) for e in (l[1:] if drop else l)])
    return out


@pytest.mark.parametrize("lists", [
    [[(1, 10), (5, 1)], [(5, 2), (9, 4)]],                                          # one seam
    [[(1, 10), (5, 1)], [(6, 2), (9, 4)]],                                          # none
    [[(5, 1)], [(5, 2)], [(5, 3)], [(5, 4), (7, 1)]],                               # a chain through ranks of one key
    [[(2, 1), (5, 1)], [], [(5, 2)], [], [(5, 3)], [(8, 1)]],                       # ... and through empty ranks; the chain ends at a rank of one key
    [[], [(0, 3)], [(0, 4), (1, 1)], [(1, 2), (2, 5)], [(2, 6)], []],               # chains back to back; key 0; empty ends
    [[(0, 1)], [(0, 2)], [(1, 1)], [(1, 2)], [(2, 1)], [(2, 2)], [(3, 1)], [(3, 2)]],     # four prefixes over eight ranks
    [[], [], []],
    [[(7, 1), (8, 2), (9, 3)], [], [], [], []],                                     # three k-mers on one rank
])
def test_seam_verdict(lists):
    flat = {}
    for l in lists:
        assert all(a[0] < b[0] for a, b in zip(l, l[1:]))
        for k, s in l:
            flat[k] = flat.get(k, 0) + s
    kept = [e for l in apply_seams(lists) for e in l]
    assert kept == sorted(flat.items())          # strictly ascending over the ranks in rank order, every sum whole


def test_seam_verdict_verdicts():
    t = [(2, 1, 10, 5), (1, 5, 2, 5), (0, 0, 0, 0), (2, 5, 3, 9), (1, 9, 1, 9)]
    assert [parallel.seam_verdict(t, r) for r in range(5)] == [(False, 5), (True, 0), (False, 0), (True, 1), (True, 0)]


# ---- the sharded read ------------------------------------------------------------------------------------------------------------

def test_count_shard_moves():
    klens, clens = [3, 0, 4, 2], [1, 5, 0, 3]
    moves = [vectors.count_shard_moves(klens, clens, r) for r in range(4)]
    for r, (send, send_off, recv, recv_off) in enumerate(moves):
        assert sum(send) == clens[r] and sum(recv) == klens[r]
        assert [moves[q][2][r] for q in range(4)] == send          # what I send to q is what q receives from me
        for cnt, off, n in ((send, send_off, clens[r]), (recv, recv_off, klens[r])):
            assert all(0 <= o and o + c <= n for c, o in zip(cnt, off))
            assert all(off[q + 1] == off[q] + cnt[q] for q in range(3))          # contiguous slices in peer order
    assert moves[1][0] == [2, 0, 3, 0] and moves[2][2] == [0, 3, 0, 1]


class NumpyShardIO:
    """vectors.DeviceShardIO on CPU tensors"""

    def decode(self, words):
        vals = vectors._dec(words.tobytes(), False) if len(words) else np.zeros(0, dtype=np.uint64)
        return tensor(vals), len(vals)

    def undelta(self, t, n):
        if n == 0:
            return 0
        v = u64(t, n)
        v[:] = np.cumsum(v, dtype=np.uint64)
        return int(v[-1])

    def add(self, t, n, base):
        if n:
            u64(t, n)[:] += np.uint64(base)

    def empty(self, n):
        return torch.empty(max(int(n), 1), dtype=torch.int64)

    def before_comm(self):
        pass

    def after_comm(self):
        pass


def _read_worker(rank, world, port, outdir, path, bad):
    _init(rank, world, port)
    try:
        comm = parallel.TorchComm(dist)
        with KmerSet(path, "r") as z:
            try:
                k, c, n = vectors.device_read_kmers_and_counts_shard(None, z, rank, world, comm, io=NumpyShardIO())
            except vectors.CodecError as e:
                assert bad and "differ in length" in str(e)
                k, c, n = tensor([]), tensor([]), 0
            else:
                assert not bad
        np.savez(os.path.join(outdir, "k%d.npz" % rank), k=u64(k, n).copy(), c=u64(c, n).copy())
    finally:
        dist.destroy_process_group()


def write_set(path, K, kmers, counts):
    with KmerSet(str(path), "w") as z:
        vectors.write_kmers_and_counts(z, kmers, counts)
        z.meta.update({"K": K, "kmers": "kmers", "counts": "counts"})
    return str(path)


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_read_of_a_golden_container_gloo(tmp_path, world):
    info, km, ct, _, _ = G.load_case("g4_part0")
    ct = ct.astype(np.uint64).copy()
    ct[::7] += np.uint64(1 << 33)          # counts of different widths: the count words hold other numbers of values than the k-mer words
    path = write_set(tmp_path / "a.k25", info["K"], km, ct)
    mp.spawn(_read_worker, args=(world, _free_port(), str(tmp_path), path, False), nprocs=world, join=True)
    parts = [np.load(str(tmp_path / ("k%d.npz" % r))) for r in range(world)]
    assert all(len(p["k"]) == len(p["c"]) and len(p["k"]) > 0 for p in parts)
    assert np.array_equal(np.concatenate([p["k"] for p in parts]), km)
    assert np.array_equal(np.concatenate([p["c"] for p in parts]), ct)


def test_sharded_read_of_a_damaged_set_gloo(tmp_path):
    """one count too few: every rank raises"""
    info, km, ct, _, _ = G.load_case("g4_part0")
    with KmerSet(str(tmp_path / "bad.k25"), "w") as z:
        z.add("kmers", vectors.encode_kmers(km))
        z.add("counts", vectors.encode_counts(ct[:-1]))
        z.meta.update({"K": info["K"], "kmers": "kmers", "counts": "counts"})
    mp.spawn(_read_worker, args=(2, _free_port(), str(tmp_path), str(tmp_path / "bad.k25"), True), nprocs=2, join=True)
