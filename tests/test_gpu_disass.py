"""`zot disass` on the device: zk_contig_spectra and zk_count_spectrum against a Python dict brute force of the definition over the
same stream, at the sizes where a kernel changes path; the library's batches; the command against the reference's fixture
(tests/golden/d1_disass.json) and, for the documented deviations, against the restatement."""
import contextlib
import ctypes as C
import io
import json
import math
import os
import random
import re

import numpy as np
import pytest

from tests import _disass_restatement as R
from tests._disass_cases import argv, make_cases, write_files

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "d1_disass.json")))
CASES = make_cases()
IDS = [c["name"] for c in CASES]
ALL = 8.0            # murmer / (2^61 - 1) is below 8: a p that keeps every k-mer


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    from zotmer_amd.library import engine
    yield engine.context()
    engine.close()


def tile():
    from zotmer_amd import native
    return native.CONTIG_TILE


def test_tile_matches_the_header():
    text = open(os.path.join(ROOT, "include", "zotk.h")).read()
    assert int(re.search(r"#define ZK_CONTIG_TILE (\d+)", text).group(1)) == tile()


# ---- the brute force --------------------------------------------------------------------------------------------------------

def rc(K, x):
    y = 0
    for _ in range(K):
        y = (y << 2) | (3 - (x & 3))
        x >>= 2
    return y


def render(K, x):
    return "".join("ACGT"[(x >> (2 * (K - 1 - j))) & 3] for j in range(K))


def bins_of(d):
    h = {}
    for c in d.values():
        h[c] = h.get(c, 0) + 1
    return sorted(h.items())


class Brute:
    """the definition, record by record: the reference's dicts (disass.py:91-99) and the counted key list"""

    def __init__(self, stream, K, both, seed, p):
        assert stream == b"" or stream.endswith(b"\n")
        recs = stream.decode("latin-1").split("\n")[:-1]
        keep = {}
        self.n_records, self.n_windows = len(recs), 0
        self.words, self.keys, self.glob = [], {}, {}
        for r, seq in enumerate(recs):
            d = {}
            for x in R.kmers_list(K, seq, both):
                if x not in keep:
                    keep[x] = R.sub(seed, p, x)
                if keep[x]:
                    d[x] = d.get(x, 0) + 1
            for x in R.kmers_list(K, seq, False):
                k = min(x, rc(K, x)) if both else x
                self.keys[k] = self.keys.get(k, 0) + 1
                self.n_windows += 1
            self.words += [((r << 32) | c, f) for c, f in bins_of(d)]
            for x, c in d.items():
                self.glob[x] = self.glob.get(x, 0) + c
        self.key_list = sorted(self.keys.items())


def run_both(ctx, stream, K, both, seed=17, p=1.0, **caps):
    """the two entries on a stream -> (words+freq pairs, key list pairs, stats, global bins)"""
    d = ctx.upload_stream(stream)
    words, freq, keys, counts, st = ctx.contig_spectra(d, K, both, seed, p, **caps)
    glob = ctx.count_spectrum(keys, counts, K, both, seed, p)
    return (list(zip(words.to_host().tolist(), freq.to_host().tolist())), list(zip(keys.to_host().tolist(), counts.to_host().tolist())),
            st, glob)


def check(ctx, stream, K, both, seed=17, p=1.0):
    want = Brute(stream, K, both, seed, p)
    words, keys, st, glob = run_both(ctx, stream, K, both, seed, p)
    assert (st.n_records, st.n_windows, st.n_keys, st.n_bins) == (want.n_records, want.n_windows, len(want.key_list), len(want.words))
    assert keys == want.key_list
    assert words == want.words
    assert glob == bins_of(want.glob)
    return want


def rand_stream(rng, n_records, lo, hi, genome=None, n_rate=0.02):
    g = genome or "".join(rng.choice("ACGT") for _ in range(600))
    out = []
    for _ in range(n_records):
        L = rng.randrange(lo, hi + 1)
        p = rng.randrange(0, len(g) - L)
        s = list(g[p:p + L])
        for i in range(L):
            if rng.random() < n_rate:
                s[i] = rng.choice("Nnx-")
        out.append("".join(s))
    return ("\n".join(out) + "\n").encode()


# ---- key lengths, modes, sampling ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("both", [True, False], ids=["both", "single"])
@pytest.mark.parametrize("K", [1, 2, 16, 31, 32])
def test_k_modes_and_p(ctx, K, both):
    rng = random.Random(100 * K + both)
    stream = rand_stream(rng, 7, K, K + 250)
    if K <= 2:        # every k-mer of the length, palindromes (AT, TA, CG, GC at K = 2) and the rest, in one record and spread over others
        every = "".join(render(K, x) for x in range(4 ** K))
        stream += (every + "N" + every[::-1] + "\n" + "ATATATAT\nCG\nGC\nAC\n").encode()
    for p in (1.0, 0.5, 0.0, ALL):
        want = check(ctx, stream, K, both, 17, p)
        if p == ALL:
            assert want.glob and len(want.glob) >= len(want.keys)
            if K == 2 and both:
                assert all(want.glob[x] % 2 == 0 for x in (0b0011, 0b1100, 0b0110, 0b1001))      # AT TA CG GC: counted twice a window
        if p == 0.0:
            assert not want.words and not want.glob and want.keys
    check(ctx, stream, K, both, 5, 0.3)


def test_lowercase_u_and_bad_bytes(ctx):
    stream = b"acgtuacgtuACGUNacgtt\n\nNNNN\nacgu acgu\tacgu\n>not a base\nTTTTTTTTTT\n"
    for both in (True, False):
        check(ctx, stream, 4, both, 17, ALL)


# ---- sizes around the tile --------------------------------------------------------------------------------------------------

DK = 8          # the designed arrays: windows of 8 bases, each cut off by an N, so every window is an entry of its own


def designed(N, T, seed):
    """a stream whose sorted (key, record) array has N entries, laid out around the multiples of T:
    at T a (key, record) run straddles the border; at 2T a key's run straddles it with the record changing exactly there;
    entry 3T - 1 is a run of one.  -> (stream, the sorted entries)"""
    rng = random.Random(seed)
    canon = sorted(x for x in rng.sample(range(4 ** DK), 3 * N + 64) if x < rc(DK, x))[:N + 16]
    n_rec = 37
    runs, pos, ki, last_rec = [], 0, 0, n_rec

    def put(new_key, rec, n):
        nonlocal pos, ki, last_rec
        n = min(n, N - pos)
        if n <= 0:
            return
        if new_key:
            ki += 1
        runs.append((canon[ki], rec, n))
        pos, last_rec = pos + n, rec

    def fill(to):
        while pos < min(to, N):
            n = min(rng.choice([1, 1, 2, 3]), to - pos)
            if last_rec < n_rec - 1 and rng.random() < 0.4:
                put(False, rng.randrange(last_rec + 1, n_rec), n)          # the same key in a later record
            else:
                put(True, rng.randrange(n_rec), n)

    fill(T - 3)
    put(True, 5, 5)                          # T - 3 .. T + 2: one run over the border
    fill(2 * T - 4)
    put(True, 7, 4)                          # ... 2T: the key goes on,
    put(False, 9, 3)                         # the record changes exactly at 2T
    fill(3 * T - 1)
    put(True, 11, 1)                         # 3T - 1: a run of one, the tile's last entry
    put(True, 11, 2)
    fill(N)
    assert pos == N
    per_rec = [[] for _ in range(n_rec)]
    for key, rec, n in runs:
        per_rec[rec] += [render(DK, key)] * n
    for l in per_rec:
        rng.shuffle(l)
    stream = ("\n".join("N".join(l) for l in per_rec) + "\n").encode()
    entries = [(key, rec) for key, rec, n in runs for _ in range(n)]
    assert entries == sorted(entries)
    return stream, entries


@pytest.mark.parametrize("both", [True, False], ids=["both", "single"])
@pytest.mark.parametrize("which", range(4))
def test_sizes_around_the_tile(ctx, which, both):
    T = tile()
    N = [T - 1, T, T + 1, 3 * T + 5][which]
    stream, e = designed(N, T, 40 + which)
    if N > T:
        assert e[T - 1] == e[T]                                                     # a (key, record) run over the border
    if N > 2 * T:
        assert e[2 * T - 1][0] == e[2 * T][0] and e[2 * T - 1][1] != e[2 * T][1]      # the record changes exactly at the border
        assert e[2 * T - 2] == e[2 * T - 1] and e[2 * T] == e[2 * T + 1]
    if N > 3 * T:
        assert e[3 * T - 2] != e[3 * T - 1] != e[3 * T]                              # a tile's last entry is a run of one
    want = check(ctx, stream, DK, both, 17, ALL)
    assert want.n_windows == N
    check(ctx, stream, DK, both, 17, 1.0)


@pytest.mark.parametrize("both", [True, False], ids=["both", "single"])
def test_one_run_longer_than_two_tiles(ctx, both):
    T, K = tile(), 11
    stream = ("ACGTACGTACGTAGG\n" + "A" * (2 * T + K + 99) + "\n" + "AAAAAAAAAAAAC\n").encode()
    want = check(ctx, stream, K, both, 17, ALL)
    assert max(want.keys.values()) == 2 * T + 100 + 2 and ((1 << 32) | (2 * T + 100), 2 if both else 1) in want.words


def test_records_without_windows(ctx):
    K = 9
    body = rand_stream(random.Random(7), 4, 30, 60, n_rate=0.0).decode().split("\n")[:-1]
    recs = ["", "ACGT", body[0], "", "NNNNNNNNNNNNNNNN", body[1], body[2], "ACGTACGT", "", ""]
    stream = ("\n".join(recs) + "\n").encode()
    for both in (True, False):
        want = check(ctx, stream, K, both, 17, ALL)
        assert want.n_records == len(recs)
        assert {w >> 32 for w, _ in want.words} == {2, 5, 6}


def test_many_records(ctx):
    """70 000 records of K + 1 bases: record numbers past 16 bits, many bins, more than one tile of everything"""
    K, n = 16, 70000
    rng = random.Random(99)
    g = "".join(rng.choice("ACGT") for _ in range(3000))
    recs = []
    for i in range(n):
        p = rng.randrange(0, len(g) - K - 1)
        s = g[p:p + K + 1]
        recs.append(s[:K] + s[K - 1] if i % 7 == 0 else s)
    recs[12345] = "A" * (K + 1)
    recs[65536] = "AC" * 8 + "A"
    stream = ("\n".join(recs) + "\n").encode()
    want = check(ctx, stream, K, True, 17, ALL)
    assert want.n_windows == 2 * n and len(want.words) >= n and max(w >> 32 for w, _ in want.words) == n - 1
    check(ctx, stream, K, False, 17, 1.0)


def test_empty_stream_and_one_newline(ctx):
    for both in (True, False):
        words, keys, st, glob = run_both(ctx, b"", 25, both)
        assert (words, keys, glob) == ([], [], []) and (st.n_records, st.n_windows, st.n_keys, st.n_bins) == (0, 0, 0, 0)
        words, keys, st, glob = run_both(ctx, b"\n", 25, both)
        assert (words, keys, glob) == ([], [], []) and (st.n_records, st.n_windows, st.n_keys, st.n_bins) == (1, 0, 0, 0)


def test_same_call_same_bits(ctx):
    stream = rand_stream(random.Random(3), 300, 40, 400)
    a = run_both(ctx, stream, 13, True, 17, 1.0)
    b = run_both(ctx, stream, 13, True, 17, 1.0)
    assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3]


def test_counts_of_64_bits(ctx):
    from zotmer_amd import native
    K = 6
    keys = sorted(random.Random(5).sample(range(4 ** K), 300))
    pal = [x for x in range(4 ** K) if rc(K, x) == x][:20]
    canon = sorted(set(min(x, rc(K, x)) for x in keys) | set(pal))
    rng = random.Random(6)
    counts = [rng.choice([1, 2, 3, (1 << 33) + 5, (1 << 40), 4095, 4096, 4097]) for _ in canon]
    for both, ks in ((True, canon), (False, keys)):
        cs = counts[:len(ks)]
        d = {}
        for x, c in zip(ks, cs):
            if both and rc(K, x) == x:
                if R.sub(17, 1.0, x):
                    d[x] = 2 * c
            else:
                for y in ([x, rc(K, x)] if both else [x]):
                    if R.sub(17, 1.0, y):
                        d[y] = c
        got = ctx.count_spectrum(ctx.upload(np.array(ks, dtype=np.uint64)), ctx.upload(np.array(cs, dtype=np.uint64)), K, both, 17, 1.0)
        assert got == bins_of(d) and got
    # a palindrome whose doubled count does not fit
    k, c = ctx.upload(np.array([pal[0]], dtype=np.uint64)), ctx.upload(np.array([1 << 63], dtype=np.uint64))
    vals, freq, n = np.zeros(4, np.uint64), np.zeros(4, np.uint64), C.c_uint64(0)
    rc_ = ctx.lib.zk_count_spectrum(ctx.h, k.ptr, c.ptr, 64, 1, K, 1, 17, ALL, vals.ctypes.data_as(native._pu64), freq.ctypes.data_as(native._pu64), 4,
                                    C.byref(n))
    assert rc_ == native.ZK_EOVERFLOW


def test_count_spectrum_more_bins_than_room(ctx):
    from zotmer_amd import native
    K, n = 12, 5000
    ks = np.arange(n, dtype=np.uint64)
    cs = (np.arange(n, dtype=np.uint32) % 3000) + 1
    d = {}
    for x, c in zip(ks.tolist(), cs.tolist()):
        if R.sub(17, ALL, x):
            d[x] = c
    want = bins_of(d)
    dk, dc = ctx.upload(ks), ctx.upload(cs)
    vals, freq, nb = np.zeros(10, np.uint64), np.zeros(10, np.uint64), C.c_uint64(0)
    rc_ = ctx.lib.zk_count_spectrum(ctx.h, dk.ptr, dc.ptr, 32, n, K, 0, 17, ALL, vals.ctypes.data_as(native._pu64), freq.ctypes.data_as(native._pu64), 10,
                                    C.byref(nb))
    assert rc_ == native.ZK_ENOSPC and nb.value == len(want) == 3000
    assert list(zip(vals.tolist(), freq.tolist())) == want[:10]
    assert ctx.count_spectrum(dk, dc, K, False, 17, ALL) == want


# ---- capacities and refusals ------------------------------------------------------------------------------------------------

def raw_call(ctx, d, K, both, seed, p, cap_bins, cap_keys):
    from zotmer_amd import native
    words, freq = ctx.empty(cap_bins, np.uint64), ctx.empty(cap_bins, np.uint64)
    keys, counts = ctx.empty(cap_keys, np.uint64), ctx.empty(cap_keys, np.uint32)
    st = native.ContigStats()
    rc_ = ctx.lib.zk_contig_spectra(ctx.h, d.ptr if d is not None else None, d.n if d is not None else 0, K, int(both), seed, p,
                                    words.ptr, freq.ptr, cap_bins, keys.ptr, counts.ptr, cap_keys, C.byref(st))
    return rc_, st, words, freq, keys, counts


def test_enospc_on_each_capacity(ctx):
    from zotmer_amd import native
    stream = rand_stream(random.Random(11), 40, 40, 200)
    want = Brute(stream, 9, True, 17, ALL)
    nb, nk = len(want.words), len(want.key_list)
    d = ctx.upload_stream(stream)
    for cb, ck in ((nb - 1, nk), (nb, nk - 1), (0, 0), (1, 1)):
        rc_, st, *_ = raw_call(ctx, d, 9, True, 17, ALL, cb, ck)
        assert rc_ == native.ZK_ENOSPC and (st.n_bins, st.n_keys, st.n_records, st.n_windows) == (nb, nk, 40, want.n_windows)
        assert b"%d bins and %d keys" % (nb, nk) in ctx.lib.zk_last_error(ctx.h)
    rc_, st, words, freq, keys, counts = raw_call(ctx, d, 9, True, 17, ALL, nb, nk)            # the sizes reported are enough
    assert rc_ == 0
    assert list(zip(words.to_host().tolist(), freq.to_host().tolist())) == want.words
    assert list(zip(keys.to_host().tolist(), counts.to_host().tolist())) == want.key_list
    # the array that fits is written even when the other does not
    rc_, st, words, freq, keys, counts = raw_call(ctx, d, 9, True, 17, ALL, nb, 0)
    assert rc_ == native.ZK_ENOSPC and list(zip(words.to_host().tolist(), freq.to_host().tolist())) == want.words
    # and the binding grows what was too small
    w, f, k, c, st = ctx.contig_spectra(d, 9, True, 17, ALL, cap_bins=1, cap_keys=1)
    assert list(zip(w.to_host().tolist(), f.to_host().tolist())) == want.words and k.n == nk


def test_refused_arguments(ctx):
    from zotmer_amd import native
    d = ctx.upload_stream(b"ACGTACGTACGT\n")
    for K, p in ((0, 1.0), (33, 1.0), (-1, 1.0), (25, float("nan")), (25, float("inf")), (25, -float("inf"))):
        rc_, st, *_ = raw_call(ctx, d, K, True, 17, p, 16, 16)
        assert rc_ == native.ZK_EINVAL, (K, p)
        vals, freq, n = np.zeros(4, np.uint64), np.zeros(4, np.uint64), C.c_uint64(0)
        keys, counts = ctx.upload(np.array([1, 2], dtype=np.uint64)), ctx.upload(np.array([1, 1], dtype=np.uint32))
        assert ctx.lib.zk_count_spectrum(ctx.h, keys.ptr, counts.ptr, 32, 2, K, 1, 17, p, vals.ctypes.data_as(native._pu64),
                                         freq.ctypes.data_as(native._pu64), 4, C.byref(n)) == native.ZK_EINVAL
    assert ctx.lib.zk_count_spectrum(ctx.h, keys.ptr, counts.ptr, 16, 2, 5, 1, 17, 1.0, vals.ctypes.data_as(native._pu64),
                                     freq.ctypes.data_as(native._pu64), 4, C.byref(n)) == native.ZK_EINVAL
    rc_, st, *_ = raw_call(ctx, ctx.upload_stream(b"ACGTACGTACGT\nACGT"), 4, True, 17, 1.0, 16, 16)       # the last record is not ended
    assert rc_ == native.ZK_EINVAL and b"'\\n'" in ctx.lib.zk_last_error(ctx.h)
    check(ctx, b"ACGTACGTACGT\n", 4, True, 17, ALL)          # the context is as good as before


# ---- the library ------------------------------------------------------------------------------------------------------------

def records_of(rng, lengths):
    g = "".join(rng.choice("ACGT") for _ in range(2000))
    out = []
    for i, L in enumerate(lengths):
        p = rng.randrange(0, len(g) - L)
        out.append(("r%d" % i, g[p:p + L].encode()))
    return out


def test_batches_equal_one_batch(ctx, monkeypatch):
    from zotmer_amd.library import disass
    K = 12
    recs = records_of(random.Random(21), [100, 150, 90, 700, 120, 80, 60, 130, 11, 5, 140])
    one = disass.spectra(ctx, recs, K, True, 17, ALL)
    calls = []
    real = ctx.contig_spectra
    monkeypatch.setattr(ctx, "contig_spectra", lambda d, *a, **k: calls.append(d.n) or real(d, *a, **k), raising=False)
    cut = disass.spectra(ctx, recs, K, True, 17, ALL, budget=300)
    sizes = [[len(s) for _, s in b] for b in disass.pack_batches(recs, K, 300, 10 ** 9)]
    assert len(calls) == len(sizes) >= 4 and [700] in sizes                       # three batches and more, one record over the budget alone
    assert cut == one
    names, bins, glob = one
    want = Brute(b"".join(s + b"\n" for _, s in recs), K, True, 17, ALL)
    assert names == [nm for nm, _ in recs] and glob == bins_of(want.glob)
    assert [((r << 32) | c, f) for r, b in enumerate(bins) for c, f in b] == want.words
    # a record that cannot fit the device is named with both sizes
    monkeypatch.setattr(disass, "device_limit", lambda ctx: 500)
    with pytest.raises(disass.TooLarge) as e:
        disass.spectra(ctx, recs, K, True, 17, ALL, budget=300)
    assert '"r3"' in str(e.value) and "689" in str(e.value) and "500" in str(e.value)


def test_counts_widen_past_the_threshold(ctx, monkeypatch):
    from zotmer_amd.library import disass
    K = 12
    recs = records_of(random.Random(22), [200] * 9)
    one = disass.spectra(ctx, recs, K, False, 17, ALL)
    seen = []
    real = ctx.union_sum
    monkeypatch.setattr(ctx, "union_sum", lambda xk, xc, yk, yc, **k: seen.append((xc.dtype.itemsize, yc.dtype.itemsize)) or real(xk, xc, yk, yc, **k),
                        raising=False)
    assert disass.spectra(ctx, recs, K, False, 17, ALL, budget=200) == one
    assert seen and all(s == (4, 4) for s in seen)
    del seen[:]
    monkeypatch.setattr(disass, "WIDEN_AT", 4 * 189)          # the window total of a merge of two pairs of batches
    assert disass.spectra(ctx, recs, K, False, 17, ALL, budget=200) == one
    assert (4, 4) in seen and (8, 8) in seen


# ---- the command ------------------------------------------------------------------------------------------------------------

def zot(args):
    from zotmer_amd import cli
    out, err = io.StringIO(), io.StringIO()
    code = None
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            code = cli.main_inner(args)
        except SystemExit as e:
            code = e.code
    return code, out.getvalue(), err.getvalue()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixture(ctx, tmp_path, monkeypatch, case):
    from zotmer_amd.library import disass
    write_files(case, str(tmp_path))
    monkeypatch.chdir(tmp_path)
    code, out, err = zot(["disass"] + argv(case))
    assert (code, err) == (0, "")
    assert out == disass.dump_yaml(GOLD[case["name"]])


def test_verbose_changes_nothing(ctx, tmp_path, monkeypatch):
    case = CASES[0]
    write_files(case, str(tmp_path))
    monkeypatch.chdir(tmp_path)
    assert zot(["disass", "-v"] + argv(case)) == zot(["disass"] + argv(case))


def test_deviations_follow_the_restatement(ctx, tmp_path, monkeypatch):
    from zotmer_amd.library import disass
    monkeypatch.chdir(tmp_path)
    # exactly one distinct k-mer in a contig, and in a file: median = float(count) where the reference dies
    text = ">one\n" + "A" * 30 + "\n>more\nACGTTGCAAGGCTTAACCGGTTAGCATCGA\n"
    (tmp_path / "one.fa").write_text(text)
    (tmp_path / "only.fa").write_text(">only\n" + "C" * 40 + "\n")
    with pytest.raises(IndexError):
        R.disass([("one.fa", text)], K=25, P=ALL, both=False)
    code, out, err = zot(["disass", "-s", "-p", "8", "one.fa", "only.fa"])
    want = R.disass([("one.fa", text), ("only.fa", ">only\n" + "C" * 40 + "\n")], K=25, P=ALL, both=False, single_ok=True)
    assert (code, err) == (0, "") and out == disass.dump_yaml(want)
    assert want[0]["contigs"][0]["median"] == 6.0 and want[1]["global"]["median"] == 16.0
    # quantiles in ascending count, for count values that collide in a small hash table (1, 9, 17 modulo 8)
    seq = "ACGTTGCAAGGCTTAACCGGTTAGCATCGATTTGACCA"
    text = ">q\n" + "N".join([seq[:12]] * 17 + [seq[13:25]] * 9 + [seq[26:38]]) + "\n"
    (tmp_path / "q.fa").write_text(text)
    code, out, err = zot(["disass", "-s", "-k", "12", "-p", "8", "-q", "7", "q.fa"])
    want = R.disass([("q.fa", text)], K=12, P=ALL, Q=7, both=False)
    assert (code, err) == (0, "") and out == disass.dump_yaml(want)
    assert want[0]["global"]["histogram"] == [[1, 1], [9, 1], [17, 1]] and want[0]["global"]["quantiles"] == sorted(want[0]["global"]["quantiles"])
    assert math.isclose(want[0]["global"]["mean"], 9.0)
