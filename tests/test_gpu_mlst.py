"""`zot mlst` on the device: zk_bait_tally, zk_bait_record_sizes, zk_bait_table_arrays and zk_bait_table_from_arrays
(csrc/allele_tally.hip) against a numpy brute force (np.isin on the keys, np.add.at over the postings) at the sizes where the
kernel changes path, and the command against the reference's fixtures (tests/golden/m1_mlst.json)."""
import base64
import contextlib
import io
import json
import os
import re
import zipfile

import numpy as np
import pytest

from tests._mlst_cases import make_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "m1_mlst.json")
INPUTS = {c["name"]: c for c in make_cases()}
CASES = [dict(INPUTS[c["name"]], **c) for c in json.load(open(GOLD))]
IDS = [c["name"] for c in CASES]
U32 = np.uint32


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    from zotmer_amd.library import engine
    yield engine.context()
    engine.close()


def tile():
    from zotmer_amd import native
    return native.TALLY_TILE


def short_bound():
    """the longest list a lane adds itself (csrc/allele_tally.hip)"""
    text = open(os.path.join(ROOT, "zotmer_amd", "csrc", "allele_tally.hip")).read()
    return int(re.search(r"constexpr u32 TL_SHORT = (\d+);", text).group(1))


def test_tile_matches_the_header():
    text = open(os.path.join(ROOT, "include", "zotk.h")).read()
    assert int(re.search(r"#define ZK_TALLY_TILE (\d+)", text).group(1)) == tile()


# ---- tables and the brute force -----------------------------------------------------------------------------------------

class Arrays:
    def __init__(self, K, keys, lists, n_records):
        self.K, self.n_records = K, n_records
        self.keys = np.asarray(keys, dtype=np.uint64)
        self.offs = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(U32)
        self.ids = (np.concatenate(lists) if len(lists) else np.empty(0)).astype(U32)

    def table(self, ctx):
        return ctx.bait_table_from_arrays(self.K, ctx.upload(self.keys), ctx.upload(self.offs), ctx.upload(self.ids), self.n_records)

    def sizes(self):
        return np.bincount(self.ids, minlength=self.n_records).astype(U32)

    def brute(self, kmers):
        m = np.isin(self.keys, np.asarray(kmers, dtype=np.uint64))          # an entry repeated in the set counts once
        hits = np.zeros(self.n_records, dtype=U32)
        np.add.at(hits, self.ids[np.repeat(m, np.diff(self.offs))], 1)
        return hits, int(m.sum())


def rand_keys(rng, K, n, lo=0, hi=None):
    """n distinct values of [lo, hi) (hi = 4^K by default), ascending"""
    hi = (1 << (2 * K)) if hi is None else hi
    got = set()
    while len(got) < n:
        got.update((int(a) << 32 | int(b)) % (hi - lo) + lo for a, b in zip(rng.integers(0, 1 << 32, size=n), rng.integers(0, 1 << 32, size=n)))
    return np.sort(rng.permutation(np.array(sorted(got), dtype=np.uint64))[:n])


def make_arrays(seed, K, n_keys, n_records, lengths, lo=0, hi=None):
    rng = np.random.default_rng(seed)
    keys = rand_keys(rng, K, n_keys, lo, hi)
    lists = [np.sort(rng.choice(n_records, size=min(lengths[i % len(lengths)], n_records), replace=False)) for i in range(len(keys))]
    return Arrays(K, keys, lists, n_records)


def make_set(rng, arr, n, K, share=3):
    """n ascending distinct k-mers: a share of them keys, the first and the last key among them, entries below the first key and
    above the last, the rest other values"""
    keys = arr.keys
    if n == 0:
        return np.empty(0, dtype=np.uint64)
    if n == 1:
        return keys[:1].copy()
    pick = {int(keys[0]), int(keys[-1])}
    pick.update(int(x) for x in rng.choice(keys, size=min(len(keys), max(n // share, 1)), replace=False))
    pick = set(sorted(pick)[:max(n - 4, 2)]) | {int(keys[0]), int(keys[-1])}
    out = set(pick)
    if int(keys[0]) > 1:
        out.update([0, int(keys[0]) - 1])
    top = (1 << (2 * K)) - 1
    if int(keys[-1]) < top - 1:
        out.update([top, int(keys[-1]) + 1])
    known = set(int(x) for x in keys)
    while len(out) < n:
        x = (int(rng.integers(0, 1 << 32)) << 32 | int(rng.integers(0, 1 << 32))) & top
        if x not in known:
            out.add(x)
    out = sorted(out)
    while len(out) > n:                     # drop others than the two ends
        out.pop(len(out) // 2)
    return np.array(out, dtype=np.uint64)


def tally(ctx, table, kmers):
    return ctx.bait_tally(table, ctx.upload(np.asarray(kmers, dtype=np.uint64))).to_host()


def lengths_around_the_bound():
    s = short_bound()
    return [1, 1, 2, 1, s, s + 1, 1, 3, 63, 64, 65, 200, 1, 2, s - 1 if s > 1 else 1, s + 2]


@pytest.fixture(scope="module")
def big(ctx):
    arr = make_arrays(11, 25, 1500, 300, lengths_around_the_bound(), lo=1 << 20, hi=(1 << 50) - (1 << 20))
    return arr, arr.table(ctx)


@pytest.mark.parametrize("which", range(9))
def test_tally_sizes(ctx, big, which):
    T = tile()
    n = [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17][which]
    arr, table = big
    assert (table.n_keys, table.n_ids, table.n_records) == (len(arr.keys), len(arr.ids), 300)
    assert {1, short_bound(), short_bound() + 1, 63, 64, 65, 200} <= set(np.diff(arr.offs).tolist())
    kmers = make_set(np.random.default_rng(100 + n), arr, n, 25)
    assert len(kmers) == n and np.all(kmers[1:] > kmers[:-1])
    want, matched = arr.brute(kmers)
    if n >= 64:
        assert kmers[0] < arr.keys[0] and kmers[-1] > arr.keys[-1] and matched >= min(n // 4, len(arr.keys) // 2)
        assert arr.keys[0] in kmers and arr.keys[-1] in kmers
    got = tally(ctx, table, kmers)
    assert got.dtype == U32 and np.array_equal(got, want)
    assert int(got.sum()) <= len(arr.ids)


@pytest.mark.parametrize("K", [1, 2, 16, 25, 32])
def test_tally_k(ctx, K):
    n_keys = {1: 3, 2: 11}.get(K, 700)
    arr = make_arrays(50 + K, K, n_keys, 40, [1, 2, 7, 33, 1, 40])
    table = arr.table(ctx)
    rng = np.random.default_rng(K)
    if K == 32:
        assert (arr.keys >> np.uint64(63)).sum() > 100 and (arr.keys >> np.uint64(63) == 0).sum() > 100
    for n in ((2, 4) if K == 1 else (5, 16) if K == 2 else (65, tile() + 1)):
        if K <= 2:
            kmers = np.sort(rng.choice(1 << (2 * K), size=n, replace=False)).astype(np.uint64)
        else:
            kmers = make_set(rng, arr, n, K, share=2)
        want, matched = arr.brute(kmers)
        assert matched > 0
        assert np.array_equal(tally(ctx, table, kmers), want), (K, n)


def test_clustered_keys_and_empty_stretches(ctx):
    """3000 consecutive values under one directory bucket, a few keys far away, long empty stretches in between"""
    K, rng = 25, np.random.default_rng(3)
    base = 0x2345678 << 20
    keys = np.concatenate([[5, 77], base + np.arange(3000), [(1 << 50) - 9, (1 << 50) - 1]]).astype(np.uint64)
    lists = [np.sort(rng.choice(50, size=1 + i % 6, replace=False)) for i in range(len(keys))]
    arr = Arrays(K, keys, lists, 50)
    table = arr.table(ctx)
    stretch = np.sort(rng.integers(100, base - 1, size=2000).astype(np.uint64))
    after = np.sort(rng.integers(base + 3000, (1 << 50) - 10, size=2000).astype(np.uint64))
    kmers = np.unique(np.concatenate([[5], stretch, base + np.arange(0, 3000, 2), [base + 2999, base + 3000], after, [(1 << 50) - 1]]).astype(np.uint64))
    want, matched = arr.brute(kmers)
    assert matched == 1 + 1500 + 1 + 1
    assert np.array_equal(tally(ctx, table, kmers), want)


def test_many_lanes_add_to_one_address(ctx):
    rng = np.random.default_rng(8)
    keys = rand_keys(rng, 27, 5000)
    lists = [np.array([0, 1 + i % 99]) for i in range(5000)]
    arr = Arrays(27, keys, lists, 100)
    table = arr.table(ctx)
    kmers = make_set(rng, arr, 2 * tile() + 5, 27, share=1)
    want, matched = arr.brute(kmers)
    got = tally(ctx, table, kmers)
    assert matched > 3000 and got[0] == matched and np.array_equal(got, want)


def test_set_equal_to_the_keys_and_minus_one(ctx, big):
    arr, table = big
    sizes = ctx.bait_record_sizes(table).to_host()
    assert np.array_equal(sizes, arr.sizes())
    assert np.array_equal(tally(ctx, table, arr.keys), sizes)          # every record complete
    i = int(np.argmax(np.diff(arr.offs) == 65))
    got = tally(ctx, table, np.delete(arr.keys, i))
    listed = arr.ids[arr.offs[i]:arr.offs[i + 1]]
    assert len(listed) == 65 and np.array_equal(np.nonzero(got != sizes)[0], np.sort(listed))
    assert np.array_equal(got, arr.brute(np.delete(arr.keys, i))[0])
    from zotmer_amd.library import mlst
    lens = ctx.bait_record_sizes(table)
    assert np.array_equal(mlst.complete(ctx, table, lens, ctx.upload(arr.keys)), np.arange(300))
    assert np.array_equal(mlst.complete(ctx, table, lens, ctx.upload(np.delete(arr.keys, i))), np.setdiff1d(np.arange(300), listed))


def test_repeated_entries_count_once(ctx, big):
    arr, table = big
    rng = np.random.default_rng(21)
    kmers = make_set(rng, arr, tile() + 300, 25)
    rep = np.sort(np.concatenate([kmers, kmers[::3], kmers[::3], arr.keys[:5], kmers[255:258], kmers[tile() - 1:tile() + 1]]))
    assert len(rep) > len(np.unique(rep)) + 1000 and np.all(rep[1:] >= rep[:-1])
    want, matched = arr.brute(np.unique(rep))
    assert matched > 500 and np.array_equal(tally(ctx, table, rep), want)


def test_empty_table_no_records_and_no_entries(ctx, big):
    from zotmer_amd import native
    empty = Arrays(25, [], [], 5)
    t = empty.table(ctx)
    assert (t.n_keys, t.n_ids, t.n_records) == (0, 0, 5)
    assert tally(ctx, t, [1, 2, 3]).tolist() == [0] * 5 and ctx.bait_record_sizes(t).to_host().tolist() == [0] * 5
    t0 = Arrays(25, [], [], 0).table(ctx)
    assert t0.n_records == 0
    assert ctx.lib.zk_bait_tally(ctx.h, t0.h, ctx.upload(np.arange(3, dtype=np.uint64)).ptr, 3, None) == 0
    assert ctx.lib.zk_bait_record_sizes(ctx.h, t0.h, None) == 0
    arr, table = big
    hits = ctx.upload(np.full(301, 7, dtype=U32))
    assert ctx.lib.zk_bait_tally(ctx.h, table.h, None, 0, hits.ptr) == 0
    assert hits.to_host().tolist() == [0] * 300 + [7]                    # n_records words, overwritten
    # a record that no key lists
    a = Arrays(9, [3, 9], [np.array([0, 4]), np.array([4])], 7)
    assert ctx.bait_record_sizes(a.table(ctx)).to_host().tolist() == [1, 0, 0, 0, 2, 0, 0]
    assert tally(ctx, a.table(ctx), [9]).tolist() == [0, 0, 0, 0, 1, 0, 0]
    assert native.ZK_OK == 0


@pytest.mark.parametrize("K", [12, 32])
def test_a_table_of_one_key(ctx, K):
    """the directory at its smallest (two buckets, one key): entries below the key, equal to it and above it, at both ends of the
    key range, and -- below K = 32 -- entries with bits above the 2K of a k-mer, which no bucket answers for"""
    top = (1 << (2 * K)) - 1
    for key in (0, 1, 0x5A5A5A, top >> 1, (top >> 1) + 1, top - 1, top):
        t = Arrays(K, [key], [np.array([1])], 3).table(ctx)
        assert (t.n_keys, t.n_ids) == (1, 1)
        others = {0, 1, key - 1, key + 1, top >> 1, (top >> 1) + 1, top - 1, top} - {key, -1, top + 1}
        if K < 32:
            others |= {key | (1 << (2 * K)), key | (1 << 63), (1 << 64) - 1}
        for x in sorted(others):
            assert tally(ctx, t, [x]).tolist() == [0, 0, 0], (key, x)
        assert tally(ctx, t, [key]).tolist() == [0, 1, 0], key
        assert tally(ctx, t, sorted(others | {key})).tolist() == [0, 1, 0], key


def test_same_call_same_bits_and_a_fresh_context(ctx, big):
    from zotmer_amd import native
    arr, table = big
    kmers = make_set(np.random.default_rng(77), arr, 3 * tile() + 17, 25)
    want, _ = arr.brute(kmers)
    d = ctx.upload(kmers)
    first = ctx.bait_tally(table, d).to_host()
    other = make_arrays(5, 16, 100, 20, [1, 9])
    tally(ctx, other.table(ctx), other.keys)
    again = ctx.bait_tally(table, d).to_host()
    assert np.array_equal(first, want) and np.array_equal(again, want)
    with native.Context(0) as fresh:
        assert np.array_equal(fresh.bait_tally(arr.table(fresh), fresh.upload(kmers)).to_host(), want)


# ---- a built table out of the device and back ---------------------------------------------------------------------------

def test_arrays_round_trip(ctx):
    case = CASES[1]
    assert case["K"] == 27
    from tests import _mlst_restatement as R
    seqs = [s for _, text in case["files"] for _, s in R.read_fasta(text)]
    stream = "".join(s + "\n" for s in seqs).encode()
    built = ctx.bait_table(ctx.upload_stream(stream), 27)
    keys, offs, ids = (a.to_host() for a in built.arrays())
    assert keys.tolist() == case["S"] and offs.tolist() == case["T"] and ids.tolist() == case["U"]
    assert ctx.bait_record_sizes(built).to_host().tolist() == case["lens"]
    back = ctx.bait_table_from_arrays(27, ctx.upload(keys), ctx.upload(offs), ctx.upload(ids), built.n_records)
    assert (back.n_keys, back.n_ids, back.n_records) == (built.n_keys, built.n_ids, built.n_records) == (len(keys), len(ids), len(seqs))
    assert all(np.array_equal(a.to_host(), b.to_host()) for a, b in zip(built.arrays(), back.arrays()))
    for _, xs, _ in case["samples"]:
        d = ctx.upload(np.array(xs, dtype=np.uint64))
        assert np.array_equal(ctx.bait_tally(built, d).to_host(), ctx.bait_tally(back, d).to_host())
    # zk_capture_hits sees the same table through both
    reads = [seqs[1][3:60], seqs[4][10:70], "ACGT" * 15, seqs[10][:50], seqs[0][5:45] + "N" + seqs[11][2:40]]
    text = ctx.upload_stream("".join("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)) for i, r in enumerate(reads)).encode())
    lines = ctx.line_ends(text)
    p1 = ctx.capture_hits(built, 27, text, lines, len(reads)).to_host()
    p2 = ctx.capture_hits(back, 27, text, lines, len(reads)).to_host()
    assert len(p1) >= 6 and np.array_equal(p1, p2)


def from_arrays_rc(ctx, K, keys, offs, ids, n_records, n_keys=None, n_ids=None):
    from zotmer_amd import native
    h = native.C.c_void_p(0xDEAD)
    k, o, i = ctx.upload(np.asarray(keys, np.uint64)), ctx.upload(np.asarray(offs, U32)), ctx.upload(np.asarray(ids, U32))
    rc = ctx.lib.zk_bait_table_from_arrays(ctx.h, K, k.ptr, len(keys) if n_keys is None else n_keys, o.ptr, i.ptr,
                                           len(ids) if n_ids is None else n_ids, n_records, native.C.byref(h))
    return rc, h.value, ctx.lib.zk_last_error(ctx.h)


GOOD = dict(K=9, keys=[3, 8, 20, 4 ** 9 - 1], offs=[0, 2, 3, 6, 7], ids=[1, 5, 0, 0, 2, 6, 6], n_records=7)
BREAKS = {
    "keys_equal": dict(keys=[3, 8, 8, 4 ** 9 - 1]),
    "keys_descending": dict(keys=[3, 20, 8, 4 ** 9 - 1]),
    "key_too_large": dict(keys=[3, 8, 20, 4 ** 9]),
    "offs0": dict(offs=[1, 2, 3, 6, 7]),
    "empty_list": dict(offs=[0, 2, 2, 6, 7]),
    "offs_descending": dict(offs=[0, 3, 2, 6, 7]),
    "offs_last": dict(offs=[0, 2, 3, 6, 8]),
    "id_is_n_records": dict(ids=[1, 5, 0, 0, 2, 7, 6]),
    "ids_descending": dict(ids=[1, 5, 0, 2, 0, 6, 6]),
    "ids_equal": dict(ids=[1, 1, 0, 0, 2, 6, 6]),
    "K0": dict(K=0),
    "K33": dict(K=33),
}


def test_from_arrays_takes_the_good_arrays(ctx):
    rc, h, _ = from_arrays_rc(ctx, **GOOD)
    assert rc == 0 and h not in (0, None, 0xDEAD)
    ctx.lib.zk_bait_table_free(h)
    # ids that descend across two keys are fine: each key's list ascends
    assert GOOD["ids"][1] > GOOD["ids"][2]


@pytest.mark.parametrize("name", sorted(BREAKS))
def test_from_arrays_refuses_each_broken_rule(ctx, name):
    from zotmer_amd import native
    rc, h, msg = from_arrays_rc(ctx, **dict(GOOD, **BREAKS[name]))
    assert rc == native.ZK_EINVAL and h == 0xDEAD and b"zk_bait_table_from_arrays" in msg, (name, msg)
    words = {"keys": b"keys are not strictly ascending", "key_": b"below 4^K", "offs0": b"offs[0]", "empty": b"strictly increasing",
             "offs_d": b"strictly increasing", "offs_l": b"offs[n_keys]", "id_is": b"below n_records", "ids_": b"ids of a key", "K": b"1 <= K <= 32"}
    assert [w for p, w in words.items() if name.startswith(p)][0] in msg, (name, msg)


def test_from_arrays_on_many_ids(ctx, big):
    """the same rules where the check strides: one bad id far into a table of 1500 keys"""
    from zotmer_amd import native
    arr, _ = big
    ids = arr.ids.copy()
    i = 1000 + int(np.argmax(np.diff(arr.offs)[1000:] == 65))
    j = int(arr.offs[i]) + 40                       # inside a list: make it equal to its predecessor
    assert arr.offs[i] < j < arr.offs[i + 1]
    ids[j] = ids[j - 1]
    rc, h, msg = from_arrays_rc(ctx, 25, arr.keys, arr.offs, ids, 300)
    assert rc == native.ZK_EINVAL and h == 0xDEAD and b"ids of a key" in msg
    ids = arr.ids.copy()
    ids[-1] = 300
    assert from_arrays_rc(ctx, 25, arr.keys, arr.offs, ids, 300)[0] == native.ZK_EINVAL
    assert from_arrays_rc(ctx, 25, arr.keys, arr.offs, arr.ids, 300, n_ids=len(arr.ids) - 1)[0] == native.ZK_EINVAL


def test_refused_arguments_launch_nothing(ctx, big):
    from zotmer_amd import native
    arr, table = big
    d = ctx.upload(arr.keys)
    hits = ctx.empty(300, U32)
    ctx.profile(True)
    try:
        for args in ((None, d.ptr, d.n, hits.ptr), (table.h, None, 5, hits.ptr), (table.h, d.ptr, d.n, None)):
            assert ctx.lib.zk_bait_tally(ctx.h, *args) == native.ZK_EINVAL
            assert b"zk_bait_tally" in ctx.lib.zk_last_error(ctx.h)
        assert "bait_tally" not in ctx.profile_read()
        assert ctx.lib.zk_bait_tally(ctx.h, table.h, None, 0, hits.ptr) == 0          # nothing to do is no launch either
        assert "bait_tally" not in ctx.profile_read()
        assert ctx.lib.zk_bait_tally(ctx.h, table.h, d.ptr, d.n, hits.ptr) == 0
        rec = ctx.profile_read()["bait_tally"]
        assert rec["launches"] == 1 and rec["bytes"] == 8 * d.n
    finally:
        ctx.profile(False)


# ---- the command ----------------------------------------------------------------------------------------------------

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


def write_set(path, K, kmers):
    """a k-mer set through the project's own container code"""
    from zotmer_amd.library import vectors
    from zotmer_amd.library.container import KmerSet
    with KmerSet(str(path), "w") as z:
        z.meta = {"K": K, "kmers": len(kmers)}
        vectors.write_kmers_and_counts(z, np.array(kmers, dtype=np.uint64), np.ones(len(kmers), dtype=np.uint64))
    return str(path)


def build_case(d, case):
    fas = []
    for fn, text in case["files"]:
        (d / fn).write_text(text)
        fas.append(str(d / fn))
    idx = str(d / (case["name"] + ".idx"))
    code, out, err = zot(["mlst", "-XK", str(case["K"]), idx] + fas)
    assert (code, out, err) == (0, "", "")
    return idx


def expected(case, sample, path):
    return case["stdout"][sample].replace("set_%s_%s\t" % (case["name"], sample), path + "\t")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixture(ctx, tmp_path, case):
    from zotmer_amd.library import mlst
    idx = build_case(tmp_path, case)
    got = mlst.read_index_arrays(idx)
    assert got["K"] == case["K"] and got["names"] == case["names"]
    assert [got[a].tolist() for a in ("keys", "offs", "ids", "lens")] == [case[b] for b in ("S", "T", "U", "lens")]
    with zipfile.ZipFile(idx) as z:          # and the file holds the very bytes the reference wrote
        for name, b64 in case["members"].items():
            assert z.read(name) == base64.b64decode(b64), name
    for name, xs, _ in case["samples"]:
        ks = write_set(tmp_path / ("%s.k%d" % (name, case["K"])), case["K"], xs)
        code, out, err = zot(["mlst", idx, ks])
        assert code == 0 and err == "" and out == expected(case, name, ks), name
        assert ks + "\t%d\t" % case["records"]["tiny"] in out


def test_default_k_is_27(ctx, tmp_path):
    from zotmer_amd.library import mlst
    case = CASES[1]
    fa = tmp_path / "a.fa"
    fa.write_text(case["files"][0][1] + case["files"][1][1])
    assert zot(["mlst", "-X", str(tmp_path / "d.idx"), str(fa)])[0] == 0
    got = mlst.read_index_arrays(str(tmp_path / "d.idx"))
    assert got["K"] == 27 and got["keys"].tolist() == case["S"] and got["names"] == case["names"]


def test_several_inputs_share_one_index_load(ctx, tmp_path, monkeypatch):
    from zotmer_amd import native
    case = CASES[0]
    idx = build_case(tmp_path, case)
    sets = [(name, write_set(tmp_path / (name + ".k"), case["K"], xs)) for name, xs, _ in case["samples"]]
    calls = []
    real = native.Context.bait_table_from_arrays
    monkeypatch.setattr(native.Context, "bait_table_from_arrays", lambda self, *a: calls.append(1) or real(self, *a))
    code, out, err = zot(["mlst", idx] + [p for _, p in sets] + [sets[0][1]])
    assert code == 0 and err == "" and len(calls) == 1
    assert out == "".join(expected(case, name, p) for name, p in sets) + expected(case, sets[0][0], sets[0][1])


def test_input_of_another_k(ctx, tmp_path):
    case = CASES[0]
    idx = build_case(tmp_path, case)
    name, xs, _ = case["samples"][0]
    good = write_set(tmp_path / "good.k", case["K"], xs)
    other = write_set(tmp_path / "other.k", case["K"] + 2, xs)
    code, out, err = zot(["mlst", idx, good, other, good])
    assert code == 1 and out == expected(case, name, good)          # as the reference: the inputs before it are printed
    assert other in err and "K = %d" % (case["K"] + 2) in err and "K = %d" % case["K"] in err


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_index_written_by_the_reference(ctx, tmp_path, case):
    """the container rebuilt from the member bytes the reference wrote, its meta as Python 2 pickles it"""
    nm = "%d-mers" % case["K"]
    meta = {"kmers": nm, "K": case["K"], nm + "-N": len(case["S"]), "T": len(case["T"]), "U": len(case["U"]), "lens": len(case["lens"]),
            "names": case["names"]}
    idx = str(tmp_path / "ref.idx")
    with zipfile.ZipFile(idx, "w", allowZip64=True) as z:
        for name, b64 in case["members"].items():
            z.writestr(name, base64.b64decode(b64), compress_type=zipfile.ZIP_DEFLATED)
        z.writestr("__meta__", py2_pickle(meta))
    for name, xs, _ in case["samples"][:3]:
        ks = write_set(tmp_path / (name + ".k"), case["K"], xs)
        code, out, err = zot(["mlst", idx, ks])
        assert code == 0 and err == "" and out == expected(case, name, ks), name


def py2_pickle(meta):
    """cPickle.dumps(meta) of Python 2 (protocol 0) for a dict of str -> int | str | list of str"""
    out, memo = [b"(dp1\n"], [1]

    def put():
        memo[0] += 1
        return b"p%d\n" % memo[0]

    def s(v):
        return b"S" + repr(v.encode("latin-1"))[1:].encode() + b"\n" + put()

    for k, v in meta.items():
        out.append(s(k))
        if isinstance(v, bool):
            out.append(b"I01\n" if v else b"I00\n")
        elif isinstance(v, int):
            out.append(b"I%d\n" % v)
        elif isinstance(v, str):
            out.append(s(v))
        else:
            out.append(b"(l" + put())
            for item in v:
                out.append(s(item) + b"a")
        out.append(b"s")
    return b"".join(out) + b"."


def test_index_with_altered_lens_is_refused(ctx, tmp_path):
    from zotmer_amd.library import mlst
    case = CASES[0]
    lens = list(case["lens"])
    lens[3] += 1
    idx = str(tmp_path / "bad.idx")
    mlst.write_index_arrays(idx, case["K"], case["S"], case["T"], case["U"], lens, case["names"])
    name, xs, _ = case["samples"][0]
    ks = write_set(tmp_path / "s.k", case["K"], xs)
    code, out, err = zot(["mlst", idx, ks])
    assert code == 1 and out == "" and "damaged index" in err and "bad.idx" in err
    # ... and so are arrays that are no table
    U = list(case["U"])
    U[5] = len(case["names"])
    mlst.write_index_arrays(idx, case["K"], case["S"], case["T"], U, case["lens"], case["names"])
    code, out, err = zot(["mlst", idx, ks])
    assert code == 1 and out == "" and "damaged index" in err and "n_records" in err
