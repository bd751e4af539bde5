"""`zot strand` on the device: the three entries of csrc/strand_bias.hip against the restatement of the reference's
semantics (tests/_strand_restatement.py) at the sizes where they change path, and the command against the reference's
fixtures (tests/golden/s1_strand.json)."""
import contextlib
import hashlib
import io
import json
import os
import random

import numpy as np
import pytest

from tests import _strand_restatement as R
from tests._strand_cases import make_cases

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "s1_strand.json")
INPUTS = {c["name"]: c for c in make_cases()}
CASES = [dict(c, inputs=INPUTS[c["name"]]["inputs"]) for c in json.load(open(GOLD))]
IDS = [c["name"] for c in CASES]
TILE = 4096          # csrc/compact.hpp: CP_TILE


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    from zotmer_amd.library import engine
    yield engine.context()
    engine.close()


# ---- zk_strand_keys ---------------------------------------------------------------------------------------------

def key_reads(K):
    """reads at the step borders of the kernel (64 windows per step), with N's where a window run must restart, and enough
    of them (2000) for many waves to meet at the output cursor"""
    rng = random.Random(100 + K)
    g = "".join(rng.choice("ACGT") for _ in range(2000))

    def piece(n):
        p = rng.randrange(0, len(g) - n) if n < len(g) else 0
        s = g[p:p + n]
        return s if rng.random() < 0.5 else s[::-1].translate(str.maketrans("ACGT", "TGCA"))

    seqs = [piece(n) for n in (max(K - 1, 0), K, K + 1)]
    seqs += [piece(w + K - 1) for w in (63, 64, 65, 64 + K - 1, 127, 128, 129, 200)]
    seqs.append("N" * 70)
    for n in (64, 65, 100, 130, 193):
        s = piece(n)
        seqs += ["N" + s[1:], s[:-1] + "N", "N" + s[1:-1] + "N", "".join("N" if i % 64 == 63 else ch for i, ch in enumerate(s)),
                 "".join("N" if i % 64 == 0 else ch for i, ch in enumerate(s))]
    seqs += ["", "acgtu" * 20, "ACGU" * 20 + " " + "ACGT" * 10]
    while len(seqs) < 2000:
        seqs.append(piece(rng.randrange(1, 90)))
    return seqs


def fastq_text(seqs, eol="\n"):
    return "".join("@r%d%s%s%s+%s%s%s" % (i, eol, s, eol, eol, "I" * len(s), eol) for i, s in enumerate(seqs)).encode()


@pytest.mark.parametrize("K", [1, 2, 5, 16, 25, 31])
def test_strand_keys(ctx, K):
    from zotmer_amd import native
    seqs = key_reads(K)
    text = ctx.upload_stream(fastq_text(seqs))
    lines = ctx.line_ends(text)
    assert lines.n == 4 * len(seqs)
    M = (1 << (2 * K)) - 1
    memo = {}
    for reverse in (0, 1):
        for T in (0, M // 10, M):
            want = np.array(R.tagged_keys(K, seqs, reverse, T, memo=memo), dtype=np.uint64)
            out = ctx.empty(len(want) + 8, np.uint64)
            n, fits = ctx.strand_keys(text, lines, len(seqs), K, reverse, T, out)
            assert fits and n == len(want), (reverse, T)
            assert np.array_equal(np.sort(out.to_host(n)), want), (reverse, T)
            if len(want):
                # one place short: ZK_ENOSPC, the exact count, nothing written past the capacity
                guard = np.full(len(want) + 8, 0xABCDABCDABCDABCD, dtype=np.uint64)
                out = ctx.upload(guard)
                n, fits = ctx.strand_keys(text, lines, len(seqs), K, reverse, T, out.view(len(want) - 1))
                assert not fits and n == len(want)
                assert np.all(out.to_host()[len(want) - 1:] == guard[0])
    assert len(R.tagged_keys(K, seqs, 0, M, memo=memo)) > 64 * 300          # many waves, many steps
    # zero reads; an offset into the buffer (mate 2 behind mate 1)
    out = ctx.empty(16, np.uint64)
    assert ctx.strand_keys(text, lines, 0, K, 0, M, out) == (0, True)
    want1 = R.tagged_keys(K, seqs[:40], 0, M, memo=memo)
    want2 = R.tagged_keys(K, seqs[:40], 1, M, memo=memo)
    out = ctx.empty(len(want1) + len(want2), np.uint64)
    n1, _ = ctx.strand_keys(text, lines.view(160), 40, K, 0, M, out)
    n2, fits = ctx.strand_keys(text, lines.view(160), 40, K, 1, M, out, offset=n1)
    assert fits and (n1, n2) == (len(want1), len(want2))
    assert np.array_equal(np.sort(out.to_host()), np.sort(np.array(want1 + want2, dtype=np.uint64)))


def test_strand_keys_refuses_k32(ctx):
    from zotmer_amd import native
    text = ctx.upload_stream(fastq_text(["ACGT" * 10]))
    lines = ctx.line_ends(text)
    out = ctx.empty(64, np.uint64)
    for K in (0, 32):
        with pytest.raises(native.ZotkError, match="2K \\+ 1 bits"):
            ctx.strand_keys(text, lines, 1, K, 0, 0, out)
    with pytest.raises(native.ZotkError, match="2K \\+ 1 bits"):
        ctx.strand_pairs(ctx.upload(np.array([2], np.uint64)), ctx.upload(np.array([1], np.uint32)), 32)


# ---- zk_strand_pairs ----------------------------------------------------------------------------------------------

def tagged_table(K, n, rng, wide):
    """n ascending distinct tagged keys and counts: an orphan first and last, a (tag 0, tag 1) pair across every tile border,
    the three kinds mixed elsewhere, palindromes where K has them; counts at the ends of the count type"""
    canon = set()
    if 4 ** K <= 1 << 16:
        canon = {x for x in range(4 ** K) if x <= R.rc(K, x)}
    else:
        while len(canon) < n + 8:
            x = rng.randrange(4 ** K)
            canon.add(min(x, R.rc(K, x)))
    keys = []
    for c in sorted(canon):
        if len(keys) >= n:
            break
        pal = R.rc(K, c) == c
        room = n - len(keys)
        i = len(keys)
        if pal:
            kind = 0
        elif i == 0 or room == 1:
            kind = 1                                   # an orphan as the first and as the last entry
        elif i % TILE == TILE - 1:
            kind = 2                                   # tag 0 closes a tile, its partner opens the next
        elif room == 2 or i % TILE == TILE - 2:
            kind = 0                                   # (one entry, so that the next one is a tile's last)
        else:
            kind = rng.choice((0, 1, 2, 2))
        keys += [(c << 1)] if kind == 0 else [(c << 1) | 1] if kind == 1 else [c << 1, (c << 1) | 1]
    keys = keys[:n]
    top = [2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 12345, 10 ** 19, 2 ** 64 - 1] if wide else [2 ** 32 - 1, 2 ** 32 - 2, 2 ** 31]
    counts = [rng.choice(top) if rng.random() < 0.2 else rng.randrange(1, 1000) for _ in keys]
    return keys, counts


@pytest.mark.parametrize("wide", [False, True], ids=["u32", "u64"])
@pytest.mark.parametrize("K,n", [(16, 0), (16, 1), (16, 2), (16, TILE - 1), (16, TILE), (16, TILE + 1), (16, 3 * TILE + 7),
                                 (31, 2 * TILE + 1), (2, 10), (2, 16), (6, 2080), (1, 2)])
def test_strand_pairs(ctx, K, n, wide):
    rng = random.Random(K * 100003 + n)
    keys, counts = tagged_table(K, n, rng, wide)
    if K == 16:
        assert len(keys) == n
    if K >= 16:
        for t in range(TILE, len(keys), TILE):
            assert keys[t - 1] + 1 == keys[t]          # a pair across every tile border
    dk = ctx.upload(np.array(keys, dtype=np.uint64))
    dc = ctx.upload(np.array(counts, dtype=np.uint64 if wide else np.uint32))
    for orphans in (False, True):
        wa, wb, st = R.pairs_of(K, keys, counts, orphans)
        a, b, got = ctx.strand_pairs(dk, dc, K, orphans)
        assert (got.n_pairs, got.n_orphans, got.n_palindromes) == (st["pairs"], st["orphans"], st["palindromes"])
        assert np.array_equal(a.to_host(), np.array(wa, dtype=np.uint64))
        assert np.array_equal(b.to_host(), np.array(wb, dtype=np.uint64))
    if K in (2, 6):
        assert st["palindromes"] > 0
    if len(keys) > 2:
        assert st["orphans"] >= 2


def test_strand_pairs_capacity(ctx):
    from zotmer_amd import native
    keys, counts = tagged_table(16, 100, random.Random(5), False)
    dk, dc = ctx.upload(np.array(keys, np.uint64)), ctx.upload(np.array(counts, np.uint32))
    _, _, st = R.pairs_of(16, keys, counts)
    a, b = ctx.empty(100, np.uint64), ctx.empty(100, np.uint64)
    got = native.StrandStats()
    rc = ctx.lib.zk_strand_pairs(ctx.h, dk.ptr, dc.ptr, 32, dk.n, 16, 17, 0, a.ptr, b.ptr, st["pairs"] - 1, native.C.byref(got))
    assert rc == native.ZK_ENOSPC and got.n_pairs == st["pairs"]


# ---- zk_format_pairs ------------------------------------------------------------------------------------------------

EDGES = [0, 9, 10, 99, 100, 2 ** 32 - 1, 2 ** 32, 10 ** 19 - 1, 10 ** 19, 2 ** 64 - 1]


@pytest.mark.parametrize("n", [0, 1, len(EDGES) ** 2, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 7])
def test_format_pairs(ctx, n):
    from zotmer_amd import native
    rng = random.Random(n)
    pairs = [(x, y) for x in EDGES for y in EDGES]
    pairs = (pairs * (n // len(pairs) + 1))[:n] if n >= len(pairs) else [(rng.choice(EDGES), rng.choice(EDGES)) for _ in range(n)]
    pairs = [(x, y) if i % 3 else (rng.randrange(10 ** rng.randrange(1, 20)), y) for i, (x, y) in enumerate(pairs)]
    a = ctx.upload(np.array([p[0] for p in pairs], dtype=np.uint64))
    b = ctx.upload(np.array([p[1] for p in pairs], dtype=np.uint64))
    want = "".join("%d\t%d\n" % p for p in pairs).encode()
    assert ctx.format_pairs(a, b).to_host().tobytes() == want
    if n:
        guard = np.full(len(want) + 16, 0x5A, dtype=np.uint8)
        out = ctx.upload(guard)
        nb = native.C.c_uint64(0)
        rc = ctx.lib.zk_format_pairs(ctx.h, a.ptr, b.ptr, n, out.ptr, len(want) - 1, native.C.byref(nb))
        assert rc == native.ZK_ENOSPC and nb.value == len(want)
        assert np.all(out.to_host() == 0x5A)
        rc = ctx.lib.zk_format_pairs(ctx.h, a.ptr, b.ptr, n, out.ptr, len(want), native.C.byref(nb))
        assert rc == native.ZK_OK and out.to_host().tobytes() == want + b"\x5a" * 16


# ---- the command ----------------------------------------------------------------------------------------------------

def zot(args):
    from zotmer_amd import cli
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        code = cli.main_inner(args)
    return code, out.getvalue(), err.getvalue()


def write_inputs(d, case, eol=None):
    d.mkdir(parents=True, exist_ok=True)
    paths = []
    for i, text in enumerate(case["inputs"]):
        p = d / ("in%d.fastq" % i)
        p.write_bytes(text.encode())
        paths.append(str(p))
    return paths


@pytest.fixture(scope="module")
def restated():
    return {c["name"]: R.strand(c["k"], c["p"], c["inputs"]) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixture(ctx, tmp_path, restated, case):
    paths = write_inputs(tmp_path, case)
    args = ["strand", "-k", str(case["k"]), "-p", repr(case["p"])]
    code, out, err = zot(args + paths)
    assert code == 0 and err == ""
    lines = out.splitlines(keepends=True)
    assert len(lines) == case["lines"]
    assert hashlib.sha256("".join(sorted(lines)).encode()).hexdigest() == case["sha256_sorted"]
    assert lines == restated[case["name"]][1]               # as printed: ascending canonical k-mer order
    code, out_m1, _ = zot(args + ["-m", "1"] + paths)
    assert code == 0 and out_m1 == out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_batch_size_does_not_matter(ctx, tmp_path, restated, case):
    """batches of a dozen records: many batch tables, a merge tree several levels deep, mates cut at different bytes"""
    from zotmer_amd.library import strand
    paths = write_inputs(tmp_path, case)
    for batch in (1531, 4000):
        table = strand.StrandTable(ctx, case["k"], strand.threshold(case["k"], case["p"]))
        strand.count_inputs(ctx, table, paths, False, batch)
        keys, counts = table.result()
        out = io.StringIO()
        strand.write_lines(ctx, keys, counts, case["k"], False, out)
        assert out.getvalue() == "".join(restated[case["name"]][1]), batch


def test_counts_widen_before_they_can_wrap(ctx, tmp_path, restated):
    """a merge whose inputs could hold 2^32 windows between them runs on 64-bit counts"""
    from zotmer_amd.library import strand
    case = next(c for c in CASES if c["name"] == "k25_p1")
    paths = write_inputs(tmp_path, case)
    table = strand.StrandTable(ctx, 25, strand.threshold(25, 1.0))
    real = table.add_batch

    def add_batch(*a):
        real(*a)
        if len(table.stack) == 1 and table.stack[0][2] == 0:
            k, c, lvl, w = table.stack[0]
            table.stack[0] = (k, c, lvl, w + (1 << 32))
    table.add_batch = add_batch
    strand.count_inputs(ctx, table, paths, False, 4000)
    keys, counts = table.result()
    assert counts.dtype == np.uint64
    out = io.StringIO()
    strand.write_lines(ctx, keys, counts, 25, False, out)
    assert out.getvalue() == "".join(restated["k25_p1"][1])


@pytest.mark.parametrize("name", ["k25_p1", "k6_p1", "two_pairs"])
def test_single_ended_and_orphans(ctx, tmp_path, name):
    case = next(c for c in CASES if c["name"] == name)
    paths = write_inputs(tmp_path, case)
    args = ["strand", "-k", str(case["k"]), "-p", repr(case["p"])]
    _, want, st = R.strand(case["k"], case["p"], case["inputs"], orphans=True)
    code, out, err = zot(args + ["-a", "-v"] + paths)
    assert code == 0 and out == "".join(want) and st["orphans"] > 0
    assert "%d lines, %d k-mers seen only on their greater strand (printed), %d palindromes" % (
        st["pairs"], st["orphans"], st["palindromes"]) in err
    _, want, st = R.strand(case["k"], case["p"], case["inputs"], single=True)
    code, out, err = zot(args + ["-s", "-v"] + paths + paths[:1])          # an odd number of files is fine with -s
    _, want3, st3 = R.strand(case["k"], case["p"], case["inputs"] + case["inputs"][:1], single=True)
    assert code == 0 and out == "".join(want3) and out != "".join(want)
    assert "(not printed)" in err and "%d lines" % st3["pairs"] in err


def test_negative_p_prints_nothing(ctx, tmp_path):
    paths = write_inputs(tmp_path, CASES[0])
    assert zot(["strand", "-p", "-0.5"] + paths) == (0, "", "")
