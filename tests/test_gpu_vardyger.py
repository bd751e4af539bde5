"""`zot vardyger` on the GPU: zk_dup_join against the literal restatement of the reference's findDup + positions
(tests/_vardyger_restatement.py) -- the coverage of every occurrence and the rows as exact ordered lists, indices mapped to values
-- on K = 2, 4, 24, 30 and 32, units around J, counts around the threshold, halves that may not agree, repeated k-mers,
low-complexity sequences on either side of ZK_DUP_WAVE_PAIRS, an N, 1 to 300 sequences, empty inputs, capacities and refusals;
then the command end to end on every fixture case (tests/golden/v1_vardyger.json) and behind `zot spikein`.  Every device array of
every call is a view at an odd element offset of a larger guarded array."""
import contextlib
import ctypes as C
import io
import json
import os
import random
import re

import numpy as np
import pytest

from tests import _spikein_cases as spike
from tests import _vardyger_restatement as R
from tests._vardyger_cases import counted_from, duplicated, fixture_cases, join_by_its_contract, rand_seq, write_case
from zotmer_amd import native
from zotmer_amd.library import vardyger

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "v1_vardyger.json")))
CASES = {c["name"]: c for c in fixture_cases()}
OK, EINVAL, ENOSPC = native.ZK_OK, native.ZK_EINVAL, native.ZK_ENOSPC
BOUND = native.DUP_WAVE_PAIRS
G32, G64 = 0xABCDABCD, 0xABCDABCDABCDABCD


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "zotk.h")).read()
    assert int(re.search(r"#define ZK_DUP_WAVE_PAIRS (\d+)", text).group(1)) == BOUND
    for name, tag in (("DUP_COVER", 48), ("DUP_JOIN", 49)):
        assert int(re.search(r"#define ZK_PROF_%s (\d+)" % name, text).group(1)) == native.Context.PROF_TAGS[name.lower()] == tag
    assert "zk_dup_join" in native.SIGNATURES and re.search(r"int zk_dup_join\(", text)


# ---- one call on guarded views --------------------------------------------------------------------------------------------------
def call(ctx, K, lists, tables, cap, min_count=10, lead=1, room=7, n=None, m=None):
    """zk_dup_join with every array a view at element `lead` of a guarded array -> (rc, n_out, cover, e, i, j); the guards and the
    inputs are checked here"""
    dts = (np.uint32, np.uint64, np.uint32, np.uint32, np.uint64, np.uint32, np.uint32)
    guard = lambda a, dt: np.concatenate((np.full(lead, G64 if dt == np.uint64 else G32, dt), np.asarray(a, dtype=dt),
                                          np.full(room, G64 if dt == np.uint64 else G32, dt)))
    hosts = [guard(a, dt) for a, dt in zip(list(lists) + list(tables), dts)]
    devs = [ctx.upload(h) for h in hosts]
    n_ = len(lists[0]) if n is None else n
    m_ = len(tables[0]) if m is None else m
    cover = ctx.upload(np.full(lead + len(tables[0]) + room, G32, np.uint32))
    outs = [ctx.upload(np.full(lead + cap + room, G32, np.uint32)) for _ in range(3)]
    got = C.c_uint64(0)
    at = lambda d: d.ptr + lead * d.dtype.itemsize
    rc_ = ctx.lib.zk_dup_join(ctx.h, at(devs[0]), at(devs[1]), at(devs[2]), n_, at(devs[3]), at(devs[4]), at(devs[5]), at(devs[6]), m_, K, min_count,
                              at(cover), at(outs[0]), at(outs[1]), at(outs[2]), cap, C.byref(got))
    for d, h in zip(devs, hosts):
        assert np.array_equal(d.to_host(), h)                          # inputs are not changed
    hc = cover.to_host()
    wrote_c = len(tables[0]) if rc_ in (OK, ENOSPC) and m_ == len(tables[0]) else 0
    assert np.all(hc[:lead] == G32) and np.all(hc[lead + wrote_c:] == G32)
    ho = [o.to_host() for o in outs]
    wrote = got.value if rc_ == OK else 0
    for o in ho:
        assert np.all(o[:lead] == G32) and np.all(o[lead + wrote:] == G32), rc_       # a refusal writes no row at all
    return (rc_, got.value, hc[lead:lead + len(tables[0])]) + tuple(o[lead:lead + wrote] for o in ho)


def expect(K, records, X, min_count=10):
    """from the restatement: the cover of every occurrence in table order, and the rows as values in the kernel's order:
    (sequence, c, b, a, pa, d, pc)"""
    ref = R.Index(K, records)
    rows = []
    for n in range(len(records)):
        xs = {x: c for x, c in X[n].items() if c >= min_count}
        rows += [(n, c, b, a, pa, d, pc) for a, b, c, d, pa, pc in R.candidates(ref, n, xs)]
    return sorted(rows)


def check(ctx, K, records, X, min_count=10, want_rows=None, lead=1):
    """size the rows with cap = 0, run with exactly that room, compare with the restatement (and the contract in Python)"""
    index = vardyger.Index(K, records)
    tables = [a.tolist() for a in (index.rseq, index.rkmer, index.rpos, index.by_second)]
    lists = counted_from(X)
    want = expect(K, records, X, min_count)
    assert want_rows is None or len(want) == want_rows, len(want)
    rc_, n, cover, _, _, _ = call(ctx, K, lists, tables, 0, min_count, lead)
    assert (rc_, n) == ((ENOSPC if want else OK), len(want)), (rc_, n, len(want), ctx.lib.zk_last_error(ctx.h))
    assert cover.tolist() == [X[s].get(x, 0) for s, x in zip(tables[0], tables[1])]
    rc_, n, cover2, e, i, j = call(ctx, K, lists, tables, len(want), min_count, lead)
    assert (rc_, n) == (OK, len(want)) and np.array_equal(cover, cover2)
    low = (1 << K) - 1
    rk, rp = tables[1], tables[2]
    got = [(lists[0][ee], lists[1][ee] >> K, lists[1][ee] & low, rk[ii] >> K, rp[ii], rk[jj] & low, rp[jj]) for ee, ii, jj in zip(e.tolist(), i.tolist(), j.tolist())]
    assert got == want
    for ee, ii, jj in zip(e.tolist(), i.tolist(), j.tolist()):          # the rows are what they claim to be
        assert tables[0][ii] == tables[0][jj] == lists[0][ee] and rk[ii] & low == lists[1][ee] & low and rk[jj] >> K == lists[1][ee] >> K
    c_cover, c_rows = join_by_its_contract(*lists, *tables, K, min_count)
    assert c_cover == cover.tolist() and c_rows == list(zip(e.tolist(), i.tolist(), j.tolist()))
    return want


def kmers_of(K, seq, both=True):
    return R.kmers_list(K, seq, both)


def sample_counts(rng, K, records, genomes, extra=20, choices=(9, 10, 11, 40)):
    """per record a counted dict: the k-mers of its sample genome, both strands, and a few random ones"""
    X = []
    for g in genomes:
        xs = {x: rng.choice(choices) for x in kmers_of(K, g)}
        for _ in range(extra):
            xs.setdefault(rng.randrange(1 << (2 * K)), rng.choice(choices))
        X.append(xs)
    return X


# ---- K, units, counts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 4, 24, 30, 32])
def test_duplications_at_every_k(ctx, K):
    rng = random.Random(100 + K)
    J = K // 2
    records, genomes = [], []
    for r, unit in enumerate((J - 1, J, J + 1, 3 * J + 1)):
        if unit < 1:
            continue
        alphabet = "ACGT" if K > 4 else "AC"
        seq = rand_seq(rng, 4 * K + 40 + r, alphabet)
        records.append(("s%d" % r, seq))
        genomes.append(duplicated(seq, K + 5, unit))
    X = sample_counts(rng, K, records, genomes)
    want = check(ctx, K, records, X)
    assert want
    if K >= 24:                                          # random bases: the unit of J + 1 gives a row, the units up to J none
        firsts = {(n, pa) for n, _, _, _, pa, _, _ in want}
        assert any(n == len(records) - 2 for n, _ in firsts) and not any(n < len(records) - 2 for n, _ in firsts)
    X = sample_counts(rng, K, records, genomes, choices=(40,))
    check(ctx, K, records, X)


def test_counts_around_the_threshold_for_mid_and_right(ctx):
    K = 24
    # (a sequence whose duplication cannot be moved by a base: one placement, one row)
    seq = next(s for s in (rand_seq(random.Random(g), 300) for g in range(5, 50)) if s[130] != s[100] and s[99] != s[129])
    g = duplicated(seq, 101, 30)
    base = {x: 50 for x in kmers_of(K, g)}
    cb = kmers_of(K, g[100 + 30 - 12:100 + 30 + 12], False)[0]
    cd = kmers_of(K, seq[100 + 30 - 12:100 + 30 + 12], False)[0]
    for n_cb in (9, 10, 11):
        for n_cd in (9, 10, 11):
            X = dict(base)
            X[cb], X[cd] = n_cb, n_cd
            check(ctx, K, [("s", seq)], [X], want_rows=1 if n_cb >= 10 and n_cd >= 10 else 0)
    X = dict(base)
    X[cb], X[cd] = 3, 4
    check(ctx, K, [("s", seq)], [X], min_count=3, want_rows=None)
    assert len(expect(K, [("s", seq)], [X], 4)) == 0 and len(expect(K, [("s", seq)], [X], 3)) >= 1


def test_halves_that_agree_make_no_row(ctx):
    """a == c alone, b == d alone, and a k-mer that is ab twice and cd twice"""
    K = 4
    h = lambda s: kmers_of(2, s, False)[0]
    km = lambda a, b: kmers_of(4, a + b, False)[0]
    # the sequence holds AC|GT at 1 and AC|TG at 11 (a == c = AC): the entry AC|GT would pair them, and may not
    seq = "ACGT" + "TTTTTT" + "ACTG" + "CC"
    X = {x: 10 for x in kmers_of(K, seq, False)}
    assert km("AC", "GT") in X and km("AC", "TG") in X
    check(ctx, K, [("s", seq)], [X])
    # ... GT|AC at 1 and TG|AC at 11 (b == d = AC)
    seq = "GTAC" + "TTTTTT" + "TGAC" + "CC"
    X = {x: 10 for x in kmers_of(K, seq, False)}
    check(ctx, K, [("s", seq)], [X])
    # ab = GG|AC at 1 and at 9, cd = TC|AA at 21 and 29; cb = TC|AC: four rows, by (pa, pc)
    seq = "GGAC" + "CCCC" + "GGAC" + "CCCCCCCC" + "TCAA" + "GGGG" + "TCAA"
    X = {km("TC", "AC"): 12, km("TC", "AA"): 10, km("GG", "AC"): 1}
    want = check(ctx, K, [("s", seq)], [X])
    picked = [r for r in want if r[1:4] == (h("TC"), h("AC"), h("GG"))]
    assert [(r[4], r[6]) for r in picked] == [(1, 21), (1, 29), (9, 21), (9, 29)]


# ---- low complexity: on either side of the wave bound ------------------------------------------------------------------------------
@pytest.mark.parametrize("seq,K,product", [("AC" * 9, 4, 56), ("AC" * 9 + "A", 4, 64), ("AC" * 10, 4, 72), ("ACG" * 12, 6, 110),
                                            ("AC" * 70, 4, 69 * 68), ("ACG" * 9, 6, 56)])
def test_low_complexity_groups(ctx, seq, K, product):
    assert min(56, BOUND) == 56 and 64 == BOUND < 72
    J = K // 2
    records = [("pad", "GATTACAGATTACA" * 3), ("lc", seq), ("tail", "TTGACCA" * 5)]
    rot = seq[:J]
    k1, k2 = kmers_of(K, seq, False)[0], kmers_of(K, seq, False)[1]
    low = (1 << K) - 1
    cb = (k2 >> K) << K | (k1 & low)                   # first half of the second k-mer, second half of the first
    X = [{x: 11 for x in kmers_of(K, s, False)} for _, s in records]
    X[1][cb] = 10
    X[1][(k1 >> K) << K | (k2 & low)] = 30
    index = vardyger.Index(K, records)
    n1 = int(((index.rseq == 1) & (index.rkmer == k1)).sum())
    n2 = int(((index.rseq == 1) & (index.rkmer == k2)).sum())
    assert n1 * n2 == product and rot
    want = check(ctx, K, records, X)
    assert len([r for r in want if r[0] == 1]) > product // 3
    check(ctx, K, records, X, lead=3)


def test_many_sequences_and_rows_across_scan_tiles(ctx):
    """300 sequences, 20000 entries and more, rows at either end and a large group in the middle"""
    K, rng = 8, random.Random(9)
    records, genomes = [], []
    for r in range(300):
        seq = "AC" * 40 if r == 150 else rand_seq(rng, 70 + r % 13)
        if r % 50 == 7:
            seq = seq[:30] + "N" + seq[31:]
        records.append(("s%03d" % r, seq))
        genomes.append(seq if r == 150 else duplicated(seq, 20, 5 + r % 9))
    X = sample_counts(rng, K, records, genomes, extra=5, choices=(9, 10, 40))
    lc = kmers_of(K, "AC" * 8, False)
    X[150].update({lc[0]: 10, lc[1]: 11, (lc[1] >> K) << K | (lc[0] & 0xFF): 10})        # K = 8 bits a half
    assert sum(len(x) for x in X) > 20000
    want = check(ctx, K, records, X)
    assert len({r[0] for r in want}) > 100 and len([r for r in want if r[0] == 150]) > 500 and want[0][0] < 10 and want[-1][0] > 290
    for n_seq in (1, 2):
        check(ctx, K, records[:n_seq], X[:n_seq])


def test_an_n_in_the_sequence(ctx):
    K, rng = 24, random.Random(12)
    seq = rand_seq(rng, 400)
    g = duplicated(seq, 151, 33)
    for p in (100, 150, 170, 200):
        s = seq[:p] + "N" + seq[p + 1:]
        X = {x: 20 for x in kmers_of(K, g)}
        check(ctx, K, [("s", s)], [X])
    check(ctx, K, [("s", "N" * 30), ("t", seq)], [{}, {x: 20 for x in kmers_of(K, g)}], want_rows=1)


# ---- empties, capacities, refusals --------------------------------------------------------------------------------------------------
def test_empty_list_and_empty_table(ctx):
    K = 24
    seq = rand_seq(random.Random(1), 100)
    index = vardyger.Index(K, [("s", seq)])
    tables = [a.tolist() for a in (index.rseq, index.rkmer, index.rpos, index.by_second)]
    rc_, n, cover, e, _, _ = call(ctx, K, ([], [], []), tables, 4)
    assert (rc_, n) == (OK, 0) and cover.tolist() == [0] * len(tables[0]) and len(e) == 0
    lists = counted_from([{x: 10 for x in kmers_of(K, seq)}])
    rc_, n, cover, e, _, _ = call(ctx, K, lists, ([], [], [], []), 4)
    assert (rc_, n) == (OK, 0) and len(cover) == 0
    rc_, n, _, _, _, _ = call(ctx, K, ([], [], []), ([], [], [], []), 0)
    assert (rc_, n) == (OK, 0)
    n_out = C.c_uint64(7)
    assert ctx.lib.zk_dup_join(ctx.h, None, None, None, 0, None, None, None, None, 0, K, 10, None, None, None, None, 0, C.byref(n_out)) == OK
    assert n_out.value == 0
    check(ctx, K, [("s", ""), ("t", "ACGT")], [{}, {}], want_rows=0)


def test_capacities(ctx):
    K = 4
    seq = "AC" * 10
    records = [("lc", seq), ("r", "GGACCCCCGGACCCCCCCCCTCAAGGGGTCAA")]
    X = [{x: 11 for x in kmers_of(K, s, False)} for _, s in records]
    k = kmers_of(K, seq, False)
    X[0][(k[1] >> K) << K | (k[0] & 0xF)] = 10          # K = 4 bits a half
    X[1][kmers_of(4, "TCAC", False)[0]] = 12
    want = check(ctx, K, records, X)
    need = len(want)
    assert need > 40
    index = vardyger.Index(K, records)
    tables = [a.tolist() for a in (index.rseq, index.rkmer, index.rpos, index.by_second)]
    lists = counted_from(X)
    full = call(ctx, K, lists, tables, need)
    for cap in (need - 1, 1, 0):
        rc_, n, cover, e, _, _ = call(ctx, K, lists, tables, cap)
        assert (rc_, n) == (ENOSPC, need) and np.array_equal(cover, full[2]) and len(e) == 0
        assert b"zk_dup_join" in ctx.lib.zk_last_error(ctx.h)
    for cap in (need, need + 1, need + 100):
        got = call(ctx, K, lists, tables, cap)
        assert got[:2] == (OK, need) and all(np.array_equal(a, b) for a, b in zip(got[2:], full[2:]))


def test_every_einval(ctx):
    K = 24
    seq = rand_seq(random.Random(2), 120)
    index = vardyger.Index(K, [("s", seq)])
    tables = [a.tolist() for a in (index.rseq, index.rkmer, index.rpos, index.by_second)]
    lists = counted_from([{x: 10 for x in kmers_of(K, duplicated(seq, 40, 30))}])
    for bad_k in (0, 1, 3, 23, 25, 31, 33, 34, -2, 64):
        rc_, n, _, e, _, _ = call(ctx, bad_k, lists, tables, 8)
        assert rc_ == EINVAL and len(e) == 0, bad_k
    assert call(ctx, K, lists, tables, 8, n=1 << 32)[0] == EINVAL and call(ctx, K, lists, tables, 8, m=1 << 32)[0] == EINVAL
    assert call(ctx, K, lists, tables, 8, n=(1 << 40) + 1)[0] == EINVAL
    d = [ctx.upload(np.zeros(4, dt)) for dt in (np.uint32, np.uint64, np.uint32, np.uint32, np.uint64, np.uint32, np.uint32, np.uint32, np.uint32,
                                                np.uint32, np.uint32)]
    n_out = C.c_uint64(0)
    good = [ctx.h, d[0].ptr, d[1].ptr, d[2].ptr, 1, d[3].ptr, d[4].ptr, d[5].ptr, d[6].ptr, 1, K, 10, d[7].ptr, d[8].ptr, d[9].ptr, d[10].ptr, 4,
            C.byref(n_out)]
    for k in (1, 2, 3, 5, 6, 7, 8, 12, 13, 14, 15, 17):
        args = list(good)
        args[k] = None
        assert ctx.lib.zk_dup_join(*args) == EINVAL, k
    assert ctx.lib.zk_dup_join(*([None] + good[1:])) == EINVAL
    assert ctx.lib.zk_dup_join(*good) == OK and n_out.value == 0                 # the context stays usable
    check(ctx, K, [("s", seq)], [{x: 10 for x in kmers_of(K, duplicated(seq, 40, 30))}], want_rows=1)


def test_the_binding_grows_its_rows(ctx):
    K = 4
    records = [("lc", "AC" * 60)]
    k = kmers_of(K, records[0][1], False)
    X = [{k[0]: 10, k[1]: 10, (k[1] >> K) << K | (k[0] & 0xF): 10}]
    index = vardyger.Index(K, records)
    dev = vardyger.DeviceIndex(ctx, index)
    b, x, c = [np.array(a, dtype=dt) for a, dt in zip(counted_from(X), (np.uint32, np.uint64, np.uint64))]
    cover, rows = vardyger.join(ctx, dev, index, b, x, c, 10)
    want = expect(K, records, X)
    assert len(rows) == len(want) > 1024 and cover.tolist() == [10] * index.m
    low = (1 << K) - 1
    got = sorted((0, int(x[e]) >> K, int(x[e]) & low, int(index.rkmer[i]) >> K, int(index.rpos[i]), int(index.rkmer[j]) & low, int(index.rpos[j]))
                 for e, i, j in rows.tolist())
    assert got == want


# ---- the command -------------------------------------------------------------------------------------------------------------------
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


def split_gold(lines):
    cover = [l for l in lines if l == "" or set(l) <= set(".X")]
    rest = [l for l in lines if not (l == "" or set(l) <= set(".X"))]
    assert not rest or rest[0] == R.HEADER
    return cover, rest[1:]


@pytest.mark.parametrize("gold", GOLD, ids=[c["name"] for c in GOLD])
def test_command_on_the_fixture(ctx, gold, tmp_path):
    """stdout: the header and the rows -- without n as sorted lists against the reference's, n = 1 .. rows, and in the product's
    own order the restatement's; stderr under -v: the reads per file, the coverage lines and the warnings"""
    case = CASES[gold["name"]]
    args = write_case(case, str(tmp_path))
    want_cover, want_rows = split_gold(gold["stdout"])
    code, out, err = zot(["vardyger", "-v"] + args)
    assert code == 0, err
    lines = out.split("\n")[:-1]
    if want_rows:
        assert lines[0] == R.HEADER
    rows = lines[1:]
    assert sorted(r.split("\t", 1)[1] for r in rows) == sorted(r.split("\t", 1)[1] for r in want_rows)
    assert [r.split("\t")[0] for r in rows] == [str(i + 1) for i in range(len(want_rows))]
    elines = err.split("\n")[:-1]
    warnings = [l for l in elines if l.startswith("warning: ")]
    assert sorted(warnings) == sorted(gold["stderr"])
    assert [l for l in elines if l == "" or set(l) <= set(".X")] == want_cover
    assert any(l.startswith("in0.fastq: ") and l.endswith(" reads") for l in elines)
    index = R.Index(case["K"], list(R.read_fasta(case["fasta"])))
    reads = [s for t in case["inputs"] for s in R.read_fastq(t)]
    o = case["opts"]
    _, mine = R.call(index, R.count_reads(index, reads), int(o[o.index("-m") + 1]) if "-m" in o else 10, "-a" in o, "-s" in o)
    assert [r.split("\t", 1)[1] for r in rows] == R.ordered(mine)
    # without -v: the same stdout, the warnings alone; tiny batches: the same again
    code, out2, err2 = zot(["vardyger", "-b", "1"] + args)
    assert code == 0 and out2 == out and err2.split("\n")[:-1] == warnings


def test_spikein_then_vardyger(ctx, tmp_path):
    """no hgvs-gen: a dup variant spiked into simulated pairs, both mate files read as single reads, found again"""
    genome = str(tmp_path / "g")
    spike.write_genome(genome, gz=False)
    (tmp_path / "z.bed").write_text("chrA\t1000\t1400\tmid1\n")
    var = "chrA:g.1250_1279dup"
    assert zot(["spikein", "-g", genome, "-b", str(tmp_path / "z.bed"), "-S", "11", "-N", "600", "-V", "1.0", str(tmp_path / "r"), var])[0] == 0
    gene = spike.GENOME["chrA"][900:1500]
    (tmp_path / "genes.fa").write_text(">FLT3\n%s\n" % gene)
    code, out, err = zot(["vardyger", "-a", str(tmp_path / "genes.fa"), str(tmp_path / "r_1.fastq"), str(tmp_path / "r_2.fastq")])
    assert code == 0, err
    lines = out.split("\n")[:-1]
    assert lines[0] == R.HEADER
    rows = [dict(zip(lines[0].split("\t"), l.split("\t"))) for l in lines[1:]]
    hit = [r for r in rows if r["hgvs"] == "FLT3:c.350_379dup"]
    assert len(hit) == 1 and hit[0]["len"] == "30" and int(hit[0]["midCov"]) >= 10 and float(hit[0]["vaf"]) > 0.5
    assert hit[0]["left"] == gene[349 - 12:349 + 12].upper() and hit[0]["right"] == gene[379 - 12:379 + 12].upper()
    assert all(r["hgvs"].startswith("FLT3:c.") and r["len"] == "30" for r in rows)
