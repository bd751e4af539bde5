"""`zot fizzle` on the GPU: zk_fizzle_votes against the restatement of the reference's loops (tests/_fizzle_restatement.py) -- the
tallies of the one-class records, the histogram and the (record, class, hits) lists, bit for bit -- on the fixture's cases, batch
sizes around a wave, mates and orientations, class counts around ZK_FIZZLE_CLASSES (where the kernel changes its path), preloaded
tallies, the histogram's clamp, batch cuts, capacities and refusals; and the command end to end on every fixture case
(tests/golden/z1_fizzle.json).  Every device array of every call is a view at an odd element offset of a larger guarded array."""
import contextlib
import ctypes as C
import io
import json
import os
import random
import re

import numpy as np
import pytest

from tests import _fizzle_restatement as R
from tests._fizzle_cases import fastq_text, fixture_cases, rc, write_case
from zotmer_amd import native
from zotmer_amd.library import fizzle
from zotmer_amd.library.hgvsindex import dump_yaml

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = {g["name"]: g for g in json.load(open(os.path.join(ROOT, "tests", "golden", "z1_fizzle.json")))}
CASES = {c["name"]: c for c in fixture_cases()}
OK, EINVAL, ENOSPC, ERANGE = native.ZK_OK, native.ZK_EINVAL, native.ZK_ENOSPC, native.ZK_ERANGE
CLASSES = native.FIZZLE_CLASSES
G32, G64, G8 = 0xABCDABCD, 0xABCDABCDABCDABCD, 0xAB


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "zotk.h")).read()
    assert int(re.search(r"#define ZK_FIZZLE_CLASSES (\d+)", text).group(1)) == CLASSES
    for name, tag in (("FIZZLE_COUNT", 42), ("FIZZLE_EMIT", 43)):
        assert int(re.search(r"#define ZK_PROF_%s (\d+)" % name, text).group(1)) == native.Context.PROF_TAGS[name.lower()] == tag
    assert re.search(r"zk_fizzle_votes\s+d_text1, d_text2\s+any address", text)


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def ref_of(name):
    case = CASES[name]
    return R.as_loaded(R.index_bed(GOLD[name]["bed"], lambda ch: case["chroms"][ch]))


def pairs_of(case):
    return list(zip(R.read_fastq(case["reads"][0]), R.read_fastq(case["reads"][1])))


def expect(K, cls_of, pairs, n_hist, n_classes):
    """what one call leaves for the pairs given: (single u64[2 C], hist u64[n_hist], [(record, class, hits)])"""
    single, hist, entries = np.zeros(2 * n_classes, dtype=np.uint64), np.zeros(n_hist, dtype=np.uint64), []
    for p, (s1, s2) in enumerate(pairs):
        for o, xs in enumerate(R.records_of(K, s1.strip(R.WS), s2.strip(R.WS))):
            d = {}
            for x in xs:
                if x in cls_of:
                    d[cls_of[x]] = d.get(cls_of[x], 0) + 1
            if len(d) == 1:
                (c, h), = d.items()
                single[2 * c] += 1
                single[2 * c + 1] += h
                hist[min(h, n_hist - 1)] += 1
            else:
                entries += [(2 * p + o, c, d[c]) for c in sorted(d)]
    return single, hist, entries


class Votes:
    """a class table from arrays, and calls of zk_fizzle_votes on guarded arrays"""

    def __init__(self, ctx, K, cls_of, n_classes):
        self.ctx, self.K, self.cls_of, self.n_classes = ctx, K, cls_of, n_classes
        keys = np.array(sorted(cls_of), dtype=np.uint64)
        ids = np.array([cls_of[x] for x in keys.tolist()], dtype=np.uint32)
        self.table = ctx.bait_table_from_arrays(K, ctx.upload(keys), ctx.upload(np.arange(len(keys) + 1, dtype=np.uint32)), ctx.upload(ids), n_classes)

    @classmethod
    def of_index(cls, ctx, K, ref):
        ci = fizzle.ClassIndex(K, ref)
        return cls(ctx, K, dict(zip(ci.keys.tolist(), ci.key_class.tolist())), len(ci.tuples))

    def free(self):
        self.table.free()

    def mate(self, fastq, lead):
        """(text view at byte `lead` of a guarded buffer, line ends as a view at u64 `lead` of another)"""
        ctx = self.ctx
        raw = np.frombuffer(fastq.encode("latin-1"), dtype=np.uint8)
        buf = ctx.upload(np.concatenate((np.full(lead, G8, np.uint8), raw, np.full(5, G8, np.uint8))))
        text = buf.view(len(raw), lead)
        ends = ctx.line_ends(text).to_host() if len(raw) else np.empty(0, np.uint64)
        lbuf = ctx.upload(np.concatenate((np.full(lead, G64, np.uint64), ends, np.full(2, G64, np.uint64))))
        return text, lbuf.view(len(ends), lead), (buf, lbuf)

    def call(self, pairs, cap=0, n_hist=256, single0=None, hist0=None, lead=1, room=9, n_reads=None, K=None, n_classes=None, eol="\n"):
        """one call -> (rc, n, single, hist, rec, cls, cnt): the arrays' payload [0, size); the guards around them are checked here"""
        ctx, C2 = self.ctx, 2 * self.n_classes
        t1, l1, keep1 = self.mate(fastq_text([p[0] for p in pairs], "p%d/1", eol), lead)
        t2, l2, keep2 = self.mate(fastq_text([p[1] for p in pairs], "p%d/2", eol), lead)
        guard = lambda payload, g, dt: np.concatenate((np.full(lead, g, dt), np.asarray(payload, dtype=dt), np.full(room, g, dt)))
        single = ctx.upload(guard(single0 if single0 is not None else np.zeros(C2, np.uint64), G64, np.uint64))
        hist = ctx.upload(guard(hist0 if hist0 is not None else np.zeros(n_hist, np.uint64), G64, np.uint64))
        outs = [ctx.upload(np.full(lead + cap + room, G32, np.uint32)) for _ in range(3)]
        n = C.c_uint64(0)
        rc_ = ctx.lib.zk_fizzle_votes(ctx.h, self.table.h, self.K if K is None else K, t1.ptr, l1.ptr, t2.ptr, l2.ptr,
                                      len(pairs) if n_reads is None else n_reads, self.n_classes if n_classes is None else n_classes,
                                      single.ptr + 8 * lead, hist.ptr + 8 * lead, n_hist, *(o.ptr + 4 * lead for o in outs), cap, C.byref(n))
        hs, hh = single.to_host(), hist.to_host()
        assert np.all(hs[:lead] == G64) and np.all(hs[lead + C2:] == G64) and np.all(hh[:lead] == G64) and np.all(hh[lead + n_hist:] == G64)
        ho = [o.to_host() for o in outs]
        wrote = n.value if rc_ == OK else 0
        for o in ho:
            assert np.all(o[:lead] == G32) and np.all(o[lead + wrote:] == G32)
        for (buf, lbuf), fq_len in ((keep1, t1.n), (keep2, t2.n)):                  # inputs are not changed
            assert np.all(buf.to_host()[[0, lead + fq_len]] == G8) and np.all(lbuf.to_host()[[0, -1]] == G64)
        return rc_, n.value, hs[lead:lead + C2], hh[lead:lead + n_hist], ho[0][lead:lead + cap], ho[1][lead:lead + cap], ho[2][lead:lead + cap]

    def check(self, pairs, n_hist=256, **kw):
        """size the lists with cap = 0, run with exactly that room, compare everything with the restatement"""
        single, hist, entries = expect(self.K, self.cls_of, pairs, n_hist, self.n_classes)
        rc_, n, s, h, _, _, _ = self.call(pairs, 0, n_hist, **kw)
        err = self.ctx.lib.zk_last_error(self.ctx.h)
        assert (rc_, n) == ((ENOSPC if entries else OK), len(entries)), (rc_, n, len(entries), err)
        if entries:
            assert not s.any() and not h.any()
        rc_, n, s, h, rec, cls, cnt = self.call(pairs, len(entries), n_hist, **kw)
        assert (rc_, n) == (OK, len(entries)), (rc_, n, err)
        assert s.tolist() == single.tolist() and h.tolist() == hist.tolist()
        assert list(zip(rec.tolist(), cls.tolist(), cnt.tolist())) == entries
        return single, hist, entries


# ---- the fixture's cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k5", "k25", "k32"])
def test_cases_and_batches_around_a_wave(ctx, name):
    case = CASES[name]
    v = Votes.of_index(ctx, case["K"], ref_of(name))
    try:
        pairs = pairs_of(case)
        single, hist, entries = v.check(pairs)
        assert (single.any() or name == "k5") and entries and len({r for r, _, _ in entries}) >= 8      # at K = 5 every record hits many classes
        for n in (1, 63, 64, 65):
            v.check(pairs[-n:])
            v.check(pairs[:n], eol="\r\n")
    finally:
        v.free()


def two_exons(ctx, K=25, seed=7):
    rng = random.Random(seed)
    a, b = rand_seq(rng, 120), rand_seq(rng, 120)
    cls_of = {x: 0 for x, _, _ in R.kmers_with_pos(K, a)}
    cls_of.update({x: 1 for x, _, _ in R.kmers_with_pos(K, b)})
    return rng, a, b, Votes(ctx, K, cls_of, 3)


def test_mates_and_orientations(ctx):
    """a class hit from mate 1 only, from mate 2 only, and from both, where the counts add; orientation 0 only and 1 only"""
    K = 25
    rng, a, b, v = two_exons(ctx, K)
    try:
        junk = lambda: rand_seq(rng, 50)
        w = lambda n: n - K + 1
        for pairs, want in (
                ([(a[:40], junk())], {0: (0, w(40))}), ([(junk(), rc(a[10:60]))], {0: (0, w(50))}),
                ([(a[:40], rc(a[30:90]))], {0: (0, w(40) + w(60))}), ([(rc(a[:40]), junk())], {1: (0, w(40))}),
                ([(junk(), b[5:45])], {1: (1, w(40))}), ([(rc(b[:30]), b[20:70])], {1: (1, w(30) + w(50))}),
                ([(a[:40], a[50:90])], {0: (0, w(40)), 1: (0, w(40))}), ([(junk(), junk())], {})):
            single, hist, entries = v.check(pairs)
            assert not entries
            got = {}
            for o, (c, h) in want.items():
                got[c] = (got.get(c, (0, 0))[0] + 1, got.get(c, (0, 0))[1] + h)
            assert {c: (int(single[2 * c]), int(single[2 * c + 1])) for c in range(3) if single[2 * c]} == got
            assert int(hist.sum()) == len(want) and all(hist[h] for _, h in want.values())
    finally:
        v.free()


def test_one_class_records_are_tallied_and_the_others_listed(ctx):
    K = 25
    rng, a, b, v = two_exons(ctx, K)
    try:
        pairs = [(a[:40], rand_seq(rng, 40)), (a[:40] + "N" + b[:30], rand_seq(rng, 40)), (a[60:100], rc(b[10:70])), (rc(b[:50]), b[40:90]),
                 (rc(a[:33] + "n" + b[:29]), a[5:35])]
        single, hist, entries = v.check(pairs)
        assert entries == [(2, 0, 16), (2, 1, 6), (4, 0, 16), (4, 1, 36), (9, 0, 15), (9, 1, 5)]
        assert single.tolist() == [1, 16, 1, 26 + 26, 0, 0] and int(hist.sum()) == 2 and hist[16] == 1 and hist[52] == 1
    finally:
        v.free()


# ---- around ZK_FIZZLE_CLASSES ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd", [CLASSES - 1, CLASSES, CLASSES + 1, 2 * CLASSES + 3])
def test_distinct_classes_around_the_bound(ctx, nd):
    """every window of two long lines in a class of its own (the table straight from arrays, the classes numbered against the
    order of the windows); that record first, last and between ordinary ones; two of its windows occur twice"""
    K = 16
    rng = random.Random(nd)
    n1 = nd // 2 + 5
    l1, l2 = rand_seq(rng, n1 + K - 1), rand_seq(rng, nd - n1 + K - 1)
    xs = [x for x, _, _ in R.kmers_with_pos(K, l1)] + [x for x, _, _ in R.kmers_with_pos(K, l2)]
    assert len(set(xs)) == nd
    order = list(range(nd))
    rng.shuffle(order)
    cls_of = dict(zip(xs, order))
    other = rand_seq(rng, 90)
    for x, _, _ in R.kmers_with_pos(K, other):
        cls_of.setdefault(x, nd)
    v = Votes(ctx, K, cls_of, nd + 1)
    try:
        big = (l1 + "N" + l1[:K + 1], rc(l2))
        plain = [(other[:50], rc(other[30:80])), (other[:40] + "N" + l1[3:3 + K + 2], rand_seq(rng, 30)), (rand_seq(rng, 40), rand_seq(rng, 40))]
        for pairs in ([big] + plain, plain + [big], plain[:2] + [big] + plain[1:], [big]):
            single, hist, entries = v.check(pairs)
            at = pairs.index(big)
            mine = [e for e in entries if e[0] == 2 * at]
            assert len(mine) == nd and [c for _, c, _ in mine] == list(range(nd)) and sorted(k for _, _, k in mine) == [1] * (nd - 2) + [2, 2]
    finally:
        v.free()


# ---- adds, clamp, cuts, capacity ---------------------------------------------------------------------------------------------------
def small_batch(ctx):
    case = CASES["k25"]
    v = Votes.of_index(ctx, 25, ref_of("k25"))
    return v, pairs_of(case)[-14:]


def test_preloaded_tallies_are_added_to_and_the_clamp(ctx):
    v, pairs = small_batch(ctx)
    try:
        rng = np.random.default_rng(3)
        single, hist, entries = expect(25, v.cls_of, pairs, 256, v.n_classes)
        s0, h0 = rng.integers(1, 1 << 40, len(single)).astype(np.uint64), rng.integers(1, 1 << 40, 256).astype(np.uint64)
        rc_, n, s, h, rec, cls, cnt = v.call(pairs, len(entries), 256, single0=s0, hist0=h0)
        assert rc_ == OK and s.tolist() == (s0 + single).tolist() and h.tolist() == (h0 + hist).tolist()
        assert list(zip(rec.tolist(), cls.tolist(), cnt.tolist())) == entries
        top = int(np.flatnonzero(hist)[-1])
        for n_hist in (top, top + 1, 2, 1):                    # one short of the largest hit count: it lands in the last bin
            want = expect(25, v.cls_of, pairs, n_hist, v.n_classes)[1]
            assert int(want.sum()) == int(hist.sum()) and (n_hist != top or want[top - 1] > hist[top - 1])
            v.check(pairs, n_hist=n_hist)
    finally:
        v.free()


def test_a_batch_cut_anywhere_gives_the_totals_and_the_lists_of_one_call(ctx):
    v, pairs = small_batch(ctx)
    try:
        single, hist, entries = v.check(pairs)
        for cut in range(1, len(pairs)):
            ea = expect(25, v.cls_of, pairs[:cut], 256, v.n_classes)[2]
            eb = expect(25, v.cls_of, pairs[cut:], 256, v.n_classes)[2]
            rc_, n, s, h, rec, cls, cnt = v.call(pairs[:cut], len(ea))
            got = list(zip(rec.tolist(), cls.tolist(), cnt.tolist()))
            rc2, n2, s, h, rec, cls, cnt = v.call(pairs[cut:], len(eb), single0=s, hist0=h)
            got += [(r + 2 * cut, c, k) for r, c, k in zip(rec.tolist(), cls.tolist(), cnt.tolist())]
            assert (rc_, rc2) == (OK, OK) and got == entries and s.tolist() == single.tolist() and h.tolist() == hist.tolist(), cut
    finally:
        v.free()


def test_capacity_and_the_repeat_counts_once(ctx):
    v, pairs = small_batch(ctx)
    try:
        single, hist, entries = expect(25, v.cls_of, pairs, 256, v.n_classes)
        need = len(entries)
        assert need > 4
        s0, h0 = np.arange(len(single), dtype=np.uint64) + 5, np.arange(256, dtype=np.uint64) + 9
        for cap in (0, 1, need - 1):
            rc_, n, s, h, rec, cls, cnt = v.call(pairs, cap, single0=s0, hist0=h0)
            assert (rc_, n) == (ENOSPC, need) and s.tolist() == s0.tolist() and h.tolist() == h0.tolist()
            assert np.all(rec == G32) and np.all(cls == G32) and np.all(cnt == G32)
        for cap in (need, need + 1):
            rc_, n, s, h, rec, cls, cnt = v.call(pairs, cap, single0=s0, hist0=h0)
            assert (rc_, n) == (OK, need) and s.tolist() == (s0 + single).tolist() and h.tolist() == (h0 + hist).tolist()
            assert list(zip(rec[:need].tolist(), cls[:need].tolist(), cnt[:need].tolist())) == entries
    finally:
        v.free()


@pytest.mark.parametrize("lead", [1, 3, 7])
def test_views_at_odd_offsets(ctx, lead):
    v, pairs = small_batch(ctx)
    try:
        v.check(pairs, lead=lead)
    finally:
        v.free()


def test_the_same_call_twice_gives_the_same_bytes(ctx):
    case = CASES["k5"]
    v = Votes.of_index(ctx, 5, ref_of("k5"))
    try:
        pairs = pairs_of(case)
        need = len(expect(5, v.cls_of, pairs, 256, v.n_classes)[2])
        a, b = v.call(pairs, need + 3), v.call(pairs, need + 3)
        assert a[0] == OK and a[:2] == b[:2] and all(x.tobytes() == y.tobytes() for x, y in zip(a[2:], b[2:]))
    finally:
        v.free()


# ---- nothing to do, and refusals -----------------------------------------------------------------------------------------------------
def test_empty_inputs(ctx):
    rng, a, b, v = two_exons(ctx, 25)
    empty = Votes(ctx, 25, {}, 0)
    try:
        pairs = [(a[:40], b[:40])]
        rc_, n, s, h, _, _, _ = empty.call(pairs, 4)
        assert (rc_, n) == (OK, 0) and not h.any()
        rc_, n, s, h, _, _, _ = v.call(pairs, 4, n_reads=0)
        assert (rc_, n) == (OK, 0) and not s.any() and not h.any()
        rc_, n, s, h, _, _, _ = v.call([], 4)
        assert (rc_, n) == (OK, 0) and not s.any() and not h.any()
        single, hist, entries = v.check([(a[:24], b[:24]), ("", ""), (a[:24], ""), ("", rc(b[:25]))])       # lines shorter than K
        assert not entries and single.tolist() == [0, 0, 1, 1, 0, 0]
    finally:
        v.free()
        empty.free()


def test_einval_and_erange_before_any_launch(ctx):
    rng, a, b, v = two_exons(ctx, 25)
    try:
        pairs = [(a[:40] + "N" + b[:40], b[:40])]
        for kw in (dict(K=0), dict(K=33), dict(K=-1), dict(K=24), dict(n_classes=2), dict(n_classes=4), dict(n_hist=0)):
            rc_, n, s, h, rec, cls, cnt = v.call(pairs, 4, **{"n_hist": 256, **kw})
            assert rc_ == EINVAL and not s.any() and not h.any() and np.all(rec == G32), kw
        rc_ = v.call(pairs, 4, n_reads=1 << 31)[0]
        assert rc_ == ERANGE
        t1, l1, k1 = v.mate(fastq_text([pairs[0][0]]), 1)
        t2, l2, k2 = v.mate(fastq_text([pairs[0][1]]), 1)
        single, hist = ctx.upload(np.zeros(6, np.uint64)), ctx.upload(np.zeros(64, np.uint64))
        outs = [ctx.upload(np.zeros(8, np.uint32)) for _ in range(3)]
        n = C.c_uint64(0)
        good = [ctx.h, v.table.h, 25, t1.ptr, l1.ptr, t2.ptr, l2.ptr, 1, 3, single.ptr, hist.ptr, 64, outs[0].ptr, outs[1].ptr, outs[2].ptr, 8, C.byref(n)]
        for i in (1, 3, 4, 5, 6, 9, 10, 12, 13, 14, 16):
            args = list(good)
            args[i] = None
            assert ctx.lib.zk_fizzle_votes(*args) == EINVAL, i
        assert not single.to_host().any() and not hist.to_host().any()
        assert ctx.lib.zk_fizzle_votes(*good) == OK and n.value == 2 and outs[1].to_host()[:2].tolist() == [0, 1]      # the context stays usable
        args = list(good)
        args[12:16] = [None, None, None, 0]
        assert ctx.lib.zk_fizzle_votes(*args) == ENOSPC and n.value == 2                                              # cap = 0 sizes the lists
    finally:
        v.free()


# ---- the command -----------------------------------------------------------------------------------------------------------------------
def run(args):
    from zotmer_amd import cli
    out, err = io.StringIO(), io.StringIO()
    code = None
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            code = cli.main_inner(args)
        except SystemExit as e:
            code = e.code
    return code, out.getvalue(), err.getvalue()


@pytest.mark.parametrize("name", list(CASES))
def test_command_end_to_end(ctx, name, tmp_path, monkeypatch):
    """-P, then -X on its BED, then the scan and -T on that index: the text of the restatement, and of the fixture where it has it"""
    case, gold = CASES[name], GOLD[name]
    K = case["K"]
    p = write_case(case, str(tmp_path))
    bed, index = str(tmp_path / "genes.bed"), str(tmp_path / "index.yaml")
    code, out, err = run(["fizzle", "-P", p["gene_list"], p["ref_gene"], bed])
    assert (code, out, err, open(bed).read()) == (0, "", gold["bed_err"], gold["bed"])
    code, out, err = run(["fizzle", "-X", "-g", p["home"], index, bed])
    assert (code, out, err, open(index).read()) == (0, "", "", gold["index"])
    ref = ref_of(name)
    idx, _ = R.tuple_index(K, ref)
    acc, hit_counts, rn = R.scan(K, idx, pairs_of(case))
    table = "".join(l + "\n" for l in R.table(ref, acc))
    verbose = "".join(l + "\n" for l in R.verbose_lines(hit_counts, rn))
    code, out, err = run(["fizzle", "-k", str(K), "-v", index, p["reads_1"], p["reads_2"]])
    assert code in (0, None) and out == table and err.endswith(verbose), err
    want = "".join(l + "\n" for l in R.table(ref, acc, gene_count=(2, 9), min_exon_rate=20.0))
    code, out, err = run(["fizzle", "-k", str(K), "-Z", "2:9", "-r", "20", index, p["reads_1"], p["reads_2"]])
    assert code in (0, None) and out == want and err == "" and len(want.split("\n")) > 3
    # ... several batches a case, and a histogram that has to grow; both files twice: two pairs of inputs
    monkeypatch.setattr(fizzle, "FIRST_HIST", 8)
    ci = fizzle.ClassIndex(K, fizzle.load_index(index))
    stats, buf = fizzle.new_stats(), io.StringIO()
    fizzle.run_scan(ctx, ci, [p["reads_1"], p["reads_2"]] * 2, 4096, buf, stats=stats)
    acc2 = {k: [2 * a, 2 * b] for k, (a, b) in acc.items()}
    assert buf.getvalue() == "".join(l + "\n" for l in R.table(ref, acc2))
    assert stats["batches"] >= 6 and stats["pairs"] == 2 * rn and stats["multi_records"] > 0
    assert stats["hist_grown"] >= 1 or name == "k5"             # at K = 5 no record has one class: the device histogram stays empty
    if name.startswith("k25"):
        assert stats["slow_records"] >= 6
    rep = dump_yaml(R.crosstalk(K, ref, lambda ch: case["chroms"][ch]))
    code, out, err = run(["fizzle", "-T", "-k", str(K), "-g", p["home"], index])
    assert code in (0, None) and out == rep and err == "" and "GB/02" in out
