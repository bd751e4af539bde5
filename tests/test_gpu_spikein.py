"""`zot spikein` on the device: zk_spike_pairs and zk_spike_zone_counts against the restatement (tests/_spikein_restatement.py)
byte for byte, the capacity contract in guarded buffers, offset views, the command against the restatement's files, and the
round trip hgvs-index -> spikein -> hgvs-find."""
import contextlib
import gzip
import io

import numpy as np
import pytest

from tests import _spikein_cases as cases
from tests import _spikein_check as chk
from tests import _spikein_restatement as R
from tests._spikein_cases import allele_text, tables
from zotmer_amd import native, synth

pytestmark = pytest.mark.gpu

GUARD = 0xA5


@pytest.fixture(scope="module")
def ctx():
    from zotmer_amd.library import engine
    yield engine.context()
    engine.close()


class Run:
    """one set of tables on the device and its scalars"""

    def __init__(self, ctx, zones, seed, L, I, D, V, E, windows=None):
        self.ctx, self.zones = ctx, zones
        self.scalars = (seed, L, I, R.sd_q(I, D), R.frac32(V), R.frac32(E))
        self.dev = [ctx.upload(a) for a in tables(zones, windows)]
        self.n = sum(z[1] for z in zones)

    def device(self, first=0, count=None):
        count = self.n - first if count is None else count
        o1, o2 = self.ctx.spike_pairs(*self.dev, *self.scalars, first, count)
        return o1.to_host().tobytes(), o2.to_host().tobytes()

    def want(self, first=0, count=None):
        seed, L, I, q, tv, te = self.scalars
        a, b, _ = R.records(seed, L, I, q, tv, te, self.zones, first, count)
        return a.encode("latin-1"), b.encode("latin-1")

    def into(self, first, count, out1, out2):
        return self.ctx.spike_pairs_into(*self.dev, *self.scalars, first, count, out1, out2)


def small_zones(n, L):
    """three zones: none of the pairs, one pair, the rest; a zone of one position (s0 == e0); the two alleles differ"""
    G = max(4 * (L + L // 2) + 700, 1400)
    a, b = allele_text(100 + L, G), allele_text(200 + L, G + 5)
    return [("chr1:5-9 empty ", 0, [(a, 5, 9), (b, 5, 9)]),
            ("chrQ:700-700 None ", 1, [(a, 700, 700), (b, 700, 700)]),
            ("chr1:3-%d wide " % (G - 1), n - 1, [(a, 3, G - 1), (b, 3, G + 2)])]      # u from the start to the end: both clamps


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 100, 129])
def test_pairs_against_the_restatement(ctx, L):
    n_err = 0
    for E in (0.0, 0.005, 0.5, 1.0):
        for V in (0.0, 0.5, 1.0):
            I = max(2 * L, 8)
            run = Run(ctx, small_zones(20, L), seed=1000 * L + int(8 * E) + int(2 * V), L=L, I=I, D=0.15, V=V, E=E)
            got, want = run.device(), run.want()
            assert got == want, (L, E, V)
            n_err += want[0].count(b">")
            if E == 1.0:
                assert want[0].count(b">") == want[1].count(b">") == 20 * L
            if E == 0.0:
                assert b">" not in want[0] + want[1]
    assert n_err > 0


def test_both_clamps_occur(ctx):
    run = Run(ctx, small_zones(200, 100), seed=5, L=100, I=300, D=0.1, V=0.5, E=0.005)
    got, want = run.device(), run.want()
    assert got == want
    heads = [chk.parse_header(h) for h in want[0].decode("latin-1").split("\n")[0::4] if h]
    G = [len(run.zones[2][2][0][0]), len(run.zones[2][2][1][0])]
    assert any(h["u"] == h["fl"] for h in heads) and any(h["u"] + h["fl"] in G for h in heads)


CROSSINGS = [
    # name, allele length, (s0, e0), L, I, D, E, pairs, what must occur among (u, fl, last error position)
    ("u 9/10", 400, (5, 14), 1, 4, 0.0, 0.5, 100, dict(u=(9, 10))),
    ("u 99/100, fl 9/10", 600, (95, 104), 2, 10, 0.1, 0.5, 100, dict(u=(99, 100), fl=(9, 10))),
    ("u 99999/100000, fl 99/100", 100400, (99990, 100009), 63, 100, 0.02, 0.02, 200, dict(u=(99999, 100000), fl=(99, 100))),
    ("fl 99999/100000", 200400, (100100, 100120), 100, 100000, 0.00001, 0.01, 20, dict(fl=(99999, 100000))),
    ("errors 9/10 and 99/100", 1400, (400, 600), 129, 300, 0.1, 0.5, 8, dict(err=(9, 10, 99, 100))),
    ("errors 99999/100000", 300400, (150200, 150210), 100010, 150100, 0.0, 0.02, 2, dict(err=(99999, 100000))),
]


@pytest.mark.parametrize("case", CROSSINGS, ids=[c[0] for c in CROSSINGS])
def test_decimal_lengths_change_inside_a_run(ctx, case):
    name, G, (s0, e0), L, I, D, E, n, need = case
    text = allele_text(len(name), G)
    # at E < 1 the errors the case is about are not left to chance: the seed is searched on the host, in the restatement's draws
    seed = 0
    if "err" in need:
        def hits(seed):
            return all(any((R.rnd(seed, R.T_ERR, (2 * p + m) * L + j) & 0xFFFFFFFF) < R.frac32(E) for p in range(n) for m in (0, 1)) for j in need["err"])
        while not hits(seed):
            seed += 1
    run = Run(ctx, [("c:%d-%d z " % (s0, e0), n, [(text, s0, e0), (text[::-1], s0, e0)])], seed=seed, L=L, I=I, D=D, V=0.5, E=E)
    got, want = run.device(), run.want()
    assert got == want
    heads = [h.split(" ") for h in want[0].decode("latin-1").split("\n")[0::4] if h]
    for k, col in (("u", 2), ("fl", 3)):
        if k in need:
            seen = {int(h[col]) for h in heads}
            assert all(x in seen for x in need[k]), (k, sorted(seen))
    if "err" in need:
        both = (want[0] + want[1]).decode("latin-1")
        seen = {int(e[:-3]) for h in both.split("\n")[0::4] if h for e in h.split(" ")[5].split(";") if e}
        assert all(x in seen for x in need["err"])


@pytest.fixture(scope="module")
def long_run(ctx):
    """a few thousand pairs over several zones, and the restatement's records, computed once"""
    a, b = allele_text(1, 3000), allele_text(2, 3100)
    zones = [("chr1:100-900 a ", 1500, [(a, 100, 900), (b, 100, 905)]), ("chr1:901-901 None ", 0, [(a, 901, 901), (b, 901, 901)]),
             ("chr2:1000-2999 b ", 1700, [(b, 1000, 2999), (a, 1000, 2899)])]
    run = Run(ctx, zones, seed=77, L=20, I=60, D=0.1, V=0.3, E=0.05)
    seed, L, I, q, tv, te = run.scalars
    recs = R.record_list(seed, L, I, q, tv, te, zones)
    return run, [r[0].encode("latin-1") for r in recs], [r[1].encode("latin-1") for r in recs]


def test_a_few_thousand_pairs_and_the_same_call_twice(long_run):
    run, r1, r2 = long_run
    got = run.device()
    assert got == (b"".join(r1), b"".join(r2))
    assert run.device() == got


@pytest.mark.parametrize("first,count", [(0, 1), (1499, 1), (1500, 1), (3199, 1), (7, 63), (1450, 64), (1499, 65), (0, 0), (3200, 0)])
def test_counts_and_firsts(long_run, first, count):
    run, r1, r2 = long_run
    assert run.device(first, count) == (b"".join(r1[first:first + count]), b"".join(r2[first:first + count]))


def test_a_run_cut_anywhere_equals_one_call(long_run):
    run, r1, r2 = long_run
    cuts = [0, 1, 64, 65, 1000, 1499, 1501, 2222, 3199, 3200]
    parts = [run.device(a, b - a) for a, b in zip(cuts, cuts[1:])]
    assert b"".join(p[0] for p in parts) == b"".join(r1) and b"".join(p[1] for p in parts) == b"".join(r2)


# ---- capacity and views ------------------------------------------------------------------------------------------------------
def guarded(ctx, n):
    return ctx.upload(np.full(n, GUARD, dtype=np.uint8))


@pytest.mark.parametrize("front", [0, 1, 7, 13])
def test_capacities_in_guarded_buffers(ctx, long_run, front):
    """capacities one short of, equal to and beyond the need; the outputs at odd byte offsets of larger arrays"""
    run, r1, r2 = long_run
    first, count = 1490, 70
    want = (b"".join(r1[first:first + count]), b"".join(r2[first:first + count]))
    need = (len(want[0]), len(want[1]))
    PAD = 64
    for c1, c2 in ((0, 0), (need[0] - 1, need[1]), (need[0], need[1] - 1), (need[0] - 1, need[1] - 1), (1, 1), need, (need[0] + 9, need[1] + PAD)):
        bufs = [guarded(ctx, front + n + PAD) for n in need]
        nb, fit = run.into(first, count, bufs[0].view(c1, front), bufs[1].view(c2, front))
        assert nb == need and fit == (c1 >= need[0] and c2 >= need[1]), (c1, c2)
        for b, cap, w in zip(bufs, (c1, c2), want):
            h = b.to_host()
            assert np.all(h[:front] == GUARD) and np.all(h[front + (len(w) if fit else cap):] == GUARD), (c1, c2)
            if fit:
                assert h[front:front + len(w)].tobytes() == w
    # the context is as usable as before
    assert run.device(first, count) == want


def test_inputs_at_odd_offsets(ctx, long_run):
    run, r1, r2 = long_run
    text, rows, first, heads, offs = [a.to_host() for a in run.dev]
    big_text = ctx.upload(np.concatenate([np.full(3, GUARD, np.uint8), text, np.full(5, GUARD, np.uint8)]))
    big_heads = ctx.upload(np.concatenate([np.full(1, GUARD, np.uint8), heads]))
    big_rows = ctx.upload(np.concatenate([np.zeros(1, np.uint64), rows]))
    o1, o2 = ctx.spike_pairs(big_text.view(len(text), 3), big_rows.view(len(rows), 1), run.dev[2], big_heads.view(len(heads), 1), run.dev[4],
                             *run.scalars, 1400, 200)
    assert o1.to_host().tobytes() == b"".join(r1[1400:1600]) and o2.to_host().tobytes() == b"".join(r2[1400:1600])


def test_refusals_leave_the_outputs_alone(ctx):
    a = allele_text(9, 3000)
    zones = [("c:1000-2000 z ", 50, [(a, 1000, 2000), (a, 1000, 2000)])]
    bad = [dict(windows={(0, 1): (1000, 2100)}),        # fragments reach e0 + fl: the mutant's window ends before them
           dict(windows={(0, 0): (1500, 3000)})]        # ... and the wild type's starts after s0
    for kw in bad:
        run = Run(ctx, zones, seed=3, L=100, I=300, D=0.1, V=0.5, E=0.01, **kw)
        bufs = [guarded(ctx, 40000), guarded(ctx, 40000)]
        with pytest.raises(native.ZotkError) as e:
            run.into(0, 50, *bufs)
        assert e.value.code == native.ZK_EINVAL
        assert all(np.all(b.to_host() == GUARD) for b in bufs)
    # a pair beyond the last zone's, a zone table that does not ascend
    run = Run(ctx, zones, seed=3, L=100, I=300, D=0.1, V=0.5, E=0.01)
    for first, count in ((40, 11), (50, 1)):
        with pytest.raises(native.ZotkError) as e:
            run.into(first, count, guarded(ctx, 40000), guarded(ctx, 40000))
        assert e.value.code == native.ZK_EINVAL
    for L, I in ((0, 300), (100, 0), ((1 << 20) + 1, 300)):
        seed, _, _, q, tv, te = run.scalars
        with pytest.raises(native.ZotkError) as e:
            ctx.spike_pairs_into(*run.dev, seed, L, I, q, tv, te, 0, 1, guarded(ctx, 64), guarded(ctx, 64))
        assert e.value.code == native.ZK_EINVAL
    assert run.device() == run.want()


# ---- zone counts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz", [1, 2, 1000, 5000])      # 5000: beyond the zones a workgroup counts in LDS
def test_zone_counts(ctx, nz):
    lens = [1 + int(x) % 997 for x in synth.rnd(nz, 9, np.arange(nz, dtype=np.uint64))]
    cum = np.cumsum(lens, dtype=np.uint64)
    N, seed = 6000, 40 + nz
    want = R.zone_counts(seed, [int(c) for c in cum], 0, N)
    d_cum = ctx.upload(cum)
    counts = ctx.upload(np.zeros(nz, dtype=np.uint64))
    ctx.spike_zone_counts(d_cum, seed, 0, N, counts)
    assert counts.to_host().tolist() == want and sum(want) == N
    # a call split in two adds up to the same; no draws, nothing added
    split = ctx.upload(np.zeros(nz, dtype=np.uint64))
    ctx.spike_zone_counts(d_cum, seed, 0, 2500, split)
    ctx.spike_zone_counts(d_cum, seed, 2500, N - 2500, split)
    ctx.spike_zone_counts(d_cum, seed, N, 0, split)
    assert split.to_host().tolist() == want


# ---- the command -------------------------------------------------------------------------------------------------------------
def zot(args):
    from zotmer_amd import cli
    out, err = io.StringIO(), io.StringIO()
    code = 0
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            code = cli.main_inner(args) or 0
        except SystemExit as e:
            code = e.code
    return code, out.getvalue(), err.getvalue()


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    d = tmp_path_factory.mktemp("genome")
    cases.write_genome(str(d))
    return str(d)


@pytest.mark.parametrize("name", [c["name"] for c in cases.make_cases()])
def test_command_against_the_restatement(ctx, genome, tmp_path, name):
    case = next(c for c in cases.make_cases() if c["name"] == name)
    kw = cases.case_numbers(case)
    w1, w2, info = R.command(cases.GENOME, case["bed"], cases.all_variants(case), pop=case["pop"], **kw)
    words = list(case["opts"]) + ["-g", genome] + cases.write_case(case, str(tmp_path))
    log = tmp_path / "log.txt"
    code, out, err = zot(["spikein"] + words + ["-M", "0.01", "-l", str(log), str(tmp_path / "a")] + case["variants"])
    assert (code, out, err) == (0, "", "")
    assert (tmp_path / "a_1.fastq").read_text() == w1 and (tmp_path / "a_2.fastq").read_text() == w2
    assert log.read_text() == ""
    # -z inflates to the same bytes; a 1 MB buffer and -v change nothing
    assert zot(["spikein"] + words + ["-z", "-B", "1", str(tmp_path / "z")] + case["variants"])[0] == 0
    assert gzip.open(str(tmp_path / "z_1.fastq.gz"), "rt").read() == w1 and gzip.open(str(tmp_path / "z_2.fastq.gz"), "rt").read() == w2
    code, out, err = zot(["spikein"] + words + ["-B", "1", "-v", str(tmp_path / "b")] + case["variants"])
    assert code == 0 and "mean coverage = " in err
    assert (tmp_path / "b_1.fastq").read_text() == w1 and (tmp_path / "b_2.fastq").read_text() == w2
    # the checker passes on all records
    by = {(ch, z[0], z[1]): [wt[0], mut[0]] for ch, z, wt, mut in info["zones"]}
    which, rejects = chk.check_pairs(w1, w2, lambda h: by[(h["ch"], h["st"], h["en"])], kw.get("L", 100))
    assert rejects == [] and len(which) == kw["N"]


def test_command_cut_into_many_calls(ctx, genome, tmp_path, monkeypatch):
    """the loop over device calls with buffers that are too small for a call's records: grown, same bytes"""
    from zotmer_amd.library import spikein
    case = cases.make_cases()[1]
    kw = cases.case_numbers(case)
    w1, w2, _ = R.command(cases.GENOME, case["bed"], cases.all_variants(case), pop=case["pop"], **kw)
    o = dict(zip(*[iter(cases.write_case(case, str(tmp_path)))] * 2))
    plan = spikein.make_plan(dict(bed=o["-b"], home=genome, names=None, file=o.get("-f"), pop=o.get("-m"), seed=kw["seed"], L=100, I=300, D=0.1),
                             case["variants"])
    stats = spikein.new_stats()
    counts = spikein.run(ctx, plan, kw["N"], kw["V"], kw["E"], str(tmp_path / "c"), buffer_bytes=3000, stats=stats)
    assert (tmp_path / "c_1.fastq").read_text() == w1 and (tmp_path / "c_2.fastq").read_text() == w2
    assert stats["calls"] > 5 and stats["pairs"] == kw["N"] and int(counts.sum()) == kw["N"]


def test_command_without_a_bed_and_with_names(ctx, tmp_path):
    """every sequence file is one zone; -n maps an accession to its file stem"""
    d = tmp_path / "g"
    cases.write_genome(str(d), gz=False)
    (tmp_path / "names.txt").write_text("NC_A.1 chrA\nNC_B.2 chrB\n")
    var = cases._sub("chrA", 4000).replace("chrA", "NC_A.1")
    code, out, err = zot(["spikein", "-g", str(d), "-n", str(tmp_path / "names.txt"), "-S", "9", "-N", "150", "-V", "0.5", str(tmp_path / "w"), var])
    assert (code, out, err) == (0, "", "")
    w1, w2, info = R.command(cases.GENOME, None, [var], seed=9, N=150, V=0.5, names={"NC_A.1": "chrA", "NC_B.2": "chrB"})
    assert (tmp_path / "w_1.fastq").read_text() == w1 and (tmp_path / "w_2.fastq").read_text() == w2
    assert [z[1] for z in info["zones"]] == [(1, 8192, "chrA"), (1, 4096, "chrB")]


# ---- round trip --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sub", "del"])
@pytest.mark.parametrize("V,call", [("0.5", "wt/mut"), ("1.0", "mut")])
def test_round_trip_on_the_device(ctx, genome, tmp_path, kind, V, call):
    """hgvs-index, spikein, hgvs-find: the calls tests/test_spikein_host.py established on the CPU"""
    text = cases.ROUND_VARIANTS[kind]
    (tmp_path / "z.bed").write_text(cases.ROUND_ZONE)
    assert zot(["hgvs-index", "-g", genome, str(tmp_path / "index.yaml"), text])[0] == 0
    assert zot(["spikein", "-g", genome, "-b", str(tmp_path / "z.bed"), "-S", "11", "-N", str(cases.ROUND_N), "-V", V, str(tmp_path / "r"), text])[0] == 0
    code, out, err = zot(["hgvs-find", str(tmp_path / "index.yaml"), str(tmp_path / "r_1.fastq"), str(tmp_path / "r_2.fastq")])
    assert code == 0, err
    lines = out.split("\n")
    row = dict(zip(lines[0].split("\t"), lines[1].split("\t")))
    assert row["res"] == call, out
