"""
`zot hgvs-gen` on the CPU: the lines of the restatement (tests/_hgvsgen_restatement.py) against the reference's
(tests/golden/g1_hgvsgen.json) and against the variants of library/hgvsindex.py, the statistics of the draws, the tables of
zotmer_amd/synth.py, the refusals of the command, and the round trip into hgvs-index, spikein and hgvs-find.  No device.
"""
import json
import math
import os

import pytest

from tests import _hgvsfind_restatement as HF
from tests import _hgvsgen_cases as cases
from tests import _hgvsgen_restatement as R
from tests import _spikein_cases as genome
from tests import _spikein_restatement as SR
from zotmer_amd import cli, synth
from zotmer_amd.library import hgvsgen, hgvsindex, spikein

HERE = os.path.dirname(os.path.abspath(__file__))
KIND_NAMES = {R.SUB: "sub", R.DEL: "del", R.INS: "ins", R.DELINS: "delins", R.DUP: "dup", R.ANI: "insN", R.AND: "delinsN"}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "g1_hgvsgen.json")) as f:
        return {c["name"]: c for c in json.load(f)}


def check_line(text):
    """a -T line: parsed into a row it is spelled again exactly so, and its columns are what library/hgvsindex.py says of
    the variant in its last column -> (accession, row)"""
    acc, row = R.parse_line(text)
    big = genome.GENOME[acc]
    assert R.line(acc, row, cases.base_at(acc), True) == text
    cols = text.split("\t")
    v = hgvsindex.make_variant(cols[6])
    assert v is not None and str(v) == cols[6] and v.kind == KIND_NAMES[row[0]] and v.acc == acc
    assert [int(cols[1]), int(cols[2])] == list(v.range()) and int(cols[3]) == v.size()
    assert cols[4] == big[v.range()[0]:v.range()[1]].upper() and cols[5] == v.sequence(big)
    assert R.line(acc, row, cases.base_at(acc), False) == cols[6]
    return acc, row


def check_text(lines, bed):
    """every line of a -T -V text; the `#` lines stand where the name of the zone changes -> the rows"""
    zl = R.zone_list(R.read_bed(bed))
    rows, prev, expect = [], None, None
    for text in lines:
        if text.startswith("# "):
            assert expect is None
            expect = text
            continue
        acc, row = check_line(text)
        inside = [z for z in zl if z[0] == acc and z[1] <= row[1] <= row[2] <= z[2]]
        assert len(inside) == 1, text
        name = inside[0][3]
        assert (expect == "# %s : %s" % (acc, name)) if name != prev else expect is None, text
        prev, expect = name, None
        rows.append(row)
    assert expect is None
    return rows


def test_golden_lines_are_the_restatements(golden):
    kinds, starts, ends, single = set(), 0, 0, 0
    for name, case in golden.items():
        if case["error"]:
            continue
        rows = check_text(case["lines"], case["bed"])
        assert len(rows) == int(case["opts"][case["opts"].index("-N") + 1])
        kinds |= {r[0] for r in rows}
        if name in cases.KINDS:
            assert {r[0] for r in rows} == {cases.KINDS.index(name)}
        starts += sum(r[1] == 0 for r in rows)
        ends += sum(r[2] in (genome.SIZES["chrA"] - 1, genome.SIZES["chrB"] - 1) for r in rows)
        single += sum(r[1] == r[2] and r[0] in (R.DEL, R.DUP, R.DELINS, R.AND) for r in rows)
    assert kinds == set(range(7)) and starts > 0 and ends > 0 and single > 0
    assert max(len(l) for l in golden["long"]["lines"]) > 1000


def test_a_mean_of_exactly_one(golden):
    """the reference's geomvar dies there (log1p(-1)); here the length is always 1, the law the nearby means approach"""
    for name in ("D1_I3", "D3_I1"):
        assert golden[name]["error"] == "ValueError: math domain error" and golden[name]["lines"] == []
    near = check_text(golden["D1.001_I3"]["lines"], cases.BED)
    assert sum(r[2] - r[1] > 1 for r in near) <= 1 and all(r[3] > 1 for r in near if r[2] - r[1] == 1)
    P = R.Params(R.parse_types("delins,and"), D=1.0, I=3.0)
    assert P.QD == [] and P.mix == 1 << 32
    assert all(R.lengths(5, v, P)[0] == 1 and R.lengths(5, v, P)[1] > 1 for v in range(300))
    P = R.Params(R.parse_types("delins,and"), D=3.0, I=1.0)
    assert P.QI == [] and P.mix == 0
    assert all(R.lengths(5, v, P)[0] > 1 and R.lengths(5, v, P)[1] == 1 for v in range(300))


@pytest.mark.parametrize("types,D,I,U", [(cases.ALL, 1.5, 1.5, 3.0), ("sub,dup", 1.5, 1.5, 40.0), ("3:delins,and,ins", 1.0, 2.0, 1.0)])
def test_restatement_lines_pass_the_same_check(types, D, I, U):
    P = R.Params(R.parse_types(types), D, I, U)
    text = R.command(cases.BED, genome.GENOME, 31, 300, P, tab=True, heads=True)
    rows = check_text(text.split("\n")[:-1], cases.BED)
    assert len(rows) == 300
    plain = R.command(cases.BED, genome.GENOME, 31, 300, P)
    assert plain.split("\n")[:-1] == [l.split("\t")[6] for l in text.split("\n")[:-1] if not l.startswith("#")]
    for s in plain.split("\n")[:-1]:
        assert str(hgvsindex.make_variant(s)) == s


def test_library_tables_are_the_restatements(tmp_path):
    genome.write_genome(str(tmp_path))
    (tmp_path / "z.bed").write_text(cases.BED)
    plan = hgvsgen.make_plan(dict(bed=str(tmp_path / "z.bed"), home=str(tmp_path), names=None, seed=3, types="2:sub,del,0.5:and,sub", D=2.0, I=1.5, U=40))
    P = R.Params(R.parse_types("2:sub,del,0.5:and,sub"), 2.0, 1.5, 40)
    assert (plan.thr, plan.tables, plan.mix) == (P.thr, [P.QD, P.QI, P.QU], P.mix) and synth.hg_words(plan.tables[1]) == P.W
    zl = R.zone_list(R.read_bed(cases.BED))
    assert plan.zones == zl and [w.decode() for w in plan.windows] == [genome.GENOME[c][s:e + 1] for c, s, e, _ in zl]
    counts = R.zone_counts(3, zl, 500)
    assert [synth.spike_zone_of(3, n, [int(c) for c in plan.cum]) for n in range(40)] == \
        [next(z for z in range(len(zl)) if R.zone_counts(3, zl, n + 1)[z] != R.zone_counts(3, zl, n)[z]) for n in range(40)]
    text, rows, first, accs, acc_offs, names, name_offs = plan.device_tables(counts)
    used = [z for z, n in enumerate(counts) if n]
    assert first.tolist() == [sum(counts[z] for z in used[:k]) for k in range(len(used) + 1)] and int(first[-1]) == 500
    assert rows.reshape(-1, 3)[:, 1:].tolist() == [[zl[z][1], zl[z][2]] for z in used]
    got = [names[int(a):int(b)].tobytes().decode() for a, b in zip(name_offs[:-1], name_offs[1:])]
    assert got == [zl[z][3] if k == 0 or zl[z][3] != zl[used[k - 1]][3] else "" for k, z in enumerate(used)] and "" in got


# ---- statistics ------------------------------------------------------------------------------------------------------------------
def test_statistics_of_the_draws():
    """20000 variants at the defaults: every figure within 5 standard deviations of its expectation"""
    N, seed, D, I, U = 20000, 77, 1.5, 1.5, 3.0
    P = R.Params()
    zl = R.zone_list(R.read_bed(cases.BED))
    counts = R.zone_counts(seed, zl, N)
    T = sum(e - s + 1 for _, s, e, _ in zl)

    def share(k, n, p):
        assert abs(k - n * p) <= 5 * math.sqrt(n * p * (1 - p)), (k, n, p)

    def mean_of(xs, mean, success):
        """a geometric variable on 1, 2, ... has the variance (1 - success) / success^2"""
        sd = math.sqrt((1 - success) / success ** 2 / len(xs))
        assert abs(sum(xs) / len(xs) - mean) <= 5 * sd, (sum(xs) / len(xs), mean, sd)
    for (_, s, e, _), k in zip(zl, counts):
        share(k, N, (e - s + 1) / T)
    kinds = [R.kind_of(seed, v, P.thr) for v in range(N)]
    for k in range(5):
        share(kinds.count(k), N, 0.2)
    assert kinds.count(R.ANI) == kinds.count(R.AND) == 0
    raw = {k: [R.raw_lengths(seed, v, k, P) for v in range(N) if kinds[v] == k] for k in range(5)}
    mean_of([l for l, _ in raw[R.DEL]], D, 1 / D)
    mean_of([m for _, m in raw[R.INS]], I, 1 / I)
    mean_of([u for u, _ in raw[R.DUP]], U, 1 / U)
    # delins: the conditional law of the reference's rejection loop
    pd, pi = 1 / D, 1 / I
    both = raw[R.DELINS]
    assert all(l > 1 or m > 1 for l, m in both)
    share(sum(l == 1 for l, _ in both), len(both), pd * (1 - pi) / (1 - pd * pi))
    mean_of([m - 1 for l, m in both if l == 1], I, pi)              # m = 1 + geom(I) given l = 1
    mean_of([l - 1 for l, m in both if l > 1], D, pd)               # l = 1 + geom(D) otherwise
    mean_of([m for l, m in both if l > 1], I, pi)


# ---- the geometric table -------------------------------------------------------------------------------------------------------
def test_geometric_tables():
    assert synth.hg_geom_table(1) == synth.hg_geom_table(1.0) == [] and synth.hg_geom(synth.hg_geom_table(1), 0) == 1
    q = synth.hg_geom_table(1.5)
    assert q == R.geom_table(1.5) and len(q) == 19 and q[:3] == [1431655765, 477218588, 159072862] and q[-2:] == [10, 3]
    assert q[0] == R.frac32(1 / 3) and all(q[k] == (q[k - 1] * q[0]) >> 32 for k in range(1, 19)) and (q[-1] * q[0]) >> 32 == 0
    for r, want in ((0, 20), (2, 20), (3, 19), (q[0] - 1, 2), (q[0], 1), ((1 << 32) - 1, 1)):
        assert synth.hg_geom(q, r) == R.geom(q, r) == want
    # the largest whole mean whose table fits: 65536 entries, down to 1
    big = synth.hg_geom_table(4574)
    assert len(big) == synth.HG_TABLE_MAX == 65536 and big[-3:] == [3, 2, 1] and big[:2] == [4294028300, 4293089509] and big == R.geom_table(4574)
    assert all(a > b for a, b in zip(big, big[1:]))
    for bad in (4575, 1e9, 0.999, 0, -2, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            synth.hg_geom_table(bad)
    assert synth.hg_words(q) == 1 and synth.hg_words(big) == (65536 + 2 + 31) // 32
    assert synth.hg_type_thresholds([1, 1, 1, 1, 1, 0, 0]) == R.type_thresholds([1, 1, 1, 1, 1, 0, 0]) == \
        [858993459, 1717986918, 2576980378, 3435973837, 1 << 32, 1 << 32, 1 << 32]
    assert synth.hg_type_thresholds([0, 0, 2, 0, 0, 0, 0]) == [0, 0] + [1 << 32] * 5
    assert synth.hg_mix_thr(1.5, 1.5) == R.mix_thr(1.5, 1.5) == R.frac32(0.4)
    with pytest.raises(ValueError):
        synth.hg_mix_thr(1, 1)


# ---- the command ------------------------------------------------------------------------------------------------------------
def _refused(capsys, argv):
    with pytest.raises(SystemExit) as e:
        cli.main_inner(["hgvs-gen"] + argv)
    assert e.value.code == 1
    return capsys.readouterr().err


def test_refusals(tmp_path, capsys, monkeypatch):
    d = str(tmp_path)
    genome.write_genome(d)
    bed = os.path.join(d, "z.bed")
    with open(bed, "w") as f:
        f.write(cases.BED)
    base = ["-g", d, "-S", "1", "-N", "10", "-o", os.path.join(d, "out.txt")]
    assert "unknown variant type inv" in _refused(capsys, base + ["-t", "sub,inv", bed])
    assert "negative or not finite" in _refused(capsys, base + ["-t", "-1:sub", bed])
    assert "negative or not finite" in _refused(capsys, base + ["-t", "nan:sub,del", bed])
    assert "negative or not finite" in _refused(capsys, base + ["-t", "inf:sub", bed])
    assert "every type has probability 0" in _refused(capsys, base + ["-t", "0:sub,0:del", bed])
    assert "unexpected variant category descriptor" in _refused(capsys, base + ["-t", "1:2:sub", bed])
    assert "option -D" in _refused(capsys, base + ["-D", "0.5", bed])
    assert "option -I" in _refused(capsys, base + ["-I", "nan", bed])
    assert "option -U" in _refused(capsys, base + ["-U", "4575", bed])
    assert "option -U" in _refused(capsys, base + ["-U", "inf", bed])
    assert "nothing to draw" in _refused(capsys, base + ["-D", "1", "-I", "1", bed])
    for text, word in (("chrA\t50\t40\tx\n", "empty or starts below 0"), ("chrA\t-1\t40\tx\n", "empty or starts below 0"),
                       ("chrA\t8000\t%d\tx\n" % genome.SIZES["chrA"], "ends beyond the 8192 bases"), ("chrZ\t1\t2\tx\n", "no sequence file for chrZ"),
                       ("chrA\t1\tx\n", "no integer"), ("chrA\t1\n", "expected a chromosome"), ("", "no zones")):
        with open(os.path.join(d, "bad.bed"), "w") as f:
            f.write(text)
        assert word in _refused(capsys, base + [os.path.join(d, "bad.bed")])
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert "single GPU" in _refused(capsys, base + [bed])
    assert not os.path.exists(os.path.join(d, "out.txt"))
    # -D 1 -I 1 is fine where neither delins nor `and` can be drawn; a zone without ACGT is refused once it has draws
    monkeypatch.delenv("WORLD_SIZE")
    plan = hgvsgen.make_plan(dict(bed=bed, home=d, names=None, seed=1, types="sub,del", D=1, I=1, U=1))
    assert plan.mix == 0 and plan.tables == [[], [], []]
    with open(os.path.join(d, "n.bed"), "w") as f:
        f.write("chrA\t2505\t2530\tenn\nchrA\t100\t200\tfine\n")
    plan = hgvsgen.make_plan(dict(bed=os.path.join(d, "n.bed"), home=d, names=None, seed=1, types="sub,del", D=1.5, I=1.5, U=3))
    plan.check_counts([0, 5])
    with pytest.raises(hgvsgen.InputError) as e:
        plan.check_counts([1, 5])
    assert "chrA:2505-2530 holds no base of ACGT" in str(e.value)
    hgvsgen.make_plan(dict(bed=os.path.join(d, "n.bed"), home=d, names=None, seed=1, types="ins,del", D=1.5, I=1.5, U=3)).check_counts([1, 5])


def test_unnamed_zones_and_names(tmp_path):
    d = str(tmp_path)
    genome.write_genome(d, gz=False)
    (tmp_path / "u.bed").write_text(cases.BED_UNNAMED.replace("chrA", "NC_A.1"))
    plan = hgvsgen.make_plan(dict(bed=str(tmp_path / "u.bed"), home=d, names={"NC_A.1": "chrA"}, seed=1, types="sub", D=1.5, I=1.5, U=3))
    assert plan.zones == [("NC_A.1", 100, 200, "x"), ("NC_A.1", 300, 400, "None"), ("chrB", 100, 200, "None")]
    assert plan.zones == R.zone_list(R.read_bed(cases.BED_UNNAMED.replace("chrA", "NC_A.1")))
    names = plan.device_tables([1, 1, 1])[5].tobytes()
    assert names == b"xNone"                      # the third zone repeats the name before it: no `#` line


def test_help_and_listing(capsys):
    assert "hgvs-gen" in cli.available()
    assert cli.main_inner(["help", "hgvs-gen"]) == 0
    text = capsys.readouterr().out
    for word in ("zot hgvs-gen [options] <regions>", "-B MB", "-n NAMES", "-o FILE", "Differences from the reference", "counter-based",
                 "2^-32", "rejection loop", "64 positions", "called None", "one GPU for now", "Nothing touches the device"):
        assert word in " ".join(text.split()), word


# ---- round trip -------------------------------------------------------------------------------------------------------------
def round_variants():
    P = R.Params(R.parse_types(cases.ROUND_TYPES))
    return R.command(cases.ROUND_BED, genome.GENOME, cases.ROUND_SEED, cases.ROUND_N, P).split()


def test_round_trip_file_is_accepted(tmp_path, capsys):
    texts = round_variants()
    vs = [hgvsindex.make_variant(t) for t in texts]
    assert len(vs) == 8 and sum(v.kind == "sub" for v in vs) >= 2 and len({v.kind for v in vs}) >= 4
    assert not any(spikein.ranges_overlap(x.range(), y.range()) for i, x in enumerate(vs) for y in vs[i + 1:])
    assert min(abs(x.range()[0] - y.range()[0]) for i, x in enumerate(vs) for y in vs[i + 1:]) > 300
    # the host part of hgvs-index: the items of the panel
    genome.write_genome(str(tmp_path))
    items, variants = hgvsindex.make_items(texts, hgvsindex.Home(str(tmp_path)), 75)
    assert [i["hgvs"] for i in items] == texts and len(variants) == 8
    # ... and of spikein: -f with a zone that holds them all
    (tmp_path / "v.txt").write_text("".join(t + "\n" for t in texts))
    (tmp_path / "z.bed").write_text(cases.ROUND_SPIKE_BED)
    plan = spikein.make_plan(dict(bed=str(tmp_path / "z.bed"), home=str(tmp_path), names=None, file=str(tmp_path / "v.txt"), pop=None, seed=1,
                                  L=100, I=300, D=0.1), [])
    assert [str(v) for v in plan.zones[0][3].applied] == texts and capsys.readouterr().err == ""


def test_round_trip_through_hgvs_find():
    """on the restatements of the three commands: one row per variant, every one called mut at -V 1.0"""
    texts = round_variants()
    vs = [hgvsindex.make_variant(t) for t in texts]
    index = [hgvsindex.indexed_variant(v, 75, genome.GENOME["chrA"]) for v in vs]
    t1, t2, _ = SR.command(genome.GENOME, cases.ROUND_SPIKE_BED, texts, seed=11, N=cases.ROUND_SPIKE_N, V=1.0)
    out = HF.find(index, [t1, t2]).split("\n")
    rows = [dict(zip(out[0].split("\t"), l.split("\t"))) for l in out[1:] if l]
    assert [r["hgvs"] for r in rows] == texts
    assert [r["res"] for r in rows] == ["mut"] * 8
