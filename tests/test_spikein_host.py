"""
`zot spikein` on the CPU: the alleles of library/spikein.py against the reference's (tests/golden/s1_spikein.json), the
checker against the reference's records, the restatement against the checker, the statistics of the draws, the refusals of
the command, and a round trip of the restatement's reads through the restatement of `zot hgvs-find`.
"""
import json
import math
import os

import pytest

from tests import _hgvsfind_restatement as HF
from tests import _spikein_cases as cases
from tests import _spikein_check as chk
from tests import _spikein_restatement as R
from zotmer_amd import cli, synth
from zotmer_amd.library import hgvsindex, spikein

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "s1_spikein.json")) as f:
        return {c["name"]: c for c in json.load(f)}


@pytest.fixture(scope="module")
def restated():
    """the restatement's output for every case, computed once"""
    out = {}
    for case in cases.make_cases():
        out[case["name"]] = R.command(cases.GENOME, case["bed"], cases.all_variants(case), pop=case["pop"], **cases.case_numbers(case))
    return out


def test_the_draws_of_synth_are_the_restatements():
    for seed, tag, i in ((0, 16, 0), (1, 21, 12345678901), (2 ** 64 - 1, 19, 2 ** 63), (20261020, 17, 999)):
        assert synth.rnd_int(seed, tag, i) == R.rnd(seed, tag, i)
        assert int(synth.rnd(seed, tag, i)) == R.rnd(seed, tag, i)
    assert (synth.T_ZONE, synth.T_ALLELE, synth.T_POS, synth.T_LEN, synth.T_STRAND, synth.T_ERR, synth.T_ANON, synth.T_POP) == \
        (R.T_ZONE, R.T_ALLELE, R.T_POS, R.T_LEN, R.T_STRAND, R.T_ERR, R.T_ANON, R.T_POP)
    for I, D, L in ((300, 0.1, 100), (80, 0.2, 30), (10, 0.0, 100), (100000, 0.001, 1)):
        q = synth.spike_sd_q(I, D)
        assert q == R.sd_q(I, D) and synth.spike_flmax(I, q, L) == R.flmax(I, q, L)
        for p in (0, 1, 77, 2 ** 33):
            fl = synth.spike_frag_len(5, p, I, q, L)
            assert fl == R.frag_len(5, p, I, q, L) and L + L // 2 <= fl <= synth.spike_flmax(I, q, L)
            assert abs(synth.spike_len_z(5, p)) <= synth.IH_MAX
    cum = [10, 11, 500, 501]
    for n in range(200):
        assert synth.spike_zone_of(9, n, cum) == R.zone_counts(9, cum, n, 1).index(1)


@pytest.mark.parametrize("name", [c["name"] for c in cases.make_cases()])
def test_alleles_equal_the_references(golden, name):
    g = golden[name]
    anon = dict((a, s) for a, s in g["anonymous"])
    assert g["alleles"]
    for rec in g["alleles"]:
        vs = []
        for text in rec["variants"]:
            v = hgvsindex.make_variant(text)
            assert v is not None and str(v) == text
            v.spike_seq = anon[text] if v.anonymous() else None
            vs.append(v)
        want = cases.golden_allele(rec)
        a = spikein.Allele(cases.GENOME[rec["ch"]], tuple(rec["zone"]), vs)
        assert [a.s0, a.e0] == rec["sourceRange"], (rec["ch"], rec["zone"])
        assert a.G == len(want) and a.flat() == want, (rec["ch"], rec["zone"])
        lo, hi = a.window(480)
        assert a.cut(lo, hi) == want[lo:hi] and a.cut(7, 7) == "" and a.cut(a.G - 3, a.G + 9) == want[-3:]
        # ... and the restatement's
        rv = [R.parse_variant(t) for t in rec["variants"]]
        for v in rv:
            v.seq = anon.get(v.text)
        assert list(R.allele(cases.GENOME[rec["ch"]], rec["zone"], rv)) == [want] + rec["sourceRange"]


def _alleles_of(g):
    by = {}
    for rec in g["alleles"]:
        by.setdefault((rec["ch"], rec["zone"][0], rec["zone"][1]), []).append(cases.golden_allele(rec))
    return lambda h: by[(h["ch"], h["st"], h["en"])]


def _texts(pairs):
    return "".join("\n".join(a) + "\n" for a, _ in pairs), "".join("\n".join(b) + "\n" for _, b in pairs)


def _L(g):
    return int(dict(zip(g["opts"][0::2], g["opts"][1::2])).get("-L", 100))


@pytest.mark.parametrize("name", [c["name"] for c in cases.make_cases()])
def test_checker_reads_the_references_records(golden, name):
    g = golden[name]
    L, al = _L(g), _alleles_of(g)
    t1, t2 = _texts(g["pairs"])
    which, rejects = chk.check_pairs(t1, t2, al, L, upper_first=False)
    assert len(which) == len(g["pairs"]) == 25 and rejects == []
    n_err = 0
    for a, b in g["pairs"]:
        for mate, rec in ((0, a), (1, b)):
            h = chk.parse_header(rec[0])
            zone = al(h)
            came_from = set(chk.fits(tuple(rec), mate, zone, L, upper_first=False))
            # (beside a one-base deletion a record moved by one fits the other allele: what counts is the allele it came from)
            ok = lambda r: bool(came_from & set(chk.fits(tuple(r), mate, zone, L, upper_first=False)))
            assert ok(rec)
            head, read = rec[0], rec[1]
            words = head.split(" ")
            # one base changed
            other = "A" if read[L // 2] != "A" else "C"
            assert not ok([head, read[:L // 2] + other + read[L // 2 + 1:], rec[2], rec[3]])
            # u and the strand changed (a read from inside the run of N says nothing about either)
            for k, w in ((2, str(h["u"] + 1)), (4, "+" if h["s"] == "-" else "-")) if len(set(read)) > 1 else ():
                assert not ok([" ".join(words[:k] + [w] + words[k + 1:]), read, rec[2], rec[3]]), (k, head)
            # one error entry changed: dropped, and pointed at the base beside it
            if h["errors"]:
                n_err += 1
                p, c, d = h["errors"][0]
                rest = ["%d%s>%s" % e for e in h["errors"][1:]]
                assert not ok([" ".join(words[:5] + [";".join(rest)]), read, rec[2], rec[3]])
                q = p + 1 if p + 1 < L else p - 1
                if q not in [e[0] for e in h["errors"]] and read[q] != d:
                    assert not ok([" ".join(words[:5] + [";".join(["%d%s>%s" % (q, c, d)] + rest)]), read, rec[2], rec[3]])
        # fl changed, in both headers: one mate of a pair does not depend on it (mate 1 on '+', mate 2 on '-'), the other does
        fl = chk.parse_header(a[0])["fl"]
        longer = [[" ".join(r[0].split(" ")[:3] + [str(fl + 1)] + r[0].split(" ")[4:])] + list(r[1:]) for r in (a, b)]
        x1, x2 = _texts([longer])
        if len(set(a[1])) > 1 and len(set(b[1])) > 1:
            assert chk.check_pairs(x1, x2, al, L, upper_first=False)[1] == [0], a[0]
    assert 4 * n_err > 2 * len(g["pairs"])      # the entries were exercised: at -e 0.02 more than a quarter of the records list one


@pytest.mark.parametrize("name", [c["name"] for c in cases.make_cases()])
def test_restatement_passes_the_checker(restated, name):
    case = [c for c in cases.make_cases() if c["name"] == name][0]
    kw = cases.case_numbers(case)
    t1, t2, info = restated[name]
    assert sum(info["counts"]) == kw["N"] and len(info["counts"]) == len(info["zones"])
    by = {(ch, z[0], z[1]): [wt[0], mut[0]] for ch, z, wt, mut in info["zones"]}
    which, rejects = chk.check_pairs(t1, t2, lambda h: by[(h["ch"], h["st"], h["en"])], kw.get("L", 100))
    assert rejects == [] and len(which) == kw["N"]
    assert all(w in s for w, s in zip(info["which"], which))
    heads = [chk.parse_header(h) for h in t1.split("\n")[0::4] if h]
    if case["bed"] == cases.BED:
        assert any(h["nm"] == "None" for h in heads), "the unnamed zone got no pair"
    # both clamps occur where the BED has the zones for them
    if case["bed"] == cases.BED and kw.get("I", 300) == 300:
        assert any(h["nm"] == "start" and h["u"] == h["fl"] for h in heads)
        assert any(h["nm"] == "end" and h["u"] + h["fl"] == len(by[(h["ch"], h["st"], h["en"])][0]) for h in heads)


def test_library_plan_is_the_restatements(restated, tmp_path):
    """the library's zones, alleles, windows and draws on the host against the restatement's, case by case"""
    cases.write_genome(str(tmp_path))
    for case in cases.make_cases():
        kw = cases.case_numbers(case)
        words = cases.write_case(case, str(tmp_path))
        o = dict(zip(words[0::2], words[1::2]))
        plan = spikein.make_plan(dict(bed=o["-b"], home=str(tmp_path), names=None, file=o.get("-f"), pop=o.get("-m"), seed=kw["seed"],
                                      L=kw.get("L", 100), I=kw.get("I", 300), D=kw.get("D", 0.1)), case["variants"])
        info = restated[case["name"]][2]
        assert len(plan.zones) == len(info["zones"])
        for (ch, zone, wt, mut), (rch, rzone, rwt, rmut) in zip(plan.zones, info["zones"]):
            assert (ch, zone) == (rch, rzone)
            for a, r in ((wt, rwt), (mut, rmut)):
                assert (a.flat(), a.s0, a.e0) == r
        assert [int(x) for x in plan.cum] == [sum(z[1][1] - z[1][0] + 1 for z in info["zones"][:i + 1]) for i in range(len(info["zones"]))]
        text, rows, first, heads, offs = plan.tables(info["counts"])
        assert int(first[-1]) == kw["N"] and len(rows) == 12 * len(plan.zones) and int(offs[-1]) == len(heads)


STAT = dict(seed=7, N=4000, L=100, I=300, D=0.1, E=0.005, V=0.5)


def test_statistics_of_the_draws():
    s = STAT
    N, L, I, D = s["N"], s["L"], s["I"], s["D"]
    zone = [("chrA:3000-3600 mid2 ", N, [(cases.GENOME["chrA"], 3000, 3600)] * 2)]
    t1, t2, which = R.records(s["seed"], L, I, R.sd_q(I, D), R.frac32(s["V"]), R.frac32(s["E"]), zone)
    h1 = [chk.parse_header(h) for h in t1.split("\n")[0::4] if h]
    h2 = [chk.parse_header(h) for h in t2.split("\n")[0::4] if h]
    assert len(h1) == len(h2) == N

    def within(k, n, p):
        assert abs(k - n * p) <= 5 * math.sqrt(n * p * (1 - p)), (k, n, p)
    within(sum(which), N, s["V"])
    within(sum(h["s"] == "-" for h in h1), N, 0.5)
    within(sum(len(h["errors"]) for h in h1 + h2), 2 * N * L, s["E"])
    fl = [h["fl"] for h in h1]
    mean = sum(fl) / N
    sd = math.sqrt(sum((x - mean) ** 2 for x in fl) / (N - 1))
    assert abs(mean - I) <= 5 * I * D / math.sqrt(N), mean
    assert abs(sd / (I * D) - 1) <= 5 / math.sqrt(2 * N), sd
    assert all(3000 <= h["u"] <= 3600 for h in h1)


def test_edges_of_the_rates():
    zone = [("z:1-2 n ", 40, [("ACGT" * 300, 400, 500), ("TTGA" * 300, 400, 500)])]
    L, I, q = 50, 200, R.sd_q(200, 0.1)
    for V, want in ((0.0, 0), (1.0, 1)):
        t1, t2, which = R.records(3, L, I, q, R.frac32(V), R.frac32(0.01), zone)
        assert set(which) == {want}
        al = [zone[0][2][0][0], zone[0][2][1][0]]
        got, rejects = chk.check_pairs(t1, t2, lambda h: al, L)
        assert rejects == [] and all(g == {want} for g in got)
    t1, t2, _ = R.records(3, L, I, q, R.frac32(0.5), R.frac32(0.0), zone)
    for t in (t1, t2):
        heads = t.split("\n")[0::4][:-1]
        assert len(heads) == 40 and all(h.endswith(" ") and chk.parse_header(h)["errors"] == [] for h in heads)
    t1, t2, _ = R.records(3, L, I, q, R.frac32(0.5), R.frac32(1.0), zone)
    for t in (t1, t2):
        for h in t.split("\n")[0::4][:-1]:
            e = chk.parse_header(h)["errors"]
            assert [x[0] for x in e] == list(range(L))


# ---- the command ------------------------------------------------------------------------------------------------------------
def _refused(capsys, argv):
    with pytest.raises(SystemExit) as e:
        cli.main_inner(["spikein"] + argv)
    assert e.value.code == 1
    return capsys.readouterr().err


def test_refusals(tmp_path, capsys, monkeypatch):
    d = str(tmp_path)
    cases.write_genome(d)
    bed = os.path.join(d, "z.bed")
    with open(bed, "w") as f:
        f.write(cases.BED)
    base = ["-g", d, "-b", bed, "-S", "1", "-N", "10", os.path.join(d, "out")]
    sub, dele = cases._sub("chrA", 1100), "chrA:g.1095_1105del"
    assert "unable to parse variant: chrA:g.12_11bogus" in _refused(capsys, base + ["chrA:g.12_11bogus"])
    assert "variants overlap: %s <> %s" % (dele, sub) in _refused(capsys, base + [sub, dele])
    assert "insALU" in _refused(capsys, base + ["chrA:g.1200_1201insALU"])
    assert "no sequence file for chrZ" in _refused(capsys, base + ["chrZ:g.12A>C"])
    tiny = os.path.join(d, "tiny")
    os.makedirs(tiny)
    with open(os.path.join(tiny, "chrA.fa"), "w") as f:
        f.write(">chrA\n" + cases.GENOME["chrA"][:900] + "\n")
    err = _refused(capsys, ["-g", tiny, "-S", "1", "-N", "10", os.path.join(d, "out")])
    assert "zone chrA:1-900" in err and "fewer than twice the longest fragment (479)" in err
    err = _refused(capsys, base + ["chrA:g.990_1410del"])
    assert "zone chrA:1000-1400" in err and "leave nothing" in err
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert "single GPU" in _refused(capsys, base)
    assert not os.path.exists(os.path.join(d, "out_1.fastq"))


def test_help_and_listing(capsys):
    assert "spikein" in cli.available()
    assert cli.main_inner(["help", "spikein"]) == 0
    text = capsys.readouterr().out
    for word in ("zot spikein [options] <output-prefix> [<variant>...]", "-B MB", "-n NAMES", "Differences from the reference", "insALU",
                 "name order", "upper-cased before", "FASTQ only"):
        assert word in text, word


# ---- round trip -------------------------------------------------------------------------------------------------------------
ROUND_ZONE, ROUND_N, ROUND_VARIANTS = cases.ROUND_ZONE, cases.ROUND_N, cases.ROUND_VARIANTS


@pytest.mark.parametrize("kind", ["sub", "del"])
@pytest.mark.parametrize("V,call", [(0.5, "wt/mut"), (1.0, "mut")])
def test_round_trip_through_hgvs_find(kind, V, call):
    """about 200-fold coverage of the variant: 600 pairs, a quarter of whose first mates and an eighth of whose second mates
    cover it"""
    text = ROUND_VARIANTS[kind]
    v = hgvsindex.make_variant(text)
    index = [hgvsindex.indexed_variant(v, 75, cases.GENOME["chrA"])]
    t1, t2, _ = R.command(cases.GENOME, ROUND_ZONE, [text], seed=11, N=ROUND_N, V=V)
    out = HF.find(index, [t1, t2]).split("\n")
    row = dict(zip(out[0].split("\t"), out[1].split("\t")))
    assert row["res"] == call and row["hgvs"] == str(v), out
