"""`zot vars` without a GPU: the host formulas (zotmer_amd/library/varscan.py) against the restatement as text, the restatement
against the reference's fixture (tests/golden/v1_vars.json), the predicate that the device applies against the exact values,
and the command's refusals."""
import contextlib
import io
import json
import math
import os
import random

import numpy as np
import pytest

from tests import _vars_restatement as R
from tests._vars_cases import make_cases, missing_case
from tests._vars_compare import same_line, same_lines, same_number
from zotmer_amd.library import varscan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = {c["name"]: c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "v1_vars.json")))}
CASES = make_cases()
IDS = [c["name"] for c in CASES]


def test_the_fixture_covers_the_cases():
    assert sorted(GOLD) == sorted(IDS) and {c["K"] for c in CASES} == {1, 2, 7, 25, 31, 32}
    for c in CASES:
        assert GOLD[c["name"]]["K"] == c["K"] and GOLD[c["name"]]["inputs"] == [nm for nm, _ in c["samples"]]
        assert len(c["samples"]) >= 2 and sum(len(v) for v in GOLD[c["name"]]["stdout"].values()) >= 5
        assert 0 < GOLD[c["name"]]["noise"] < 1e-6
        assert any(len(g) == 4 for _, g in R.groups(c["ref"]))
    letters = [l.split("\t")[1] for c in GOLD.values() for ls in c["stdout"].values() for l in ls]
    assert any(x not in "ACGT" for x in letters)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_against_the_fixture(case):
    g = GOLD[case["name"]]
    for nm, pairs in case["samples"]:
        assert same_lines(R.stdout_lines(case["K"], case["ref"], pairs), g["stdout"][nm], g["noise"]), nm
    assert R.noise(case["K"], case["ref"], case["samples"]) < 100 * g["noise"]


def test_the_comparison_rule():
    assert same_number("-11", "-11", 1e-8) and same_number("4.3e-10", "-2e-09", 1e-8) and same_number("-11", "-12", 1e-8)
    assert same_number("-5.5e+02", "-5.6e+02", 1e-8) and same_number("  0", "1e-09", 1e-8)
    assert not same_number("-11", "-13", 1e-8) and not same_number("  0", "-1e-05", 1e-8) and not same_number("-5.5e+02", "-5.7e+02", 1e-8)
    assert not same_line("AC\tA\t-11\t0\t0\t0", "AC\tC\t-11\t0\t0\t0", 1e-8) and not same_line("AC\tA\t-11\t0\t0\t0", "AG\tA\t-11\t0\t0\t0", 1e-8)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_formulas_reproduce_the_restatement_as_text(case):
    K = case["K"]
    by_ctx = dict(R.groups(case["ref"]))
    for nm, pairs in case["samples"]:
        got = []
        for ctx, grp in R.groups(pairs):
            _, _, sx, gx = R.group_values(by_ctx[ctx], grp)
            b, vs = varscan.eval_row(sx, gx)
            if b > 0:
                got.append(varscan.format_row(K - 1, ctx, b, vs))
        assert got == R.stdout_lines(K, case["ref"], pairs), nm
        # ... and through the rows as the device hands them back (numpy words)
        vals = []
        R.stdout_lines(K, case["ref"], pairs, values=vals)
        ctxs = np.array([v[0] for v in vals], dtype=np.uint64)
        rows = np.array([v[3] + v[4] for v in vals], dtype=np.uint64).reshape(-1, 8)
        assert varscan.lines_of_rows(K, ctxs, rows) == got


def test_host_functions_are_the_restatements():
    rng = random.Random(5)
    for _ in range(300):
        n = rng.choice([1, 2, 24, 25, 26, 100, 377])
        k = rng.randint(0, n)
        p = rng.choice([rng.random(), 1e-9, 1 - 1e-9, 0.5])
        assert varscan.log_bin_ge(p, n, k) == R.log_bin_ge(p, n, k)
        assert varscan.first_term(p, n, k) == R.log_bin_eq(p, n, k)
    assert [varscan.render(J, x) for J, x in ((0, 0), (1, 2), (3, 0b000111), (31, (1 << 62) - 1))] == \
        [R.render(J, x) for J, x in ((0, 0), (1, 2), (3, 0b000111), (31, (1 << 62) - 1))]
    assert list(varscan.FASTA) == R._FAS


def test_the_predicate_misses_no_flagged_lane():
    """v >= F and, for k <= n p, v >= log(1/2) - noise: every lane the reference flags passes the O(1) predicate without any
    guard; with the guard it passes a fortiori"""
    rng = random.Random(11)
    flagged = passed = 0
    for _ in range(4000):
        gx = [rng.choice([0, rng.randint(1, 300)]) for _ in range(4)]
        sx = [rng.choice([0, rng.randint(1, 120)]) for _ in range(4)]
        if sum(gx) == 0 or sum(sx) == 0:
            continue
        b, vs = varscan.eval_row(sx, gx)
        st, gt = sum(sx), sum(gx)
        for j in range(4):
            c0 = varscan.candidate(sx[j], st, gx[j], gt, guards=0.0)
            assert varscan.candidate(sx[j], st, gx[j], gt, guards=1.0) >= c0
            passed += c0
            if (b >> j) & 1:
                flagged += 1
                assert c0 and sx[j] * gt > st * gx[j]
                assert vs[j] >= varscan.first_term(float(gx[j]) / float(gt), st, sx[j])
    assert flagged > 500 and passed >= flagged


def test_the_guard_is_a_bound_in_the_terms_it_names():
    assert varscan.guard(100, 100, 0.5) == 100 * math.log(2) * 2.0 ** -47          # k == n: no factorial terms
    assert varscan.guard(10, 3, 0.5) == (10 * math.log(2) + 3 * 64.0) * 2.0 ** -47
    n, k, p = 1000, 300, 0.25
    want = (k * abs(math.log(p)) + (n - k) * abs(math.log1p(-p)) + sum(m * math.log(m) + m + 64.0 for m in (n, n - k, k))) * 2.0 ** -47
    assert varscan.guard(n, k, p) == want and want < 1e-9
    # perturbing every log of the first term by 4 ulp moves it by less than the guard
    for n, k, p in ((1000, 300, 0.25), (1 << 31, 1 << 30, 0.3), (50, 49, 1e-6), (10 ** 12, 10 ** 11, 0.999)):
        f = varscan.first_term(p, n, k)
        eps = 4 * 2.0 ** -52
        moved = sum(abs(t) * eps for t in (n * math.log(n), (n - k) * math.log(n - k), k * math.log(k), k * math.log(p), (n - k) * math.log1p(-p)))
        assert moved < varscan.guard(n, k, p) and math.isfinite(f)


# ---- the command, before it reaches the device ------------------------------------------------------------------------------

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


def write_set(path, K, pairs):
    from zotmer_amd.library import vectors
    from zotmer_amd.library.container import KmerSet
    with KmerSet(str(path), "w") as z:
        vectors.write_kmers_and_counts(z, np.array([x for x, _ in pairs], dtype=np.uint64), np.array([c for _, c in pairs], dtype=np.uint64))
        z.meta.update({"K": K, "kmers": "kmers", "counts": "counts"})
    return str(path)


@pytest.mark.parametrize("args", [["vars"], ["vars", "a.k"], ["vars", "a.k", "b.k"], ["vars", "-r"], ["vars", "-r", "ref.k"], ["vars", "-x", "a.k"],
                                  ["vars", "-r", "ref.k", "-q", "a.k"]])
def test_bad_arguments_end_before_the_device(args, monkeypatch):
    from zotmer_amd.library import engine
    monkeypatch.setattr(engine, "context", lambda: pytest.fail("the device was touched"))
    code, out, err = run(args)
    assert code == 1 and out == "" and "zot vars -r ref <input>..." in err


def test_good_arguments_parse():
    from zotmer_amd.commands import vars as cmd
    assert cmd.parse(["-r", "ref.k", "a.k"]) == ("ref.k", ["a.k"])
    assert cmd.parse(["a.k", "-rref.k", "b.k"]) == ("ref.k", ["a.k", "b.k"])


def test_several_processes_are_refused(monkeypatch):
    from zotmer_amd.library import engine
    monkeypatch.setattr(engine, "context", lambda: pytest.fail("the device was touched"))
    monkeypatch.setenv("WORLD_SIZE", "2")
    code, out, err = run(["vars", "-r", "ref.k", "a.k"])
    assert code not in (0, None) and "single GPU" in str(code) + err


def test_mismatched_k_is_refused_before_the_device(tmp_path, monkeypatch):
    from zotmer_amd.library import engine
    monkeypatch.setattr(engine, "context", lambda: pytest.fail("the device was touched"))
    m = missing_case()
    ref = write_set(tmp_path / "ref.k", m["K"], m["ref"])
    a = write_set(tmp_path / "a.k", m["K"], m["shared"])
    b = write_set(tmp_path / "b.k", m["K"] + 1, m["shared"])
    code, out, err = run(["vars", "-r", ref, a, b])                    # the inputs disagree (the reference: MismatchedK)
    assert code == 1 and out == "" and "mismatched K" in err
    code, out, err = run(["vars", "-r", b, a])                         # the reference set's K differs (the reference never looks)
    assert code == 1 and out == "" and "K=6" in err and "K=5" in err and "reference set" in err


def test_help_prints_the_deviations():
    code, out, _ = run(["help", "vars"])
    assert code == 0 and "zot vars -r ref <input>..." in out
    for word in ("are not in the reference (first:", "AssertionError", "AttributeError", "whose K differs", "rounding noise", "single GPU"):
        assert word in out, word
    code, out, _ = run(["help"])
    assert "\tvars\n" in out
