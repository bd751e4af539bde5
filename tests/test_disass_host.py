"""`zot disass` without a GPU: the restatement against the reference's fixture (tests/golden/d1_disass.json), summarize_bins
against the restatement's summarize, the YAML emitter against PyYAML's loader, the batch packing, and the command's refusals."""
import contextlib
import io
import json
import os
import random

import pytest

from tests import _disass_restatement as R
from tests._disass_cases import make_cases
from zotmer_amd.library import disass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "d1_disass.json")))
CASES = make_cases()
IDS = [c["name"] for c in CASES]


def same(a, b):
    """equal, the int or float type of every number included"""
    return json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)


def bins_of(d):
    h = {}
    for c in d.values():
        h[c] = h.get(c, 0) + 1
    return sorted(h.items())


def test_the_fixture_covers_the_cases():
    assert sorted(GOLD) == sorted(IDS)
    assert {"defaults", "k4", "k6", "k5_single", "sampled", "sampled_single", "c2_q4", "edges", "two_files", "gzip"} <= set(IDS)
    meds = [c["median"] for name in GOLD for f in GOLD[name] for c in f["contigs"]]
    assert any(isinstance(m, int) for m in meds) and any(isinstance(m, float) for m in meds)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_reproduces_the_fixture(case):
    o = case["opts"]
    assert same(R.disass(case["files"], o["K"], o["C"], o["P"], o["Q"], o["S"], o["both"]), GOLD[case["name"]])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_summarize_bins_on_the_fixture_dicts(case):
    o = case["opts"]
    for (_, text), fres in zip(case["files"], GOLD[case["name"]]):
        contigs, glob = R.contig_dicts(text, o["K"], o["both"], o["S"], o["P"])
        for (nm, d), want in zip(contigs, fres["contigs"]):
            assert same(dict(disass.summarize_bins(bins_of(d), o["C"], o["Q"]), name=nm), want)
        assert same(disass.summarize_bins(bins_of(glob), o["C"], o["Q"]), fres["global"])


SIZES = [0, 1, 2, 3, 4, 5, 10, 11, 64, 99, 100, 255, 300, 301]


@pytest.mark.parametrize("n", SIZES)
def test_summarize_bins_on_random_dicts(n):
    rng = random.Random(1000 + n)
    for trial in range(12):
        top = [3, 40, 1 << 33][trial % 3]
        d = {i: rng.randrange(1, top + 1) if rng.random() < 0.8 else 1 for i in range(n)}
        for Q in ([1, 2, 3, 7, 10, 20] if trial % 2 else range(1, 21)):
            cut = rng.choice([0, 1, 2, 5, top // 2, top + 1])
            want = R.summarize(d, cut, Q, single_ok=True)
            got = disass.summarize_bins(bins_of(d), cut, Q)
            assert same(got, want), (n, trial, Q, cut)


def test_one_distinct_kmer_is_the_deviation():
    with pytest.raises(IndexError):
        R.summarize({7: 4}, 5, 10)
    got = disass.summarize_bins([(4, 1)], 5, 10)
    assert got["median"] == 4.0 and isinstance(got["median"], float)
    assert same(got, R.summarize({7: 4}, 5, 10, single_ok=True))
    assert set(got["quantiles"]) == {4} and got["histogram"] == [[4, 1]] and got["low-count"] == 1 and got["mean"] == 4.0


def test_odd_median_is_the_reference_quirk():
    # five values 1 2 3 4 5: the reference takes (cs[2] + cs[3]) / 2 = 3.5, not 3
    assert disass.summarize_bins([(1, 1), (2, 1), (3, 1), (4, 1), (5, 1)], 5, 10)["median"] == 3.5
    assert disass.summarize_bins([(1, 2), (9, 1)], 5, 10)["median"] == 5.0          # 1 1 9 -> (1 + 9) / 2
    m = disass.summarize_bins([(1, 2), (9, 2)], 5, 10)["median"]                     # 1 1 9 9 -> cs[2]
    assert m == 9 and isinstance(m, int)


def test_quantiles_walk_ascending_counts():
    """the deviation: whatever order a dict of the reference's time would have had, the bins are walked in ascending count"""
    d = {i: c for i, c in enumerate([1] * 5 + [9] * 3 + [1 << 20] * 2)}
    got = disass.summarize_bins(bins_of(d), 5, 5)
    assert got["quantiles"] == sorted(got["quantiles"]) == [1, 1, 9, 1 << 20]
    assert same(got, R.summarize(d, 5, 5))


def test_mean_comes_from_exact_sums():
    big = (1 << 33) + 1
    got = disass.summarize_bins([(1, 3), (big, 1 << 21)], 5, 10)
    assert got["mean"] == float(3 + big * (1 << 21)) / float(3 + (1 << 21))


# ---- YAML -------------------------------------------------------------------------------------------------------------------

NAMES = ["plain", "two words", "with: colon", "trailing:", "#hash", "a #comment", "'single'", '"double"', "-dash", "- item", "é non-ascii ü",
         "back\\slash", "tab\there", "1", "1.5", "yes", "No", "null", "~", "", " lead", "trail ", "a,b", "[x]", "{y}", "&anchor", "*alias", "!tag",
         "|", ">", "%dir", "@at", "`tick", "contig_1 length=300 cov=12.5", "NODE_1_length_5_cov_2.0", "x\x85y", "\x7f", "日本", "?q", "a: b: c",
         "=", "/path/to/file.fa", "C:\\dir\\f.fa", "line\nbreak"]


def structure():
    contig = lambda nm, med: {"histogram": [[1, 20], [2, 3], [1 << 33, 1]], "mean": 1.25, "median": med, "low-count": 23, "high-count": 1,
                              "quantiles": [1] * 9 + [2], "name": nm}
    empty = {"histogram": [], "mean": 0.0, "median": 0, "low-count": 0, "high-count": 0, "quantiles": [], "name": "none"}
    files = [{"file": nm, "contigs": [contig(nm, 1), contig(nm + nm, 1.0), empty], "global": dict(contig(nm, 2.5), mean=1e22)} for nm in NAMES]
    for f in files:
        del f["global"]["name"]
    files.append({"file": "no contigs", "contigs": [], "global": {k: v for k, v in empty.items() if k != "name"}})
    return files


def test_dump_yaml_loads_back():
    yaml = pytest.importorskip("yaml")
    res = structure()
    text = disass.dump_yaml(res)
    assert same(yaml.safe_load(text), res)
    assert same(yaml.safe_load(disass.dump_yaml([])), [])
    for name in GOLD:
        assert same(yaml.safe_load(disass.dump_yaml(GOLD[name])), GOLD[name])


def test_dump_yaml_layout():
    res = [{"file": "a.fa", "contigs": [{"name": "c 1", "histogram": [[1, 2], [3, 4]], "mean": 2.0, "median": 3, "low-count": 2, "high-count": 0,
                                         "quantiles": [1, 3]}],
            "global": {"histogram": [], "mean": 0.0, "median": 0, "low-count": 0, "high-count": 0, "quantiles": []}}]
    assert disass.dump_yaml(res) == ("- contigs:\n"
                                     "  - high-count: 0\n"
                                     "    histogram:\n"
                                     "    - [1, 2]\n"
                                     "    - [3, 4]\n"
                                     "    low-count: 2\n"
                                     "    mean: 2.0\n"
                                     "    median: 3\n"
                                     "    name: c 1\n"
                                     "    quantiles: [1, 3]\n"
                                     "  file: a.fa\n"
                                     "  global:\n"
                                     "    high-count: 0\n"
                                     "    histogram: []\n"
                                     "    low-count: 0\n"
                                     "    mean: 0.0\n"
                                     "    median: 0\n"
                                     "    quantiles: []\n")


def test_dump_yaml_is_what_pyyaml_writes_when_lines_are_short():
    yaml = pytest.importorskip("yaml")
    res = [{"file": "a.fa", "contigs": [{"name": "c1", "histogram": [[1, 2], [3, 4]], "mean": 2.0, "median": 3.5, "low-count": 2,
                                         "high-count": 0, "quantiles": [1, 3]}],
            "global": {"histogram": [], "mean": 1e+16, "median": 0, "low-count": 0, "high-count": 0, "quantiles": []}}]
    # default_flow_style=None was PyYAML's default until 5.1: leaf collections in flow style
    assert disass.dump_yaml(res) == yaml.safe_dump(res, default_flow_style=None)


# ---- batches ----------------------------------------------------------------------------------------------------------------

def test_pack_batches():
    recs = [("r%d" % i, b"A" * n) for i, n in enumerate([30, 30, 10, 200, 30, 5, 5, 40])]
    K = 11
    got = list(disass.pack_batches(recs, K, budget=45, limit=1000))
    assert [nm for b in got for nm, _ in b] == [nm for nm, _ in recs]              # whole records, in order
    assert [[nm for nm, _ in b] for b in got] == [["r0", "r1", "r2"], ["r3"], ["r4", "r5", "r6"], ["r7"]]
    for b in got:
        w = sum(disass.windows_of(len(s), K) for _, s in b)
        assert w <= 45 or len(b) == 1                                                # a record over the budget is alone
    assert list(disass.pack_batches([], K, 45, 1000)) == []
    with pytest.raises(disass.TooLarge) as e:
        list(disass.pack_batches(recs, K, budget=45, limit=100))
    assert "r3" in str(e.value) and "190" in str(e.value) and "100" in str(e.value)


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


@pytest.mark.parametrize("args", [["disass"], ["disass", "-q", "0", "a.fa"], ["disass", "-q", "-3", "a.fa"], ["disass", "-q", "x", "a.fa"],
                                  ["disass", "-k", "0", "a.fa"], ["disass", "-k", "33", "a.fa"], ["disass", "-k", "x", "a.fa"],
                                  ["disass", "-p", "nan", "a.fa"], ["disass", "-p", "inf", "a.fa"], ["disass", "-p", "-inf", "a.fa"],
                                  ["disass", "-p", "half", "a.fa"], ["disass", "-c", "x", "a.fa"], ["disass", "-S", "x", "a.fa"],
                                  ["disass", "-S", "-1", "a.fa"], ["disass", "-Z", "a.fa"], ["disass", "-k"]])
def test_bad_arguments_end_before_the_device(args, monkeypatch):
    from zotmer_amd.library import engine
    monkeypatch.setattr(engine, "context", lambda: pytest.fail("the device was touched"))
    code, out, err = run(args)
    assert code == 1 and out == "" and "zot disass" in err


def test_good_arguments_parse():
    from zotmer_amd.commands import disass as cmd
    assert cmd.parse(["a.fa"]) == dict(K=25, C=5, Q=10, S=17, P=1.0, both=True, inputs=["a.fa"])
    assert cmd.parse(["-k", "7", "-c2", "-q", "4", "-S", "5", "-p", "0.3", "-s", "-v", "a.fa", "b.fa.gz"]) == \
        dict(K=7, C=2, Q=4, S=5, P=0.3, both=False, inputs=["a.fa", "b.fa.gz"])


def test_several_processes_are_refused(monkeypatch):
    from zotmer_amd.library import engine
    monkeypatch.setattr(engine, "context", lambda: pytest.fail("the device was touched"))
    monkeypatch.setenv("WORLD_SIZE", "2")
    code, out, err = run(["disass", "a.fa"])
    assert code not in (0, None) and "single GPU" in str(code) + err


def test_help_prints_the_deviations():
    code, out, _ = run(["help", "disass"])
    assert code == 0 and "zot disass [options] <input>..." in out
    for word in ("ascending count", "IndexError", "-q below 1", "1 .. 32", "finite", "80 columns", "single GPU", "cs[m+1]"):
        assert word in out, word
    code, out, _ = run(["help"])
    assert "\tdisass\n" in out
