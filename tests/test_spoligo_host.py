"""`zot spoligo` without a GPU: the restatement of the reference's route (neighbour enumeration and range searches) reproduces
every fixture the reference produced (tests/golden/sp1_spoligo.json); the probe-file reader, the window cutter, the help and
the argument errors work before any device is touched."""
import contextlib
import io
import json
import os

import pytest

from tests import _spoligo_restatement as R
from tests._spoligo_cases import encode, make_cases, nearest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sp1_spoligo.json")
INPUTS = {c["name"]: c for c in make_cases()}
FIXTURE = json.load(open(GOLD))
CASES = [dict(INPUTS[c["name"]], **c) for c in FIXTURE if c["name"] in INPUTS]
BAD = [c for c in FIXTURE if c["name"] == "bad_file"][0]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_reproduces_the_reference(case):
    seqs = [p["seq"] for p in case["probes"]]
    assert len(case["present"]) == len(seqs)
    assert R.spoligo(case["K"], case["kmers"], seqs) == case["present"]
    # ... and means "every window has a k-mer within distance D", for every D the command accepts
    near = [nearest(s, case["K"], case["kmers"]) for s in seqs]
    for D in (0, 1, 2):
        assert R.spoligo(case["K"], case["kmers"], seqs, D) == "".join("1" if max(n) <= D else "0" for n in near), D


def test_fixtures_cover_the_issue_cases():
    assert {"k25", "k32", "k12", "k5"} <= {c["name"] for c in CASES}
    seen = set()
    for c in CASES:
        for p, b in zip(c["probes"], c["present"]):
            n, K = len(p["seq"]), c["K"]
            seen.add(("short" if n < K else "K" if n == K else "long", b))
            if c["name"] in ("k25", "k32") and p["design"] is not None:
                assert nearest(p["seq"], K, c["kmers"]) == p["design"], (c["name"], p["name"])
                seen.update(p["tags"])
                seen.update(["K32"] if n == K == 32 else [])
    assert {(k, b) for k in ("short", "K", "long") for b in "01"} <= seen
    assert {"d0", "d1", "d2", "d3", "first", "last", "both_bits", "below_window", "all_present", "one_absent", "K32"} <= seen


# ---- the probe file -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_probe_file_names_and_ordinals(tmp_path, case):
    from zotmer_amd.library import spoligo
    pf = tmp_path / "panel.txt"
    pf.write_text(case["probe_text"])
    err = io.StringIO()
    names, probes, bad = spoligo.read_probes(str(pf), err)
    assert not bad and err.getvalue() == ""
    assert names == [p["name"] for p in case["probes"]]
    assert [spoligo.encode(s) for s in probes] == [encode(p["seq"]) for p in case["probes"]]
    assert any(nm.isdigit() for nm in names) and any(not nm.isdigit() for nm in names) and "#" in case["probe_text"]
    assert not spoligo.bad_probes(names, probes)


def test_probe_file_ordinals_skip_comments_only(tmp_path):
    from zotmer_amd.library import spoligo
    pf = tmp_path / "p.txt"
    pf.write_text("#one\nACGT\n#two\n#three\nname TTTT\n  GGGG  \n")
    assert spoligo.read_probes(str(pf))[:2] == (["1", "name", "3"], ["ACGT", "TTTT", "GGGG"])


def test_badly_formatted_lines_are_all_reported_then_exit_1(tmp_path, no_device):
    from zotmer_amd.library import spoligo
    pf = tmp_path / "bad.probes"
    pf.write_text(BAD["probe_text"])
    want = BAD["stderr"].replace("{path}", str(pf))
    assert want.count("badly formatted.") == 2          # one before and one after good lines: the whole file is read
    err = io.StringIO()
    names, probes, bad = spoligo.read_probes(str(pf), err)
    assert bad and err.getvalue() == want
    assert probes == ["ACGTACGT", "ACGTTTGA", "ACGTAAAA"] and names == ["1", "n1", "5"]
    code, out, err = _cli(["spoligo", "-p", str(pf), "some.k25"])
    assert (code, out, err) == (BAD["exit"], "", want) and code == 1


# ---- windows --------------------------------------------------------------------------------------------------------------

def test_window_cutting():
    from zotmer_amd.library import spoligo
    s = "ACGTTGCAGGATCCAATTGGCCAAGTCTAGCATGCATTTACG"          # 42 bases
    assert spoligo.cut_windows(s[:16], 25) == [(16, encode(s[:16]))]                      # Kp < K
    assert spoligo.cut_windows(s[:25], 25) == [(25, encode(s[:25]))]                      # Kp = K
    assert spoligo.cut_windows(s[:30], 25) == [(25, encode(s[i:i + 25])) for i in range(6)]        # Kp > K
    w = spoligo.cut_windows(s, 32)                                                        # Kp > 32
    assert w == [(32, encode(s[i:i + 32])) for i in range(11)] and all(v < 1 << 64 for _, v in w)
    # the reference's own cut: the low 2K bits of the probe's value, moved down a base at a time
    x = R.kmer(s)
    assert sorted(v for _, v in w) == sorted((x >> (2 * i)) & ((1 << 64) - 1) for i in range(11))
    assert spoligo.cut_windows("acgu", 4) == [(4, encode("ACGT"))] and spoligo.cut_windows("A", 1) == [(1, 0)]
    p = spoligo.Panel(["a", "b"], [s[:30], s[:7]])
    windows, spans = p.plan(25)
    assert spans == [(0, 6), (6, 7)] and len(windows) == 7 and p.plan(25) is p.plan(25)
    assert p.plan(5)[1] == [(0, 26), (26, 29)]


def test_lines():
    from zotmer_amd.library import spoligo
    assert spoligo.lines("x.k25", ["1", "n"], [True, False], False) == ["x.k25\t10\n"]
    assert spoligo.lines("x.k25", ["1", "n"], [True, False], True) == ["x.k25\t1\t1\n", "x.k25\tn\t0\n"]


# ---- the command, as far as it goes without a device --------------------------------------------------------------------------

def _cli(args):
    from zotmer_amd import cli
    out, err = io.StringIO(), io.StringIO()
    code = 0
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            code = cli.main_inner(args) or 0
        except SystemExit as e:
            code = e.code
    return code, out.getvalue(), err.getvalue()


@pytest.fixture
def no_device(monkeypatch):
    from zotmer_amd import native
    from zotmer_amd.library import engine

    def refuse(*a, **k):
        raise AssertionError("the device library was requested")
    monkeypatch.setattr(engine, "context", refuse)
    monkeypatch.setattr(native, "load", refuse)


def test_help_spoligo(no_device):
    code, out, _ = _cli(["help", "spoligo"])
    assert code == 0
    assert "zot spoligo [-l] [-d D] -p PROBES <input>..." in out
    for word in ("-p is required", "not shipped", "-d is new", "AaCcGgTtUu", "TypeError", "no k-mers prints all zeros", "single GPU"):
        assert word in " ".join(out.split()), word
    code, out, _ = _cli(["help"])
    assert "\tspoligo" in out


def test_argument_errors_never_load_the_library(no_device, monkeypatch, tmp_path):
    good = tmp_path / "good.txt"
    good.write_text("ACGTACGT\n")
    code, _, err = _cli(["spoligo"])
    assert code == 1 and "wrong number of arguments" in err
    code, _, err = _cli(["spoligo", "a.k25"])
    assert code == 1 and "-p PROBES is required" in err and "one `[name] probe` per line" in err
    for d in ("3", "-1", "x", "1.5"):
        code, _, err = _cli(["spoligo", "-d", d, "-p", str(good), "a.k25"])
        assert code == 1 and "-d must be 0, 1 or 2" in err, d
    code, _, err = _cli(["spoligo", "-q", "-p", str(good), "a.k25"])
    assert code == 1 and "unknown option" in err
    bad = tmp_path / "n.txt"
    bad.write_text("ACGTACGT\nwithN ACGTNCGT\nACGT-\n")
    code, out, err = _cli(["spoligo", "-p", str(bad), "a.k25"])
    assert code == 1 and out == ""
    assert "probe withN (ACGTNCGT)" in err and "probe 3 (ACGT-)" in err and "probe 1 " not in err
    monkeypatch.setenv("WORLD_SIZE", "2")
    code, _, err = _cli(["spoligo", "-p", str(good), "a.k25"])
    assert code == "zot spoligo: runs on a single GPU for now"
