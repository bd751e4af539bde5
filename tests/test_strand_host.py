"""`zot strand` without a GPU: the restatement of the reference's semantics reproduces every fixture the reference
produced (tests/golden/s1_strand.json), and the command's help and argument errors work before any device is touched."""
import contextlib
import hashlib
import io
import json
import os

import pytest

from tests import _strand_restatement as R
from tests._strand_cases import make_cases

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "s1_strand.json")
INPUTS = {c["name"]: c for c in make_cases()}
CASES = [dict(c, inputs=INPUTS[c["name"]]["inputs"]) for c in json.load(open(GOLD))]


def digest(lines):
    return hashlib.sha256("".join(sorted(lines)).encode()).hexdigest()


@pytest.fixture(scope="module")
def restated():
    return {c["name"]: R.strand(c["k"], c["p"], c["inputs"]) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_reproduces_the_reference(restated, case):
    lines, ascending, st = restated[case["name"]]
    assert len(lines) == case["lines"] == st["pairs"]
    assert digest(lines) == case["sha256_sorted"]
    assert sorted(ascending) == sorted(lines)


def test_fixtures_cover_the_issue_cases(restated):
    names = {c["name"] for c in CASES}
    assert {"k25_p0.1", "k25_p1", "k31_p0.3", "k6_p1", "k4_p0.5", "lower_and_U", "short_reads", "mate2_fewer",
            "incomplete_record", "crlf", "two_pairs"} <= names
    rows = [tuple(int(v) for v in l.split("\t")) for lines, _, _ in restated.values() for l in lines]
    assert any(a and b for a, b in rows) and any(not (a and b) for a, b in rows)
    assert sum(st["palindromes"] for _, _, st in restated.values()) > 0
    assert sum(st["orphans"] for _, _, st in restated.values()) > 0
    assert restated["k6_p1"][2]["palindromes"] > 0 and restated["k4_p0.5"][2]["palindromes"] > 0


def test_palindrome_prints_its_count_twice_and_an_orphan_nothing():
    fq = lambda s: "@r\n%s\n+\n%s\n" % (s, "I" * len(s))
    lines, _, st = R.strand(4, 1.0, [fq("ACGT"), fq("TTTT")])          # ACGT = rc ACGT; mate 2: rc TTTT = AAAA, the smaller strand
    assert sorted(lines) == ["1\t0\n", "1\t1\n"] or sorted(lines) == ["0\t1\n", "1\t1\n"]
    assert st == dict(pairs=2, orphans=0, palindromes=1)
    lines, _, st = R.strand(4, 1.0, [fq("TTTT"), fq("ACGT")])          # TTTT forward is the greater strand: nothing for it
    assert lines == ["1\t1\n"] and st == dict(pairs=1, orphans=1, palindromes=1)
    lines, _, st = R.strand(4, 1.0, [fq("TTTT"), fq("ACGT")], orphans=True)
    assert len(lines) == 2 and st["pairs"] == 2 and sorted(sum(int(v) for v in l.split()) for l in lines) == [1, 2]


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


def test_help_strand(no_device):
    code, out, _ = _cli(["help", "strand"])
    assert code == 0
    assert "zot strand [options] <fastq>..." in out
    for word in ("ascending canonical k-mer order", "evident intent", "-r is refused", "single GPU", "palindrome"):
        assert word in out, word
    code, out, _ = _cli(["help"])
    assert "\tstrand" in out


def test_argument_errors_never_load_the_library(no_device, monkeypatch):
    code, _, err = _cli(["strand"])
    assert code == 1 and "wrong number of arguments" in err
    code, _, err = _cli(["strand", "-r", "ref.fa", "a.fq", "b.fq"])
    assert code == 1 and "-r is not supported" in err and "random" in err
    code, _, err = _cli(["strand", "-k", "32", "a.fq", "b.fq"])
    assert code == 1 and "-k 32 is not supported" in err and "2K + 1" in err
    for k in ("0", "33", "x"):
        code, _, err = _cli(["strand", "-k", k, "a.fq", "b.fq"])
        assert code == 1 and "-k" in err
    code, _, err = _cli(["strand", "a.fq", "b.fq", "c.fq"])
    assert code == 1 and "even number of inputs" in err
    code, _, err = _cli(["strand", "-p", "much", "a.fq", "b.fq"])
    assert code == 1 and "-p" in err
    code, _, err = _cli(["strand", "-m", "x", "a.fq", "b.fq"])
    assert code == 1 and "-m" in err
    code, _, err = _cli(["strand", "-q", "a.fq", "b.fq"])
    assert code == 1 and "unknown option" in err
    monkeypatch.setenv("WORLD_SIZE", "2")
    code, _, err = _cli(["strand", "a.fq", "b.fq"])
    assert code == "zot strand: runs on a single GPU for now"


def test_threshold_is_pythons_own_arithmetic():
    from zotmer_amd.library import strand
    for K, p in ((25, 0.1), (31, 0.3), (4, 0.5), (1, 0.1), (16, 1e-9)):
        assert strand.threshold(K, p) == R.threshold(K, p)[1]
    assert strand.threshold(31, 1.0) == (1 << 62) - 1 < R.threshold(31, 1.0)[1]        # float(M) rounds up: nothing is above it
    assert strand.threshold(25, 7.5) == (1 << 50) - 1
    assert strand.threshold(25, -0.1) is None
