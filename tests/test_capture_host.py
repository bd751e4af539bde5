"""`zot capture` without a GPU: the restatement of the reference's semantics reproduces every fixture the reference
produced (tests/golden/c1_capture.json), and the command's help and usage errors work before any device is touched."""
import contextlib
import hashlib
import io
import json
import os

import pytest

from tests import _capture_restatement as R
from tests._capture_cases import make_cases

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c1_capture.json")
INPUTS = {c["name"]: c for c in make_cases()}
CASES = [dict(c, baits=INPUTS[c["name"]]["baits"], inputs=INPUTS[c["name"]]["inputs"]) for c in json.load(open(GOLD))]


def matches(files, err, case):
    assert err == case["stderr"]
    assert sorted(files) == sorted(case["files"])
    for fn, want in case["files"].items():
        assert (hashlib.sha256(files[fn]).hexdigest(), len(files[fn])) == (want["sha256"], want["size"]), fn


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_reproduces_the_reference(case):
    files, err, warnings = R.capture(case["baits"], case["inputs"], case["k"], case.get("paired", False))
    matches(files, err, case)
    assert not warnings


def test_fixtures_cover_the_issue_cases():
    names = {c["name"] for c in CASES}
    assert {"k24", "k25", "k12", "k31", "crlf", "paired", "two_files"} <= names
    k24 = next(c for c in CASES if c["name"] == "k24")
    assert "<P>/nohit.fastq: 0\n" in k24["stderr"] and "nohit.fastq" not in k24["files"]
    assert "geneB desc.fastq" in k24["files"]
    # the -k 24 quirk: read 25-mers against bait 24-mers differ from -k 25 on the same inputs
    k25 = next(c for c in CASES if c["name"] == "k25")
    assert k24["stderr"] != k25["stderr"]


def test_read_k_is_25_whatever_k_says():
    bait = "ACGTTGCAAGGCTTACCGATAGCA"               # 24 bases
    read = "A" + bait                                # a 25-mer whose value equals the bait's 24-mer
    fq = "@r\n%s\n+\n%s\n" % (read, "I" * len(read))
    files, err, _ = R.capture(">b\n%s\n" % bait, [fq], 24)
    assert files == {"b.fastq": fq.encode()}
    files, err, _ = R.capture(">b\n%s\n" % bait, [fq], 25)
    assert files == {}


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
    from zotmer_amd.library import engine

    def refuse():
        raise AssertionError("a device context was requested")
    monkeypatch.setattr(engine, "context", refuse)


def test_help_capture(no_device):
    code, out, _ = _cli(["help", "capture"])
    assert code == 0
    assert "zot capture [options] <sequences> <input>..." in out
    assert "25-mers whatever -k says" in out
    code, out, _ = _cli(["help"])
    assert "\tcapture" in out


def test_usage_errors(no_device, tmp_path):
    code, _, err = _cli(["capture"])
    assert code == 1 and "wrong number of arguments" in err
    code, _, err = _cli(["capture", "baits.fa"])
    assert code == 1 and "wrong number of arguments" in err
    fa = tmp_path / "baits.fa"
    fa.write_text(">b\nACGT\n")
    for reads in ("reads.fa", "reads.fasta.gz", "x.fna"):
        code, _, err = _cli(["capture", str(fa), "r.fastq", reads])
        assert code == 1 and "FASTQ only" in err and reads in err
    code, _, err = _cli(["capture", "-k", "33", str(fa), "r.fastq"])
    assert code == 1 and "-k" in err
    code, _, err = _cli(["capture", "-m", "x", str(fa), "r.fastq"])
    assert code == 1 and "-m" in err
    code, _, err = _cli(["capture", "-q", str(fa), "r.fastq"])
    assert code == 1 and "unknown option" in err
