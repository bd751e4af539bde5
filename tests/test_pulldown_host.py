"""`zot pulldown` without a GPU: the restatement of the reference's semantics reproduces every fixture the reference produced
(tests/golden/p1_pulldown.json), the member-name rule, the archive writer on fabricated spans, and the command's help and
refusals, which happen before the native library is loaded."""
import contextlib
import io
import json
import os
import zipfile

import numpy as np
import pytest

from tests import _pulldown_restatement as R
from tests._pulldown_cases import make_cases

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "p1_pulldown.json")
INPUTS = {c["name"]: c for c in make_cases()}
CASES = [dict(INPUTS[g["name"]], gold=g) for g in json.load(open(GOLD))]
IDS = [c["name"] for c in CASES]


def gold_members(g):
    return [(nm, g["digests"][i]["sha256"], g["digests"][i]["size"]) for nm, i in g["members"]]


def fns(case):
    return ["in%d.fastq" % i for i in range(len(case["inputs"]))]


def test_fixtures_cover_the_issue_cases():
    assert {"paired", "paired_U", "edges", "edges_U", "many", "unequal_5_3", "unequal_3_5", "crlf", "emptybaits_U", "emptyreads",
            "second", "two_pairs"} == set(IDS) == set(INPUTS)
    g = {c["name"]: c["gold"] for c in CASES}
    assert g["many"]["stdout"] == "0\t1\n1500\t1\n" and len(g["many"]["members"]) == 3000
    assert g["paired"]["stdout"] != g["paired_U"]["stdout"]
    assert g["unequal_5_3"]["stdout"] == g["unequal_3_5"]["stdout"] == "2\t3\n"
    assert g["emptybaits_U"]["stdout"] == "0\t18\n" and g["emptybaits_U"]["members"] == []
    assert g["emptyreads"]["stdout"] == "" and g["emptyreads"]["members"] == []
    assert g["crlf"]["stdout"] == g["edges_U"]["stdout"]
    assert "e1/with/words/in0.fastq" in [m[0] for m in g["edges"]["members"]]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_reproduces_the_reference(case):
    hist, members, vetoed = R.pulldown(case["baits"], case["up"], case["inputs"], fns(case))
    assert R.rows(hist) == case["gold"]["stdout"]
    n_pairs = sum(min(len(R.fastq_records(a)), len(R.fastq_records(b))) for a, b in zip(case["inputs"][0::2], case["inputs"][1::2]))
    assert sum(hist.values()) + vetoed == n_pairs
    if case["name"] == "two_pairs":             # the reference's archive keeps the last file pair only
        members = [m for m in members if m[0].endswith(("in2.fastq", "in3.fastq"))]
    assert R.digest(members) == gold_members(case["gold"])


def test_the_veto_cases_vanish():
    by = {c["name"]: c for c in CASES}
    names, idx, anti = R.tables(by["edges_U"]["baits"], by["edges_U"]["up"])
    hits, r1, _ = R.walk(idx, anti, *by["edges_U"]["inputs"])
    gone = [r1[i][0] for i, h in enumerate(hits) if h is None]
    assert gone == ["@veto_last_window_of_mate2/1", "@veto_and_three_baits/1", "@veto_first_window_of_mate1/1",
                    "@veto_given_as_reverse_complement/1", "@veto_reverse_strand_of_the_read/1"]
    free, _, _ = R.walk(idx, set(), *by["edges"]["inputs"])
    what = {r1[i][0][1:-2]: h for i, h in enumerate(free)}
    assert what["len24"] == set() and what["both_short"] == set() and what["n_in_the_window"] == set() and what["no_hit"] == set()
    for nm in ("len25", "len88", "len89", "len152", "len153", "lower_case"):
        assert len(what[nm]) == 1, nm
    assert what["mate2_only"] == {2} and what["reverse_strand"] == {3} and what["three_baits"] == {0, 1, 2}
    assert what["veto_and_three_baits"] == {0, 1, 2}


def test_member_names():
    from zotmer_amd.library import pulldown
    for name, fn, want in [("geneB desc", "in0.fastq", "geneB/desc/in0.fastq"),
                           ("geneB desc", "/data/x/in0.fastq", "geneB/desc/data/x/in0.fastq"),
                           ("b0", "./a/../b/r_1.fastq", "b0/b/r_1.fastq"),
                           ("  a \t x ", "reads/r.fastq.gz", "a/x/reads/r.fastq.gz")]:
        assert pulldown.member_name(name, fn) == want
        assert R.member_name(name, fn) == want
        assert zipfile.ZipInfo.from_file(__file__, "/".join(name.split()) + "/" + fn).filename == want
    assert pulldown.name_clashes(["a x", "b", "a  x", "", "a/x"]) == [("a  x", "gives the same member path as 'a x'"), ("", "has no name"),
                                                                       ("a/x", "gives the same member path as 'a x'")]
    assert pulldown.name_clashes(["a", "b c", "b"]) == []


def test_archive_writer_on_fabricated_spans(tmp_path):
    from zotmer_amd.library import pulldown
    tmp = tmp_path / "t"
    tmp.mkdir()
    ar = pulldown.Archive(str(tmp_path / "o.zip"), ["b0", "skipped", "g desc"], str(tmp))
    ar.begin("x/r_1.fq", "/abs/r_2.fq")
    text = np.frombuffer(b"AAAAbbCCCCCC", np.uint8)
    ar.write(0, text[:6], np.array([0, 4, 4, 6], np.uint64))            # batch 1: bait 0 and bait 2
    ar.write(1, text[:6], np.array([0, 2, 2, 6], np.uint64))
    ar.write(0, text[6:], np.array([0, 0, 0, 6], np.uint64))            # batch 2: bait 2 only
    ar.write(1, text[6:], np.array([0, 0, 0, 6], np.uint64))
    assert sorted(os.listdir(tmp)) == ["0_1.fastq", "0_2.fastq", "2_1.fastq", "2_2.fastq"]
    ar.end()
    assert os.listdir(tmp) == []
    ar.begin("second_1.fq", "second_2.fq")
    ar.write(0, text[:4], np.array([0, 0, 4, 4], np.uint64))
    ar.write(1, text[:4], np.array([0, 0, 4, 4], np.uint64))
    ar.end()
    ar.close()
    with zipfile.ZipFile(tmp_path / "o.zip") as z:
        assert all(i.compress_type == zipfile.ZIP_DEFLATED for i in z.infolist())
        assert [(i.filename, z.read(i)) for i in z.infolist()] == [
            ("b0/x/r_1.fq", b"AAAA"), ("b0/abs/r_2.fq", b"AA"), ("g/desc/x/r_1.fq", b"bbCCCCCC"), ("g/desc/abs/r_2.fq", b"AAbbCCCCCC"),
            ("skipped/second_1.fq", b"AAAA"), ("skipped/second_2.fq", b"AAAA")]


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
        raise AssertionError("the native library or a device context was requested")
    monkeypatch.setattr(engine, "context", refuse)
    monkeypatch.setattr(native, "load", refuse)


def test_help_pulldown(no_device):
    from zotmer_amd import cli
    assert "pulldown" in cli.available()
    code, out, _ = _cli(["help", "pulldown"])
    assert code == 0
    assert "zot pulldown [options] <baits> <output> <input>..." in out
    for word in ("-p is required", "members of all of them", "same member path", "FASTA read inputs are refused", "-m is new",
                 "several processes", "temporary directory"):
        assert word in " ".join(out.split()), word
    code, out, _ = _cli(["help"])
    assert "\tpulldown" in out


def test_refusals_come_before_the_device(no_device, tmp_path, monkeypatch):
    fa = tmp_path / "baits.fa"
    fa.write_text(">b\nACGT\n")
    out = str(tmp_path / "o.zip")
    code, _, err = _cli(["pulldown", "-p", str(fa), out])
    assert code == 1 and "wrong number of arguments" in err
    code, _, err = _cli(["pulldown", str(fa), out, "r_1.fastq", "r_2.fastq"])                # decision 1: no -p
    assert code == 1 and "use -p" in err
    code, _, err = _cli(["pulldown", "-p", str(fa), out, "r_1.fastq", "r_2.fastq", "s_1.fastq"])
    assert code == 1 and "even number of inputs" in err
    for reads in ("reads.fa", "reads.fasta.gz"):                                              # decision 4
        code, _, err = _cli(["pulldown", "-p", str(fa), out, "r_1.fastq", reads])
        assert code == 1 and "FASTQ only" in err and reads in err
    code, _, err = _cli(["pulldown", "-p", "-m", "x", str(fa), out, "r_1.fastq", "r_2.fastq"])
    assert code == 1 and "-m" in err
    code, _, err = _cli(["pulldown", "-p", "-k", "25", str(fa), out, "r_1.fastq", "r_2.fastq"])
    assert code == 1 and "unknown option" in err
    clash = tmp_path / "clash.fa"                                                             # decision 3
    clash.write_text(">a x\nACGT\n>a  x\nACGT\n")
    code, _, err = _cli(["pulldown", "-p", str(clash), out, "r_1.fastq", "r_2.fastq"])
    assert code == 1 and "same member path" in err
    noname = tmp_path / "noname.fa"
    noname.write_text(">\nACGT\n")
    code, _, err = _cli(["pulldown", "-p", str(noname), out, "r_1.fastq", "r_2.fastq"])
    assert code == 1 and "has no name" in err
    monkeypatch.setenv("WORLD_SIZE", "2")                                                     # decision 6
    code, _, err = _cli(["pulldown", "-p", str(fa), out, "r_1.fastq", "r_2.fastq"])
    assert code == "zot pulldown: runs on a single GPU for now"
    assert not os.path.exists(out)
