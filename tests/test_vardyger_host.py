"""`zot vardyger` without a GPU: the literal restatement against what the reference's main printed (tests/golden/v1_vardyger.json),
the product's index, filters and table against the restatement with zk_dup_join replaced by its contract in plain Python, the
contract against findDup + positions on random cases, the refusals (all before anything touches a device) and the usage text."""
import contextlib
import io
import json
import os
import random

import numpy as np
import pytest

from tests import _vardyger_restatement as R
from tests._vardyger_cases import counted_from, digest, fixture_cases, join_by_its_contract, rand_seq, write_case
from zotmer_amd.library import hgvsfind, vardyger

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "v1_vardyger.json")))
INPUTS = {c["name"]: c for c in fixture_cases()}


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


def split_stdout(lines):
    """the reference's stdout -> (coverage lines, table lines without the header)"""
    cover = [l for l in lines if l == "" or set(l) <= set(".X")]
    rest = [l for l in lines if not (l == "" or set(l) <= set(".X"))]
    assert not rest or rest[0] == R.HEADER
    return cover, rest[1:]


def min_cov_of(opts):
    return int(opts[opts.index("-m") + 1]) if "-m" in opts else 10


# ---- the restatement and the fixture -------------------------------------------------------------------------------------------
def test_the_fixture_covers_what_it_should():
    assert [c["name"] for c in GOLD] == [c["name"] for c in fixture_cases()] and len(GOLD) >= 15
    rows = {c["name"]: [l.split("\t")[-1] for l in split_stdout(c["stdout"])[1]] for c in GOLD}
    assert rows["u30"] == ["GENE1:c.201_230dup"] == rows["u30_strict"]
    assert rows["u31"] == [] and rows["u31_all"] == ["GENE1:c.201_231dup"]
    assert len(rows["u13_all_rolled3"]) == 3 and rows["u12_all"] == [] and len(rows["u48_k32_rolled2"]) == 2
    assert rows["gap"] and rows["gap_strict"] == [] and len(rows["two_depths"]) == 2 and len(rows["two_depths_m30"]) == 1
    assert {h.split(":")[0] for h in rows["shared"]} == {"GENE1", "SHARED"}
    assert [c["name"] for c in GOLD if c["stderr"]] == ["phantom"]
    assert all(l.startswith("warning: phantom dumplication: ") for c in GOLD for l in c["stderr"])
    assert {c["K"] for c in GOLD} == {24, 30, 32}
    assert any("\r\n" in t for t in INPUTS["dressed_two_files"]["inputs"]) and len(INPUTS["dressed_two_files"]["inputs"]) == 2


@pytest.mark.parametrize("gold", GOLD, ids=[c["name"] for c in GOLD])
def test_restatement_reproduces_the_reference(gold):
    """the coverage lines in order; the rows without their number and the warnings as sorted lists; n = 1 .. rows"""
    case = INPUTS[gold["name"]]
    assert (case["K"], case["opts"]) == (gold["K"], gold["opts"])
    assert gold["params"]["fasta"] == digest([case["fasta"]]) and gold["params"]["inputs"] == digest(case["inputs"])
    index = R.Index(case["K"], list(R.read_fasta(case["fasta"])))
    reads = [s for t in case["inputs"] for s in R.read_fastq(t)]
    assert len(reads) == gold["params"]["reads"]
    ties = []
    cover, rows = R.call(index, R.count_reads(index, reads), min_cov_of(case["opts"]), "-a" in case["opts"], "-s" in case["opts"], ties)
    want_cover, want_rows = split_stdout(gold["stdout"])
    assert cover == want_cover and not ties
    assert sorted(R.ordered(rows)) == sorted(l.split("\t", 1)[1] for l in want_rows)
    assert [l.split("\t")[0] for l in want_rows] == [str(i + 1) for i in range(len(want_rows))]
    assert sorted(index.warnings) == sorted(gold["stderr"])


# ---- the host layer, the join replaced by its contract ----------------------------------------------------------------------------
def host_call(case):
    """library/vardyger.py's index, order, filters and table on a case, zk_dup_join being join_by_its_contract"""
    K, opts = case["K"], case["opts"]
    records = list(R.read_fasta(case["fasta"]))
    index = vardyger.Index(K, records)
    tables = [a.tolist() for a in (index.rseq, index.rkmer, index.rpos, index.by_second)]
    _, own = join_by_its_contract(*[a.tolist() for a in index.own_list()], *tables, K, 1)
    warnings = list(vardyger.phantom_warnings(index, vardyger.order_rows(index, *zip(*own)) if own else np.zeros((0, 3), np.int64)))
    ref = R.Index(K, records)
    X = R.count_reads(ref, [s for t in case["inputs"] for s in R.read_fastq(t)])
    baits, kmers, counts = [np.array(a, dtype=dt) for a, dt in zip(counted_from(X), (np.uint32, np.uint64, np.uint64))]
    cover, rows = join_by_its_contract(baits.tolist(), kmers.tolist(), counts.tolist(), *tables, K, vardyger.THRESHOLD)
    rows = vardyger.order_rows(index, *zip(*rows)) if rows else np.zeros((0, 3), np.int64)
    counted = hgvsfind.Counted(baits, kmers, counts, len(records))
    lines = list(vardyger.table_rows(index, counted, np.array(cover, dtype=np.uint32), rows, min_cov_of(opts), "-a" in opts, "-s" in opts,
                                     vardyger.new_stats()))
    return warnings, [vardyger.coverage_line(index, np.array(cover), n) for n in range(len(records))], lines


@pytest.mark.parametrize("gold", GOLD, ids=[c["name"] for c in GOLD])
def test_host_layer_reproduces_the_reference(gold):
    """the lines in the product's order are the restatement's rows ordered by (sequence, c, b, d, a, pa, pc); as sorted lists they
    are the reference's"""
    case = INPUTS[gold["name"]]
    warnings, cover, lines = host_call(case)
    want_cover, want_rows = split_stdout(gold["stdout"])
    assert cover == want_cover
    assert sorted(lines) == sorted(l.split("\t", 1)[1] for l in want_rows)
    assert sorted(warnings) == sorted(gold["stderr"])
    index = R.Index(case["K"], list(R.read_fasta(case["fasta"])))
    reads = [s for t in case["inputs"] for s in R.read_fastq(t)]
    _, rows = R.call(index, R.count_reads(index, reads), min_cov_of(case["opts"]), "-a" in case["opts"], "-s" in case["opts"])
    assert lines == R.ordered(rows)


def test_the_index_is_the_restatements():
    rng = random.Random(3)
    for K in (2, 4, 24, 32):
        records = [("a", rand_seq(rng, 90)), ("b", "acgu" * 3 + rand_seq(rng, 50) + "N" + rand_seq(rng, 40)), ("c", "ACG"), ("d", "")]
        index = vardyger.Index(K, records)
        want = sorted((n, x, p) for n, (_, seq) in enumerate(records) for x, p in R.kmers_with_pos_list(K, seq))
        assert list(zip(index.rseq.tolist(), index.rkmer.tolist(), index.rpos.tolist())) == want
        low = (1 << K) - 1
        key = lambda i: (want[i][0], want[i][1] & low, want[i][1] >> K, want[i][2])
        assert index.by_second.tolist() == sorted(range(len(want)), key=key)
        for n, (_, seq) in enumerate(records):
            walk = index.walk[index.cuts[n]:index.cuts[n + 1]]
            assert [want[i][1:] for i in walk.tolist()] == R.kmers_with_pos_list(K, seq)
        b, x, c = index.own_list()
        assert list(zip(b.tolist(), x.tolist())) == sorted({w[:2] for w in want}) and set(c.tolist()) <= {1}
    with pytest.raises(vardyger.InputError, match="two sequences are named a"):
        vardyger.Index(4, [("a", "ACGT"), ("b", "ACGT"), ("a", "ACGT")])
    with pytest.raises(vardyger.InputError):
        vardyger.Index(5, [("a", "ACGT")])


def test_the_contract_is_find_dup_and_positions():
    """zk_dup_join's rows, as the header words them, against the literal findDup + positions: random sequences over two and four
    letters with an N, K in {2, 4, 6, 8}, random counts around the threshold"""
    rng = random.Random(17)
    total = 0
    for trial in range(120):
        K = rng.choice((2, 4, 6, 8))
        alphabet = rng.choice(("AC", "ACGT", "ACG"))
        seq = rand_seq(rng, rng.randrange(K, 60), alphabet)
        if trial % 3 == 0 and len(seq) > 4:
            p = rng.randrange(len(seq))
            seq = seq[:p] + "N" + seq[p + 1:]
        records = [("s", seq)]
        index, ref = vardyger.Index(K, records), R.Index(K, records)
        pool = sorted(set(index.rkmer.tolist()) | {rng.randrange(1 << (2 * K)) for _ in range(30)})
        X = {x: rng.choice((9, 10, 11)) for x in pool if rng.random() < 0.7}
        xs = {x: c for x, c in X.items() if c >= 10}
        want = sorted(R.candidates(ref, 0, xs))
        tables = [a.tolist() for a in (index.rseq, index.rkmer, index.rpos, index.by_second)]
        _, rows = join_by_its_contract(*counted_from([X]), *tables, K, 10)
        low = (1 << K) - 1
        got = sorted((tables[1][i] >> K, tables[1][i] & low, tables[1][j] >> K, tables[1][j] & low, tables[2][i], tables[2][j]) for _, i, j in rows)
        assert got == want, (K, seq)
        total += len(want)
    assert total > 2000


# ---- refusals and the usage text -------------------------------------------------------------------------------------------------
def test_refusals(tmp_path, monkeypatch):
    from zotmer_amd.library import engine

    def no_device(*a, **kw):
        raise AssertionError("the command reached for the device")
    monkeypatch.setattr(engine, "context", no_device)
    args = write_case(INPUTS["u30"], str(tmp_path))
    fa, fq = args[-2], args[-1]
    code, out, err = run(["vardyger", "-k", "23", fa, fq])
    assert code is None and out == "" and err == "K must be even.\n"
    for k in ("0", "34", "-2", "x"):
        code, out, err = run(["vardyger", "-k", k, fa, fq])
        assert code == 1 and out == "" and "-k" in err, k
    code, out, err = run(["vardyger", "-m", "x", fa, fq])
    assert code == 1 and out == "" and "-m" in err
    code, out, err = run(["vardyger", "-b", "0", fa, fq])
    assert code == 1 and out == "" and "-b" in err
    code, out, err = run(["vardyger", "-A", fa, fq])
    assert code == 1 and out == "" and "-A is not implemented" in err
    code, out, err = run(["vardyger", fa, fa])
    assert code == 1 and "FASTQ only" in err
    code, out, err = run(["vardyger", fa])
    assert code == 1 and "wrong number of arguments" in err
    code, out, err = run(["vardyger", "-x", fa, fq])
    assert code == 1 and "unknown option" in err
    twice = str(tmp_path / "twice.fa")
    with open(twice, "w") as f:
        f.write(">a x\nACGTACGTAC\n>b\nACGT\n>a x\nGGGG\n")
    code, out, err = run(["vardyger", "-k", "4", twice, fq])
    assert code == 1 and out == "" and "two sequences are named a x" in err
    code, out, err = run(["vardyger", str(tmp_path / "missing.fa"), fq])
    assert code == 1 and out == "" and err.startswith("zot vardyger: ")
    monkeypatch.setenv("WORLD_SIZE", "2")
    code, out, err = run(["vardyger", fa, fq])
    assert code == "zot vardyger: runs on a single GPU for now"


def test_usage_text():
    code, out, err = run(["help", "vardyger"])
    assert code == 0 and err == ""
    for word in ("zot vardyger [options] <sequences> <input>...", "-k K", "-m MIN", "-b MEM", "[default: 24]", "[default: 10]", "-s ", "-a ",
                 "(sequence, c, b, d, a, pa, pc)", "-A is refused", "FASTA read", "single GPU", "-b is new", "K must be even",
                 "Nothing touches the device", "phantom dumplication", "stops before its caller"):
        assert word in out, word
    code, out, err = run(["help"])
    assert "\tvardyger\n" in out
    code, out, err = run(["vardyger", "-h"])
    assert code == 0 and "zot vardyger - search for tandem duplications" in out
