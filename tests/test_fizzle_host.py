"""`zot fizzle` without a GPU: the restatement against what the reference's own functions gave (tests/golden/z1_fizzle.json), the
host side of the product against the restatement (-P, -X, the loader, the class index, the grouped evaluation of the multi-class
records, the table and its filters, -T's report from given counts), the refusals (all of them before anything touches a device:
there is none here) and the usage text."""
import contextlib
import io
import json
import os
import random

import numpy as np
import pytest

from tests import _fizzle_restatement as R
from tests._fizzle_cases import case_digests, fixture_cases, write_case
from zotmer_amd.library import fizzle
from zotmer_amd.library.hgvsindex import InputError, dump_yaml, rc_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "z1_fizzle.json")))
CASES = {c["name"]: c for c in fixture_cases()}
IDS = [g["name"] for g in GOLD]


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


def read(path):
    with open(path, newline="") as f:
        return f.read()


def ref_of(gold):
    case = CASES[gold["name"]]
    return R.as_loaded(R.index_bed(gold["bed"], lambda ch: case["chroms"][ch]))


def pairs_of(case):
    return list(zip(R.read_fastq(case["reads"][0]), R.read_fastq(case["reads"][1])))


# ---- the restatement and the fixture ---------------------------------------------------------------------------------------------
def test_the_fixture_covers_what_it_should():
    assert IDS == [c["name"] for c in fixture_cases()] and {g["K"] for g in GOLD} >= {5, 25, 32}
    for g in GOLD:
        assert g["params"] == case_digests(CASES[g["name"]]) and len(g["records"]) == 2 * g["pairs"]
        assert "multiple chromosomes" in g["bed_err"] and "no annotated" in g["bed_err"] and "not found" in g["bed_tx_err"]
        assert "exon: '01'" in g["index"] and "strand: '-'" in g["index"] and "strand: +" in g["index"]
        assert any(n > 0 and not res for n, res in g["records"]) and any(len(res) > 1 for n, res in g["records"])


@pytest.mark.parametrize("gold", GOLD, ids=IDS)
def test_restatement_reproduces_the_reference(gold):
    case = CASES[gold["name"]]
    K = case["K"]
    assert R.prepare_gene(case["gene_list"], case["ref_gene"]) == (gold["bed"], gold["bed_err"])
    assert R.prepare_gene_tx(case["tx_list"], case["ref_gene"]) == (gold["bed_tx"], gold["bed_tx_err"])
    items = R.index_bed(gold["bed"], lambda ch: case["chroms"][ch])
    assert fizzle.dump_all(items) == gold["index"]
    idx, _ = R.tuple_index(K, R.as_loaded(items))
    got = []
    for s1, s2 in pairs_of(case):
        for xs in R.records_of(K, s1, s2):
            res, n = R.rec_hits(idx, xs)
            got.append([n, sorted([list(k), v] for k, v in res.items())])
    assert got == gold["records"]


def test_the_example_of_the_threshold_loop():
    for f in (R.rec_hits_sdx, fizzle.rec_hits):
        assert f({(0, 1): 3, (1, 2): 1, (0, 2): 2}) == ({(0,): 5}, 6)
        assert f({(0, 1): 2, (1, 2): 2, (0, 2): 2}) == ({}, 6)
        assert f({(0, 1): 4, (1, 2): 3, (0, 2): 3, (0,): 1}) == ({(0, 1): 4}, 11)
        assert f({(0, 1): 2, (1, 2): 2, (0, 2): 2, (5, 6): 3, (6,): 1}) == ({(6,): 4}, 10)
        assert f({}) == ({}, 0) and f({(3, 4): 7}) == ({(3, 4): 7}, 7)


# ---- -P, -X and the loader ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gold", GOLD[:2], ids=IDS[:2])
def test_prepare_with_and_without_t(gold, tmp_path):
    p = write_case(CASES[gold["name"]], str(tmp_path))
    bed = str(tmp_path / "out.bed")
    code, out, err = run(["fizzle", "-P", p["gene_list"], p["ref_gene"], bed])
    assert (code, out, err, read(bed)) == (0, "", gold["bed_err"], gold["bed"])
    code, out, err = run(["fizzle", "-P", "-t", p["tx_list"], p["ref_gene"], bed + ".gz"])
    assert (code, out, err) == (0, "", gold["bed_tx_err"])
    with fizzle.open_text(bed + ".gz") as f:
        assert f.read() == gold["bed_tx"]


@pytest.mark.parametrize("gold", GOLD, ids=IDS)
def test_index_and_loader(gold, tmp_path):
    """-X writes the reference's bytes; the loader reads them back as BaseLoader does; the class index is the tuple index"""
    case = CASES[gold["name"]]
    p = write_case(case, str(tmp_path), bed=gold["bed"])
    index = str(tmp_path / "index.yaml")
    code, out, err = run(["fizzle", "-X", "-v", "-g", p["home"], index, p["bed"]])
    assert (code, out, err) == (0, "", "processing c1\nprocessing c2\nprocessing c3\n") and read(index) == gold["index"]
    ref = fizzle.load_index(index)
    assert ref == ref_of(gold)
    K = case["K"]
    idx, lens = R.tuple_index(K, ref)
    ci = fizzle.ClassIndex(K, ref)
    assert ci.lens == lens and ci.keys.tolist() == sorted(idx) and ci.tuples == sorted(set(idx.values()))
    assert [ci.tuples[c] for c in ci.key_class.tolist()] == [idx[x] for x in ci.keys.tolist()]
    assert all(tuple(ci.exons[a:b].tolist()) == idx[x] for x, a, b in zip(ci.keys.tolist(), ci.offs[:-1].tolist(), ci.offs[1:].tolist()))


def test_loader_forms(tmp_path):
    p = str(tmp_path / "i.yaml")
    with open(p, "w") as f:
        f.write("chr: c1\nen: 9\nexon: '01'\ngene: it''s\nseq: ''\nst: 5\nstrand: '-'\n---\nchr: c1\nexon: 2\ngene: G\nseq: ACGT\n...\n")
    assert fizzle.load_index(p) == [dict(chr="c1", en="9", exon="01", gene="it''s", seq="", st="5", strand="-"),
                                    dict(chr="c1", exon="2", gene="G", seq="ACGT")]
    for text in ("", "---\n", "- a\n", "gene: G\n", "gene: [a]\nexon: 1\nchr: c\nseq: A\n", "gene\n"):
        with open(p, "w") as f:
            f.write(text)
        with pytest.raises(InputError):
            fizzle.load_index(p)


def test_yaml_text_is_pyyamls():
    yaml = pytest.importorskip("yaml")
    for gold in GOLD:
        case = CASES[gold["name"]]
        items = R.index_bed(gold["bed"], lambda ch: case["chroms"][ch])
        assert fizzle.dump_all(items) == yaml.safe_dump_all(items, default_flow_style=False)
        assert list(yaml.load_all(gold["index"], Loader=yaml.BaseLoader)) == R.as_loaded(items)
        rep = R.crosstalk(case["K"], R.as_loaded(items), lambda ch: case["chroms"][ch])
        assert dump_yaml(rep) == yaml.safe_dump(rep, default_flow_style=False)
    odd = [dict(gene="NO", exon="1e3", chr="~", st=0, en=0, strand="+", seq=""), dict(gene="0x1F", exon="010", chr="c:1", st=1, en=2, strand="-", seq="ACGTN")]
    assert fizzle.dump_all(odd) == yaml.safe_dump_all(odd, default_flow_style=False)
    empty = {"aliasing-within": {}, "aliasing-genomic": {}}
    assert dump_yaml(empty) == yaml.safe_dump(empty, default_flow_style=False)


# ---- -T from given counts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gold", GOLD, ids=IDS)
def test_crosstalk_report_from_a_tally(gold):
    """the keys and their reverse complements, the forward windows of the chromosomes counted here in Python: the report is the
    restatement's"""
    case = CASES[gold["name"]]
    K, ref = case["K"], ref_of(gold)
    ci = fizzle.ClassIndex(K, ref)
    keys2 = np.unique(np.concatenate((ci.keys, rc_keys(K, ci.keys))))
    at = {x: j for j, x in enumerate(keys2.tolist())}
    tally = np.zeros(len(keys2), dtype=np.uint64)
    for ch in sorted({itm["chr"] for itm in ref}):
        for x, _, _ in R.kmers_with_pos(K, case["chroms"][ch]):
            if x in at:
                tally[at[x]] += 1
    rep = fizzle.crosstalk_report(ci, fizzle.genome_counts(ci, keys2, tally))
    want = R.crosstalk(K, ref, lambda ch: case["chroms"][ch])
    assert rep == want and "GB/02" in rep["aliasing-genomic"] and rep["aliasing-within"]
    assert any(len(v) == 3 for v in rep["aliasing-within"].values())


# ---- the grouped evaluation ----------------------------------------------------------------------------------------------------------
def random_universe(rng, n_exons, n_tuples):
    tuples = {(e,) for e in range(n_exons)}
    while len(tuples) < n_tuples:
        tuples.add(tuple(sorted(rng.sample(range(n_exons), rng.randrange(2, 4)))))
    return sorted(tuples)


@pytest.mark.parametrize("seed,n_exons,n_tuples", [(1, 5, 12), (2, 7, 20), (3, 9, 30), (4, 4, 9)])
def test_grouped_evaluation_is_rec_hits_on_every_record(seed, n_exons, n_tuples):
    rng = random.Random(seed)
    tuples = random_universe(rng, n_exons, n_tuples)
    accu = fizzle.Accumulator(tuples)
    acc, hist = {}, {}
    single = np.zeros(2 * len(tuples), dtype=np.uint64)
    dev_hist = np.zeros(64, dtype=np.uint64)
    empties = 0
    for batch in range(4):
        rec, cls, cnt = [], [], []
        for r in range(900):
            classes = sorted(rng.sample(range(len(tuples)), rng.choice((1, 2, 2, 3, 3, 4, 5))))
            counts = [rng.randrange(1, 4) for _ in classes]
            res, n = R.rec_hits_sdx({tuples[c]: k for c, k in zip(classes, counts)})
            if res:
                a = acc.setdefault(tuple(sorted(res)), [0, 0])
                a[0] += 1
                a[1] += sum(res.values())
                hist[n] = hist.get(n, 0) + 1
            else:
                empties += 1
            if len(classes) == 1:                         # what the device tallies itself
                single[2 * classes[0]] += 1
                single[2 * classes[0] + 1] += counts[0]
                dev_hist[counts[0]] += 1
            else:
                rec += [7 * r + batch] * len(classes)
                cls += classes
                cnt += counts
        accu.add_entries(np.array(rec, dtype=np.uint32), np.array(cls, dtype=np.uint32), np.array(cnt, dtype=np.uint32))
    accu.add_entries(np.empty(0, np.uint32), np.empty(0, np.uint32), np.empty(0, np.uint32))
    accu.add_single(single, dev_hist)
    assert accu.acc == acc and accu.hist == hist
    assert accu.slow > 50 and empties > 10 and accu.multi > 2000 and len(accu.plan) < accu.multi      # a set met again is not evaluated again


# ---- the table -----------------------------------------------------------------------------------------------------------------------
def scan_of(gold):
    case = CASES[gold["name"]]
    ref = ref_of(gold)
    idx, _ = R.tuple_index(case["K"], ref)
    return (ref,) + R.scan(case["K"], idx, pairs_of(case))


def test_table_filters_one_at_a_time_and_the_row_order():
    ref, acc, hit_counts, rn = scan_of(GOLD[0])
    full = R.table(ref, acc)
    assert fizzle.table_lines(ref, acc) == full and len(full) > 30
    assert full[0].split("\t") == list(fizzle.HEADER)
    groups = [l.split("\t")[9].encode("latin-1") for l in full[1:]]
    assert groups == sorted(groups) and len(set(groups)) == len(groups)
    for kw in (dict(gene_count=(2, 2)), dict(gene_count=(0, 1)), dict(exon_count=(2, 999999)), dict(exon_count=(0, 1)), dict(exon_count=(3, 3)),
               dict(min_gene_reads=5), dict(min_exon_reads=3), dict(min_gene_rate=52.0), dict(min_exon_rate=50.5)):
        want = R.table(ref, acc, **kw)
        assert fizzle.table_lines(ref, acc, fizzle.Filters(**kw)) == want and 1 < len(want) < len(full), kw
    # -z counts the distinct exons of the row's own key: GA/02|GC/01|GD/02 is one answer of three exons
    three = [l for l in R.table(ref, acc, exon_count=(3, 3))[1:]]
    assert three and all(l.split("\t")[9].count("/") == 3 for l in three)
    hist = {}
    for h in hit_counts:
        hist[h] = hist.get(h, 0) + 1
    assert fizzle.verbose_lines(hist, rn) == R.verbose_lines(hit_counts, rn)
    assert fizzle.verbose_lines({}, 3) == ["total read hits: 0", "total reads: 3"]
    assert fizzle.table_lines(ref, {}) == [full[0]]


# ---- refusals and the usage text -----------------------------------------------------------------------------------------------------
def test_refusals(tmp_path, monkeypatch):
    gold = GOLD[0]
    p = write_case(CASES[gold["name"]], str(tmp_path), bed=gold["bed"])
    index = str(tmp_path / "index.yaml")
    with open(index, "w") as f:
        f.write(gold["index"])
    import zotmer_amd.library.engine as engine
    monkeypatch.setattr(engine, "context", lambda *a, **k: pytest.fail("a context was asked for"))
    r1, r2 = p["reads_1"], p["reads_2"]
    for k in ("0", "33", "-1", "x"):
        code, out, err = run(["fizzle", "-k", k, index, r1, r2])
        assert code == 1 and out == "" and "-k" in err, k
    for opt, v in (("-M", "x"), ("-m", "1.5"), ("-R", "x"), ("-r", ""), ("-Z", "3"), ("-z", "1:x"), ("-b", "0")):
        code, out, err = run(["fizzle", opt, v, index, r1, r2])
        assert code == 1 and out == "" and opt in err, opt
    code, out, err = run(["fizzle", index, r1])
    assert code == 1 and "odd number of inputs" in err
    code, out, err = run(["fizzle", index, r1, r2, r1])
    assert code == 1 and "odd number of inputs" in err
    code, out, err = run(["fizzle", index])
    assert code == 1 and "wrong number of arguments" in err
    fa = str(tmp_path / "reads.fa")
    open(fa, "w").write(">a\nACGT\n")
    code, out, err = run(["fizzle", index, fa, r2])
    assert code == 1 and "FASTQ only" in err
    empty = str(tmp_path / "empty.yaml")
    open(empty, "w").write("")
    for args in ([empty, r1, r2], ["-T", "-g", p["home"], empty]):
        code, out, err = run(["fizzle"] + args)
        assert code == 1 and out == "" and "holds no documents" in err
    code, out, err = run(["fizzle", str(tmp_path / "missing.yaml"), r1, r2])
    assert code == 1 and out == "" and err.startswith("zot fizzle: ")
    code, out, err = run(["fizzle", "-T", "-g", str(tmp_path), index])
    assert code == 1 and out == "" and "no sequence file for c1" in err
    code, out, err = run(["fizzle", "-T", "-g", str(tmp_path / "nowhere"), index])
    assert code == 1 and "is not a directory" in err
    code, out, err = run(["fizzle", "-X", "-g", str(tmp_path), index + ".2", p["bed"]])
    assert code == 1 and "no sequence file for c1" in err and not os.path.exists(index + ".2")
    for args in (["-P", "-X", index, p["bed"]], ["-T", index, r1], ["-X", index], ["-P", p["gene_list"], p["ref_gene"]]):
        code, out, err = run(["fizzle"] + args)
        assert code == 1 and out == "", args
    bad = str(tmp_path / "bad.txt")
    open(bad, "w").write("0\tNM_1\tc1\t+\t1\t2\t1\t2\t1\tx,\t9,\t0\tGA\n")
    code, out, err = run(["fizzle", "-P", p["gene_list"], bad, str(tmp_path / "o.bed")])
    assert code == 1 and err.startswith("zot fizzle: ")
    monkeypatch.setenv("WORLD_SIZE", "2")
    for args in ([index, r1, r2], ["-T", "-g", p["home"], index]):
        code, out, err = run(["fizzle"] + args)
        assert code == "zot fizzle: runs on a single GPU for now"


def test_usage_text():
    code, out, err = run(["help", "fizzle"])
    assert code == 0 and err == ""
    for word in ("zot fizzle -P [options] <gene-list> <refgene> <bedfile>", "zot fizzle -X [options] <index> <must-have>",
                 "zot fizzle -T [options] <index>", "zot fizzle [options] <index> <input>...", "[default: 25]", "[default: 0:999999]",
                 "dies there", "debugging print", "sorted by the bytes of exonGroup", "row's own key", "as many bins as the longest pair needs",
                 "An index without documents is refused", "K outside 1..32 is refused", "FASTA read inputs are refused",
                 "An odd number of\ninputs is refused", "torch.distributed.run", "Nothing\ntouches the device before"):
        assert word in out, word
    code, out, err = run(["help"])
    assert "\tfizzle\n" in out
    code, out, err = run(["fizzle", "-h"])
    assert code == 0 and "zot fizzle - exon groups" in out
