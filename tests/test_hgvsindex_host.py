"""`zot hgvs-index` on the host: the index against the reference's files (tests/golden/x1_hgvsindex.json), the YAML emitter
against PyYAML, the fold against a brute force, usage and refusals.  No device."""
import contextlib
import functools
import io
import itertools
import json
import os
import random
import re

import numpy as np
import pytest

from tests import _hgvsindex_restatement as R
from tests._hgvsindex_cases import CHROMS, PALINDROME, make_cases, make_genome, names_text, write_genome

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "x1_hgvsindex.json")
IUPAC = "ACGTUNRYSWKMBDHV"


@functools.lru_cache(maxsize=None)
def cases():
    inputs = {c["name"]: c for c in make_cases()}
    gold = json.load(open(GOLD))
    assert [g["name"] for g in gold] == [c["name"] for c in make_cases()]
    return [dict(inputs[g["name"]], gold_index=g["index"], gold_test=g["test"], gold_opts=g["opts"]) for g in gold]


CASE_NAMES = [c["name"] for c in make_cases()]


def case(name):
    return next(c for c in cases() if c["name"] == name)


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    d = tmp_path_factory.mktemp("genome")
    write_genome(str(d))
    return str(d)


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


def command_words(c, genome, tmp_path):
    """the option words of a case for `zot hgvs-index`, its -f and -n files written"""
    words = list(c["opts"]) + ["-g", genome]
    if c["file"] is not None:
        (tmp_path / "variants.txt").write_text(c["file"])
        words += ["-f", str(tmp_path / "variants.txt")]
    if c["names"] is not None:
        (tmp_path / "names.txt").write_text(c["names"])
        words += ["-n", str(tmp_path / "names.txt")]
    return words


def test_fixtures_cover_the_issue_cases():
    seqs, texts = make_genome()
    assert list(seqs) == CHROMS and len(CHROMS) == 24 and all(300 <= len(s) <= 600 for s in seqs.values())
    assert seqs["chr1"][200:270].upper() == seqs["chr2"][100:170].upper() and "N" * 40 in seqs["chr3"].upper()
    assert PALINDROME in seqs["chr5"].upper() and R.rc(16, R.kmers(16, PALINDROME)[0]) == R.kmers(16, PALINDROME)[0]
    assert any(ch.islower() for ch in seqs["chr8"]) and any(ch.isupper() for ch in seqs["chr8"]) and "\r\n" in texts["chr9"]
    assert texts["chr10"].count(">") == 2 and not texts["chr11"].startswith(">") and not texts["chr13"].endswith("\n")
    allv = [v for c in make_cases() for v in c["variants"] + (c["file"] or "").split()]
    from zotmer_amd.library import hgvsindex
    kinds = {hgvsindex.make_variant(v).kind for v in allv if hgvsindex.make_variant(v) is not None}
    assert kinds == {"sub", "del", "dup", "ins", "insN", "insALU", "inv", "delins", "delinsN", "repeat"}
    assert any(hgvsindex.make_variant(v) is None for v in allv)
    k25 = case("kinds_k25")
    assert len(k25["variants"]) != len(set(k25["variants"]))                         # a string said twice
    assert "lhsFlank: ''" in k25["gold_index"] and "rhsFlank: ''" in k25["gold_index"] and "wtSeq: N\n" in k25["gold_index"]
    assert "wtSeq: Y\n" in k25["gold_index"] and "mutSeq: null" in k25["gold_index"] and "wtSeq: ''" in k25["gold_index"]
    assert "NC_000007.13:g.100A>G" in case("names_k16")["gold_index"] and "wtSeq: %s\n" % PALINDROME in case("names_k16")["gold_index"]
    assert any(int(k) > 1 for k in re.findall(r"^    (\d+):", k25["gold_test"], flags=re.M))     # counts above 1 occur
    for c in cases():
        assert c["gold_opts"] == c["opts"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_index_file_is_the_references(name, genome, tmp_path, no_device):
    c = case(name)
    idx = tmp_path / "index.yaml"
    code, out, err = _cli(["hgvs-index"] + command_words(c, genome, tmp_path) + [str(idx)] + c["variants"])
    assert code == 0 and out == ""
    assert idx.read_text() == c["gold_index"]
    from zotmer_amd.library import hgvsindex
    bad = [v for v in c["variants"] + (c["file"] or "").split() if hgvsindex.make_variant(v) is None]
    assert err == "".join("unable to parse %s\n" % v for v in bad)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_parse_index_reads_the_file_back(name, genome, tmp_path, no_device):
    pytest.importorskip("yaml")
    from zotmer_amd.library import hgvsfind, hgvsindex
    c = case(name)
    texts = c["variants"] + (c["file"] or "").split()
    home = hgvsindex.Home(genome, {"NC_000007.13": "chr7"} if c["names"] else None)
    W = int(c["opts"][c["opts"].index("-w") + 1]) if "-w" in c["opts"] else 75
    items, variants = hgvsindex.make_items(texts, home, W, err=io.StringIO())
    back, parsed = hgvsfind.parse_index(hgvsindex.dump_yaml(items))
    assert back == items and [str(v) for v in parsed] == [i["hgvs"] for i in items]
    # the canonical spelling parses to itself, and sizes agree with what scanning derives from it
    for v in variants:
        w = hgvsindex.make_variant(str(v))
        assert str(w) == str(v) and w.range() == v.range() and w.kind == v.kind
        assert hgvsfind.parse_hgvs(str(v)).size() == v.size()


def test_canonical_spellings():
    from zotmer_amd.library import hgvsindex
    for text, want, rng in [("c:g.50delA", "c:g.50del", (49, 50)), ("c:g.60_62delACG", "c:g.60_62del", (59, 62)),
                            ("c:g.198_205insGG", "c:g.204_205insGG", (204, 204)), ("c:g.5_6ins12", "c:g.5_6ins12", (5, 5)),
                            ("c:g.9_10insALU", "c:g.9_10insALU", (9, 9)), ("c:g.140_141invAC", "c:g.140_141inv", (139, 141)),
                            ("c:g.220ACG[2]", "c:g.220_222[2]", (219, 222)), ("c:g.230_232ACG[5]", "c:g.230_232[5]", (229, 232)),
                            ("c:g.210[3]", "c:g.210[3]", (209, 210)), ("c:g.7_7dup", "c:g.7dup", (6, 7)), ("c:g.7delinsT", "c:g.7delinsT", (6, 7)),
                            ("c:g.7_9delins4", "c:g.7_9delins4", (6, 9)), ("c:g.3A>T", "c:g.3A>T", (2, 3))]:
        v = hgvsindex.make_variant(text)
        assert (str(v), v.range()) == (want, rng), text
    v = hgvsindex.make_variant("c:g.3_5inv")
    assert v.sequence("aaCGNtt") == "NCG" and hgvsindex.make_variant("c:g.3_4[3]").sequence("aacgtt") == "CGCGCG"
    assert hgvsindex.make_variant("c:g.3_4[3]").size() == 6 and hgvsindex.make_variant("c:g.3CG[3]").size() == 6
    # Python's slices, as the reference leans on them
    assert hgvsindex.indexed_variant(hgvsindex.make_variant("c:g.0A>T"), 3, "ACGTACGT") == \
        {"hgvs": "c:g.0A>T", "lhsFlank": "ACGTACG", "rhsFlank": "ACG", "wtSeq": "", "mutSeq": "T"}       # seq[0:-1], seq[0:3], seq[-1:0]
    assert hgvsindex.indexed_variant(hgvsindex.make_variant("c:g.20del"), 3, "ACGTACGT")["lhsFlank"] == ""
    recs = hgvsindex.test_records([{"hgvs": "h", "lhsFlank": "ACG", "rhsFlank": "TTG", "wtSeq": "A", "mutSeq": None}], 1)
    assert recs == [("h", "ACGA", "")]


# ---- the emitter -----------------------------------------------------------------------------------------------------------
def test_emitter_equals_pyyaml():
    yaml = pytest.importorskip("yaml")
    from zotmer_amd.library.hgvsindex import dump_yaml

    def same(x):
        assert dump_yaml(x) == yaml.safe_dump(x, default_flow_style=False), x
    strings = ["".join(t) for n in range(3) for t in itertools.product(IUPAC, repeat=n)]
    same(strings)
    same([{"hgvs": s, "lhsFlank": s, "rhsFlank": "", "wtSeq": s, "mutSeq": None} for s in strings[:40]])
    same({s: {"wt": {0: 1}} for s in strings if s})
    rng = random.Random(5)
    long = ["".join(rng.choice("ACGT") for _ in range(n)) for n in (79, 80, 81, 127, 128, 129, 200, 1000)]
    same(long)
    same([{"hgvs": "chr1:g.5_6ins" + s, "lhsFlank": s, "rhsFlank": s, "wtSeq": "", "mutSeq": s} for s in long])
    for n in range(100, 140):                                  # a long key is written as `? key`
        same({"c:g." + "A" * (n - 4): {"mut": {0: 3, 12: 1}, "wt": {1: 40}}, "b:g.5del": {"wt": {7: 7}}})
    same({"chr1:g.49_50[5]": {"mut": {0: 10, 2: 2, 10: 1, 100: 5}, "wt": {2: 12}}, "chr1:g.5del": {"wt": {4974: 1}}})
    same({1: {2: {3: 4}}, 10: {0: {0: 0}}, 2: {11: {5: 6, 40: 1}}})
    same([])
    same({})
    words = ["N", "Y", "n", "y", "NO", "no", "No", "ON", "on", "yes", "Yes", "true", "TRUE", "false", "off", "null", "Null", "~", "-", "?", ":", "a:", ":a", "-a",
             "?a", "<<", "=", "!", "&", "*", "!a", "&a", "*a", "1", "12", "1_0", "0x1F", "0b1", "017", "09", "1e3", "1.", "1.5", ".5", "+1", "-1", "-.inf", ".inf",
             ".NaN", "1:30", "12:30:45", "1:30.5", "2001-01-01", "2001-1-1", "2001-01-01T10:00:00", "2001-1-1t1:00:00.5Z", "2001-01-01T10:00:00+01:00",
             "---", "---a", "...", "..", "a#b", "#a", "a'b", "'a", '"a', "%a", "@a", "`a", "|a", ">a", ",a", "[a", "]a", "{a", "}a", "a,b", "a[b]", "a{b}",
             "chr1:g.5A>T", "NC_000007.13:g.100A>G", "a:b:c:", "0o7", "+", ".", "_", "0", "00", "0_", "1__", "+0x_", "<", "<<<", "=="]
    same(words)
    same({w: {"wt": {1: 1}} for w in words})
    with pytest.raises(ValueError):
        dump_yaml(["a b"])


# ---- the fold ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 5, 16, 31, 32])
def test_fold_against_a_brute_force(K):
    from zotmer_amd.library import hgvsindex
    rng = random.Random(70 + K)
    pal = "".join(rng.choice("ACGT") for _ in range(K // 2))
    pal += "".join("TGCA"["ACGT".index(ch)] for ch in reversed(pal)) if K % 2 == 0 else ""
    genome = "".join(rng.choice("ACGT") for _ in range(400)) + "N" + pal * 3
    recs = [genome[10:10 + K + 8], genome[200:200 + 2 * K] + "N" + genome[14:14 + K], "", pal * 2 + "ACG", genome[10:10 + K + 3], "ACGTN"]
    names = ["v0", "v1", "v2"]
    keys, owners = R.table_of(K, recs)
    got, _, _, _ = R.tally(K, genome.encode(), keys)
    counts = [got.get(x, 0) for x in keys]
    # brute force: per record and distinct canonical k-mer, the occurrences of either strand in the genome
    want = {}
    both = R.kmers(K, genome) + [R.rc(K, x) for x in R.kmers(K, genome)]
    for r, seq in enumerate(recs):
        for z in {min(x, R.rc(K, x)) for x in R.kmers(K, seq)}:
            c = both.count(z) if z != R.rc(K, z) else 2 * R.kmers(K, genome).count(z)
            h = want.setdefault(names[r >> 1], {}).setdefault("mut" if r & 1 else "wt", {})
            h[c] = h.get(c, 0) + 1
    assert R.fold(K, keys, owners, counts, names) == want
    offs = np.cumsum([0] + [len(o) for o in owners]).astype(np.uint32)
    ids = np.array([r for o in owners for r in o], dtype=np.uint32)
    assert hgvsindex.fold(K, np.array(keys, np.uint64), offs, ids, np.array(counts, np.uint64), names) == want
    assert np.array_equal(hgvsindex.rc_keys(K, np.array(keys, np.uint64)), np.array([R.rc(K, x) for x in keys], np.uint64))
    if K % 2 == 0:
        assert any(x == R.rc(K, x) for x in keys)


def test_restated_tally_in_pieces():
    rng = random.Random(3)
    text = ("".join(rng.choice("ACGTacgtUuN\n\n\r>") for _ in range(600))).encode()
    for K in (1, 3, 16, 32):
        keys = set(R.kmers(K, text.decode().replace("\n", "").replace("\r", "")))
        whole = R.tally(K, text, keys)
        for cut in (0, 1, 299, 600):
            a = R.tally(K, text[:cut], keys)
            b = R.tally(K, text[cut:], keys, a[1])
            merged = dict(a[0])
            for x, c in b[0].items():
                merged[x] = merged.get(x, 0) + c
            assert (merged, b[1], a[2] + b[2]) == whole[:3]


# ---- the command -------------------------------------------------------------------------------------------------------------
def test_help_hgvs_index(no_device):
    from zotmer_amd import cli
    assert "hgvs-index" in cli.available()
    code, out, _ = _cli(["help", "hgvs-index"])
    assert code == 0
    assert "zot hgvs-index [options] <index> [<variant>...]" in out and "zot hgvs-index -T [options] [<variant>...]" in out
    flat = " ".join(out.split())
    for word in ("-f FILENAME", "-g PATH", "-k K", "-n NAMES", "-w WIDTH", "-W WIDTH", "-m MEM", "accepted and ignored", "a command of its own",
                 "grouped by accession in order of first appearance", "Python 2 dict", "-n gives the mapping", "every *.fa.gz / *.fa of -g in name order",
                 "exactly the files it names", "the same counts when the directory holds the 24 chromosomes", "a missing sequence file",
                 ".fa is read where there is no .fa.gz", "must not begin or end with blanks", "a palindromic k-mer counts twice",
                 "-m and -n are new", "several processes", "Nothing touches the device before", "does not touch it at all"):
        assert word in flat, word
    code, out, _ = _cli(["help"])
    assert "\thgvs-index" in out


def test_hgvs_find_still_refuses_indexing(no_device, tmp_path):
    code, _, err = _cli(["hgvs-find", "-X", str(tmp_path / "i.yaml"), "chr1:g.5A>T"])
    assert code == 1 and "indexing (-X) is not implemented" in err


def test_usage_and_refusals(no_device, genome, tmp_path, monkeypatch):
    idx = str(tmp_path / "i.yaml")
    v = "chr1:g.5A>T"
    code, _, err = _cli(["hgvs-index"])
    assert code == 1 and "wrong number of arguments" in err
    for opt in (["-k", "33"], ["-k", "0"], ["-k", "x"], ["-w", "x"], ["-w", "-1"], ["-W", "x"], ["-m", "0"], ["-m", "x"], ["-q"], ["-X"], ["-k"]):
        code, _, err = _cli(["hgvs-index", "-g", genome] + opt + [idx, v])
        assert code == 1 and ("option" in err), opt
    code, _, err = _cli(["hgvs-index", "-g", str(tmp_path / "nowhere"), idx, v])
    assert code == 1 and "is not a directory" in err
    code, _, err = _cli(["hgvs-index", "-g", genome, idx, "chr77:g.5A>T"])
    assert code == 1 and "zot hgvs-index: no sequence file for chr77" in err
    code, _, err = _cli(["hgvs-index", "-g", genome, "-f", str(tmp_path / "none.txt"), idx])
    assert code == 1 and "zot hgvs-index:" in err and "none.txt" in err
    code, _, err = _cli(["hgvs-index", "-g", genome, "-n", str(tmp_path / "none.txt"), idx, v])
    assert code == 1 and "none.txt" in err
    (tmp_path / "bad.txt").write_text("acc chr1 extra\n")
    code, _, err = _cli(["hgvs-index", "-g", genome, "-n", str(tmp_path / "bad.txt"), idx, v])
    assert code == 1 and "line 1" in err
    code, _, err = _cli(["hgvs-index", "-g", genome, idx, "chr 1:g.5A>T"])
    assert code == 1 and "blank" in err
    (tmp_path / "empty.fa").write_text("ACGT\n")
    code, _, err = _cli(["hgvs-index", "-g", str(tmp_path), idx, "empty:g.2del"])
    assert code == 1 and "holds no FASTA record" in err
    assert not os.path.exists(idx)
    # .fa where there is no .fa.gz; -W is taken; an index without variants is an empty list
    (tmp_path / "plain.fa").write_text(">plain\nACGTAC\nGTTT\n")
    code, _, err = _cli(["hgvs-index", "-g", str(tmp_path), "-W", "7", "-w", "2", idx, "plain:g.6_7insG"])
    assert code == 0 and open(idx).read() == "- hgvs: plain:g.6_7insG\n  lhsFlank: AC\n  mutSeq: G\n  rhsFlank: GT\n  wtSeq: ''\n"
    code, _, err = _cli(["hgvs-index", "-g", genome, idx])
    assert code == 0 and open(idx).read() == "[]\n"
    monkeypatch.setenv("WORLD_SIZE", "2")
    code, _, err = _cli(["hgvs-index", "-g", genome, idx, v])
    assert code == "zot hgvs-index: runs on a single GPU for now"
    monkeypatch.delenv("WORLD_SIZE")
    # -T: refusals first, the device only after them
    code, _, err = _cli(["hgvs-index", "-T", "-g", genome, "chr77:g.5A>T"])
    assert code == 1 and "no sequence file for chr77" in err
    (tmp_path / "names.txt").write_text("acc chr1\nother chr99\n")
    code, _, err = _cli(["hgvs-index", "-T", "-g", genome, "-n", str(tmp_path / "names.txt"), v])
    assert code == 1 and "no sequence file for other" in err
    with pytest.raises(AssertionError, match="a device context was requested"):
        _cli(["hgvs-index", "-T", "-g", genome, v])


def test_the_files_T_scans(genome, tmp_path):
    from zotmer_amd.library import hgvsindex
    assert [os.path.basename(p) for p in hgvsindex.Home(genome).files()] == sorted(c + ".fa.gz" for c in CHROMS)
    (tmp_path / "names.txt").write_text(names_text())
    named = hgvsindex.Home(genome, hgvsindex.read_names(str(tmp_path / "names.txt"))).files()
    assert sorted(named) == sorted(hgvsindex.Home(genome).files()) and os.path.basename(named[0]) == "chr7.fa.gz"
    for nm in ("b.fa", "a.fa.gz", "a.fa", "c.fasta", "d.fa.gz.tmp", ".fa"):
        (tmp_path / nm).write_text(">x\nA\n")
    assert [os.path.basename(p) for p in hgvsindex.Home(str(tmp_path)).files()] == ["a.fa.gz", "b.fa"]
    where = hgvsindex.RecordBody()
    assert (where.phase, where.at_bol) == (where.SEEK, True)
