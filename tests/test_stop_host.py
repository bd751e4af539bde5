"""`zot stop` without a GPU: the restatement against the lines the reference's main printed (tests/golden/s1_stop.json), the FASTA
index of the product against the restatement's (the polyA trim, the name order, the layout, the known stops), the draw, the
refusals (all of them before anything touches a device: there is none here) and the usage text."""
import contextlib
import io
import json
import os
import random

import numpy as np
import pytest

from tests import _stop_restatement as R
from tests._stop_cases import digest, fixture_cases, write_case
from zotmer_amd import synth
from zotmer_amd.library import stopscan
from zotmer_amd.library.alufinder import InputError, anchor_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "s1_stop.json")))
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


# ---- the restatement and the fixture ---------------------------------------------------------------------------------------------
def test_the_fixture_covers_what_it_should():
    assert [c["name"] for c in GOLD] == [c["name"] for c in fixture_cases()] and len(GOLD) >= 24
    assert {c["K"] for c in GOLD} >= {15, 25, 27, 31, 32}
    lines = [l for c in GOLD for l in c["lines"]]
    assert any(l.startswith("known\t") for l in lines) and any(l.startswith("novel\t") for l in lines)
    assert all(10 * c["tied"] <= len(c["lines"]) for c in GOLD) and all(len(c["lines"]) >= 30 for c in GOLD)


@pytest.mark.parametrize("gold", GOLD, ids=[c["name"] for c in GOLD])
def test_restatement_reproduces_the_reference(gold):
    """every line's k-mer, count, distance, known flag and name; the nearest k-mer wherever the minimum is untied"""
    case = INPUTS[gold["name"]]
    assert (case["K"], case["S"]) == (gold["K"], gold["S"])
    assert gold["params"]["fasta"] == digest([case["fasta"]]) and gold["params"]["inputs"] == digest(case["inputs"])
    index = R.Index(case["K"], R.read_fasta(case["fasta"]))
    reads = [s for t in case["inputs"] for s in R.read_fastq(t)]
    assert len(reads) == gold["params"]["reads"]
    rows = R.rows(index, R.count_stops(index, reads, case["S"]))
    key = lambda line: (line.split("\t")[:4], line.split("\t")[5])
    mine = sorted(((R.line_of(case["K"], r), r[6]) for r in rows), key=lambda m: key(m[0]))
    want = sorted(gold["lines"], key=key)
    assert len(mine) == len(want)
    tied = 0
    for (line, is_tied), ref in zip(mine, want):
        assert key(line) == key(ref)
        tied += is_tied
        assert is_tied or line == ref
    assert tied == gold["tied"]
    # the lines come out ordered by name (bytes) and then k-mer
    assert [(r[5], r[1]) for r in rows] == sorted((r[5], r[1]) for r in rows)


# ---- the index ---------------------------------------------------------------------------------------------------------------------
def test_the_trim():
    for seq, want in (("ACGTAAAA", "ACGTAAAA"), ("ACGTAAAAA", "ACGT"), ("ACGTAAAAAA", "ACGT"), ("ACGTaaaaaa", "ACGTaaaaaa"),
                      ("ACGTAAAAAAC", "ACGTAAAAAAC"), ("AAAAAAAAAA", ""), ("ACGaAAAAA", "ACGa"), ("ACGTAAAAAaAAAA", "ACGTAAAAAaAAAA"),
                      ("AAAAAACGAAAAAT", "AAAAAACGAAAAAT"), ("", "")):
        assert R.trim(seq) == want and stopscan.trim_poly_a(seq.encode()) == want.encode(), seq


def write(tmp_path, name, text):
    p = str(tmp_path / name)
    with open(p, "w", newline="") as f:
        f.write(text)
    return p


def test_fasta_parsing_and_the_index(tmp_path):
    """lines joined and stripped, the header line without `>` and blanks as the name, text before the first header dropped; the
    trim on the joined text; transcripts in byte order of their names; a k-mer's anchors; the known stops test p, not p + K - 3"""
    K = 9
    rng = random.Random(5)
    body = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    s1, s2, s3 = body(40) + "TAAGGG", body(30) + "n" + body(24) + "C", body(33)
    text = "ignored\n>zeta  the last \r\n" + s1[:20] + "  \n\t" + s1[20:] + "AAA\nAAA\n\n>Beta\n" + s2 + "AAAA\n>alpha\n" + s3.lower() + "\n>empty\n\n>short\nACGT\n"
    path = write(tmp_path, "tx.fa", text)
    index = stopscan.load_index(path, K)
    ref = R.Index(K, R.read_fasta(text))
    assert index.names == ["Beta", "alpha", "empty", "short", "zeta  the last"] == sorted(ref.kmers)
    assert index.span == [len(s2) + 4, len(s3), 0, 4, len(s1)]
    tk, offs = index.transcript_kmers()
    for t, nm in enumerate(index.names):
        assert tk[int(offs[t]):int(offs[t + 1])].tolist() == sorted(ref.kmers[nm])
    assert index.known_stops().tolist() == sorted(ref.known)
    layout = stopscan.layout_of(index, pad=50)
    starts = stopscan.starts_of(layout)
    assert starts.tolist() == sorted(starts.tolist()) and starts[0] == 50
    assert all(int(b) - int(a) >= 100 for a, b in zip(starts, starts[1:]))
    keys, koffs, ids = anchor_arrays(stopscan._Zones(index), layout)
    got = {}
    for i, x in enumerate(keys.tolist()):
        for a in ids[int(koffs[i]):int(koffs[i + 1])].tolist():
            t = int(np.searchsorted(starts, a, side="right")) - 1
            got.setdefault(x, set()).add((index.names[t], a - int(starts[t])))
    assert got == ref.anchors
    # known: x at p % 3 == 0 ending with a stop, wherever the stop itself lies
    x = R.kmers_with_pos(K, "ACGTACTAA")[0][0]
    assert R.Index(K, [("a", "ACGTACTAA")]).known == {x} and R.Index(K, [("a", "GACGTACTAA")]).known == set()
    assert stopscan.Index(K, [("a", b"ACGTACTAA")]).known_stops().tolist() == [x]
    assert stopscan.Index(K, [("a", b"GACGTACTAA")]).known_stops().tolist() == []


def test_render_and_ham():
    assert stopscan.render(5, 0b1101100011) == R.render(5, 0b1101100011) == "TCGAT"
    assert R.render(27, ((1 << 54) - 1) >> 3) == "AC" + "T" * 25
    assert R.ham(0b0110, 0b0101) == 1 and R.ham(0b0110 >> 3, 0b1110 >> 3) == 1 and R.ham(0b0010 >> 3, 0b0110 >> 3) == 0


# ---- the draw ------------------------------------------------------------------------------------------------------------------------
def test_stop_draw():
    for g in range(50):
        assert synth.stop_draw(17, g, 1) == 0
        f = synth.stop_fraction(17, g)
        assert 0 <= f < (1 << 53) and f == synth.rnd_int(17, synth.T_STOP, g) >> 11
        for n in (2, 3, 7, 1000, (1 << 32) - 1, 1 << 32, (1 << 32) + 1):
            r = synth.stop_draw(17, g, n)
            assert 0 <= r < n and r == (f * n) // (1 << 53)
            assert r == int(np.uint64(synth.rnd(17, synth.T_STOP, g)) >> np.uint64(11)) * n >> 53
    assert synth.T_STOP not in (synth.T_ZONE, synth.T_ALLELE, synth.T_POS, synth.T_LEN, synth.T_STRAND, synth.T_ERR, synth.T_ANON, synth.T_POP)
    assert len({synth.stop_draw(17, g, 1 << 32) for g in range(100)}) == 100 and synth.stop_draw(17, 0, 100) != synth.stop_draw(18, 0, 100)


def test_the_rank_on_both_sides_of_every_boundary():
    frames = {("a", -3, 1): 4, ("a", 5, 0): 1, ("b", 0, 0): 7, ("a", 5, 1): 2}
    order = sorted(frames)
    assert order == [("a", -3, 1), ("a", 5, 0), ("a", 5, 1), ("b", 0, 0)]
    at = 0
    for k in order:
        assert R.pick(frames, at) == k and R.pick(frames, at + frames[k] - 1) == k
        at += frames[k]
    with pytest.raises(AssertionError):
        R.pick(frames, at)
    assert R.pick({("a", 0, 0): 1}, 0) == ("a", 0, 0)
    # names compare as bytes: an upper-case name before a lower-case one, a prefix before its extensions
    assert sorted({("b", 0, 0): 1, ("B", 9, 1): 1, ("Ba", -9, 0): 1}) == [("B", 9, 1), ("Ba", -9, 0), ("b", 0, 0)]


def test_the_rank_is_the_frame_of_the_references_walk():
    """stop.py:133-150 with random.random() = u = fraction / 2^53, on frames and draws as they come"""
    rng = random.Random(11)
    for g in range(3000):
        cnts = [rng.randrange(1, 300) for _ in range(rng.randrange(1, 7))]
        n = sum(cnts)
        v = synth.stop_fraction(17, g) / 9007199254740992.0
        walk = None
        for i, c in enumerate(cnts):
            pv = float(c) / float(n)
            if v < pv:
                walk = i
                break
            v -= pv
        r = synth.stop_draw(17, g, n)
        mine = next(i for i in range(len(cnts)) if r < sum(cnts[:i + 1]))
        assert walk == mine, (g, cnts)


# ---- refusals and the usage text ---------------------------------------------------------------------------------------------------
def test_refusals(tmp_path, monkeypatch):
    case = INPUTS["k27_plain"]
    args = write_case(case, str(tmp_path))
    fa, fq = args[5], args[6]
    code, out, err = run(["stop", fq])
    assert code == 1 and out == "" and "-r FILE" in err
    for k in ("2", "33", "0", "x"):
        code, out, err = run(["stop", "-k", k, "-r", fa, fq])
        assert code == 1 and out == "" and "-k" in err, k
    code, out, err = run(["stop", "-S", "-1", "-r", fa, fq])
    assert code == 1 and out == ""
    code, out, err = run(["stop", "-r", fa, fa])
    assert code == 1 and "FASTQ only" in err
    code, out, err = run(["stop", "-r", fa])
    assert code == 1 and "wrong number of arguments" in err
    twice = write(tmp_path, "twice.fa", ">a x\nACGTACGTAC\n>b\nACGT\n>a x\nGGGG\n")
    code, out, err = run(["stop", "-k", "5", "-r", twice, fq])
    assert code == 1 and out == "" and "two records are named a x" in err
    code, out, err = run(["stop", "-r", str(tmp_path / "missing.fa"), fq])
    assert code == 1 and out == "" and err.startswith("zot stop: ")
    monkeypatch.setenv("WORLD_SIZE", "2")
    code, out, err = run(["stop", "-r", fa, fq])
    assert code == "zot stop: runs on a single GPU for now"


def test_an_axis_of_2_to_the_32_is_refused():
    index = stopscan.Index(25, [("t%d" % i, b"") for i in range(3)])
    index.span = [1 << 31, 1 << 30, (1 << 30) - 3 * 2 * stopscan.PAD - 1]
    with pytest.raises(InputError, match="2\\^32"):
        stopscan.layout_of(index)
    index.span[2] -= 1
    assert stopscan.layout_of(index).total == (1 << 32) - 2


def test_usage_text():
    code, out, err = run(["help", "stop"])
    assert code == 0 and err == ""
    for word in ("zot stop [options] <input>...", "-k K", "-r FILE", "-S SEED", "[default: 27]", "[default: 17]", "dies on import",
                 "counter-based", "-S is new", "ordered by transcript name", "goes to the smallest", "Without -r the command refuses",
                 "Two records of", "FASTA read inputs are refused", "K outside 3..32", "2^32", "longer than 4096", "single GPU"):
        assert word in out, word
    code, out, err = run(["help"])
    assert "\tstop\n" in out
    code, out, err = run(["stop", "-h"])
    assert code == 0 and "zot stop - search for stop codons" in out
