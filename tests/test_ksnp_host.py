"""`zot ksnp` without a GPU: the restatement against the reference's fixture (tests/golden/k1_ksnp.json) and against a NumPy
brute force that shares nothing with it, what basics.lev really computes, the command's options and every refusal before it
reaches the device, the round trip of an output file, and the boundary (header, binding, help text)."""
import contextlib
import io
import json
import os
import random
import re

import numpy as np
import pytest

from tests import _ksnp_brute as B
from tests import _ksnp_restatement as R
from tests._ksnp_cases import (DEFAULT, FIXTURE_KS, FIXTURE_MODES, HAMMING, LEVENSHTEIN, around, chain_lows, digest, fixture_cases,
                               geometry, group, random_set)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = {c["name"]: c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "k1_ksnp.json")))}
CASES = fixture_cases()
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from zotmer_amd import native
    return native


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


# ---- the fixture, the restatement, the brute force ------------------------------------------------------------------------------

def test_the_fixture_covers_the_cases():
    assert sorted(GOLD) == sorted(IDS) and len(CASES) == len(FIXTURE_KS) * len(FIXTURE_MODES) == 42
    for c in CASES:
        g = GOLD[c["name"]]
        assert (g["K"], g["mode"], g["d"]) == (c["K"], c["mode"], c["d"])
        assert g["params"]["n"] == len(c["kmers"]) <= 400 and g["params"]["digest"] == digest(c["kmers"])      # the generator still makes the sets
        assert list(c["kmers"]) == sorted(set(c["kmers"])) and c["kmers"][-1] < 4 ** c["K"]
        assert g["kept"] == sorted(set(g["kept"])) and set(g["kept"]) <= set(c["kmers"])
    for K in FIXTURE_KS:
        kept = {(m, d): set(GOLD["k%d_%s_%d" % (K, m, d)]["kept"]) for m, d in FIXTURE_MODES}
        assert kept[(HAMMING, 0)] == set() and kept[(DEFAULT, 0)] and kept[(DEFAULT, 0)] <= kept[(HAMMING, 1)] <= kept[(HAMMING, 2)]
        if K >= 12:
            assert kept[(LEVENSHTEIN, 2)] - kept[(HAMMING, 2)] and len(kept[(LEVENSHTEIN, 2)]) < len(GOLD["k%d_default_0" % K]["kept"]) + 400


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_against_the_fixture(case):
    assert R.run(case["K"], case["mode"], case["d"], list(case["kmers"])) == GOLD[case["name"]]["kept"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_brute_force_against_the_fixture(case):
    assert B.run(case["K"], case["mode"], case["d"], case["kmers"]).tolist() == GOLD[case["name"]]["kept"]


@pytest.mark.parametrize("K", [1, 2, 3, 5, 8, 13, 32])
def test_restatement_against_the_brute_force_on_random_sets(K):
    n = min(400, 4 ** K * 3 // 4) if K < 13 else 1200 // K          # (the table of basics.lev has (K + 1)^2 cells a pair)
    if K < 13:
        xs = random_set(K, n, seed=K)
    else:                # random k-mers of this length share no prefix: three prefixes, the first and the last among them
        _, S, _ = geometry(K)
        rng = np.random.default_rng(K)
        low = rng.integers(0, 1 << 12, size=n, dtype=np.uint64) | (rng.integers(0, 4, size=n, dtype=np.uint64) << np.uint64(S - 2))
        top = np.array([0, 5, (1 << (2 * K - S)) - 1], dtype=np.uint64)[rng.integers(0, 3, size=n)]
        xs = np.unique(low | (top << np.uint64(S)))
    for mode, ds in ((DEFAULT, [0]), (HAMMING, [0, 1, 2, K, 10 ** 6]), (LEVENSHTEIN, [1, 2, K])):
        for d in ds:
            if mode == LEVENSHTEIN and K >= 8 and d == K:
                continue          # (every pair of a group: the table of a few hundred thousand pairs in plain Python)
            assert R.run(K, mode, d, xs.tolist()) == B.run(K, mode, d, xs).tolist(), (K, mode, d)


def test_lev_is_basics_lev():
    """a table that starts from a row of zeros: the end of the second k-mer may be left out, the end of the first may not"""
    K = 6
    kmer = lambda s: sum("ACGT".index(c) << (2 * (K - 1 - i)) for i, c in enumerate(s))
    assert R.lev(K, kmer("ACGTAC"), kmer("ACGTAC")) == 0
    assert R.lev(K, kmer("AAAAAC"), kmer("AAAACG")) == 1          # AAAAAC against the leading AAAAC: one A too many
    assert R.lev(K, kmer("AAAACG"), kmer("AAAAAC")) == 2          # ... but the G of the first k-mer has to go somewhere
    assert R.lev(K, kmer("ACGTAC"), kmer("ACGTAG")) == 1 and R.ham(kmer("ACGTAC"), kmer("ACGTAG")) == 1
    a, b = kmer("ACGTAC"), kmer("CGTACG")
    assert R.ham(a, b) == 6 and R.lev(K, a, b) == 1 and R.lev(K, b, a) == 2
    rng = random.Random(5)
    for _ in range(300):
        K = rng.randrange(1, 33)
        J, S, _ = geometry(K)
        p, u, v = rng.getrandbits(2 * K - S) << S, rng.getrandbits(S), rng.getrandbits(S)
        assert R.lev(K, p | u, p | v) == R.lev(J + 1, u, v) <= R.ham(u, v)          # a common prefix changes nothing
        assert B.lev_pairs(K, np.array([p | u], dtype=np.uint64), np.array([p | v], dtype=np.uint64))[0] == R.lev(K, p | u, p | v)


def test_the_shapes_are_what_they_say():
    for d in (1, 2):
        lows = chain_lows(13, d)[:-1]
        assert len(lows) == (27 if d == 1 else 13) and lows != sorted(lows)
        for i in range(len(lows)):
            for j in range(i + 1, len(lows)):
                assert (R.ham(lows[i], lows[j]) == d) if j == i + 1 else (R.ham(lows[i], lows[j]) > d)
    xs = around(13, 64, seed=1)
    sizes = [b - a for a, b in B.group_slices(13, xs)]
    assert sizes[-3:] == [63, 64, 65] and set(sizes[:-3]) == {1} and len(sizes) - 3 == 4096 - 32
    assert len(np.unique(xs)) == len(xs) and group(13, 5, [7]) == [(5 << 14) | 7]


# ---- the command, before the device -----------------------------------------------------------------------------------------------

def test_parse():
    from zotmer_amd.commands import ksnp as cmd
    assert cmd.parse(["out", "in"]) == (DEFAULT, 0, "out", "in")
    assert cmd.parse(["-H", "2", "out", "in"]) == (HAMMING, 2, "out", "in")
    assert cmd.parse(["-H0", "out", "in"]) == (HAMMING, 0, "out", "in")
    assert cmd.parse(["out", "-L", "1000000", "in"]) == (LEVENSHTEIN, 10 ** 6, "out", "in")


@pytest.mark.parametrize("args", [["-H", "-1", "o", "i"], ["-L", "-3", "o", "i"], ["-H", "1.5", "o", "i"], ["-L", "two", "o", "i"],
                                  ["-H", "1", "-L", "1", "o", "i"], ["-H", "1", "o"], ["o"], [], ["o", "i", "extra"], ["-X", "o", "i"],
                                  ["o", "i", "-H"]])
def test_usage_errors(args, tmp_path):
    code, out, err = run(["ksnp"] + args)
    assert code == 1 and out == "" and "zot ksnp [(-H DIST|-L DIST)] <output> <ref>" in err
    assert not os.path.exists("o")


def write_input(path, K, xs, counts=True, meta=None):
    from zotmer_amd.library import vectors
    from zotmer_amd.library.container import KmerSet
    xs = np.asarray(xs, dtype=np.uint64)
    with KmerSet(str(path), "w") as z:
        if counts:
            vectors.write_kmers_and_counts(z, xs, np.arange(1, len(xs) + 1, dtype=np.uint64))
            z.meta.update({"K": K, "kmers": "kmers", "counts": "counts"})
        else:
            z.add("kmers", vectors.encode_kmers(xs))
            z.meta.update({"K": K, "kmers": "kmers"})
        if meta is not None:
            z.meta = meta
    return str(path)


def test_refusals_come_before_the_device(native, tmp_path, monkeypatch):
    """on a box without a GPU the device context cannot be made: whatever is refused below is refused before it is asked for"""
    from zotmer_amd.library import engine
    asked = []
    monkeypatch.setattr(engine, "context", lambda: asked.append(1) or (_ for _ in ()).throw(AssertionError("the device was asked for")))
    out = str(tmp_path / "out.k")
    good = write_input(tmp_path / "in.k", 5, [1, 2, 3])
    # several processes
    monkeypatch.setenv("WORLD_SIZE", "2")
    code, _, _ = run(["ksnp", out, good])
    assert code == "zot ksnp: runs on a single GPU for now"
    monkeypatch.delenv("WORLD_SIZE")
    # an input without k-mers: dump's message
    bare = write_input(tmp_path / "bare.k", 5, [], meta={"K": 5})
    code, so, err = run(["ksnp", out, bare])
    assert code == 1 and so == "" and err == 'cannot dump "%s" as it contains no k-mers\n' % bare
    assert run(["dump", bare])[2] == err
    # a K this build has no k-mers for
    code, _, err = run(["ksnp", out, write_input(tmp_path / "k33.k", 33, [1, 2])])
    assert code == 1 and "1 <= K <= 32" in err
    # no such file
    with pytest.raises(IOError):
        run(["ksnp", out, str(tmp_path / "missing.k")])
    assert not asked and not os.path.exists(out)
    # ... and a good input is the first thing that asks
    with pytest.raises(AssertionError, match="the device was asked for"):
        run(["ksnp", out, good])
    assert asked == [1] and not os.path.exists(out)


def test_too_many_kmers_is_refused_with_a_message():
    from zotmer_amd.library import ksnp

    class Huge:
        n = (1 << 32) - 1
    with pytest.raises(ksnp.TooManyKmers, match="4294967295 k-mers"):
        ksnp.candidates(None, Huge(), 25)
    assert ksnp.MAX_KMERS == (1 << 32) - 2 and geometry(25) == (12, 26, 24)


def test_output_round_trip(native, tmp_path):
    """the file of an output, written from a host array: this project's readers open it, and it is the reference's layout"""
    from zotmer_amd.library import ksnp, vectors
    from zotmer_amd.library.container import KmerSet
    case = CASES[[c["name"] for c in CASES].index("k25_hamming_1")]
    kept = np.array(GOLD[case["name"]]["kept"], dtype=np.uint64)
    for xs in (kept, kept[:0]):
        path = str(tmp_path / ("out%d.k" % len(xs)))
        ksnp.write_set(path, 25, kmers_bytes=vectors.encode_kmers(xs))
        with KmerSet(path, "r") as z:
            assert z.meta == {"K": 25, "kmers": "kmers"} and sorted(z.toc) == ["__meta__", "kmers"]
            assert np.array_equal(vectors.read_kmers(z), xs)
        code, out, err = run(["dump", path])
        from zotmer_amd.commands.dump import render
        assert err == "" and out.split() == render(25, xs)
        code, out, err = run(["info", path])
        assert err == "" and "25" in out


def test_every_fixture_output_can_be_stored(native):
    """codec64 has no code for a delta of 2^60 or more: the fixture's sets are made so that their outputs have none"""
    from zotmer_amd.library import vectors
    for c in CASES:
        kept = np.array(GOLD[c["name"]]["kept"], dtype=np.uint64)
        assert np.array_equal(vectors.decode_kmers(vectors.encode_kmers(kept)), kept), c["name"]
    with pytest.raises(vectors.CodecError):
        vectors.encode_kmers(np.array([5, 5 + (1 << 60)], dtype=np.uint64))


# ---- the boundary -------------------------------------------------------------------------------------------------------------

def test_header_binding_and_help(native):
    text = open(os.path.join(ROOT, "include", "zotk.h")).read()
    assert "int zk_ksnp_flank(" in text and "int zk_ksnp_components(" in text
    assert "zk_ksnp_flank" in native.SIGNATURES and "zk_ksnp_components" in native.SIGNATURES
    const = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))
    assert (const("ZK_KSNP_WAVE_GROUP"), const("ZK_KSNP_LDS_GROUP"), const("ZK_KSNP_PAIR_TILE")) == \
        (native.KSNP_WAVE_GROUP, native.KSNP_LDS_GROUP, native.KSNP_PAIR_TILE)
    assert (const("ZK_KSNP_HAMMING"), const("ZK_KSNP_LEVENSHTEIN")) == (native.KSNP_HAMMING, native.KSNP_LEVENSHTEIN)
    assert const("ZK_PROF_KSNP_FLANK") == native.Context.PROF_TAGS["ksnp_flank"] and \
        const("ZK_PROF_KSNP_PAIRS") == native.Context.PROF_TAGS["ksnp_pairs"]
    code, out, err = run(["help", "ksnp"])
    assert code == 0 and err == ""
    for words in ("zot ksnp [(-H DIST|-L DIST)] <output> <ref>", "Differences from the reference", "NameError", "usage error",
                  "`zot dump`", "2^32 - 1", "torch.distributed.run", "quadratic"):
        assert words in out, words
    code, out, err = run(["help"])
    assert "\tksnp\n" in out
