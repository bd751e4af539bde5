"""Both strands rebuilt block by block (ZK_TUNE_STRAND_BLOCKS, strand_blocks.hip) against the mirror sort + merge-path union and the
oracle: the block dedupe with 18 block bits forced on small inputs (ZK_TUNE_DEDUPE_BITS), odd K (the route) and even K (not taken),
blocks that fit a tile, blocks of the counted list or of its mirror image 1.7 and 7 times a tile (declined, cut into sub-tiles by
value), and counts beyond the packed field (the route is not taken).  Which way each call went is read from the profile records:
the copy that writes the mirror words books 16 bytes a canonical k-mer on the route against 24 on the other (the dense copy of the
counted list is not made), and the declined blocks' kernel is one more union record."""
import numpy as np
import pytest

from oracle import zkoracle as zo
from tests import _core_cases as cc
from zotmer_amd import native, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def stream_of(reads):
    return ("".join(r + "\n" for r in reads)).encode()


def _revcomp(k, K):
    k = np.asarray(k, dtype=np.uint64)
    r = np.zeros_like(k)
    for i in range(K):
        r = (r << np.uint64(2)) | (np.uint64(3) - ((k >> np.uint64(2 * i)) & np.uint64(3)))
    return r


def _inputs(K):
    rng = np.random.default_rng(700 + K)
    deep = synth.read_strings(31, 0, 6000, 150, genome=12000, sub_thr=synth.frac32(0.004), n_thr=synth.frac32(0.001))
    def rnd(n):
        return "".join(rng.choice(list("ACGT"), size=n))
    # 14 000 distinct canonical k-mers under one 9-base prefix: one block of the counted list 1.7 times a tile (their mirror images
    # spread over random blocks); the builder is shared with the `dense` input of tests/_core_cases.py
    dense = deep + cc.dense_block(rnd, K)
    # 60 000 under one prefix: 7 times a tile
    big_c = deep + ["AAAAAAAAA" + rnd(K - 9) for _ in range(60000)] * 2
    # 60 000 canonical k-mers that end in GGGGGGGGG: their mirror images all sit in block CCCCCCCCC, 7 times a tile
    big_m = deep + ["A" + rnd(K - 10) + "GGGGGGGGG" for _ in range(60000)] * 2
    # a genome that is one 30-base unit repeated, read with errors: every k-mer sits under one of 60 prefixes
    unit = "".join(rng.choice(list("ACGT"), size=30))
    g = unit * 200
    rep = []
    for _ in range(6000):
        s = rng.integers(0, len(g) - 150)
        r = np.array(list(g[s:s + 150]))
        m = rng.random(150) < 0.01
        r[m] = rng.choice(list("ACGT"), size=int(m.sum()))
        rep.append("".join(r))
    # two letters only: 512 of the 262 144 prefixes hold every k-mer (and the 512 of their reverse complements)
    two = ["".join(rng.choice(list("AC"), size=150)) for _ in range(8000)]
    two = two + two
    # poly-A and a dinucleotide repeat: counts beyond the packed field
    heavy = deep[:1500] + ["A" * 150] * 400 + ["AC" * 75] * 300
    return {"deep": deep, "dense_block": dense, "big_c_block": big_c, "big_m_block": big_m, "repeat30": rep, "two_letters": two,
            "heavy_counts": heavy}


# the route each input takes at odd K: True = block by block with no block declined, "declined" = with declined blocks, False = not
# taken (counts beyond the packed field: at K = 25 and 27), None = as the counts fall (the 30-base repeat: its k-mers' counts exceed
# the field at K = 25 and 27) -- compared with the oracle only
ROUTE = {"deep": True, "two_letters": True, "dense_block": "declined", "big_c_block": "declined", "big_m_block": "declined",
         "repeat30": None, "heavy_counts": False}


@pytest.mark.parametrize("K", [21, 25, 27, 24])
def test_strand_blocks_vs_mirror_union_and_oracle(ctx, K):
    try:
        for name, reads in _inputs(K).items():
            want = zo.kmerize(K, reads)
            wk = np.asarray(want["kmers"], dtype=np.uint64)
            n_can = int(np.count_nonzero(wk <= _revcomp(wk, K)))
            hv, hf = zo.hist(want["counts"])
            want_hist = {int(a): int(b) for a, b in zip(hv, hf)}
            d = ctx.upload_stream(stream_of(reads))
            prof = {}
            for sb in (1, 0):
                ctx.tune(dedupe_bits=18, strand_blocks=sb)
                ctx.profile(True)
                k, c, st = ctx.kmerize(d, K)
                prof[sb] = ctx.profile_read()
                ctx.profile(False)
                assert np.array_equal(k.to_host(), want["kmers"]), (name, K, sb)
                assert np.array_equal(c.to_host(), want["counts"]), (name, K, sb)
                assert st.n_unique == len(want["kmers"]) and st.n_canonical == n_can, (name, K, sb, st.n_canonical, n_can)
                assert list(st.acgt) == want["acgt"]
                assert ctx.hist(c) == want_hist, (name, K, sb)
            sel = {sb: prof[sb].get("select", {}).get("bytes", 0) for sb in (1, 0)}
            uni = {sb: prof[sb].get("union_sum", {}).get("launches", 0) for sb in (1, 0)}
            route = ROUTE[name] if K & 1 else False
            if name == "heavy_counts" and K & 1 and int(np.max(want["counts"])) < (1 << min(64 - 2 * K, 31)):
                route = True          # (K = 21: 22 count bits beside the k-mer -- every count fits, the route is taken)
            if route is False:
                assert sel[1] == sel[0] and uni[1] == uni[0], (name, K, prof)
            elif route is not None:
                assert sel[0] - sel[1] == 8 * n_can, (name, K, prof)          # the route, and the union was not made the other way
                assert uni[1] - uni[0] == (1 if route == "declined" else 0), (name, K, prof)
    finally:
        ctx.tune(dedupe_bits=0, strand_blocks=1)
