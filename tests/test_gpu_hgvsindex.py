"""`zot hgvs-index` on the device: zk_sequence_tally against the plain-Python restatement (tests/_hgvsindex_restatement.py), with
every array in a guarded frame at an element offset (tests/_frames.py), and the command end to end against the reference's
outputs (tests/golden/x1_hgvsindex.json)."""
import contextlib
import ctypes as C
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
from tests._frames import Frame, PLACEMENTS, lead_of
from tests._hgvsindex_cases import make_cases, write_genome

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "x1_hgvsindex.json")
TILE = 4096
KS = [1, 2, 16, 25, 31, 32]
EINVAL = -1
_place = itertools.cycle(PLACEMENTS)


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    from zotmer_amd.library import engine
    yield engine.context()
    engine.close()


def test_header_and_bindings_agree():
    from zotmer_amd import native
    header = open(os.path.join(ROOT, "include", "zotk.h")).read()
    assert int(re.search(r"#define ZK_SEQTALLY_TILE (\d+)", header).group(1)) == native.SEQTALLY_TILE == TILE
    assert int(re.search(r"#define ZK_PROF_SEQ_TALLY (\d+)", header).group(1)) == native.Context.PROF_TAGS["seq_tally"] == 34
    assert "zk_sequence_tally" in native.SIGNATURES


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def bases(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def wrap(seq, width, eol="\n"):
    """the sequence as lines of `width` columns (None: one line without an end)"""
    if width is None:
        return seq
    return "".join(seq[i:i + width] + eol for i in range(0, len(seq), width))


class Table:
    """a bait table of some records, its keys on the host"""

    def __init__(self, ctx, K, records):
        self.K = K
        self.t = ctx.bait_table(ctx.upload_stream("".join(r + "\n" for r in records).encode()), K)
        self.keys = [int(x) for x in self.t.arrays()[0].to_host()] if self.t.n_keys else []
        assert self.keys == R.table_of(K, records)[0]


def call(ctx, table, text, state=(0, 0), before=None, placement=None):
    """one zk_sequence_tally on guarded frames -> (counts, state after, windows, first_gt); the text is unchanged and nothing
    outside the counts is written"""
    placement = placement or next(_place)
    text = bytes(text)
    ft = Frame(ctx, np.frombuffer(text, dtype=np.uint8), lead_of("byte", placement))
    start = np.zeros(len(table.keys), dtype=np.uint64) if before is None else np.asarray(before, dtype=np.uint64)
    fc = Frame(ctx, start, lead_of("u64", placement, output=True))
    st, nw, gt = ctx.sequence_tally(table.t, ft.arr, state, fc.arr, n=len(text))
    assert ft.unchanged() and fc.outside_intact()
    return fc.result(), st, nw, gt


def expect(table, text, state=(0, 0)):
    got, st, nw, gt = R.tally(table.K, bytes(text), table.keys, state)
    return np.array([got.get(x, 0) for x in table.keys], dtype=np.uint64), st, nw, gt


def check(ctx, table, text, state=(0, 0), placement=None):
    c, st, nw, gt = call(ctx, table, text, state, placement=placement)
    wc, wst, wnw, wgt = expect(table, text, state)
    assert np.array_equal(c, wc) and (st, nw, gt) == (wst, wnw, wgt), (table.K, len(text), text[:80])
    return c, st


@functools.lru_cache(maxsize=None)
def sequence_for(K):
    """3 TILE + 5 bases: mostly ACGT, some lower case and U, an N about every 700 bases, a stretch said three times"""
    rng = random.Random(900 + K)
    s = list(bases(rng, 3 * TILE + 5, "ACGTACGTACGTacgtUu"))
    for i in range(350, len(s), 700):
        s[i] = "N"
    rep = s[100:100 + K + 20]
    for at in (TILE - 10, 2 * TILE + 300):
        s[at:at + len(rep)] = rep
    return "".join(s)


def records_for(K, seq):
    """alleles whose k-mers the sequence holds (one across the first tile edge, one the repeated stretch), and some it does not"""
    rng = random.Random(950 + K)
    u = seq.upper().replace("U", "T")
    return [u[100:100 + K + 20], u[TILE - K - 3:TILE + K + 3].replace("N", "A"), u[2 * TILE - 40:2 * TILE + 40], bases(rng, K + 30), "ACGTN", ""]


# ---- against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_lengths_and_line_widths(ctx, K):
    seq = sequence_for(K)
    table = Table(ctx, K, records_for(K, seq))
    assert table.keys
    lengths = sorted({0, 1, max(K - 1, 0), K, K + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5})
    hits = 0
    for n in lengths:
        for width, eol in ((None, ""), (1, "\n"), (7, "\n"), (60, "\n"), (64, "\n"), (60, "\r\n")):
            text = wrap(seq[:n], width, eol)[:n]          # n text bytes: at width 1 every other byte is a line break
            assert len(text) == n
            c, _ = check(ctx, table, text.encode())
            hits += int(c.sum())
    assert hits > 0


def test_content_at_the_tile_edges(ctx):
    K = 25
    rng = random.Random(7)
    seq = bases(rng, 3 * TILE)
    table = Table(ctx, K, [seq[TILE - 40:TILE + 40], seq[2 * TILE - 40:2 * TILE + 40], seq[:60]])
    for edge in (TILE, 2 * TILE):
        for what in ("\n", "\r", "\r\n", "N", ">", " ", "\n\n"):
            for at in (edge - 2, edge - 1, edge):                     # the break (or breaker) just before, on and after the edge
                text = seq[:at] + what + seq[at:2 * TILE + 100]
                check(ctx, table, text.encode())
    # a window whose bases straddle the edge, the line break on the edge; then 300 line breaks inside one window
    text = seq[:TILE - 1] + "\n" + seq[TILE - 1:TILE + 60]
    c, _ = check(ctx, table, text.encode())
    assert c.sum() > 0
    text = seq[:TILE - 12] + "\n" * 150 + "\r\n" * 75 + seq[TILE - 12:TILE + 100]
    c, _ = check(ctx, table, text.encode())
    assert c.sum() >= 40
    # lower case and U are bases; everything else but the line breaks ends a run
    low = seq[:200].lower().replace("t", "u")
    c, _ = check(ctx, table, low.encode())
    assert c.sum() > 0
    for ch in "NnRYxX*-. \t0>@":
        check(ctx, table, (seq[:30] + ch + seq[30:90]).encode())
    check(ctx, table, bytes(range(256)) + seq[:80].encode() + bytes(range(255, -1, -1)))
    # line breaks only: nothing is counted and the state passes through
    for n in (1, 63, 64, 65, TILE, 2 * TILE + 3):
        c, st, nw, gt = call(ctx, table, b"\n" * n, state=(0x1B1B, 7))
        assert not c.any() and (st, nw, gt) == ((0x1B1B, 7), 0, n)
        c, st, nw, gt = call(ctx, table, b"\r\n" * (n // 2) + b"N" + b"\n" * 70, state=(0x1B1B, 7))
        assert (st, nw) == ((0, 0), 0)


def test_contended_adds_and_accumulation(ctx):
    K = 25
    n = 3 * TILE
    table = Table(ctx, K, ["A" * 40, "ACGT" * 10])
    c, st, nw, gt = call(ctx, table, b"A" * n)
    assert int(c[table.keys.index(0)]) == n - K + 1 == nw and int(c.sum()) == nw and st == (0, K - 1)
    c2, _, _, _ = call(ctx, table, b"A" * n, before=c)
    assert np.array_equal(c2, 2 * c)
    # the same call gives the same bits, on counts that start high
    text = wrap("ACGT" * 700 + "A" * 500, 60).encode()
    high = np.full(len(table.keys), (1 << 63) + 5, dtype=np.uint64)
    a, _, _, _ = call(ctx, table, text, before=high, placement="P1")
    b, _, _, _ = call(ctx, table, text, before=high, placement="P3")
    want, _, _, _ = expect(table, text)
    assert np.array_equal(a, b) and np.array_equal(a - high, want) and want.sum() > 2000


@pytest.mark.parametrize("K", [2, 25, 32])
def test_pieces_give_the_whole(ctx, K):
    seq = sequence_for(K)
    table = Table(ctx, K, records_for(K, seq))
    text = wrap(seq[:2 * TILE + 100], 60).encode()
    whole, wst = check(ctx, table, text)
    assert whole.sum() > 0
    for cut in range(TILE - K - 2, TILE + K + 3):
        a, st, nw_a, _ = call(ctx, table, text[:cut])
        b, st, nw_b, _ = call(ctx, table, text[cut:], state=st, before=a)
        assert np.array_equal(b, whole) and st == wst, cut
    # three pieces, both cuts inside a run of line breaks that sits inside a window
    text = (seq[:TILE - 5] + "\n" * 300 + seq[TILE - 5:TILE + 200]).encode()
    whole, wst = check(ctx, table, text)
    a, st, _, _ = call(ctx, table, text[:TILE + 10])
    b, st, _, _ = call(ctx, table, text[TILE + 10:TILE + 200], state=st, before=a)
    c, st, _, _ = call(ctx, table, text[TILE + 200:], state=st, before=b)
    assert np.array_equal(c, whole) and st == wst
    # a piece shorter than the state it gets; pieces of one byte
    text = seq[:3 * K + 5].encode()
    whole, wst = check(ctx, table, text)
    acc, st = np.zeros(len(table.keys), dtype=np.uint64), (0, 0)
    for i in range(len(text)):
        acc, st, _, _ = call(ctx, table, text[i:i + 1], state=st, before=acc)
    assert np.array_equal(acc, whole) and st == wst


def test_first_gt(ctx):
    table = Table(ctx, 4, ["ACGTACGT"])
    for text, want in ((b">abc\nACGT", 0), (b"ACGT\n>x\nAC", 5), (b"ACGT\r>x", 5), (b"AC\r\n>x\n>y", 4), (b"AC>GT", 5), (b"ACGTACGT\n", 9), (b">", 0), (b"", 0),
                       (b"A" * (TILE - 1) + b"\n>" + b"ACGT" * 20, TILE), (b"A" * (TILE - 2) + b"\n>" + b"C" * 20, TILE - 1),
                       (b"A" * (2 * TILE + 7) + b"x>" + b"C" * TILE + b"\r>" + b"G" * 40 + b"\n>", 3 * TILE + 10)):
        c, st, nw, gt = call(ctx, table, text)
        wc, wst, wnw, wgt = expect(table, text)
        assert gt == want == wgt and np.array_equal(c, wc) and (st, nw) == (wst, wnw), text[:20]


def test_degenerate_inputs(ctx):
    K = 5
    table = Table(ctx, K, ["ACGTACG"])
    empty = Table(ctx, K, ["ACGN", "", "N"])
    assert empty.t.n_keys == 0 and not empty.keys
    text = np.frombuffer(b"ACGTACGTAC\nGTNAC", dtype=np.uint8)
    ft = Frame(ctx, text, 7)
    # a table without keys: the counts are not touched (a null pointer is taken), the state still moves
    st, nw, gt = C.c_uint64 * 2, C.c_uint64(0), C.c_uint64(0)
    s = st(0, 0)
    assert ctx.lib.zk_sequence_tally(ctx.h, empty.t.h, ft.arr.ptr, len(text), s, None, C.byref(nw), C.byref(gt)) == 0
    _, wst, wnw, _ = R.tally(K, text.tobytes(), [])
    assert ((s[0], s[1]), nw.value, gt.value) == (wst, wnw, len(text)) == ((0b0001, 2), 8, len(text))
    # n == 0: nothing moves
    fc = Frame(ctx, np.arange(5, 5 + len(table.keys), dtype=np.uint64), 3)
    s = st(0b111001, 3)
    assert ctx.lib.zk_sequence_tally(ctx.h, table.t.h, None, 0, s, fc.arr.ptr, C.byref(nw), C.byref(gt)) == 0
    assert (s[0], s[1], nw.value, gt.value) == (0b111001, 3, 0, 0) and fc.unchanged()
    # a state above its length is cut to it
    s = st(0xFFFF, 1)
    assert ctx.lib.zk_sequence_tally(ctx.h, table.t.h, None, 0, s, fc.arr.ptr, C.byref(nw), C.byref(gt)) == 0 and (s[0], s[1]) == (3, 1)
    good = lambda: st(0, 0)
    for args in ((None, ft.arr.ptr, len(text), good(), fc.arr.ptr, C.byref(nw), C.byref(gt)),
                 (table.t.h, None, len(text), good(), fc.arr.ptr, C.byref(nw), C.byref(gt)),
                 (table.t.h, ft.arr.ptr, len(text), None, fc.arr.ptr, C.byref(nw), C.byref(gt)),
                 (table.t.h, ft.arr.ptr, len(text), good(), None, C.byref(nw), C.byref(gt)),
                 (table.t.h, ft.arr.ptr, len(text), good(), fc.arr.ptr, None, C.byref(gt)),
                 (table.t.h, ft.arr.ptr, len(text), good(), fc.arr.ptr, C.byref(nw), None),
                 (table.t.h, ft.arr.ptr, len(text), st(0, K), fc.arr.ptr, C.byref(nw), C.byref(gt)),
                 (table.t.h, ft.arr.ptr, len(text), st(0, 1 << 40), fc.arr.ptr, C.byref(nw), C.byref(gt))):
        assert ctx.lib.zk_sequence_tally(ctx.h, *args) == EINVAL
    assert ctx.lib.zk_sequence_tally(None, table.t.h, ft.arr.ptr, len(text), good(), fc.arr.ptr, C.byref(nw), C.byref(gt)) == EINVAL
    assert fc.unchanged() and ft.unchanged()
    s = st(0, K - 1)                                       # the longest state there is
    assert ctx.lib.zk_sequence_tally(ctx.h, table.t.h, ft.arr.ptr, len(text), s, fc.arr.ptr, C.byref(nw), C.byref(gt)) == 0
    got, wst, wnw, _ = R.tally(K, text.tobytes(), table.keys, (0, K - 1))
    assert ((s[0], s[1]), nw.value) == (wst, wnw) and wnw == 12 and fc.outside_intact()
    assert np.array_equal(fc.result(), np.array([5 + i + got.get(x, 0) for i, x in enumerate(table.keys)], dtype=np.uint64))


# ---- the command -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    d = tmp_path_factory.mktemp("genome")
    write_genome(str(d))
    return str(d)


def _cli(args):
    from zotmer_amd import cli
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        code = cli.main_inner(args) or 0
    return code, out.getvalue(), err.getvalue()


@pytest.mark.parametrize("name", [c["name"] for c in make_cases()])
def test_command_against_the_reference(ctx, genome, tmp_path, name):
    c = next(c for c in make_cases() if c["name"] == name)
    gold = next(g for g in json.load(open(GOLD)) if g["name"] == name)
    words = list(c["opts"]) + ["-g", genome]
    if c["file"] is not None:
        (tmp_path / "variants.txt").write_text(c["file"])
        words += ["-f", str(tmp_path / "variants.txt")]
    if c["names"] is not None:
        (tmp_path / "names.txt").write_text(c["names"])
        words += ["-n", str(tmp_path / "names.txt")]
    idx = tmp_path / "index.yaml"
    code, out, _ = _cli(["hgvs-index"] + words + [str(idx)] + c["variants"])
    assert code == 0 and out == "" and idx.read_text() == gold["index"]
    code, out, _ = _cli(["hgvs-index", "-T"] + words + c["variants"])
    assert code == 0 and out == gold["test"]
    code, small, err = _cli(["hgvs-index", "-T", "-v", "-m", "1"] + words + c["variants"])
    assert code == 0 and small == out
    if gold["test"] != "{}\n":
        assert err.count("scanning ") == 24


def test_batches_cut_inside_the_header_and_the_lines(ctx, tmp_path):
    """tally_file with batches of a few bytes: the header, the body and a second record all straddle batches"""
    from zotmer_amd.library import hgvsindex
    rng = random.Random(11)
    seq = "".join(">" if i % 37 == 5 else ch for i, ch in enumerate(bases(rng, 500)))      # '>' inside the lines: where a batch starts with one
    K = 9                                                                                  # it is no header
    table = Table(ctx, K, [seq[43:79], seq[302:338]])
    body = wrap(seq, 60)
    assert not any(line.startswith(">") for line in body.split("\n"))
    (tmp_path / "a.fa").write_text("junk line\n\n>first record with a long header line\n" + body + ">second\n" + seq[43:79] + "\n")
    want, _, nw, _ = expect(table, body.encode())
    for batch in (16, 17, 64, 100, 1 << 20):
        counts = ctx.upload(np.zeros(len(table.keys), dtype=np.uint64))
        stats = hgvsindex.new_stats()
        hgvsindex.tally_file(ctx, table.t, str(tmp_path / "a.fa"), counts, batch, stats)
        assert np.array_equal(counts.to_host(), want) and stats["windows"] == nw, batch
