"""`zot hgvs-gen` on the device: zk_hgvs_draw against the restatement (tests/_hgvsgen_restatement.py) bit for bit, zk_hgvs_render
against the reference's lines (tests/golden/g1_hgvsgen.json) and the restatement's byte for byte, the capacity contract in
guarded buffers, offset views, the refusals, the command against the restatement's text, and the chain hgvs-gen -> hgvs-index ->
spikein -> hgvs-find."""
import contextlib
import io
import json
import os

import numpy as np
import pytest

from tests import _hgvsgen_cases as cases
from tests import _hgvsgen_restatement as R
from tests import _spikein_cases as genome
from zotmer_amd import native, synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 0xA5
RW = 6
TAB, HEADS, DIRECT = 1, 2, 4
ALPHABET = np.frombuffer(b"ACGTACGTACGTacgtNn*-RyU.", dtype=np.uint8)      # upper and lower case, N, and bytes that are no base
LONG_LINE, TILE_BYTES, TILE_ROWS = 256, 32768, 256                        # ZK_HGVS_LONG_LINE, ZK_HGVS_TILE_BYTES, rows of a workgroup


@pytest.fixture(scope="module")
def ctx():
    from zotmer_amd.library import engine
    yield engine.context()
    engine.close()


def window_text(seed, n):
    """n bytes of ALPHABET as a str (latin-1)"""
    return ALPHABET[(synth.rnd(seed, 1, np.arange(n, dtype=np.uint64)) % np.uint64(len(ALPHABET))).astype(np.intp)].tobytes().decode("latin-1")


def pool_of(items):
    offs = np.zeros(len(items) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in items])
    return np.frombuffer(b"".join(items), dtype=np.uint8), offs


class Zones:
    """zones [(accession, s, e, name, window)] with their variant counts, as the arrays of the two entries"""

    def __init__(self, ctx, zones, counts):
        self.ctx, self.zones, self.counts = ctx, zones, list(counts)
        at, rows = 0, []
        for acc, s, e, name, w in zones:
            assert len(w) == e - s + 1
            rows += [at, s, e]
            at += len(w)
        self.first = [sum(self.counts[:k]) for k in range(len(zones) + 1)]
        self.n = self.first[-1]
        # a name is left empty where it repeats the name of the zone with variants before it
        names, prev = [], None
        for (acc, s, e, name, w), n in zip(zones, self.counts):
            names.append(name.encode() if n and name != prev else b"")
            prev = name if n else prev
        self.heads = [bool(x) for x in names]
        text = np.frombuffer("".join(z[4] for z in zones).encode("latin-1"), dtype=np.uint8)
        accs, acc_offs = pool_of([z[0].encode() for z in zones])
        nm, nm_offs = pool_of(names)
        self.host = dict(text=text, zones=np.asarray(rows, dtype=np.uint64), first=np.asarray(self.first, dtype=np.uint64), accs=accs, acc_offs=acc_offs,
                         names=nm, name_offs=nm_offs)
        self.dev = {k: ctx.upload(v) for k, v in self.host.items()}

    def zone_of(self, v):
        return next(z for z in range(len(self.zones)) if self.first[z] <= v < self.first[z + 1])

    def base_at(self, z):
        acc, s, e, name, w = self.zones[z]
        return lambda lo, hi: w[lo - s:hi - s]

    # ---- draw ----
    def draw_args(self, P, seed, first, count):
        d = self.dev
        geom = self.ctx.upload(np.asarray((P.QD + P.QI + P.QU) or [0], dtype=np.uint64))
        return (d["text"], d["zones"], d["first"], P.thr, geom, [len(P.QD), len(P.QI), len(P.QU)], P.mix, seed, first, count)

    def draw(self, P, seed, first=0, count=None):
        count = self.n - first if count is None else count
        rows, pool = self.ctx.hgvs_draw(*self.draw_args(P, seed, first, count))
        return rows.to_host().tolist(), pool.to_host().tobytes()

    def want_draw(self, P, seed, first=0, count=None):
        """the restatement's rows of the variants [first, first + count) -> (words, pool, [(zone, row)])"""
        count = self.n - first if count is None else count
        words, pool, rows = [], b"", []
        for v in range(first, first + count):
            z = self.zone_of(v)
            acc, s, e, name, w = self.zones[z]
            row = R.draw(seed, v, s, e, w, P)
            words += [row[0], z, row[1], row[2], row[3], len(pool)]
            pool += row[4].encode()
            rows.append((z, row))
        return words, pool, rows

    # ---- render ----
    def render_args(self, rows, pool, first, flags):
        d = self.dev
        return (rows, pool, d["text"], d["zones"], d["accs"], d["acc_offs"], d["names"], d["name_offs"], d["first"], first, flags)

    def render(self, rows, pool, first=0, flags=0):
        return self.ctx.hgvs_render(*self.render_args(rows, pool, first, flags)).to_host().tobytes()

    def want_lines(self, rows, first, flags):
        """rows: [(zone, row)] of the variants first, first + 1, ... -> their lines, a `#` line joined to the line it precedes"""
        out = []
        for i, (z, row) in enumerate(rows):
            acc = self.zones[z][0]
            text = R.line(acc, row, self.base_at(z), bool(flags & TAB)) + "\n"
            if (flags & HEADS) and first + i == self.first[z] and self.heads[z]:
                text = "# %s : %s\n" % (acc, self.zones[z][3]) + text
            out.append(text.encode("latin-1"))
        return out


def words_of(rows):
    """[(zone, (kind, p, q, m, bases))] -> (row words, pool)"""
    words, pool = [], b""
    for z, (kind, p, q, m, b) in rows:
        words += [kind, z, p, q, m, len(pool)]
        pool += b.encode()
    return np.asarray(words, dtype=np.uint64), np.frombuffer(pool, dtype=np.uint8)


def draw_zones(ctx):
    """zones of 1, 2, 63, 64, 65 and 4097 bases, one of them empty of variants, one all N but one base, one in lower case, one
    past 2^32; small zones so that p + l crosses e all the time"""
    big = 1 << 32
    lower = "".join(c for c in window_text(5, 400).lower() if c in "acgt")[:90]
    zones = [("chr1", 7, 7, "one", "g"),
             ("chr1", 20, 21, "two", "Na"),
             ("chr1", 100, 162, "z63", window_text(1, 63)),
             ("chr1", 1000, 1063, "z63", window_text(2, 64)),
             ("chr1", 5000, 5064, "none", window_text(3, 65)),
             ("chr2", 99990, 99990 + 4096, "wide", window_text(4, 4097)),
             ("chr2", 200000, 200299, "enn", "N" * 211 + "t" + "n" * 88),
             ("chr3.1", 300, 389, "lower", lower),
             ("chrX", big - 30, big + 40, "far", window_text(6, 71))]
    counts = [40, 60, 300, 300, 0, 1400, 300, 300, 300]
    return Zones(ctx, zones, counts)


ALL_P = dict(probs=(1, 1, 1, 1, 1, 1, 1), D=1.5, I=1.5, U=3.0)


@pytest.fixture(scope="module")
def long_run(ctx):
    """3000 variants of all types over the zones above and the restatement's rows, computed once"""
    zs = draw_zones(ctx)
    P = R.Params(**ALL_P)
    words, pool, rows = zs.want_draw(P, 91)
    return zs, P, 91, words, pool, rows


# ---- zk_hgvs_draw ------------------------------------------------------------------------------------------------------------
def test_three_thousand_variants_and_the_same_call_twice(long_run):
    zs, P, seed, words, pool, rows = long_run
    assert zs.n == 3000 and len(words) == RW * 3000
    got = zs.draw(P, seed)
    assert got == (words, pool)
    assert zs.draw(P, seed) == got
    kinds = [r[0] for _, r in rows]
    assert set(kinds) == set(range(7))
    # what the zones are there for: the walk round the zone, positions clamped at e, zones of one base, positions past 2^32
    enn = [r for z, r in rows if z == 6]
    assert all(r[1] == 200211 for r in enn if r[0] == R.SUB) and any(r[0] == R.SUB for r in enn)
    assert any(r[2] == zs.zones[z][2] and r[2] - r[1] < 2 and r[0] in (R.DEL, R.DUP, R.DELINS, R.AND) for z, r in rows)
    assert all(r[1] == r[2] == 7 for z, r in rows if z == 0) and any(r[1] > 1 << 32 for z, r in rows)
    assert any(len(r[4]) > 1 for _, r in rows if r[0] == R.INS)


@pytest.mark.parametrize("first,count", [(0, 1), (39, 1), (40, 1), (2999, 1), (7, 63), (350, 64), (699, 65), (0, 0), (3000, 0)])
def test_counts_and_firsts(long_run, first, count):
    zs, P, seed, words, pool, rows = long_run
    w, p, _ = zs.want_draw(P, seed, first, count)
    assert zs.draw(P, seed, first, count) == (w, p)


def test_a_run_cut_anywhere_equals_one_call(long_run):
    zs, P, seed, words, pool, rows = long_run
    cuts = [0, 1, 64, 65, 700, 1299, 1301, 2222, 2999, 3000]
    got_words, got_pool = [], b""
    for a, b in zip(cuts, cuts[1:]):
        w, p = zs.draw(P, seed, a, b - a)
        got_words += [x + (len(got_pool) if k % RW == 5 else 0) for k, x in enumerate(w)]      # the pool offsets restart in every call
        got_pool += p
    assert got_words == words and got_pool == pool


@pytest.mark.parametrize("kind", range(7), ids=R.KINDS)
def test_each_type_alone(ctx, kind):
    zs = Zones(ctx, draw_zones(ctx).zones[:4] + draw_zones(ctx).zones[7:], [10, 20, 40, 30, 20, 10])
    P = R.Params(probs=[1.0 if k == kind else 0.0 for k in range(7)])
    w, p, rows = zs.want_draw(P, 1000 + kind)
    assert {r[0] for _, r in rows} == {kind}
    assert zs.draw(P, 1000 + kind) == (w, p)


@pytest.mark.parametrize("D,I,U", [(1.0, 2.0, 1.0), (2.0, 1.0, 1.5), (1.0, 1.0, 1.0), (40.0, 40.0, 40.0)])
def test_means(ctx, D, I, U):
    """a mean of 1 is an empty table; -D 1 -I 1 where neither delins nor `and` can be drawn; 40: tables of some 750 entries, and
    insertions of more than 32 bases, which take a second word of the base draws"""
    zs = Zones(ctx, draw_zones(ctx).zones[2:6], [50, 50, 0, 300])
    probs = (1, 1, 1, 0, 1, 1, 0) if D * I == 1.0 else (1, 1, 1, 1, 1, 1, 1)
    P = R.Params(probs=probs, D=D, I=I, U=U)
    w, p, rows = zs.want_draw(P, 17)
    assert zs.draw(P, 17) == (w, p)
    if I == 40.0:
        assert P.W > 1 and any(r[3] > 32 for _, r in rows if r[0] == R.INS) and len(P.QD) > 700
    if D == 1.0:
        assert P.QD == [] and all(r[2] - r[1] <= 1 for _, r in rows if r[0] == R.DEL)


# ---- zk_hgvs_render ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "g1_hgvsgen.json")) as f:
        return [c for c in json.load(f) if not c["error"]]


def golden_zones(ctx, case):
    """the zones of the case's BED that hold lines, in output order, and the rows its -T lines parse back into"""
    zl = R.zone_list(R.read_bed(case["bed"]))
    per = [[] for _ in zl]
    for text in case["lines"]:
        if text.startswith("# "):
            continue
        acc, row = R.parse_line(text)
        z, = [k for k, (c, s, e, _) in enumerate(zl) if c == acc and s <= row[1] <= row[2] <= e]
        per[z].append(row)
    zones = [(c, s, e, nm, genome.GENOME[c][s:e + 1]) for c, s, e, nm in zl]
    return Zones(ctx, zones, [len(x) for x in per]), [(z, row) for z, x in enumerate(per) for row in x]


def test_golden_rows_give_the_references_lines(ctx, golden):
    total = 0
    for case in golden:
        zs, rows = golden_zones(ctx, case)
        words, pool = words_of(rows)
        d_rows, d_pool = ctx.upload(words), ctx.upload(pool)
        want = "".join(l + "\n" for l in case["lines"]).encode("latin-1")
        assert zs.render(d_rows, d_pool, 0, TAB | HEADS) == want, case["name"]
        assert zs.render(d_rows, d_pool, 0, TAB | HEADS | DIRECT) == want, case["name"]
        plain = "".join(l.split("\t")[6] + "\n" for l in case["lines"] if not l.startswith("#")).encode("latin-1")
        assert zs.render(d_rows, d_pool, 0, 0) == plain, case["name"]
        total += len(rows)
    assert total > 400


@pytest.mark.parametrize("flags", [0, TAB, HEADS, TAB | HEADS, TAB | HEADS | DIRECT])
def test_drawn_rows_give_the_restatements_lines(ctx, long_run, flags):
    zs, P, seed, words, pool, rows = long_run
    d_rows, d_pool = ctx.upload(np.asarray(words, dtype=np.uint64)), ctx.upload(np.frombuffer(pool, dtype=np.uint8))
    lines = zs.want_lines(rows, 0, flags)
    got = zs.render(d_rows, d_pool, 0, flags)
    assert got == b"".join(lines)
    if flags & HEADS:
        assert got.count(b"# ") == 7 and b"# chr1 : z63\n" in got and got.count(b": z63\n") == 1      # the second z63 repeats the name
    # a range of rows of a run: row 0 is variant `first`
    for a, b in ((0, 1), (39, 41), (40, 296), (41, 297), (339, 340), (340, 341), (2990, 3000)):
        part = zs.render(d_rows.view(RW * (b - a), RW * a), d_pool, a, flags)
        assert part == b"".join(zs.want_lines(rows[a:b], a, flags)), (a, b)


def test_decimal_lengths_change_inside_a_run(ctx):
    """positions across 9/10, 99/100, 99999/100000 and 2^32, every kind at every position"""
    big = 1 << 32
    spans = [(3, 14), (95, 104), (99990, 100009), (big - 6, big + 5), (9999999999 - 3, 9999999999 + 4)]
    zones = [("c%d" % k, s, e, "n%d" % k, window_text(40 + k, e - s + 1)) for k, (s, e) in enumerate(spans)]
    rows = []
    for z, (acc, s, e, name, w) in enumerate(zones):
        for p in range(s, e + 1):
            q = min(p + 1 + (p & 1), e)
            m = 1 + (p % 11)
            b = R.bases(z, p, m, 1)
            rows += [(z, (R.SUB, p, p, 1, "ACGT"[p & 3])), (z, (R.DEL, p, q, 0, "")), (z, (R.INS, p, p, m, b)), (z, (R.DELINS, p, q, m, b)),
                     (z, (R.DUP, p, q, 0, "")), (z, (R.ANI, p, p, 9 + p % 3, "")), (z, (R.AND, p, q, 99 + p % 3, ""))]
    rows.sort(key=lambda r: r[0])
    zs = Zones(ctx, zones, [sum(1 for r in rows if r[0] == z) for z in range(len(zones))])
    words, pool = words_of(rows)
    d_rows, d_pool = ctx.upload(words), ctx.upload(pool)
    for flags in (0, TAB | HEADS):
        want = b"".join(zs.want_lines(rows, 0, flags))
        assert zs.render(d_rows, d_pool, 0, flags) == want
    text = want.decode()
    for word in ("g.9_10ins", "g.9_10del", "g.99_100dup", "g.99999_100000ins", "g.100000_100002delins", "g.99999_100000del", "g.4294967296_4294967297ins",
                 "g.4294967295_4294967296del", "\t4294967295\t4294967298\t", "g.9999999999_10000000000ins", "ins9\n", "ins10\n", "delins99\n", "delins100\n"):
        assert word in text, word


def long_line_rows(acc_zone=0):
    """dups and delins whose -T lines run from well below ZK_HGVS_LONG_LINE to well above it, one byte at a time"""
    rows = []
    for n in range(1, 140):
        rows.append((acc_zone, (R.DELINS, 10000, 10000 + n, 60, R.bases(1, n, 60, 2))))      # 190 + n bytes or so
        rows.append((acc_zone, (R.DUP, 20000, 20000 + n, 0, "")))
        rows.append((acc_zone, (R.AND, 10000 + n, 10000 + n, 150 + n, "")))
    return rows


def test_lines_on_either_side_of_the_long_line_bound(ctx):
    zones = [("chrL", 10000, 49999, "long", window_text(9, 40000))]
    rows = long_line_rows()
    zs = Zones(ctx, zones, [len(rows)])
    words, pool = words_of(rows)
    d_rows, d_pool = ctx.upload(words), ctx.upload(pool)
    for flags in (TAB, TAB | HEADS, 0, TAB | DIRECT):
        lines = zs.want_lines(rows, 0, flags)
        if flags & TAB:
            lens = {len(l) for l in lines}
            assert {LONG_LINE - 1, LONG_LINE, LONG_LINE + 1, LONG_LINE + 2} <= lens and min(lens) < 200 and max(lens) > 400
            kinds = {(rows[i][1][0], len(l) > LONG_LINE) for i, l in enumerate(lines)}
            assert kinds == {(k, w) for k in (R.DELINS, R.DUP, R.AND) for w in (False, True)}
        assert zs.render(d_rows, d_pool, 0, flags) == b"".join(lines)


def test_tiles_on_either_side_of_the_lds_bound(ctx):
    """tiles of 256 rows whose text is exactly ZK_HGVS_TILE_BYTES, one byte more, far more, and small; the long row that sets a
    tile's size is written by a wave, into LDS in the first tile and in place in the second"""
    zones = [("chrT", 10000, 49999, "tile", window_text(10, 40000))]
    zs0 = Zones(ctx, zones, [1])
    short = [(0, (R.SUB, 10000 + 7 * k, 10000 + 7 * k, 1, "ACGT"[k & 3])) for k in range(TILE_ROWS - 1)]

    def tile(total):
        """255 substitutions and one delins whose deleted stretch makes the tile's -T text `total` bytes"""
        rest = total - sum(len(l) for l in zs0.want_lines(short, 1, TAB))
        for n in range(1, 39000):
            row = (0, (R.DELINS, 10001, 10001 + n, 3, "ACG"))
            if len(zs0.want_lines([row], 1, TAB)[0]) == rest:
                return short[:100] + [row] + short[100:]
        raise AssertionError(total)
    huge = [(0, (R.DUP, 10000 + k, 24000 + k, 0, "")) for k in range(3)]
    rows = tile(TILE_BYTES) + tile(TILE_BYTES + 1) + (short + [huge[0]]) + (huge[1:] + short[:50])
    zs = Zones(ctx, zones, [len(rows)])
    words, pool = words_of(rows)
    d_rows, d_pool = ctx.upload(words), ctx.upload(pool)
    lines = zs.want_lines(rows, 0, TAB)
    sizes = [sum(len(l) for l in lines[t:t + TILE_ROWS]) for t in range(0, len(rows), TILE_ROWS)]
    assert sizes[:2] == [TILE_BYTES, TILE_BYTES + 1] and sizes[2] > TILE_BYTES + 8000 and sizes[3] > TILE_BYTES and len(sizes) == 4
    want = b"".join(lines)
    assert zs.render(d_rows, d_pool, 0, TAB) == want
    assert zs.render(d_rows, d_pool, 0, TAB | DIRECT) == want
    # the same tiles at every phase of the output address
    for front in (1, 2, 7, 15, 16, 29):
        out = guarded(ctx, front + len(want) + 40)
        nb, fit = ctx.hgvs_render_into(*zs.render_args(d_rows, d_pool, 0, TAB), out.view(len(want), front))
        h = out.to_host()
        assert (nb, fit) == (len(want), True) and h[front:front + nb].tobytes() == want, front
        assert np.all(h[:front] == GUARD) and np.all(h[front + nb:] == GUARD), front


# ---- capacity, views, refusals -------------------------------------------------------------------------------------------------
def guarded(ctx, n, dtype=np.uint8):
    return ctx.upload(np.full(n, GUARD if dtype == np.uint8 else 0xA5A5A5A5A5A5A5A5, dtype=dtype))


G64 = 0xA5A5A5A5A5A5A5A5


@pytest.mark.parametrize("front", [0, 1, 7, 13])
def test_draw_capacities_in_guarded_buffers(long_run, front):
    """capacities one short of, equal to and beyond the need; the outputs at odd offsets of larger arrays"""
    zs, P, seed, words, pool, rows = long_run
    ctx = zs.ctx
    first, count = 330, 70
    w, p, _ = zs.want_draw(P, seed, first, count)
    need = (count, len(p))
    assert need[1] > 20
    PAD = 64
    for c1, c2 in ((0, 0), (need[0] - 1, need[1]), (need[0], need[1] - 1), (need[0] - 1, need[1] - 1), (1, 1), need, (need[0] + 9, need[1] + PAD)):
        b_rows, b_pool = guarded(ctx, RW * (front + need[0] + PAD), np.uint64), guarded(ctx, front + need[1] + PAD)
        nb, fit = ctx.hgvs_draw_into(*zs.draw_args(P, seed, first, count), b_rows.view(RW * c1, RW * front), b_pool.view(c2, front))
        assert nb == need and fit == (c1 >= need[0] and c2 >= need[1]), (c1, c2)
        hr, hp = b_rows.to_host(), b_pool.to_host()
        assert np.all(hr[:RW * front] == G64) and np.all(hr[RW * (front + (need[0] if fit else c1)):] == G64), (c1, c2)
        assert np.all(hp[:front] == GUARD) and np.all(hp[front + (need[1] if fit else c2):] == GUARD), (c1, c2)
        if fit:
            assert hr[RW * front:RW * (front + need[0])].tolist() == w and hp[front:front + need[1]].tobytes() == p
    assert zs.draw(P, seed, first, count) == (w, p)      # the context is as usable as before


@pytest.mark.parametrize("front", [0, 1, 7, 13])
def test_render_capacities_in_guarded_buffers(long_run, front):
    zs, P, seed, words, pool, rows = long_run
    ctx = zs.ctx
    first, count = 20, 600                       # three tiles, the `#` lines of three zones
    d_rows = ctx.upload(np.asarray(words[RW * first:RW * (first + count)], dtype=np.uint64))
    d_pool = ctx.upload(np.frombuffer(pool, dtype=np.uint8))
    want = b"".join(zs.want_lines(rows[first:first + count], first, TAB | HEADS))
    need, PAD = len(want), 64
    for flags in (TAB | HEADS, TAB | HEADS | DIRECT):
        for cap in (0, 1, need - 1, need, need + 9):
            out = guarded(ctx, front + need + PAD)
            nb, fit = ctx.hgvs_render_into(*zs.render_args(d_rows, d_pool, first, flags), out.view(cap, front))
            assert nb == need and fit == (cap >= need), cap
            h = out.to_host()
            assert np.all(h[:front] == GUARD) and np.all(h[front + (need if fit else cap):] == GUARD), cap
            if fit:
                assert h[front:front + need].tobytes() == want


def test_inputs_at_odd_offsets(long_run):
    zs, P, seed, words, pool, rows = long_run
    ctx, h = zs.ctx, zs.host
    big_text = ctx.upload(np.concatenate([np.full(3, GUARD, np.uint8), h["text"], np.full(5, GUARD, np.uint8)]))
    big_zones = ctx.upload(np.concatenate([np.zeros(1, np.uint64), h["zones"]]))
    big_first = ctx.upload(np.concatenate([np.zeros(5, np.uint64), h["first"]]))
    big_geom = ctx.upload(np.asarray([0, 0, 0] + P.QD + P.QI + P.QU, dtype=np.uint64))
    text, zones, first = big_text.view(len(h["text"]), 3), big_zones.view(len(h["zones"]), 1), big_first.view(len(h["first"]), 5)
    a, n = 1390, 200
    d_rows, d_pool = ctx.hgvs_draw(text, zones, first, P.thr, big_geom.view(big_geom.n - 3, 3), [len(P.QD), len(P.QI), len(P.QU)], P.mix, seed, a, n)
    w, p, part = zs.want_draw(P, seed, a, n)
    assert (d_rows.to_host().tolist(), d_pool.to_host().tobytes()) == (w, p)
    big_rows = ctx.upload(np.concatenate([np.zeros(1, np.uint64), np.asarray(w, dtype=np.uint64)]))
    big_pool = ctx.upload(np.concatenate([np.full(3, GUARD, np.uint8), np.frombuffer(p, dtype=np.uint8)]))
    big_accs = ctx.upload(np.concatenate([np.full(1, GUARD, np.uint8), h["accs"]]))
    big_names = ctx.upload(np.concatenate([np.full(7, GUARD, np.uint8), h["names"]]))
    got = ctx.hgvs_render(big_rows.view(len(w), 1), big_pool.view(len(p), 3), text, zones, big_accs.view(len(h["accs"]), 1), zs.dev["acc_offs"],
                          big_names.view(len(h["names"]), 7), zs.dev["name_offs"], first, a, TAB | HEADS)
    assert got.to_host().tobytes() == b"".join(zs.want_lines(part, a, TAB | HEADS))


def refused(call):
    with pytest.raises(native.ZotkError) as e:
        call()
    assert e.value.code == native.ZK_EINVAL, e.value


def test_draw_refusals_leave_the_outputs_alone(ctx):
    zones = [("c", 100, 199, "a", window_text(1, 100)), ("c", 300, 399, "enn", "Nn*-" * 25)]
    zs = Zones(ctx, zones, [50, 50])
    P = R.Params(**ALL_P)
    subs = R.Params(probs=(1, 0, 0, 0, 0, 0, 0))
    geom = ctx.upload(np.asarray(P.QD + P.QI + P.QU, dtype=np.uint64))
    gn = [len(P.QD), len(P.QI), len(P.QU)]
    d = zs.dev

    def call(text=d["text"], table=d["zones"], first_var=d["first"], thr=P.thr, mix=P.mix, first=0, count=50, geom=geom, geom_n=gn):
        bufs = (guarded(ctx, RW * 128, np.uint64), guarded(ctx, 512))
        refused(lambda: ctx.hgvs_draw_into(text, table, first_var, thr, geom, geom_n, mix, 5, first, count, *bufs))
        assert np.all(bufs[0].to_host() == G64) and np.all(bufs[1].to_host() == GUARD)
    call(first=60, count=41)                                            # a variant that no zone holds
    call(first=100, count=1)
    call(first_var=ctx.upload(np.asarray([10, 50, 100], dtype=np.uint64)), first=5, count=10)
    call(table=ctx.upload(np.asarray([0, 100, 99, 100, 300, 399], dtype=np.uint64)))       # e < s
    call(table=ctx.upload(np.asarray([101, 100, 199, 100, 300, 399], dtype=np.uint64)), first=0, count=10)      # a window that leaves the text
    call(text=d["text"].view(150), first=50, count=10)
    call(thr=P.thr[:3] + [(1 << 32) + 1] * 4)                           # a threshold above 2^32
    call(thr=[5, 4] + [1 << 32] * 5)                                    # ... out of order
    call(thr=[0, 1, 2, 3, 4, 5, 6])                                     # ... the last is not 2^32
    call(mix=(1 << 32) + 1)
    call(first=1 << 40, count=1)
    call(first=0, count=1 << 40)
    call(geom=ctx.upload(np.zeros(65537, dtype=np.uint64)), geom_n=[65537, 0, 0])      # a table beyond ZK_HGVS_TABLE_MAX
    call(thr=subs.thr, first=50, count=1)                               # a sub in a zone without a base of ACGT
    # ... which the other types do not mind; and the context is as usable as before
    dels = R.Params(probs=(0, 1, 1, 0, 0, 0, 0))
    assert zs.draw(dels, 5, 50, 50)[0] == zs.want_draw(dels, 5, 50, 50)[0]
    assert zs.draw(P, 5, 0, 50) == zs.want_draw(P, 5, 0, 50)[:2]
    # no variants: nothing is written, whatever the tables
    bufs = (guarded(ctx, RW * 8, np.uint64), guarded(ctx, 64))
    assert ctx.hgvs_draw_into(*zs.draw_args(P, 5, 100, 0), *bufs) == ((0, 0), True)
    assert np.all(bufs[0].to_host() == G64) and np.all(bufs[1].to_host() == GUARD)


def test_render_refusals_leave_the_output_alone(ctx):
    zones = [("c", 100, 199, "a", window_text(1, 100)), ("dd", 300, 399, "b", window_text(2, 100))]
    good = [(0, (R.SUB, 150, 150, 1, "A")), (0, (R.INS, 160, 160, 3, "ACG")), (1, (R.DELINS, 310, 312, 2, "TT")), (1, (R.AND, 320, 321, 5, ""))]
    zs = Zones(ctx, zones, [2, 2])
    words, pool = words_of(good)
    d_pool = ctx.upload(pool)
    want = b"".join(zs.want_lines(good, 0, TAB | HEADS))
    assert zs.render(ctx.upload(words), d_pool, 0, TAB | HEADS) == want

    def call(change=None, flags=TAB | HEADS, first=0, **kw):
        w = words.copy()
        for at, value in (change or {}).items():
            w[at] = value
        out = guarded(ctx, 1024)
        args = list(zs.render_args(ctx.upload(w), d_pool, first, flags))
        for k, v in kw.items():
            args[dict(pool=1, text=2, table=3, acc_offs=5, name_offs=7)[k]] = v
        refused(lambda: ctx.hgvs_render_into(*args, out))
        assert np.all(out.to_host() == GUARD)
    call({0: 7})                                 # an unknown kind
    call({1: 2})                                 # a zone beyond the table
    call({2: 99})                                # p < s
    call({RW * 2 + 3: 400})                      # q > e
    call({RW * 2 + 2: 313})                      # q < p
    call({3: 151})                               # a sub with q != p
    call({4: 2})                                 # ... with m != 1
    call({RW + 4: 0})                            # an ins of nothing
    call({RW * 3 + 4: 1 << 40})                  # an `and` of 2^40
    call({RW + 5: len(pool) - 2})                # a pool range that leaves the pool
    call({5: len(pool)})
    call(pool=d_pool.view(3))
    call(text=zs.dev["text"].view(199))          # a window that leaves the text
    call(table=ctx.upload(np.asarray([0, 100, 199, 100, 399, 300], dtype=np.uint64)))
    call(acc_offs=ctx.upload(np.asarray([0, 2, 1], dtype=np.uint64)))
    call(acc_offs=ctx.upload(np.asarray([0, 1, 4], dtype=np.uint64)))
    call(name_offs=ctx.upload(np.asarray([0, 1, 3], dtype=np.uint64)))
    call(flags=8)
    call(first=1 << 40)
    # ... the name offsets are not read without the flag; no rows: nothing is written
    assert ctx.hgvs_render(ctx.upload(words), d_pool, zs.dev["text"], zs.dev["zones"], zs.dev["accs"], zs.dev["acc_offs"], flags=TAB).to_host().tobytes() == \
        b"".join(zs.want_lines(good, 0, TAB))
    out = guarded(ctx, 64)
    assert ctx.hgvs_render_into(*zs.render_args(ctx.upload(words).view(0), d_pool, 0, TAB | HEADS), out) == (0, True)
    assert np.all(out.to_host() == GUARD)
    assert zs.render(ctx.upload(words), d_pool, 0, TAB | HEADS) == want


# ---- the command -------------------------------------------------------------------------------------------------------------
def zot(args):
    from zotmer_amd import cli
    out, err = io.StringIO(), io.StringIO()
    code = 0
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            code = cli.main_inner(args) or 0
        except SystemExit as e:
            code = e.code
    return code, out.getvalue(), err.getvalue()


@pytest.fixture(scope="module")
def home(tmp_path_factory):
    d = tmp_path_factory.mktemp("genome")
    genome.write_genome(str(d))
    return str(d)


@pytest.mark.parametrize("types,D,I,U", [(None, None, None, None), (cases.ALL, "2", "3.5", "40"), ("3:delins,0.5:and,ins", "1", "2", "1")])
def test_command_against_the_restatement(ctx, home, tmp_path, types, D, I, U):
    (tmp_path / "z.bed").write_text(cases.BED)
    P = R.Params(R.parse_types(types or cases.ROUND_TYPES), float(D or 1.5), float(I or 1.5), float(U or 3.0))
    words = ["-g", home, "-S", "31", "-N", "2000"]
    for o, v in (("-t", types), ("-D", D), ("-I", I), ("-U", U)):
        words += [o, v] if v is not None else []
    plain = R.command(cases.BED, genome.GENOME, 31, 2000, P)
    tabbed = R.command(cases.BED, genome.GENOME, 31, 2000, P, tab=True, heads=True)
    assert zot(["hgvs-gen"] + words + [str(tmp_path / "z.bed")]) == (0, plain, "")
    assert zot(["hgvs-gen"] + words + ["-T", "-V", str(tmp_path / "z.bed")]) == (0, tabbed, "")
    code, out, err = zot(["hgvs-gen"] + words + ["-T", "-V", "-B", "1", "-v", "-o", str(tmp_path / "o.txt"), str(tmp_path / "z.bed")])
    assert (code, out) == (0, "") and err == "2000 variants\n" and (tmp_path / "o.txt").read_text() == tabbed
    assert zot(["hgvs-gen"] + words + ["-V", "-o", str(tmp_path / "p.txt"), str(tmp_path / "z.bed")])[0] == 0
    assert [l for l in (tmp_path / "p.txt").read_text().split("\n") if not l.startswith("#")] == plain.split("\n")


def test_command_cut_into_many_calls(ctx, home, tmp_path, monkeypatch):
    """draw calls of 300 variants and render calls whose buffer is too small for one line: grown, the same bytes"""
    from zotmer_amd.library import hgvsgen
    (tmp_path / "z.bed").write_text(cases.BED)
    P = R.Params(R.parse_types("sub,dup,ins"), 1.5, 1.5, 40.0)
    plan = hgvsgen.make_plan(dict(bed=str(tmp_path / "z.bed"), home=home, names=None, seed=8, types="sub,dup,ins", D=1.5, I=1.5, U=40.0))
    monkeypatch.setattr(hgvsgen, "DRAW_BATCH", 300)
    stats = hgvsgen.new_stats()
    out = io.BytesIO()
    counts = hgvsgen.run(ctx, plan, 1000, out, tab=True, heads=True, buffer_bytes=60, stats=stats)
    assert out.getvalue().decode() == R.command(cases.BED, genome.GENOME, 8, 1000, P, tab=True, heads=True)
    assert stats["calls"] == 1000 and stats["variants"] == 1000 and int(counts.sum()) == 1000 and stats["bytes"] == len(out.getvalue())
    out = io.BytesIO()
    hgvsgen.run(ctx, plan, 0, out)
    assert out.getvalue() == b""


def test_command_with_names_and_seed_from_the_system(ctx, tmp_path):
    d = tmp_path / "g"
    genome.write_genome(str(d), gz=False)
    (tmp_path / "names.txt").write_text("NC_A.1 chrA\nNC_B.2 chrB\n")
    (tmp_path / "u.bed").write_text(cases.BED_UNNAMED.replace("chrA", "NC_A.1").replace("chrB", "NC_B.2"))
    words = ["hgvs-gen", "-g", str(d), "-n", str(tmp_path / "names.txt"), "-N", "60", "-V"]
    code, out, err = zot(words + ["-S", "4", str(tmp_path / "u.bed")])
    by_acc = {"NC_A.1": genome.GENOME["chrA"], "NC_B.2": genome.GENOME["chrB"]}
    assert (code, err) == (0, "") and out == R.command(cases.BED_UNNAMED.replace("chrA", "NC_A.1").replace("chrB", "NC_B.2"), by_acc, 4, 60, R.Params(), heads=True)
    assert out.startswith("# NC_A.1 : x\n") and out.count("# ") == 2 and "# NC_A.1 : None\n" in out
    code, out, err = zot(words + ["-v", str(tmp_path / "u.bed")])
    assert code == 0 and err.startswith("seed = ") and err.endswith("60 variants\n") and out.count("\n") == 62


# ---- round trip --------------------------------------------------------------------------------------------------------------
def test_round_trip_on_the_device(ctx, home, tmp_path):
    """hgvs-gen, hgvs-index, spikein, hgvs-find: what tests/test_hgvsgen_host.py established on the CPU"""
    (tmp_path / "z.bed").write_text(cases.ROUND_BED)
    (tmp_path / "s.bed").write_text(cases.ROUND_SPIKE_BED)
    panel = str(tmp_path / "panel.txt")
    assert zot(["hgvs-gen", "-g", home, "-S", str(cases.ROUND_SEED), "-N", str(cases.ROUND_N), "-o", panel, str(tmp_path / "z.bed")]) == (0, "", "")
    texts = open(panel).read().split()
    assert texts == R.command(cases.ROUND_BED, genome.GENOME, cases.ROUND_SEED, cases.ROUND_N, R.Params()).split() and len(texts) == 8
    assert zot(["hgvs-index", "-g", home, str(tmp_path / "index.yaml")] + texts)[0] == 0
    assert zot(["spikein", "-g", home, "-b", str(tmp_path / "s.bed"), "-f", panel, "-S", "11", "-N", str(cases.ROUND_SPIKE_N), "-V", "1.0",
                str(tmp_path / "r")])[0] == 0
    code, out, err = zot(["hgvs-find", str(tmp_path / "index.yaml"), str(tmp_path / "r_1.fastq"), str(tmp_path / "r_2.fastq")])
    assert code == 0, err
    lines = out.split("\n")
    rows = [dict(zip(lines[0].split("\t"), l.split("\t"))) for l in lines[1:] if l]
    assert [r["hgvs"] for r in rows] == texts
    assert [r["res"] for r in rows if ">" in r["hgvs"]] == ["mut"] * sum(">" in t for t in texts) and sum(">" in t for t in texts) >= 2
