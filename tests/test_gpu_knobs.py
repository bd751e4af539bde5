"""include/zotk.h on zk_tune: "performance only; results never depend on them".  The other tests set one knob at a time, and the two
sort geometries (ZK_TUNE_SORT_VARIANT, ZK_TUNE_PAIRS_VARIANT) for zk_sort_keys and zk_sort_pairs only.  Here:

  * test_kmerize_pairwise: zk_kmerize under a covering array of strength 2 over every knob that reaches it, K, the input and the
    flags (tests/_knob_cases.py: every two levels of every two factors meet in some row);
  * test_kmerize_every_geometry: zk_kmerize under every sort geometry, an unknown one as well, with every early collapse and the
    block plan forced -- the geometry picks the digit width the plan is laid out by, and every geometry but the default takes the
    uncounted sorts and the unfused strand kernels of pipeline.hip, dedupe_blocks.hip and strand_blocks.hip;
  * test_cases_under_ambient_knobs: every oracle-checked case of tests/_view_cases.py (all core entries) while a knob that the
    cases themselves leave alone stays set.

Every call runs on tests/_frames.py frames at lead 0: the table and the counts equal the oracle's bit for bit in arrays of exactly
the length needed, the guard behind them is intact, the stream is unchanged, and the stats are the oracle's."""
import ctypes as C
import functools

import pytest

from tests import _core_cases as cc
from tests import _knob_cases as KC
from tests import _view_cases as V
from zotmer_amd import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def kmerize_spec(reads, K, flags):
    """as _view_cases.kmerize_spec, with n_canonical among the scalars: (n_windows, n_instances, n_unique, n_canonical, acgt)"""
    wk, wc, needed = cc.kmerize_want(reads, K, flags)
    f = cc.kmerize_facts(reads, K)
    n_can = {"both": 0, "canonical_only": len(wk)}.get(flags, f["n_canonical"])          # (subsample: counted before it)
    st = native.KmerizeStats()

    def call(ctx, v):
        rc = ctx.lib.zk_kmerize(ctx.h, v[0].ptr, v[0].n, K, V.FLAGS[flags], 0.5, 3, v[1].ptr, v[2].ptr, v[1].n, C.byref(st))
        return rc, (st.n_windows, st.n_instances, st.n_unique, st.n_canonical, tuple(st.acgt))
    stream = V.bytes_of(cc.stream_of(cc.kmerize_reads(reads, K)))
    return V.Spec([V.In("stream16", stream), V.Out("u64", wk, cap=needed), V.Out("u32", wc, cap=needed)], call,
                  (f["n_windows"], f["n_instances"], len(wk), n_can, tuple(f["acgt"])))


def kmerize_checked(ctx, reads, K, flags, what):
    try:
        V.run(ctx, kmerize_spec(reads, K, flags), "P0")
    except AssertionError as e:
        raise AssertionError("%r: %s" % (what, e)) from None


# ---- the covering array ------------------------------------------------------------------------------------------------------------

ROWS = KC.pairwise_rows()


@pytest.mark.parametrize("i", range(len(ROWS)), ids=["row%02d" % i for i in range(len(ROWS))])
def test_kmerize_pairwise(ctx, i):
    """one row of the array, then the default plan on the same context: a row must leave nothing behind (V.run restores only its
    own DEFAULT_KNOBS; KC.knobs restores every knob)"""
    row = ROWS[i]
    with KC.knobs(ctx, **KC.knobs_of(row)):
        kmerize_checked(ctx, row["reads"], row["K"], row["flags"], row)
    kmerize_checked(ctx, "deep", 25, "canonical", ("all defaults, after", row))


# ---- every geometry ----------------------------------------------------------------------------------------------------------------

EIGHT_BIT = (0, 1, 5)          # radix_sort.hip: the geometries with 8-bit digits
UNKNOWN = 9                    # dispatches the default geometry, and is not "3" where the code asks for the default by number

# The strand route (strand_blocks.hip) of each input at K = 25 with 18 block bits forced, as tests/test_gpu_strand_blocks.py reads it
# from the profile: True = block by block, "declined" = with a declined block (the dense block: 1.7 tiles), None = not stated
# (`flat` does not repeat its k-mers: the dedupe's sample declines, and the strands are rebuilt from a list sorted the long way).
# K = 31 has no count field beside the k-mer (pack_bits_for: 2 spare bits), so the forced plan is not taken at all and
# ZK_TUNE_STRAND_BLOCKS is not read: False.
ROUTE_K25 = {"deep": True, "dense": "declined", "flat": None}


@pytest.mark.parametrize("reads", ["deep", "flat", "dense"])
@pytest.mark.parametrize("K", [24, 25, 31])
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5, 6, UNKNOWN])
def test_kmerize_every_geometry(ctx, variant, K, reads):
    """Every early collapse, by size and with the block plan forced (18 bits: two 9-bit passes; 16: two 8-bit ones); at odd K the
    forced calls under every ZK_TUNE_STRAND_BLOCKS but 2 as well.  Under the 9-bit geometries the profile must show the strand
    route: the copy that writes the mirror words books 8 bytes a canonical k-mer less than the other way ("whoever writes the
    words"), and the declined blocks' kernel is one more union record."""
    forced = 16 if variant in EIGHT_BIT else 18
    n_can = cc.kmerize_facts(reads, K)["n_canonical"]
    prof = {}
    for collapse in (0, 1, 2, 3):
        for bits in (0, forced):
            for sb in ((0, 1, 3, 4, 5) if bits and K & 1 else (1,)):
                setting = dict(sort_variant=variant, early_collapse=collapse, dedupe_bits=bits, strand_blocks=sb)
                with KC.knobs(ctx, **setting):
                    watched = bits == 18 and K & 1 and collapse == 1 and sb in (0, 1)
                    if watched:
                        ctx.profile(True)
                    try:
                        kmerize_checked(ctx, reads, K, "canonical", setting)
                        if watched:
                            prof[sb] = ctx.profile_read()
                    finally:
                        if watched:
                            ctx.profile(False)
    if variant in EIGHT_BIT or not K & 1:
        assert not prof
        return
    sel = {sb: prof[sb].get("select", {}).get("bytes", 0) for sb in (1, 0)}
    uni = {sb: prof[sb].get("union_sum", {}).get("launches", 0) for sb in (1, 0)}
    route = ROUTE_K25[reads] if K == 25 else False
    if route is False:
        assert sel[1] == sel[0] and uni[1] == uni[0], (variant, K, reads, prof)
    elif route is not None:
        assert sel[0] - sel[1] == 8 * n_can, (variant, K, reads, n_can, prof)
        assert uni[1] - uni[0] == (1 if route == "declined" else 0), (variant, K, reads, prof)


# ---- every core entry under a knob its cases leave alone ------------------------------------------------------------------------------

AMBIENT = [dict(sort_variant=v, pairs_variant=v) for v in range(7)] + [dict(sort_variant=3, pairs_variant=2), dict(sort_variant=5, pairs_variant=7)]
AMBIENT += [dict(xcd_group=8), dict(xcd_group=32)] + [dict(dedupe_variant=v) for v in (-1, 1, 2)]
AMBIENT += [dict(dedupe_limit=300), dict(tag_pass=1), dict(stream_ranges=3)]
assert not any(set(s) & set(V.DEFAULT_KNOBS) for s in AMBIENT)


@pytest.mark.parametrize("setting", AMBIENT, ids=["-".join("%s%d" % kv for kv in s.items()) for s in AMBIENT])
def test_cases_under_ambient_knobs(ctx, setting):
    """Every Spec of every case of tests/_view_cases.py once, at lead 0: oracle equality, intact guards, untouched inputs.  V.run sets
    a Spec's own knobs and restores only its DEFAULT_KNOBS, none of which is a key of `setting`: the ambient setting stays on
    through every call, and KC.knobs takes it back at the end.  The bait table that the capture cases hold per context is built
    again under each setting (zk_bait_table_build sorts through the same dispatch)."""
    V._capture_table.put(ctx, None)
    try:
        with KC.knobs(ctx, **setting):
            for name, build in V.CASES:
                for j, spec in enumerate(V.flat(build())):
                    assert not set(spec.knobs) & set(setting), (name, j, "the case sets the ambient knob itself")
                    try:
                        V.run(ctx, spec, "P0")
                    except AssertionError as e:
                        raise AssertionError("%s[%d] under %r: %s" % (name, j, setting, e)) from None
    finally:
        held = V._capture_table.table
        V._capture_table.put(ctx, None)          # (no later module meets a table of this context)
        if held is not None:
            held.free()
