"""The tuning knobs of zk_tune as a table: what the library starts with (DEFAULTS), the levels tests/test_gpu_knobs.py crosses for
zk_kmerize (FACTORS), and a covering array of strength 2 over them (pairwise_rows).  include/zotk.h says of the knobs
"performance only; results never depend on them": a row is one zk_kmerize call whose table and stats must be the oracle's.

Pure Python: no device, no torch, no numpy -- tests/test_knob_cases_host.py checks the table against csrc/internal.hpp and the
binding on a machine without a GPU."""
import contextlib
import functools

# every result-relevant knob at the value of its initialiser in struct zk_ctx (csrc/internal.hpp); comm_chunk and comm_self_loop
# belong to the exchange and have their own tests
DEFAULTS = dict(sort_variant=3, pairs_variant=7, short_sort=0, side_div=8, xcd_group=0, early_collapse=1, packed_pairs=1, wide_tiles=1,
                stream_pass=1, stream_ranges=0, tag_words=2, tag_pass=0, dedupe_variant=0, dedupe_limit=65536, dedupe_bits=0, tile_sort=1,
                strand_blocks=1, kway=1)


@contextlib.contextmanager
def knobs(ctx, **kw):
    """zk_tune(kw) for the block; every knob of DEFAULTS is set back afterwards, whatever the block did"""
    try:
        ctx.tune(**kw)
        yield ctx
    finally:
        ctx.tune(**DEFAULTS)


# zk_kmerize: what a call is given (K, reads, flags: tests/_core_cases.kmerize_want) and every knob that reaches it (kway is
# zk_merge_n's).  Every value is accepted by zk_tune.  dedupe_bits: 9 and 18 are whole passes of the 9-bit geometries, 16 of the
# 8-bit ones (0, 1 and 5); a geometry ignores the values that are no multiple of its digit.
FACTORS = (
    ("K", (13, 24, 25, 27, 31, 32)),
    ("reads", ("deep", "flat", "dense")),
    ("flags", ("canonical", "both", "canonical_only", "subsample")),
    ("sort_variant", (0, 1, 2, 3, 4, 5, 6)),
    ("pairs_variant", (0, 1, 2, 3, 4, 5, 6, 7)),
    ("short_sort", (0, 1)),
    ("side_div", (8, 100000)),
    ("early_collapse", (0, 1, 2, 3)),
    ("packed_pairs", (0, 1)),
    ("wide_tiles", (0, 1)),
    ("stream_pass", (0, 1, 2, 3)),
    ("stream_ranges", (0, 3, 64)),
    ("tag_words", (0, 1, 2)),
    ("tag_pass", (0, 1)),
    ("dedupe_variant", (-1, 0, 1, 2)),
    ("dedupe_limit", (65536, 300)),
    ("dedupe_bits", (0, 9, 18, 16)),
    ("tile_sort", (0, 1)),
    ("strand_blocks", (0, 1, 2, 3, 4, 5)),
    ("xcd_group", (0, 8)),
)
INPUT_FACTORS = ("K", "reads", "flags")          # the factors of a row that are arguments of the call, not knobs


def knobs_of(row):
    """the zk_tune settings of a row"""
    return {k: v for k, v in row.items() if k not in INPUT_FACTORS}


def level_pairs():
    """every (factor index, level, factor index, level) of two different factors, the first index the smaller"""
    out = []
    for i, (_, li) in enumerate(FACTORS):
        for j in range(i + 1, len(FACTORS)):
            out += [(i, a, j, b) for a in li for b in FACTORS[j][1]]
    return out


class _Lcg:
    """a generator of our own (Knuth's MMIX constants): the rows must not change with the interpreter's"""

    def __init__(self, seed):
        self.s = (seed * 2862933555777941757 + 3037000493) & 0xFFFFFFFFFFFFFFFF

    def below(self, n):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return (self.s >> 33) % n

    def shuffled(self, xs):
        xs = list(xs)
        for i in range(len(xs) - 1, 0, -1):
            j = self.below(i + 1)
            xs[i], xs[j] = xs[j], xs[i]
        return xs


CANDIDATES = 40          # rows tried per row kept


@functools.lru_cache(maxsize=None)
def pairwise_rows(seed=1):
    """A covering array of strength 2 over FACTORS, as a tuple of dicts in FACTORS' order: every pair of levels of every two
    factors occurs in at least one row.  Greedy and deterministic (Cohen et al.'s AETG): a candidate row starts from a pair not yet
    covered and gives the other factors, in a random order, the level that covers the most new pairs with those already set; of
    CANDIDATES candidates the one that covers the most is kept.  The largest two factors have 8 x 7 = 56 level pairs, so no array
    has fewer rows."""
    rng = _Lcg(seed)
    nf = len(FACTORS)
    levels = [f[1] for f in FACTORS]
    open_pairs = set(level_pairs())
    order = sorted(open_pairs, key=repr)          # (levels of mixed types: ordered by their text)

    def gain(row, f, v):
        n = 0
        for g, w in row.items():
            n += ((g, w, f, v) if g < f else (f, v, g, w)) in open_pairs
        return n

    def covered(row):
        return {(i, row[i], j, row[j]) for i in range(nf) for j in range(i + 1, nf)} & open_pairs

    rows = []
    while open_pairs:
        order = [p for p in order if p in open_pairs]
        best, best_new = None, set()
        for _ in range(CANDIDATES):
            i, a, j, b = order[rng.below(len(order))]
            row = {i: a, j: b}
            for f in rng.shuffled(k for k in range(nf) if k not in row):
                gains = [gain(row, f, v) for v in levels[f]]
                top = [v for v, g in zip(levels[f], gains) if g == max(gains)]
                row[f] = top[rng.below(len(top))]
            new = covered(row)
            if len(new) > len(best_new):
                best, best_new = row, new
        open_pairs -= best_new
        rows.append({FACTORS[f][0]: best[f] for f in range(nf)})
    return tuple(rows)
