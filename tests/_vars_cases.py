"""The inputs of the `zot vars` fixture (tests/golden/v1_vars.json): counted k-mer lists built by a seeded generator, so that the
fixture holds only what the reference made of them.  Read by tests/golden/make_golden_vars.py and by the tests.

A case is dict(name, K, ref [(k-mer, count)], samples [(name, [(k-mer, count)])]): every list ascending, every context of a
sample present in the reference.  Counts stay within a few hundred: the reference's tail sum is O(count) per base.
`missing_case()` is the one input the reference dies on (a sample context that the reference set lacks)."""
import random


def _group(rng, bases, lo, hi):
    return {b: rng.randint(lo, hi) for b in bases}


def _case(name, K, seed, n_ctx, n_samples):
    rng = random.Random(seed)
    J = K - 1
    space = 1 << (2 * J)
    if K >= 25:
        # both ends of the key range, and steps between neighbours that the set format can store (a k-mer delta below 2^60)
        step = (space - 1) // (n_ctx - 1)
        ctxs = [0] + [i * step + rng.randrange(-(step // 4), step // 4) for i in range(1, n_ctx - 1)] + [space - 1]
    else:
        ctxs = sorted(rng.sample(range(space), n_ctx)) if space > n_ctx else list(range(space))
    ref = {}
    for i, c in enumerate(ctxs):
        size = 4 if i % 3 == 0 else rng.randint(1, 4)          # reference groups of 4, and of every other size
        ref[c] = _group(rng, rng.sample(range(4), size), 1, 300)
    samples = []
    for s in range(n_samples):
        sam = {}
        for c in ctxs:
            if len(ctxs) > 4 and K < 32 and rng.random() < 0.15:
                continue                        # the reference set may hold contexts the sample lacks (K = 32: the steps would grow past 2^60)
            g, kind = ref[c], rng.random()
            gt = sum(g.values())
            if kind < 0.3:                      # the reference's proportions, roughly
                grp = {b: max(1, round(g[b] * rng.uniform(0.5, 1.5) * 200 / gt)) for b in g if rng.random() < 0.8}
            elif kind < 0.6:                    # one minor base of the reference takes over
                b = min(g, key=lambda x: (g[x], x))
                grp = {b: rng.randint(20, 300)}
                for o in g:
                    if o != b and rng.random() < 0.5:
                        grp[o] = rng.randint(1, 20)
            elif kind < 0.8:                    # two bases share the sample; a base the reference lacks may turn up
                grp = _group(rng, rng.sample(range(4), 2), 10, 150)
            else:                               # near the threshold: a mild shift of a small group
                grp = {b: max(1, round(g[b] * 40 / gt) + rng.randint(0, 12)) for b in g}
            if not grp:
                grp = {min(g): 1}
            sam[c] = grp
        samples.append(("%s_s%d" % (name, s), sam))

    def pairs(d):
        return [((c << 2) | b, n) for c in sorted(d) for b, n in sorted(d[c].items())]
    return dict(name=name, K=K, ref=pairs(ref), samples=[(nm, pairs(d)) for nm, d in samples])


def make_cases():
    return [_case("k1", 1, 101, 1, 8), _case("k2", 2, 201, 4, 3), _case("k7", 7, 701, 40, 2), _case("k25", 25, 2501, 40, 2),
            _case("k31", 31, 3101, 40, 2), _case("k32", 32, 3201, 40, 2)]


def missing_case():
    """K = 5: the sample has a context before the reference's first, one between two, and one after its last; the lines of
    the contexts it shares are the same with and without them"""
    ref = [((c << 2) | b, n) for c in (10, 20, 30) for b, n in ((0, 90), (1, 10))]
    shared = [((c << 2) | 1, 60) for c in (10, 20, 30)]
    extra = [((c << 2) | b, 5) for c in (3, 25, 200) for b in (2, 3)]
    return dict(name="missing", K=5, ref=ref, shared=shared, sample=sorted(shared + extra), missing=[3, 25, 200])
