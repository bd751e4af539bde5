"""What zk_pileup_merge computes, restated with numpy, and the lists its tests are made of.  Pure numpy: no device.

A counted list is three arrays (u32 coordinate or bait, u64 k-mer, count), strictly ascending by (coordinate, k-mer).  The keys
of the test lists are drawn from one ascending universe whose coordinates and k-mers sit on every value where a signed or a
64-bit-only comparison would go wrong: coordinates 0, 2^31 - 1, 2^31, 2^32 - 1, k-mers 0, 2^63 - 1, 2^63, 2^64 - 1."""
import numpy as np

U32, U64 = np.uint32, np.uint64
KMERS = np.array([0, 1, (1 << 31) + 7, 1 << 32, (1 << 63) - 1, 1 << 63, (1 << 64) - 2, (1 << 64) - 1], dtype=U64)


def merge_lists(a, b):
    """the union of two counted lists: concatenate, lexsort, add.reduceat in u64 (the counts wrap modulo 2^64)"""
    c = np.concatenate((np.asarray(a[0], U32), np.asarray(b[0], U32)))
    x = np.concatenate((np.asarray(a[1], U64), np.asarray(b[1], U64)))
    n = np.concatenate((np.asarray(a[2]).astype(U64), np.asarray(b[2]).astype(U64)))
    if not len(c):
        return np.empty(0, U32), np.empty(0, U64), np.empty(0, U64)
    order = np.lexsort((x, c))
    c, x, n = c[order], x[order], n[order]
    heads = np.ones(len(c), dtype=bool)
    heads[1:] = (c[1:] != c[:-1]) | (x[1:] != x[:-1])
    starts = np.nonzero(heads)[0]
    return c[starts], x[starts], np.add.reduceat(n, starts)


def merge_by_dict(a, b):
    """the same through a dictionary of Python ints -> [(coordinate, k-mer, count), ...] ascending"""
    d = {}
    for lst in (a, b):
        for c, x, n in zip(np.asarray(lst[0]).tolist(), np.asarray(lst[1]).tolist(), np.asarray(lst[2]).tolist()):
            d[(c, x)] = (d.get((c, x), 0) + n) & ((1 << 64) - 1)
    return [(c, x, d[(c, x)]) for c, x in sorted(d)]


def universe(n_coords, seed=1):
    """(coordinates, k-mers) of 8 * n_coords keys, strictly ascending: every coordinate with every k-mer of KMERS"""
    rng = np.random.default_rng(seed)
    special = np.array([0, 1, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 2, (1 << 32) - 1], dtype=np.int64)
    coords = special
    while len(coords) < n_coords:
        coords = np.unique(np.concatenate((coords, rng.integers(0, 1 << 32, size=n_coords - len(coords), dtype=np.int64))))
    coords = np.sort(coords).astype(U32)
    return np.repeat(coords, len(KMERS)), np.tile(KMERS, len(coords))


def counts_for(rng, n, bits):
    """counts of every size the field holds: small ones, ones around 2^32, the largest"""
    top = (1 << bits) - 1
    v = rng.integers(1, 1 << 20, size=n, dtype=np.uint64)
    pick = rng.integers(0, 4, size=n)
    v[pick == 1] = U64(top)
    if bits == 64:
        v[pick == 2] = rng.integers(1 << 32, 1 << 40, size=int(np.sum(pick == 2)), dtype=np.uint64)
    return v.astype(U32 if bits == 32 else U64)


def list_of(uni, idx, rng, bits):
    idx = np.asarray(idx, dtype=np.int64)
    return uni[0][idx], uni[1][idx], counts_for(rng, len(idx), bits)


LAYOUTS = ("interleaved", "disjoint", "subset", "equal", "a_below_b", "b_below_a")


def layout(uni, name, na, nb, rng, b_bits):
    """two lists of na and nb keys (subset: nb <= na, equal: nb = na) of the universe in the layout named -> (A, B)"""
    m = len(uni[0])
    if name == "interleaved":              # about a third of the smaller list shared
        ia = np.sort(rng.choice(m, size=na, replace=False))
        shared = rng.choice(ia, size=min(na, nb) // 3, replace=False) if min(na, nb) >= 3 else np.empty(0, np.int64)
        rest = np.setdiff1d(np.arange(m), ia)
        ib = np.sort(np.concatenate((shared, rng.choice(rest, size=nb - len(shared), replace=False))))
    elif name == "disjoint":
        both = np.sort(rng.choice(m, size=na + nb, replace=False))
        take = np.zeros(na + nb, dtype=bool)
        take[rng.choice(na + nb, size=na, replace=False)] = True
        ia, ib = both[take], both[~take]
    elif name == "subset":
        ia = np.sort(rng.choice(m, size=na, replace=False))
        ib = np.sort(rng.choice(ia, size=min(nb, na), replace=False))
    elif name == "equal":
        ia = np.sort(rng.choice(m, size=na, replace=False))
        ib = ia.copy()
    else:
        both = np.sort(rng.choice(m, size=na + nb, replace=False))
        ia, ib = (both[:na], both[na:]) if name == "a_below_b" else (both[nb:], both[:nb])
    return list_of(uni, ia, rng, 64), list_of(uni, ib, rng, b_bits)


def boundary_pairs(uni, tile, tiles, shift, rng, b_bits):
    """tiles * tile merged inputs (+ shift) in which, for every tile boundary t, merged input t * tile - 1 + shift is an A element
    and input t * tile + shift is the B element of the same key; every other input is A's or B's by a coin -> (A, B)"""
    total = tiles * tile + shift
    twin = np.zeros(total, dtype=bool)                   # input p has the key of input p - 1
    owner_a = rng.integers(0, 2, size=total).astype(bool)
    for t in range(1, tiles):
        p = t * tile + shift
        twin[p] = True
        owner_a[p - 1], owner_a[p] = True, False
    rank = np.cumsum(~twin) - 1
    assert rank[-1] < len(uni[0])
    return list_of(uni, rank[owner_a], rng, 64), list_of(uni, rank[~owner_a], rng, b_bits)


def random_lists(n_lists, per_list, pool, seed):
    """n_lists counted lists (u32 counts) of per_list keys each, drawn from one pool of `pool` random keys"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 1 << 32, size=pool, dtype=np.uint64).astype(U32)
    x = rng.integers(0, 1 << 64, size=pool, dtype=np.uint64)
    order = np.lexsort((x, c))
    c, x = c[order], x[order]
    keep = np.ones(pool, dtype=bool)
    keep[1:] = (c[1:] != c[:-1]) | (x[1:] != x[:-1])
    c, x = c[keep], x[keep]
    out = []
    for _ in range(n_lists):
        idx = np.sort(rng.choice(len(c), size=per_list, replace=False))
        out.append((c[idx], x[idx], rng.integers(1, 1 << 32, size=per_list, dtype=np.uint64).astype(U32)))
    return out
