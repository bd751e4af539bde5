"""Seeded inputs for the tests of `zot scan`: the gene sets and samples of the golden cases (tests/golden/make_golden_scan.py,
tests/test_scan_host.py, tests/test_gpu_scan.py) and the k-mer lists and index arrays the two device entries are tried on.
Every builder asserts the conditions its case exists for, from tests/_scan_restatement.py alone: a case that misses one is
changed, never the condition."""
import random
import zlib

from tests import _scan_restatement as R

K_SCAN = 27


# ---- golden cases: genes as FASTA records, samples as (acgt, k-mers) --------------------------------------------------------------

def _seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _substitute(rng, seq, at):
    s = list(seq)
    for p in at:
        s[p] = rng.choice([b for b in "ACGT" if b != s[p]])
    return "".join(s)


def sample_of(seqs, K=K_SCAN):
    """the k-mer set of some sequences as the command reads it: (meta acgt, ascending distinct k-mers of both strands)"""
    xs = [x for s in seqs for x, _ in R.kmers_with_pos(K, s)]
    acgt = [0, 0, 0, 0]
    for x in xs:
        acgt[x & 3] += 1
    n = float(len(xs))
    return [c / n for c in acgt], sorted(set(xs))


def golden_cases():
    """[{name, fasta: [[(name, seq)] per file], samples: [(name, acgt, X)]}]"""
    rng = random.Random(20261)
    present, close, spread, absent = _seq(rng, 150), _seq(rng, 150), _seq(rng, 180), _seq(rng, 120)
    flank = [_seq(rng, 900) for _ in range(5)]
    # substitutions within one window's reach keep the record in one fragment; spread out they cut it into fragments with gaps
    close_s = _substitute(rng, close, (93, 99, 105))
    spread_s = _substitute(rng, spread, (40, 90, 141))
    c1 = dict(name="verbatim_changed_absent",
              fasta=[[("present verbatim", present), ("three substitutions close", close), ("three substitutions spread", spread)],
                     [("absent", absent)]],
              samples=[("s1", ) + sample_of([flank[0] + present + flank[1], flank[2] + close_s + flank[3], spread_s + flank[4]])],
              changed={"three substitutions close": (close, close_s)})
    with_n = _seq(rng, 70) + "N" + _seq(rng, 90)
    short = _seq(rng, 20)
    poly = "A" * 25 + "CG" + _seq(rng, 60)
    twice = _seq(rng, 100)
    c2 = dict(name="n_short_polya_two_samples",
              fasta=[[("with an N", with_n), ("shorter than K", short), ("poly A head", poly), ("in both", twice)]],
              samples=[("s2a", ) + sample_of([flank[0] + with_n.replace("N", "G") + flank[1] + twice, poly + flank[2]]),
                       ("s2b", ) + sample_of([flank[3] + twice + flank[1], flank[2] + poly[:60]])])
    for c in (c1, c2):
        for _, acgt, X in c["samples"]:
            assert 2000 <= len(X) <= 20000 and abs(sum(acgt) - 1) < 1e-9
    return [c1, c2]


# ---- zk_lcp_resolve --------------------------------------------------------------------------------------------------------------

def _distinct(rng, K, n, draw):
    n = min(n, 4 ** K)
    out = set()
    tries = 0
    while len(out) < n:
        out.add(draw() & (4 ** K - 1))
        tries += 1
        assert tries < 200 * n + 1000, "the generator cannot give %d distinct values" % n
    return sorted(out)


def random_lists(seed, K, nS, nX):
    rng = random.Random(seed)
    if 4 ** K <= 4096:
        pool = list(range(4 ** K))
        return sorted(rng.sample(pool, min(nS, len(pool)))), sorted(rng.sample(pool, min(nX, len(pool))))
    draw = lambda: rng.getrandbits(2 * K)
    return _distinct(rng, K, nS, draw), _distinct(rng, K, nX, draw)


def clustered_lists(seed, K, nS, nX):
    """a few base values xor low bits: long shared prefixes, many carried values.  Asserts that at least 1 entry in 20 is
    changed by pass 2 and that at least 1 in 20 differs from the better of the two neighbours in X."""
    rng = random.Random(seed)
    base = [rng.getrandbits(2 * K) for _ in range(5)]
    draw = lambda: rng.choice(base) ^ rng.getrandbits(rng.choice([2, 4, 8, 12]))
    S, X = _distinct(rng, K, nS, draw), _distinct(rng, K, nX, draw)
    L1, _ = R.resolve_all(K, S, X, passes=1)
    L, _ = R.resolve_all(K, S, X)
    ideal = R.best_of_neighbours(K, S, X)
    assert 20 * sum(1 for a, b in zip(L, L1) if a != b) >= len(S), "pass 2 changes too few entries"
    assert 20 * sum(1 for a, b in zip(L, ideal) if a != b) >= len(S), "too few entries differ from best-of-neighbours"
    return S, X


def _with_first(base, K, vals):
    return [(base << (2 * K - 2)) | v for v in vals]


def shaped_lists(shape, K, n, tile):
    """the named shapes of the issue -> (S, X)"""
    rng = random.Random(zlib.crc32(repr((shape, K, n)).encode()))

    def low(m):          # m distinct values above 0 that leave the first base free (as many as there are, at a small K)
        bits = min(2 * K - 2, 40)
        return sorted(rng.sample(range(1, 1 << bits), min(m, (1 << bits) - 1)))
    if shape == "S above X":            # every S[i] meets the LAST element of X
        S, X = _with_first(2, K, low(n)), _with_first(1, K, low(7))
        assert X[-1] < S[0]
    elif shape == "S below X":
        S, X = _with_first(1, K, low(n)), _with_first(2, K, low(7))
        assert S[-1] < X[0]
    elif shape == "S equals X":
        S = _with_first(rng.randrange(4), K, low(n))
        X = list(S)
        assert all(l == K for l in R.resolve_all(K, S, X)[0])
    elif shape in ("disjoint first bases", "disjoint first bases, 0 in X"):
        # S begins with A (and G), X with C: pass 1 leaves (0, 0) everywhere, and the carried 0 matches the leading A's
        S = low(n // 2) + _with_first(2, K, low(n - n // 2))
        X = _with_first(1, K, low(7))
        if shape.endswith("0 in X"):
            X = [0] + X
        L1, Y1 = R.resolve_all(K, S, X, passes=1)
        L, Y = R.resolve_all(K, S, X)
        assert all(l == 0 and y == 0 for l, y in zip(L1, Y1)) and sum(1 for l in L if l > 0) >= n // 2 - 1 and not any(Y)
    elif shape == "two-element X":      # the walk that is linear without the stepping: 4 tiles of A-headed k-mers between two x
        assert n == 4 * tile
        S = low(n)
        X = [0, _with_first(3, K, [5])[0]]
        L, Y = R.resolve_all(K, S, X)
        assert not any(Y) and all(l > 0 for l in L[1:])
    else:
        raise KeyError(shape)
    assert S == sorted(set(S)) and X == sorted(set(X)) and S[-1] < 4 ** K and X[-1] < 4 ** K
    return S, X


def long_carry(K, brk, tail=9):
    """a value that pass 2 carries from entry 0 to entry brk - 1 and that stops exactly at brk: S[0] = v is in X, the entries
    after it are v + i (a long common prefix with v, none with the next x), and from brk on the entries begin with another
    base.  Asserts the run."""
    assert K >= 13 and brk < 1 << 20
    v = (1 << (2 * K - 2)) | (0x155 << (2 * K - 14))
    assert brk < 1 << (2 * K - 14)
    far = 3 << (2 * K - 2)
    S = [v + i for i in range(brk)] + [far + i for i in range(tail)]
    X = [v, far + tail + 3]
    assert S == sorted(set(S)) and X == sorted(set(X)) and S[-1] < 4 ** K and X[-1] < 4 ** K
    L, Y = R.resolve_all(K, S, X)
    assert all(y == v for y in Y[:brk]) and all(y != v for y in Y[brk:]) and min(L[1:brk]) >= K - 10
    L1, Y1 = R.resolve_all(K, S, X, passes=1)
    assert not any(L1[1:brk])
    return S, X


# ---- zk_scan_place -----------------------------------------------------------------------------------------------------------------

def place_case(seed, K, slots, nS, density=0.8, pairs=0.3, max_l=None):
    """random index arrays over records of the given slot counts -> dict(L, Y, T, U, V, slots): per slot, with probability
    `density`, a forward and / or a reverse entry under random k-mers of the index, and with probability `pairs` both strands
    under ONE k-mer (a reverse palindrome: the same rank, the order within its list decides).  L is drawn from few values so
    that ties are common.  Where the case has 60 slots or more (and is not filled on purpose) it asserts ties won by either
    strand, slots without entries and slots whose best L is 0."""
    rng = random.Random(seed)
    per = [[] for _ in range(nS)]
    for n, w in enumerate(slots):
        for q in range(w):
            if rng.random() >= density:
                continue
            if rng.random() < pairs:
                i = rng.randrange(nS)
                first = rng.choice((1, -1))
                per[i].append((n, first * (q + 1)))
                per[i].append((n, -first * (q + 1)))
            else:
                for sign in (1, -1):
                    if rng.random() < 0.7:
                        per[rng.randrange(nS)].append((n, sign * (q + 1)))
    T, U, V = [0], [], []
    for lst in per:
        for n, p in lst:
            U.append(n)
            V.append(p)
        T.append(len(U))
    levels = [0, 0, 1, K // 2, K] if max_l is None else [0, max_l]
    L = [rng.choice(levels) for _ in range(nS)]
    Y = [rng.getrandbits(2 * K) for _ in range(nS)]
    c = dict(K=K, L=L, Y=Y, T=T, U=U, V=V, slots=list(slots))
    if max_l is None and density < 1 and sum(slots) >= 60:
        P, Q, cnt = R.place(K, L, Y, T, U, V, slots)
        named, best = {}, {}
        owner = [i for i in range(nS) for _ in range(T[i], T[i + 1])]
        for j, (n, p) in enumerate(zip(U, V)):
            named.setdefault((n, abs(p) - 1), []).append(j)
        fwd_wins = rev_wins = 0
        for (n, q), js in named.items():
            top = max(L[owner[j]] for j in js)
            tied = [j for j in js if L[owner[j]] == top]
            if top > 0 and len({V[j] > 0 for j in tied}) == 2:
                if V[min(tied)] > 0:
                    fwd_wins += 1
                else:
                    rev_wins += 1
        assert fwd_wins and rev_wins, "no tie between the strands of a slot won by each side"
        assert len(named) < sum(slots), "every slot has an entry"
        assert any(q == 0 for row in Q for q in row) and any(all(L[owner[j]] == 0 for j in js) for js in named.values())
    return c
