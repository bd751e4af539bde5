"""
`zot hgvs-gen` restated in plain Python integers and strings, with a mix64 of its own: the BED reader, the spreading of the
draws over the zones, the seven kinds of variant and the lines of the reference's hgvs-gen.py (its genVar and main, and the
classes of its library/hgvs.py).  It is the oracle of zk_hgvs_draw, zk_hgvs_render and the command; nothing here imports the
package but the tests that compare the two.

The draws.  rnd(seed, tag, i) = mix64(mix64(seed + tag) + i) mod 2^64.  Variants are numbered v = 0, 1, ... in output order:
chromosomes by name, the zones of a chromosome in the order of their lines in the BED file, the variants of a zone in a
row.  Draw n (tag 16) falls into the zone whose inclusive cumulative weight e - s + 1 first exceeds rnd % T.  Variant v:
  kind      the first kind (sub, del, ins, delins, dup, ani, and) whose cumulative threshold exceeds the low 32 bits of tag 25, v
  p         s + rnd(26, 64 v + t) % (e - s + 1), t = 0; a sub takes the first of t = 0 .. 63 whose upper-cased base is one of
            ACGT, and if none is, the first such base at or after try 63, going round the zone once
  geom(Q)   1 + the entries of the descending table Q above the low 32 bits of a draw: tag 27 for the deleted or duplicated
            length (tables of -D and -U), tag 28 for the inserted length (table of -I), both at index v
  delins, and
            a draw of tag 29 below thr gives l = 1, m = 1 + geom(I); otherwise l = 1 + geom(D), m = geom(I)
  bases     base j is bits 2 (j & 31) of rnd(30, v W + (j >> 5)) as ACGT; a sub's alternative is element rnd(31, v) % 3 of the
            other three of ACGT
"""
import bisect

MASK = (1 << 64) - 1
T_ZONE, T_TYPE, T_POS, T_LEN, T_INS, T_MIX, T_BASES, T_ALT = 16, 25, 26, 27, 28, 29, 30, 31
KINDS = ("sub", "del", "ins", "delins", "dup", "ani", "and")
SUB, DEL, INS, DELINS, DUP, ANI, AND = range(7)
TRIES = 64
TABLE_MAX = 65536


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def rnd(seed, tag, i):
    return mix64((mix64((seed + tag) & MASK) + i) & MASK)


def frac32(p):
    return int(round(p * 4294967296.0))


# ---- the tables the host makes once -------------------------------------------------------------------------------------------
def geom_table(mean):
    """Q[0] = frac32(1 - 1/mean), Q[k] = (Q[k - 1] Q[0]) >> 32 while positive"""
    mean = float(mean)
    if not mean >= 1.0 or mean == float("inf"):
        raise ValueError(mean)
    q0 = frac32(1.0 - 1.0 / mean)
    out, q = [], q0
    while q > 0:
        out.append(q)
        if len(out) > TABLE_MAX:
            raise ValueError(mean)
        q = (q * q0) >> 32
    return out


def geom(table, r32):
    return 1 + sum(1 for q in table if q > r32)


def type_thresholds(probs):
    total = float(sum(probs))
    out, t = [], 0.0
    for p in probs:
        t += p
        out.append(min(frac32(t / total), 1 << 32))
    last = max(i for i, p in enumerate(probs) if p > 0)
    return out[:last] + [1 << 32] * (len(out) - last)


def mix_thr(D, I):
    """The reference draws (l, m), l ~ geom(pd) and m ~ geom(pi) independent, until l > 1 or m > 1; a pair is rejected with
    probability pd pi, so P(l = 1 | kept) = pd (1 - pi) / (1 - pd pi).  Given l = 1 the pair was kept for m > 1, and a
    geometric variable given that it exceeds 1 is 1 + a geometric variable; given l > 1 -- likewise l = 1 + geom(pd) -- every m
    is kept, so m ~ geom(pi)."""
    pd, pi = 1.0 / D, 1.0 / I
    if pd * pi >= 1.0:
        raise ValueError("pd pi = 1")
    return min(frac32(pd * (1.0 - pi) / (1.0 - pd * pi)), 1 << 32)


class Params:
    def __init__(self, probs=(1, 1, 1, 1, 1, 0, 0), D=1.5, I=1.5, U=3.0):
        self.probs = list(probs)
        self.thr = type_thresholds(probs)
        self.QD, self.QI, self.QU = geom_table(D), geom_table(I), geom_table(U)
        if (probs[DELINS] > 0 or probs[AND] > 0) and not D * I > 1.0:
            raise ValueError("pd pi = 1")
        self.mix = mix_thr(D, I) if D * I > 1.0 else 0
        self.W = max(1, (len(self.QI) + 2 + 31) // 32)


def parse_types(text):
    """-t: comma separated [prob:]type, probabilities of a type named twice added -> relative probabilities in KINDS order"""
    probs = [0.0] * 7
    for w in text.split(","):
        t = w.split(":")
        if len(t) == 1:
            p, k = 1.0, t[0]
        elif len(t) == 2:
            p, k = float(t[0]), t[1]
        else:
            raise ValueError(w)
        probs[KINDS.index(k)] += p
    return probs


# ---- one variant ---------------------------------------------------------------------------------------------------------------
def kind_of(seed, v, thr):
    r = rnd(seed, T_TYPE, v) & 0xFFFFFFFF
    return next(k for k in range(7) if r < thr[k])


def sub_position(seed, v, s, e, window):
    """window = seq[s .. e]; None when it holds no base of ACGT"""
    span = e - s + 1
    for t in range(TRIES):
        p = s + rnd(seed, T_POS, 64 * v + t) % span
        if window[p - s].upper() in "ACGT":
            return p
    for k in range(span):
        x = (p - s + k) % span
        if window[x].upper() in "ACGT":
            return s + x
    return None


def bases(seed, v, m, W):
    return "".join("ACGT"[(rnd(seed, T_BASES, v * W + (j >> 5)) >> (2 * (j & 31))) & 3] for j in range(m))


def lengths(seed, v, P):
    """(l, m) of a delins or an `and`, before l is clamped"""
    gl = geom(P.QD, rnd(seed, T_LEN, v) & 0xFFFFFFFF)
    gm = geom(P.QI, rnd(seed, T_INS, v) & 0xFFFFFFFF)
    if (rnd(seed, T_MIX, v) & 0xFFFFFFFF) < P.mix:
        return 1, 1 + gm
    return 1 + gl, gm


def raw_lengths(seed, v, kind, P):
    """what the statistics are taken of: (l, m) as drawn, before q = min(p + l, e) clamps l; None where the kind has none"""
    if kind in (DEL, DUP):
        return geom(P.QD if kind == DEL else P.QU, rnd(seed, T_LEN, v) & 0xFFFFFFFF), None
    if kind in (INS, ANI):
        return None, geom(P.QI, rnd(seed, T_INS, v) & 0xFFFFFFFF)
    if kind in (DELINS, AND):
        return lengths(seed, v, P)
    return None, None


def draw(seed, v, s, e, window, P):
    """-> (kind, p, q, m, bases): a row of zk_hgvs_draw without its zone; ValueError for a sub in a zone without ACGT"""
    kind = kind_of(seed, v, P.thr)
    span = e - s + 1
    p = s + rnd(seed, T_POS, 64 * v) % span
    if kind == SUB:
        p = sub_position(seed, v, s, e, window)
        if p is None:
            raise ValueError("no ACGT")
        ref = "ACGT".index(window[p - s].upper())
        t = rnd(seed, T_ALT, v) % 3
        return kind, p, p, 1, "ACGT"[t + (1 if t >= ref else 0)]
    if kind == DEL:
        return kind, p, min(p + geom(P.QD, rnd(seed, T_LEN, v) & 0xFFFFFFFF), e), 0, ""
    if kind == DUP:
        return kind, p, min(p + geom(P.QU, rnd(seed, T_LEN, v) & 0xFFFFFFFF), e), 0, ""
    if kind in (INS, ANI):
        m = geom(P.QI, rnd(seed, T_INS, v) & 0xFFFFFFFF)
        return kind, p, p, m, bases(seed, v, m, P.W) if kind == INS else ""
    l, m = lengths(seed, v, P)
    return kind, p, min(p + l, e), m, bases(seed, v, m, P.W) if kind == DELINS else ""


# ---- the lines (library/hgvs.py: __str__, range, size, sequence; hgvs-gen.py:257-271) -------------------------------------------
def spell(acc, row):
    """every kind but sub, whose spelling names the reference base"""
    kind, p, q, m, b = row
    span = "%d" % (p + 1) if p == q else "%d_%d" % (p + 1, q + 1)
    if kind == DEL:
        return "%s:g.%sdel" % (acc, span)
    if kind == DUP:
        return "%s:g.%sdup" % (acc, span)
    if kind == INS:
        return "%s:g.%d_%dins%s" % (acc, p, p + 1, b)
    if kind == ANI:
        return "%s:g.%d_%dins%d" % (acc, p, p + 1, m)
    if kind == DELINS:
        return "%s:g.%sdelins%s" % (acc, span, b)
    return "%s:g.%sdelins%d" % (acc, span, m)


def line(acc, row, base_at, tab):
    """the line of a row, without its newline; base_at(lo, hi) = seq[lo:hi] of the chromosome"""
    kind, p, q, m, b = row
    if kind == SUB:
        text = "%s:g.%d%s>%s" % (acc, p + 1, base_at(p, p + 1).upper(), b)
    else:
        text = spell(acc, row)
    if not tab:
        return text
    if kind in (INS, ANI):
        r0, r1 = p, p
    else:
        r0, r1 = p, q + 1
    wt = base_at(r0, r1).upper()
    if kind == DUP:
        size, mut = 2 * (q - p + 1), 2 * wt
    elif kind == DEL:
        size, mut = 0, ""
    elif kind in (ANI, AND):
        size, mut = m, m * "N"
    else:
        size, mut = len(b), b
    return "\t".join([acc, "%d" % r0, "%d" % r1, "%d" % size, wt, mut, text])


# ---- the command -----------------------------------------------------------------------------------------------------------------
def read_bed(text):
    """{chromosome: [(s, e, name)]} in file order; a first line `track` or `browser` is skipped; an unnamed zone is `None`"""
    res, first = {}, True
    for l in text.split("\n"):
        t = l.split()
        if first:
            first = False
            if t and t[0] in ("track", "browser"):
                continue
        if not t:
            continue
        res.setdefault(t[0], []).append((int(t[1]), int(t[2]), t[3] if len(t) > 3 else "None"))
    return res


def zone_list(zones):
    """the zones in output order: [(chromosome, s, e, name)]"""
    return [(c, s, e, nm) for c in sorted(zones) for s, e, nm in zones[c]]


def zone_counts(seed, zl, N):
    cum, t = [], 0
    for _, s, e, _ in zl:
        t += e - s + 1
        cum.append(t)
    counts = [0] * len(zl)
    for n in range(N):
        counts[bisect.bisect_right(cum, rnd(seed, T_ZONE, n) % t)] += 1
    return counts


def variants(seed, zl, counts, genome, P):
    """-> [(zone index, row)] in output order"""
    out, v = [], 0
    for z, (c, s, e, _) in enumerate(zl):
        window = genome[c][s:e + 1]
        for _ in range(counts[z]):
            out.append((z, draw(seed, v, s, e, window, P)))
            v += 1
    return out


def command(bed, genome, seed, N, P, tab=False, heads=False):
    """the text `zot hgvs-gen` writes"""
    zl = zone_list(read_bed(bed))
    counts = zone_counts(seed, zl, N)
    out, prev, seen = [], None, -1
    for z, row in variants(seed, zl, counts, genome, P):
        c, s, e, nm = zl[z]
        if z != seen:
            seen = z
            if heads and nm != prev:
                prev = nm
                out.append("# %s : %s" % (c, nm))
        seq = genome[c]
        out.append(line(c, row, lambda lo, hi: seq[lo:hi], tab))
    return "".join(l + "\n" for l in out)


def parse_line(text):
    """a -T line of the reference (or of this command) -> (accession, row): the inverse of line(..., tab=True)"""
    import re
    acc, r0, r1, size, wt, mut, s = text.split("\t")
    r0, r1, size = int(r0), int(r1), int(size)
    m = re.match(r"([^:]+):g\.([0-9]+)(?:_([0-9]+))?(.*)$", s)
    a, b, tail = int(m.group(2)), m.group(3), m.group(4)
    b = int(b) if b is not None else a
    if ">" in tail:
        return acc, (SUB, a - 1, a - 1, 1, tail[2])
    if tail == "del":
        return acc, (DEL, a - 1, b - 1, 0, "")
    if tail == "dup":
        return acc, (DUP, a - 1, b - 1, 0, "")
    if tail.startswith("delins"):
        x = tail[6:]
        return acc, ((AND, a - 1, b - 1, int(x), "") if x.isdigit() else (DELINS, a - 1, b - 1, len(x), x))
    x = tail[3:]
    return acc, ((ANI, b - 1, b - 1, int(x), "") if x.isdigit() else (INS, b - 1, b - 1, len(x), x))
