"""
`zot spikein` restated in plain Python integers and strings: the BED reader, the ten kinds of variant, the alleles, the
counter-based draws and the records.  It imports nothing from zotmer_amd; the device and the library are compared with it.

    rnd(seed, tag, i) = mix64(mix64(seed + tag) + i)      (mod 2^64)
"""
import bisect
import re

M64 = (1 << 64) - 1
T_ZONE, T_ALLELE, T_POS, T_LEN, T_STRAND, T_ERR, T_ANON, T_POP = 16, 17, 18, 19, 20, 21, 22, 23
IH_MAX = 6 * 65535
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def rnd(seed, tag, i):
    return mix64((mix64((seed + tag) & M64) + i) & M64)


def frac32(p):
    return int(round(p * 4294967296.0))


def sd_q(I, D):
    return int(round(I * D * 65536))


def flmax(I, sdq, L):
    return max(L + L // 2, I + ((sdq * IH_MAX) >> 32))


# ---- the draws of one pair ---------------------------------------------------------------------------------------------------
def frag_len(seed, p, I, sdq, L):
    z = -IH_MAX
    for k in range(3):
        r = rnd(seed, T_LEN, 3 * p + k)
        z += (r & 0xFFFF) + ((r >> 16) & 0xFFFF) + ((r >> 32) & 0xFFFF) + (r >> 48)
    return max(I + ((sdq * z) >> 32), L + L // 2)


def upper(s):
    """ASCII letters only, as the device does it"""
    return "".join(chr(ord(c) - 32) if "a" <= c <= "z" else c for c in s)


def pair_records(seed, p, L, I, sdq, thr_v, thr_e, head, alleles):
    """alleles = [(text, s0, e0) of the wild type, of the mutant] -> (record of mate 1, record of mate 2, which allele)"""
    mut = 1 if (rnd(seed, T_ALLELE, p) & 0xFFFFFFFF) < thr_v else 0
    text, s0, e0 = alleles[mut]
    G = len(text)
    u = s0 + rnd(seed, T_POS, p) % (e0 - s0 + 1)
    fl = frag_len(seed, p, I, sdq, L)
    if u - fl < 0:
        u = fl
    if u + fl > G:
        u = G - fl
    assert 0 <= u and u + fl <= G, "the fragment leaves its allele"
    frag = upper(text[u:u + fl])
    s = "+"
    if rnd(seed, T_STRAND, p) & 1:
        s = "-"
        frag = "".join(COMP.get(c, c) for c in frag)[::-1]
    out = []
    for m, read in enumerate((frag[:L], frag[-L:])):
        bases, errs = list(read), []
        for j in range(L):
            r = rnd(seed, T_ERR, (2 * p + m) * L + j)
            if (r & 0xFFFFFFFF) < thr_e:
                c = bases[j]
                d = [x for x in "ACGT" if x != c][(r >> 32) % 3] if c in "ACGT" else "ACGT"[(r >> 32) % 4]
                errs.append("%d%s>%s" % (j, c, d))
                bases[j] = d
        out.append("@%s%d %d %s %s\n%s\n+\n%s\n" % (head, u, fl, s, ";".join(errs), "".join(bases), "I" * L))
    return out[0], out[1], mut


def zone_counts(seed, cum, first, count):
    """cum: the inclusive cumulative zone lengths -> the tally of the draws [first, first + count)"""
    counts = [0] * len(cum)
    for n in range(first, first + count):
        counts[bisect.bisect_right(cum, rnd(seed, T_ZONE, n) % cum[-1])] += 1
    return counts


def records(seed, L, I, sdq, thr_v, thr_e, zones, first=0, count=None):
    """zones = [(head, pairs of the zone, [(text, s0, e0), (text, s0, e0)])] -> the two texts of the pairs [first, first + count)
    in output order, and the allele of each"""
    recs = record_list(seed, L, I, sdq, thr_v, thr_e, zones, first, count)
    return "".join(r[0] for r in recs), "".join(r[1] for r in recs), [r[2] for r in recs]


def record_list(seed, L, I, sdq, thr_v, thr_e, zones, first=0, count=None):
    """-> [(record of mate 1, record of mate 2, allele)] of the pairs [first, first + count)"""
    starts = [0]
    for _, n, _ in zones:
        starts.append(starts[-1] + n)
    count = starts[-1] - first if count is None else count
    out = []
    for p in range(first, first + count):
        z = bisect.bisect_right(starts, p) - 1
        out.append(pair_records(seed, p, L, I, sdq, thr_v, thr_e, zones[z][0], zones[z][2]))
    return out


# ---- variants ----------------------------------------------------------------------------------------------------------------
_POS = re.compile(r"^([^:]+):g\.([0-9]+)(?:_([0-9]+))?(.*)$", re.S)


class Var:
    def __init__(self, text, acc, kind, rng, arg):
        self.text, self.acc, self.kind, self.rng, self.arg, self.seq = text, acc, kind, rng, arg, None

    def sequence(self, chrom):
        k = self.kind
        if k in ("sub", "ins", "delins"):
            return self.arg
        if k == "del":
            return ""
        if k in ("insN", "delinsN"):
            return self.seq
        ref = chrom[self.rng[0]:self.rng[1]].upper()
        if k == "dup":
            return ref + ref
        if k == "repeat":
            return ref * self.arg
        return "".join(COMP.get(c, c) for c in ref)[::-1]


def parse_variant(text):
    m = _POS.match(text)
    if m is None:
        return None
    acc, p0, p1, tail = m.group(1), int(m.group(2)), m.group(3), m.group(4)
    a, b = p0 - 1, (int(p1) if p1 is not None else p0) - 1
    if re.fullmatch(r"[ACGT]>[ACGT]", tail):
        return Var(text, acc, "sub", (a, a + 1), tail[2]) if p1 is None else None
    if re.fullmatch(r"del(?:[ACGT]+)?", tail):
        return Var(text, acc, "del", (a, b + 1), None)
    if re.fullmatch(r"dup(?:[ACGT]+)?", tail):
        return Var(text, acc, "dup", (a, b + 1), None)
    if re.fullmatch(r"inv(?:[ACGT]+)?", tail):
        return Var(text, acc, "inv", (a, b + 1), None) if p1 is not None else None
    if tail == "insALU":
        return Var(text, acc, "insALU", (b, b), None) if p1 is not None else None
    q = re.fullmatch(r"ins([ACGT]+)", tail)
    if q:
        return Var(text, acc, "ins", (b, b), q.group(1)) if p1 is not None else None
    q = re.fullmatch(r"ins([0-9]+)", tail)
    if q:
        return Var(text, acc, "insN", (b, b), int(q.group(1))) if p1 is not None else None
    q = re.fullmatch(r"delins([ACGT]+)", tail)
    if q:
        return Var(text, acc, "delins", (a, b + 1), q.group(1))
    q = re.fullmatch(r"delins([0-9]+)", tail)
    if q:
        return Var(text, acc, "delinsN", (a, b + 1), int(q.group(1)))
    q = re.fullmatch(r"([ACGT]+)?\[([0-9]+)\]", tail)
    if q:
        last = int(p1) if p1 is not None else (p0 + len(q.group(1)) - 1 if q.group(1) else p0)
        return Var(text, acc, "repeat", (a, last), int(q.group(2)))
    return None


def ranges_overlap(x, y):
    return x == y or not (x[1] < y[0] or y[1] < x[0])


def zone_overlaps(st, en, r):
    return st <= r[0] <= en or st <= r[1] <= en or r[0] <= st <= r[1] or r[0] <= en <= r[1]


def allele(chrom, zone, variants):
    """-> (the flattened allele, s0, e0): the variants that overlap the zone applied to the whole chromosome, rightmost first"""
    st, en = zone[0], zone[1]
    e0, seq = en, chrom
    for v in sorted((v for v in variants if zone_overlaps(st, en, v.rng)), key=lambda v: v.rng, reverse=True):
        s = v.sequence(chrom)
        e0 += len(s) - (v.rng[1] - v.rng[0])
        seq = seq[:v.rng[0]] + s + seq[v.rng[1]:]
    return seq, st, e0


def read_bed(text):
    res, first = {}, True
    for l in text.splitlines():
        t = l.split()
        if first:
            first = False
            if t and t[0] in ("track", "browser"):
                continue
        if not t:
            continue
        res.setdefault(t[0], []).append((int(t[1]), int(t[2]), t[3] if len(t) > 3 else None))
    for ch in res:
        res[ch].sort(key=lambda z: (z[0], z[1], z[2] is not None, z[2] or ""))
    return res


class Host:
    """the host's draws: one running index per tag"""

    def __init__(self, seed):
        self.seed, self.at = seed, {}

    def next(self, tag):
        i = self.at.get(tag, 0)
        self.at[tag] = i + 1
        return rnd(self.seed, tag, i)


def background(ch, given, pop, host):
    if ch not in pop:
        return given
    extra = []
    for v, thr in pop[ch]:
        if not (host.next(T_POP) & 0xFFFFFFFF) < thr:
            continue
        if extra and ranges_overlap(extra[-1].rng, v.rng):
            continue
        if any(ranges_overlap(g.rng, v.rng) for g in given):
            continue
        extra.append(v)
    return sorted(given + extra, key=lambda v: v.rng)


def command(genome, bed, variants, seed, N, L=100, I=300, D=0.1, E=0.005, V=1.0, pop=None, names=None):
    """genome: {stem: sequence}; bed, pop: the files' texts or None; variants: the strings of the command line and of -f
    -> (text of mate 1, text of mate 2, info), info = dict(counts, zones = [(ch, zone, wt allele, mut allele)], which)"""
    names = names or {}
    host = Host(seed)
    by_ch = {}
    for t in variants:
        v = parse_variant(t)
        assert v is not None and v.kind != "insALU", t
        if v.kind in ("insN", "delinsN"):
            v.seq = "".join("ACGT"[host.next(T_ANON) & 3] for _ in range(v.arg))
        by_ch.setdefault(names.get(v.acc, v.acc), []).append(v)
    for vs in by_ch.values():
        vs.sort(key=lambda v: v.rng)
        assert not any(ranges_overlap(vs[i].rng, vs[j].rng) for i in range(len(vs)) for j in range(i + 1, len(vs)))
    pops = {}
    for l in (pop or "").splitlines():
        t = l.split()
        if t:
            v = parse_variant(t[1])
            pops.setdefault(names.get(v.acc, v.acc), []).append((v, frac32(float(t[0]))))
    for ch in pops:
        pops[ch].sort(key=lambda vp: (vp[0].rng, vp[1]))
    if bed is not None:
        zones = {names.get(ch, ch): zs for ch, zs in read_bed(bed).items()}
    else:
        zones = {ch: [(1, len(genome[ch]), ch)] for ch in genome}
    table = []
    for ch in sorted(zones):
        wt_vars = background(ch, [], pops, host)
        mut_vars = background(ch, list(by_ch.get(ch, [])), pops, host)
        for zone in zones[ch]:
            table.append((ch, zone, allele(genome[ch], zone, wt_vars), allele(genome[ch], zone, mut_vars)))
    cum, t = [], 0
    for _, zone, _, _ in table:
        t += zone[1] - zone[0] + 1
        cum.append(t)
    counts = zone_counts(seed, cum, 0, N)
    zs = [("%s:%d-%d %s " % (ch, zone[0], zone[1], zone[2]), n, [wt, mut]) for (ch, zone, wt, mut), n in zip(table, counts)]
    o1, o2, which = records(seed, L, I, sd_q(I, D), frac32(V), frac32(E), zs)
    return o1, o2, dict(counts=counts, zones=table, which=which)
