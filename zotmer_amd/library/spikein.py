"""
`zot spikein`: what the reference's spikein does (zotmer/commands/spikein.py), with counter-based draws.

Everything that is not a random draw is the reference's: the zones of the BED file (readBED, spikein.py:147-168), the variant
lists per chromosome and their overlap check (spikein.py:396-427), the -m lottery (applyBackgroundVariants, :170-191), the
variants of a zone applied rightmost first with e0 moved by size - range length (prepareAllele, :241-265), the fragment with
its two clamps and the record (makeReadFromZone, :267-317).  The draws are zotmer_amd/synth.py's rnd(seed, tag, index), integers
only: the zone of draw n, and per pair p -- numbered in output order: chromosomes by name, zones sorted within them, the
count[z] pairs of a zone in order -- the allele, the start, the fragment length, the strand and the errors.  So the output
does not depend on how the pairs are cut into device calls.

The host parses, applies the variants to a window around each zone -- the fragment length is bounded, |fl - I| <= 6 I D, so a
finite window holds every fragment a zone can give -- and uploads one text of all windows, a table of 12 words a zone and the
header prefixes.  zk_spike_zone_counts tallies the zone draws; zk_spike_pairs (csrc/spikein.hip) writes the records of a run
of pairs for both mates; the texts come back through pinned buffers and go to the two files.
"""
import gzip
import os
import sys
import time

import numpy as np

from zotmer_amd import synth
from zotmer_amd.library import hgvsindex
from zotmer_amd.library.hgvsfind import InputError

DEFAULT_BUFFER = 64 << 20
DRAWS_PER_CALL = 1 << 28


# ---- zones -------------------------------------------------------------------------------------------------------------------
def read_bed(lines, norm=lambda a: a):
    """readBED (spikein.py:147-168): {chromosome: sorted [(s, e, name or None)]}; a first line `track` or `browser` is skipped"""
    res = {}
    first = True
    for n, l in enumerate(lines, 1):
        t = l.split()
        if first:
            first = False
            if t and t[0] in ("track", "browser"):
                continue
        if not t:
            continue
        if len(t) < 3:
            raise InputError("BED line %d: expected a chromosome, a start and an end" % n)
        try:
            s, e = int(t[1]), int(t[2])
        except ValueError:
            raise InputError("BED line %d: a coordinate that is no integer" % n)
        if s < 0 or e < s:
            raise InputError("BED line %d: the zone %s:%d-%d is empty or starts below 0" % (n, t[0], s, e))
        res.setdefault(norm(t[0]), []).append((s, e, t[3] if len(t) > 3 else None))
    for ch in res:
        res[ch].sort(key=lambda z: (z[0], z[1], z[2] is not None, z[2] or ""))
    return res


def whole_zones(home):
    """without -b: every sequence file of the directory is one zone (1, length, stem)"""
    zones = {}
    for path in home.files():
        stem = os.path.basename(path)
        stem = stem[:-6] if stem.endswith(".fa.gz") else stem[:-3]
        zones[stem] = [(1, len(home[stem]), stem)]
    return zones


# ---- variants ----------------------------------------------------------------------------------------------------------------
def ranges_overlap(x, y):
    """HGVS.overlaps (library/hgvs.py:182-202) on two ranges: equal, or neither ends before the other starts"""
    return x == y or not (x[1] < y[0] or y[1] < x[0])


def zone_overlaps(st, en, v):
    """overlaps(st, en, v) (spikein.py:198-209)"""
    r = v.range()
    return st <= r[0] <= en or st <= r[1] <= en or r[0] <= st <= r[1] or r[0] <= en <= r[1]


class Draws:
    """the host's draws: a running index per tag"""

    def __init__(self, seed):
        self.seed, self.at = seed, {}

    def next(self, tag):
        i = self.at.get(tag, 0)
        self.at[tag] = i + 1
        return synth.rnd_int(self.seed, tag, i)


def parse_variants(texts, norm, draws):
    """spikein.py:403-416: {chromosome: [variant]} in order of appearance; an anonymous variant gets its bases here"""
    out = {}
    for t in texts:
        v = hgvsindex.make_variant(t)
        if v is None:
            raise InputError("unable to parse variant: %s" % t)
        if v.kind == "insALU":
            raise InputError("%s: insALU has no sequence to spike in" % t)
        v.spike_seq = "".join("ACGT"[draws.next(synth.T_ANON) & 3] for _ in range(v.size())) if v.anonymous() else None
        out.setdefault(norm(v.acc), []).append(v)
    return out


def _key(v):
    return v.range()


def check_overlaps(all_vars, err):
    """spikein.py:418-427 -> the number of overlapping pairs, each reported as the reference words it"""
    n = 0
    for xs in all_vars.values():
        xs.sort(key=_key)
        for i in range(len(xs)):
            for j in range(i + 1, len(xs)):
                if ranges_overlap(xs[i].range(), xs[j].range()):
                    err.write("variants overlap: %s <> %s\n" % (str(xs[i]), str(xs[j])))
                    n += 1
    return n


def read_pop_vars(lines, norm):
    """-m: lines of `<probability> <variant>` -> {chromosome: sorted [(variant, frac32 threshold)]}"""
    out = {}
    for n, l in enumerate(lines, 1):
        t = l.split()
        if not t:
            continue
        try:
            p = float(t[0])
            v = hgvsindex.make_variant(t[1])
        except (ValueError, IndexError):
            raise InputError("-m, line %d: expected a probability and a variant" % n)
        if v is None or v.kind == "insALU" or v.anonymous() or not 0.0 <= p <= 1.0:
            raise InputError("-m, line %d: %s is no probability with a variant that has a sequence" % (n, l.strip()))
        v.spike_seq = None
        out.setdefault(norm(v.acc), []).append((v, synth.frac32(p)))
    for ch in out:
        out[ch].sort(key=lambda vp: (_key(vp[0]), vp[1]))
    return out


def apply_background(ch, given, pop_vars, draws):
    """applyBackgroundVariants (spikein.py:170-191)"""
    if ch not in pop_vars:
        return given
    extra = []
    for m, thr in pop_vars[ch]:
        if not (draws.next(synth.T_POP) & 0xFFFFFFFF) < thr:
            continue
        if extra and ranges_overlap(extra[-1].range(), m.range()):
            continue
        if any(ranges_overlap(v.range(), m.range()) for v in given):
            continue
        extra.append(m)
    return sorted(given + extra, key=_key)


# ---- alleles -----------------------------------------------------------------------------------------------------------------
def var_seq(v, seq):
    return v.spike_seq if v.spike_seq is not None else v.sequence(seq)


class Allele:
    """a zone's allele (prepareAllele, spikein.py:241-265) as pieces of the chromosome and the variants' sequences, never
    joined: G, (s0, e0), and cut(lo, hi) = allele[lo:hi]"""

    def __init__(self, seq, zone, variants):
        st, en, _ = zone
        ws = sorted((v for v in variants if zone_overlaps(st, en, v)), key=_key)
        self.seq, self.pieces = seq, []             # (allele start, text or None, chromosome start, length)
        e0, at, pos = en, 0, 0
        for v in ws:
            r = v.range()
            if r[0] < at or r[1] > len(seq):
                raise InputError("%s does not lie on its sequence, or overlaps the variant before it" % v)
            s = var_seq(v, seq)
            e0 += len(s) - (r[1] - r[0])
            self.pieces.append((pos, None, at, r[0] - at))
            pos += r[0] - at
            self.pieces.append((pos, s, 0, len(s)))
            pos += len(s)
            at = r[1]
        self.pieces.append((pos, None, at, len(seq) - at))
        self.G = pos + len(seq) - at
        self.s0, self.e0 = st, e0
        self.applied = ws

    def cut(self, lo, hi):
        out = []
        for pos, text, at, n in self.pieces:
            a, b = max(lo, pos), min(hi, pos + n)
            if a < b:
                out.append(text[a - pos:b - pos] if text is not None else self.seq[at + a - pos:at + b - pos])
        return "".join(out)

    def flat(self):
        return self.cut(0, self.G)

    def window(self, flmax):
        """[lo, hi) of the allele that holds every fragment of the zone: u in [s0, e0] and fl <= flmax, then the two clamps"""
        lo, hi = self.s0, self.e0 + flmax
        if self.s0 < flmax:
            hi = max(hi, 2 * flmax)                 # u - fl < 0 gives u = fl
        if hi > self.G:
            lo, hi = min(lo, self.G - flmax), self.G     # u + fl > G gives u = G - fl
        return max(lo, 0), hi


def head_prefix(ch, zone):
    return "%s:%d-%d %s " % (ch, zone[0], zone[1], zone[2])


class Plan:
    """everything the device calls need, and nothing of the device: the zones in output order with their two alleles"""

    def __init__(self, zones, all_vars, pop_vars, home, seed, L, I, D, draws):
        self.seed, self.L, self.I = seed, L, I
        self.sd_q = synth.spike_sd_q(I, D)
        self.flmax = synth.spike_flmax(I, self.sd_q, L)
        self.zones = []                             # (chromosome, zone, wild-type Allele, mutant Allele)
        for ch in sorted(zones):
            wt_vars = apply_background(ch, [], pop_vars, draws)
            mut_vars = apply_background(ch, list(all_vars.get(ch, [])), pop_vars, draws)
            seq = home[ch]
            for zone in zones[ch]:
                pair = []
                for what, vs in (("wild-type", wt_vars), ("mutant", mut_vars)):
                    a = Allele(seq, zone, vs)
                    where = "%s:%d-%d" % (ch, zone[0], zone[1])
                    if a.e0 < a.s0:
                        raise InputError("zone %s: its variants leave nothing of the %s allele (s0 = %d, e0 = %d)" % (where, what, a.s0, a.e0))
                    if a.G < 2 * self.flmax:
                        raise InputError("zone %s: the %s allele has %d bases, fewer than twice the longest fragment (%d)"
                                         % (where, what, a.G, self.flmax))
                    pair.append(a)
                self.zones.append((ch, zone, pair[0], pair[1]))
        if not self.zones:
            raise InputError("no zones to sample reads from")
        self.cum = np.cumsum([z[1][1] - z[1][0] + 1 for z in self.zones], dtype=np.uint64)

    def tables(self, counts):
        """-> (text u8, zones u64[12 nz], first u64[nz + 1], heads u8, head_offs u64[nz + 1])"""
        texts, rows, at = [], [], 0
        for ch, zone, wt, mut in self.zones:
            for a in (wt, mut):
                lo, hi = a.window(self.flmax)
                t = a.cut(lo, hi).encode("latin-1")
                rows += [at, lo, len(t), a.G, a.s0, a.e0]
                texts.append(t)
                at += len(t)
        heads = [head_prefix(ch, zone).encode("latin-1") for ch, zone, _, _ in self.zones]
        first = np.zeros(len(self.zones) + 1, dtype=np.uint64)
        first[1:] = np.cumsum(np.asarray(counts, dtype=np.uint64))
        head_offs = np.zeros(len(heads) + 1, dtype=np.uint64)
        head_offs[1:] = np.cumsum([len(h) for h in heads])
        return (np.frombuffer(b"".join(texts), dtype=np.uint8), np.asarray(rows, dtype=np.int64).view(np.uint64), first,
                np.frombuffer(b"".join(heads), dtype=np.uint8), head_offs)


def make_plan(opts, variants, err=None):
    """the arguments of the command (a dict: bed, home, names, file, pop, seed, L, I, D) -> Plan; or InputError; overlapping
    variants are reported and give SystemExit(1) as in the reference"""
    err = err or sys.stderr
    names = opts.get("names") or {}
    norm = lambda a: names.get(a, a)
    home = hgvsindex.Home(opts["home"])
    draws = Draws(opts["seed"])
    texts = list(variants)
    if opts.get("file") is not None:
        with open(opts["file"]) as f:
            texts += [l.strip() for l in f if l.strip()]
    all_vars = parse_variants(texts, norm, draws)
    if check_overlaps(all_vars, err) > 0:
        raise SystemExit(1)
    pop_vars = {}
    if opts.get("pop") is not None:
        with open(opts["pop"]) as f:
            pop_vars = read_pop_vars(f, norm)
    if opts.get("bed") is not None:
        with open(opts["bed"]) as f:
            zones = read_bed(f, norm)
    else:
        zones = whole_zones(home)
    for ch in list(all_vars) + list(pop_vars) + list(zones):
        home.path(ch)                               # a missing sequence file is refused before anything is loaded
    return Plan(zones, all_vars, pop_vars, home, opts["seed"], opts["L"], opts["I"], opts["D"], draws)


# ---- the device --------------------------------------------------------------------------------------------------------------
def new_stats():
    return dict(pairs=0, calls=0, bytes=0, count_seconds=0.0, kernel_seconds=0.0, d2h_seconds=0.0, write_seconds=0.0)


def zone_counts(ctx, plan, N):
    d_cum = ctx.upload(plan.cum)
    d_counts = ctx.upload(np.zeros(len(plan.cum), dtype=np.uint64))
    for lo in range(0, N, DRAWS_PER_CALL):
        ctx.spike_zone_counts(d_cum, plan.seed, lo, min(DRAWS_PER_CALL, N - lo), d_counts)
    return d_counts.to_host()


class Writer:
    """one output file; with -z every device call's text is a gzip member of its own, as `zot capture -z` writes its batches"""

    def __init__(self, path, z):
        self.f, self.z = open(path, "wb"), z

    def write(self, data):
        self.f.write(gzip.compress(bytes(data)) if self.z else data)

    def close(self):
        self.f.close()


def run(ctx, plan, N, V, E, prefix, z=False, buffer_bytes=DEFAULT_BUFFER, verbose=False, err=None, stats=None):
    err = err or sys.stderr
    stats = stats if stats is not None else new_stats()
    for k, v in new_stats().items():
        stats.setdefault(k, v)
    L = plan.L
    t0 = time.perf_counter()
    counts = zone_counts(ctx, plan, N)
    stats["count_seconds"] += time.perf_counter() - t0
    assert int(counts.sum()) == N
    text, rows, first, heads, head_offs = plan.tables(counts)
    d_text, d_rows, d_first, d_heads, d_offs = (ctx.upload(a) for a in (text, rows, first, heads, head_offs))
    thr_v, thr_e = synth.frac32(V), synth.frac32(E)
    # a guess at a record's size decides how many pairs a call takes; a buffer that proves too small is grown
    guess = 64 + int(np.diff(head_offs).max()) + 2 * L + int(E * L * 8) + 8
    per_call = max(1, buffer_bytes // guess)
    bufs = (ctx.empty(buffer_bytes, np.uint8), ctx.empty(buffer_bytes, np.uint8))
    pins = [ctx.pinned(buffer_bytes), ctx.pinned(buffer_bytes)]
    sfx = ".gz" if z else ""
    outs = [Writer(prefix + "_1.fastq" + sfx, z), Writer(prefix + "_2.fastq" + sfx, z)]
    try:
        for lo in range(0, N, per_call):
            n = min(per_call, N - lo)
            t0 = time.perf_counter()
            args = (d_text, d_rows, d_first, d_heads, d_offs, plan.seed, L, plan.I, plan.sd_q, thr_v, thr_e, lo, n)
            nb, fit = ctx.spike_pairs_into(*args, *bufs)
            if not fit:
                bufs = tuple(b if b.n >= m else ctx.empty(m, np.uint8) for b, m in zip(bufs, nb))
                nb, fit = ctx.spike_pairs_into(*args, *bufs)
                assert fit
            o1, o2 = bufs[0].view(nb[0]), bufs[1].view(nb[1])
            t1 = time.perf_counter()
            for m, o in enumerate((o1, o2)):
                if o.n > pins[m].n:
                    pins[m].free()
                    pins[m] = ctx.pinned(o.n)
                if o.n:
                    ctx._check(ctx.lib.zk_download(ctx.h, pins[m].ptr, o.ptr, o.n))
            t2 = time.perf_counter()
            for m, o in enumerate((o1, o2)):
                outs[m].write(pins[m].array[:o.n])
            t3 = time.perf_counter()
            stats["kernel_seconds"] += t1 - t0
            stats["d2h_seconds"] += t2 - t1
            stats["write_seconds"] += t3 - t2
            stats["calls"] += 1
            stats["pairs"] += n
            stats["bytes"] += o1.n + o2.n
            if verbose:
                err.write("%d pairs\n" % (lo + n))
    finally:
        for o in outs:
            o.close()
        for p in pins:
            p.free()
    return counts
