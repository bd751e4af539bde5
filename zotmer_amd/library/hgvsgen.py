"""
`zot hgvs-gen`: what the reference's hgvs-gen does (zotmer/commands/hgvs-gen.py), with counter-based draws.

Everything that is not a random draw is the reference's: the zones of the BED file with both ends inclusive and the weight
e - s + 1 (readBED and main, hgvs-gen.py:48-69, :212-231), the order of the output -- chromosomes by name, the zones of a
chromosome in the order of their lines, zones without a draw left out (:230-241) --, the seven kinds of genVar (:120-171), the
spellings, range(), size() and sequence() of library/hgvs.py, the columns of -T and the `# chrom : name` lines of -V (:254-271).
The draws are zotmer_amd/synth.py's rnd(seed, tag, index), integers only: the zone of draw n and, per variant v numbered in
output order, the kind, the position, the lengths and the bases.  So the output does not depend on how the variants are cut
into device calls.

The host parses, loads one chromosome at a time and cuts the window seq[s .. e] of every zone, and makes the tables: the type
thresholds, a descending table per mean length in which a geometric length is a binary search, and the threshold that replaces
the rejection loop of delins.  zk_spike_zone_counts tallies the zone draws; zk_hgvs_draw (csrc/hgvs_gen.hip) makes the rows of
a run of variants and zk_hgvs_render their lines; the text comes back through a pinned buffer and goes to the file.
"""
import math
import sys
import time

import numpy as np

from zotmer_amd import synth
from zotmer_amd.library import hgvsindex, spikein
from zotmer_amd.library.hgvsfind import InputError

DEFAULT_BUFFER = 64 << 20
DRAW_BATCH = 1 << 20          # variants per zk_hgvs_draw call: 56 MB of work space, 48 MB of rows
KINDS = synth.HG_KINDS
SUB, DELINS, AND = KINDS.index("sub"), KINDS.index("delins"), KINDS.index("and")
DEFAULT_TYPES = "sub,del,ins,delins,dup"


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def parse_types(text):
    """-t (hgvs-gen.py:181-191): comma separated [prob:]type -> the relative probabilities of the seven kinds in synth.HG_KINDS
    order; the probabilities of a type that is named twice add up"""
    probs = [0.0] * len(KINDS)
    for w in text.split(","):
        t = w.split(":")
        if len(t) == 1:
            p, k = 1.0, t[0]
        elif len(t) == 2:
            try:
                p = float(t[0])
            except ValueError:
                raise InputError("-t: %s is no probability in %s" % (t[0], w))
            k = t[1]
        else:
            raise InputError("-t: unexpected variant category descriptor: %s" % w)
        if k not in KINDS:
            raise InputError("-t: unknown variant type %s (one of %s)" % (k, ", ".join(KINDS)))
        if not (p >= 0.0) or math.isinf(p):
            raise InputError("-t: the probability of %s is negative or not finite" % w)
        probs[KINDS.index(k)] += p
    if not sum(probs) > 0.0:
        raise InputError("-t: every type has probability 0")
    return probs


def read_bed(lines):
    """readBED (hgvs-gen.py:48-69) without the chromosome renaming: {chromosome: [(s, e, name)]} in file order; a first line
    `track` or `browser` is skipped, blank lines too; a zone without a name is called None"""
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
        res.setdefault(t[0], []).append((s, e, t[3] if len(t) > 3 else "None"))
    return res


def geom_table(option, mean):
    try:
        return synth.hg_geom_table(mean)
    except ValueError as e:
        raise InputError("option %s: %s" % (option, e))


class Plan:
    """everything the device calls need, and nothing of the device: the zones in output order with their windows, the tables"""

    def __init__(self, zones, home, seed, probs, D, I, U):
        self.seed, self.probs = seed, list(probs)
        self.thr = synth.hg_type_thresholds(probs)
        self.tables = [geom_table("-D", D), geom_table("-I", I), geom_table("-U", U)]
        self.mix = 0
        if D * I > 1.0:
            self.mix = synth.hg_mix_thr(D, I)
        elif probs[DELINS] > 0 or probs[AND] > 0:
            raise InputError("-D 1 with -I 1 leaves delins and `and` nothing to draw: every pair of lengths (1, 1) is rejected")
        self.zones, self.windows = [], []           # (chromosome, s, e, name); the bytes of seq[s .. e]
        for ch in sorted(zones):
            home.path(ch)                           # a missing sequence file is refused before anything is loaded
        for ch in sorted(zones):
            seq = home[ch]
            for s, e, name in zones[ch]:
                if e >= len(seq):
                    raise InputError("zone %s:%d-%d ends beyond the %d bases of its sequence" % (ch, s, e, len(seq)))
                self.zones.append((ch, s, e, name))
                self.windows.append(seq[s:e + 1].encode("latin-1"))
        if not self.zones:
            raise InputError("no zones to draw variants from")
        self.cum = np.cumsum([e - s + 1 for _, s, e, _ in self.zones], dtype=np.uint64)

    def check_counts(self, counts):
        """a zone that received draws, cannot give a substitution and may have to"""
        if not self.probs[SUB] > 0:
            return
        for z, n in enumerate(counts):
            if n and not any(c in self.windows[z] for c in b"ACGTacgt"):
                ch, s, e, _ = self.zones[z]
                raise InputError("zone %s:%d-%d holds no base of ACGT: no substitution can be drawn there" % (ch, s, e))

    def device_tables(self, counts):
        """the zones with draws -> (text u8, zones u64[3 nz], first u64[nz + 1], accs u8, acc_offs, names u8, name_offs): a name
        is left empty where it repeats the one before it, which is when the reference prints no `#` line"""
        texts, rows, first, accs, names, at, v, prev = [], [], [0], [], [], 0, 0, None
        for z, n in enumerate(counts):
            if not n:
                continue
            ch, s, e, name = self.zones[z]
            rows += [at, s, e]
            texts.append(self.windows[z])
            at += len(self.windows[z])
            v += int(n)
            first.append(v)
            accs.append(ch.encode("latin-1"))
            names.append(name.encode("latin-1") if name != prev else b"")
            prev = name

        def pool(items):
            offs = np.zeros(len(items) + 1, dtype=np.uint64)
            offs[1:] = np.cumsum([len(x) for x in items])
            return np.frombuffer(b"".join(items), dtype=np.uint8), offs
        return (np.frombuffer(b"".join(texts), dtype=np.uint8), np.asarray(rows, dtype=np.uint64), np.asarray(first, dtype=np.uint64)) + \
            pool(accs) + pool(names)


def make_plan(opts):
    """the arguments of the command (a dict: bed, home, names, seed, types, D, I, U) -> Plan; or InputError"""
    probs = parse_types(opts["types"])
    with open(opts["bed"]) as f:
        zones = read_bed(f)
    home = hgvsindex.Home(opts["home"], opts.get("names"))
    return Plan(zones, home, opts["seed"], probs, opts["D"], opts["I"], opts["U"])


# ---- the device --------------------------------------------------------------------------------------------------------------
def new_stats():
    return dict(variants=0, calls=0, bytes=0, count_seconds=0.0, draw_seconds=0.0, render_seconds=0.0, d2h_seconds=0.0, write_seconds=0.0)


def run(ctx, plan, N, out, tab=False, heads=False, buffer_bytes=DEFAULT_BUFFER, verbose=False, err=None, stats=None, direct=False):
    """N variants as lines to the binary file object `out` -> the zone counts"""
    err = err or sys.stderr
    stats = stats if stats is not None else new_stats()
    for k, v in new_stats().items():
        stats.setdefault(k, v)
    t0 = time.perf_counter()
    counts = spikein.zone_counts(ctx, plan, N) if N else np.zeros(len(plan.cum), dtype=np.uint64)
    stats["count_seconds"] += time.perf_counter() - t0
    assert int(counts.sum()) == N
    plan.check_counts(counts)
    if N == 0:
        return counts
    text, rows, first, accs, acc_offs, names, name_offs = plan.device_tables(counts)
    d_text, d_zones, d_first, d_accs, d_acc_offs, d_names, d_name_offs = (ctx.upload(a) for a in (text, rows, first, accs, acc_offs, names, name_offs))
    geom_n = [len(t) for t in plan.tables]
    d_geom = ctx.upload(np.asarray(sum(plan.tables, []) or [0], dtype=np.uint64))
    flags = (ctx.HGVS_TABULAR if tab else 0) | (ctx.HGVS_HEADERS if heads else 0) | (ctx.HGVS_DIRECT if direct else 0)
    RW = ctx.HGVS_ROW_WORDS
    batch = min(DRAW_BATCH, N)
    d_rows, d_pool = ctx.empty(RW * batch, np.uint64), ctx.empty(2 * batch + 64, np.uint8)
    # a guess at a line's size decides how many rows a render call takes; a buffer that proves too small is grown
    alen = int(np.diff(acc_offs).max())
    guess = (2 * alen + 64 if tab else alen + 32)
    per_call = max(1, buffer_bytes // guess)
    buf = ctx.empty(buffer_bytes, np.uint8)
    pin = ctx.pinned(buffer_bytes)
    try:
        for lo in range(0, N, batch):
            n = min(batch, N - lo)
            t0 = time.perf_counter()
            draw = (d_text, d_zones, d_first, plan.thr, d_geom, geom_n, plan.mix, plan.seed, lo, n)
            got, fit = ctx.hgvs_draw_into(*draw, d_rows, d_pool)
            if not fit:
                d_pool = ctx.empty(got[1], np.uint8)
                got, fit = ctx.hgvs_draw_into(*draw, d_rows, d_pool)
                assert fit
            rv, pv = d_rows.view(RW * n), d_pool.view(got[1])
            stats["draw_seconds"] += time.perf_counter() - t0
            for r0 in range(0, n, per_call):
                m = min(per_call, n - r0)
                t0 = time.perf_counter()
                args = (rv.view(RW * m, RW * r0), pv, d_text, d_zones, d_accs, d_acc_offs, d_names, d_name_offs, d_first, lo + r0, flags)
                nb, fit = ctx.hgvs_render_into(*args, buf)
                if not fit:
                    buf = ctx.empty(nb, np.uint8)
                    nb, fit = ctx.hgvs_render_into(*args, buf)
                    assert fit
                t1 = time.perf_counter()
                if nb > pin.n:
                    pin.free()
                    pin = ctx.pinned(nb)
                if nb:
                    ctx._check(ctx.lib.zk_download(ctx.h, pin.ptr, buf.ptr, nb))
                t2 = time.perf_counter()
                out.write(pin.array[:nb])
                t3 = time.perf_counter()
                stats["render_seconds"] += t1 - t0
                stats["d2h_seconds"] += t2 - t1
                stats["write_seconds"] += t3 - t2
                stats["calls"] += 1
                stats["bytes"] += nb
            stats["variants"] += n
            if verbose:
                err.write("%d variants\n" % (lo + n))
    finally:
        pin.free()
    return counts
