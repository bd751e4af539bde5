"""
`zot hgvs-find` in scanning mode (zotmer/commands/hgvs-find.py:917-1131): indexed variants called from read pairs.

The reference makes one bait per variant -- lhs + wt + rhs, and + 'N' + lhs + mut + rhs when the mutant is spelled out
(hgvs-find.py:941-956) -- and hands every read pair to capture.addReadPairAndKmers (library/capture.py:99-135): the pair
counts for every bait that holds one of its k-mers, and all its k-mers (both strands of both mates) are counted for each of
those baits.  Per variant it then looks among the bait's counted k-mers for the wild-type and the mutant allele: for a
variant that is spelled out, the Hamming neighbours of the expected k-mer path, pruned to complete paths and turned into a
consensus (findFairlySimpleAllele, library/debruijn.py:334-409); for an anonymous one, de Bruijn paths between anchors found
in the flanks (bridgingAlleles, hgvs-find.py:517-583, 758-798).  Each allele is scored, the best of each kind kept, and one
line printed per variant.

Here the baits are a bait table on the device (library/capture.py), the mates stream through in batches
(library/fastq_batches.py), and each batch is one zk_capture_hits, zk_capture_kmers over slices of the pair list whose
entries stay within a budget, and one zk_pileup_count per slice; the counted lists are merged on the device
(alufinder.DevicePileup: zk_pileup_merge).  After the last batch the merged list stays where it is: one zk_path_scan answers every position of every
definite path, one more the anchors of the anonymous variants.  The pruning, the consensus, the paths, the scores and the
table are the reference's, restated over the matches.  What is printed does not depend on where the batches or slices are
cut.
"""
import contextlib
import json
import math
import os
import re
import sys
import time

import numpy as np

from zotmer_amd.library import capture
from zotmer_amd.library.alufinder import DevicePileup
from zotmer_amd.library.fastq_batches import record_batches, whole

EMIT_BUDGET = 1 << 25           # entries one zk_capture_kmers may write: 384 MiB of entries, 1.7 GiB of work space to count them
KEYS = ("hgvs", "lhsFlank", "rhsFlank", "wtSeq", "mutSeq")
_CODE = {c: i for i, c in enumerate("ACGT")}
_CODE.update({"U": 3})
_CODE.update({c.lower(): v for c, v in list(_CODE.items())})


class InputError(Exception):
    """an input the command refuses (the message goes to stderr, the exit status is 1)"""


# ---- the index ---------------------------------------------------------------------------------------------------------------
_HEAD = r"[^:]+:g\.([0-9]+)(?:_([0-9]+))?"
_TAILS = (("sub", r"[ACGT]>[ACGT]"), ("del", r"del(?:[ACGT]+)?"), ("dup", r"dup(?:[ACGT]+)?"), ("ins", r"ins([ACGT]+)"),
          ("insN", r"ins([0-9]+)"), ("insALU", r"insALU"), ("inv", r"inv(?:[ACGT]+)?"), ("delins", r"delins([ACGT]+)"),
          ("delinsN", r"delins([0-9]+)"), ("repeat", r"(?:[ACGT]+)?\[([0-9]+)\]"))
_PATTERNS = [(kind, re.compile(_HEAD + tail + "$")) for kind, tail in _TAILS]


class Variant:
    """What scanning needs of a `g.` HGVS string (library/hgvs.py:204-675): its kind, whether the mutant allele is only a
    length (anonymous), and size(), the length of the mutant allele (None for insALU)."""

    def __init__(self, text, kind, size):
        self.text, self.kind, self._size = text, kind, size

    def anonymous(self):
        return self.kind in ("insN", "delinsN")

    def size(self):
        return self._size

    def __str__(self):
        return self.text


def parse_hgvs(text):
    """-> Variant, or None for a string that names none of the ten kinds (a substitution over a range, an insertion or an
    inversion at a single position)"""
    for kind, pat in _PATTERNS:
        m = pat.match(text)
        if m is None:
            continue
        first, last, arg = int(m.group(1)), m.group(2), m.group(3) if pat.groups > 2 else None
        if kind == "sub":
            return None if last is not None else Variant(text, kind, 1)
        if last is None and kind in ("ins", "insN", "insALU", "inv"):
            return None
        span = (int(last) if last is not None else first) - first + 1
        if kind in ("ins", "delins"):
            size = len(arg)
        elif kind in ("insN", "delinsN"):
            size = int(arg)
        else:
            size = {"del": 0, "dup": 2 * span, "inv": span, "insALU": None, "repeat": int(arg or 0) * span}[kind]
        return Variant(text, kind, size)
    return None


def parse_index(text, where="the index"):
    """the index as the reference's -X writes it: a list of dicts {hgvs, lhsFlank, rhsFlank, wtSeq, mutSeq}, mutSeq null for a
    variant that is not spelled out.  JSON is YAML: a JSON file is tried first (and is a valid index for the reference too),
    else the text is YAML, for which PyYAML is needed.  -> (items, variants)"""
    try:
        items = json.loads(text)
    except ValueError:
        try:
            import yaml
        except ImportError:
            raise InputError("%s is not JSON, and reading YAML needs the yaml module (PyYAML), which is not installed" % where)
        try:
            items = yaml.safe_load(text)
        except yaml.YAMLError as e:
            raise InputError("%s is neither JSON nor YAML: %s" % (where, " ".join(str(e).split())))
    if not isinstance(items, list):
        raise InputError("%s must be a list of variants, one dict each" % where)
    variants = []
    for n, itm in enumerate(items):
        if not isinstance(itm, dict):
            raise InputError("%s, variant %d: not a dict" % (where, n))
        for key in KEYS:
            if key not in itm:
                raise InputError("%s, variant %d: no %s" % (where, n, key))
            if not isinstance(itm[key], str) and not (key == "mutSeq" and itm[key] is None):
                raise InputError("%s, variant %d: %s must be a string%s" % (where, n, key, " or null" if key == "mutSeq" else ""))
        v = parse_hgvs(itm["hgvs"])
        if v is None:
            raise InputError("%s, variant %d: unable to parse %s" % (where, n, itm["hgvs"]))
        variants.append(v)
    return items, variants


def read_index(path):
    with open(path, "rb") as f:
        data = f.read()
    try:
        text = data.decode("utf-8")
    except UnicodeDecodeError:
        raise InputError("%s is not text" % path)
    return parse_index(text, path)


def bait_of(itm):
    """hgvs-find.py:950-954"""
    b = itm["lhsFlank"] + itm["wtSeq"] + itm["rhsFlank"]
    if itm["mutSeq"] is not None:
        b += "N" + itm["lhsFlank"] + itm["mutSeq"] + itm["rhsFlank"]
    return b


# ---- k-mers on the host ------------------------------------------------------------------------------------------------------
M1 = 0x5555555555555555


def ham(x, y):
    """basics.ham (basics.py:123-133)"""
    z = x ^ y
    return bin((z | (z >> 1)) & M1).count("1")


def windows(K, seq):
    """[(k-mer, 0-based start)] of the windows of seq that hold only AaCcGgTtUu (basics.kmersWithPosList, forward strand)"""
    out, x, run, msk = [], 0, 0, (1 << (2 * K)) - 1
    for i, ch in enumerate(seq):
        b = _CODE.get(ch)
        if b is None:
            x = run = 0
            continue
        x = ((x << 2) | b) & msk
        run += 1
        if run >= K:
            out.append((x, i + 1 - K))
    return out


def render(K, x):
    return "".join("ACGT"[(x >> (2 * (K - 1 - i))) & 3] for i in range(K))


def render_path(K, xs):
    """renderPath (hgvs-find.py:471-477)"""
    return render(K, xs[0]) + "".join("ACGT"[x & 3] for x in xs[1:]) if xs else ""


def get_mask(K, i, L):
    """fixed_path_finder.get_mask (debruijn.py:341-362), as written there: position i of a path of L k-mers compares the low
    2 (i + 1) bits while i < K, and from i = L - K + 1 on drops the low 2 (i - (L - K + 1) + 1) bits"""
    full = (1 << (2 * K)) - 1
    lhs = (1 << (2 * (i + 1))) - 1 if i < K else full
    j = i - (L - K + 1)
    rhs = full if j < 0 else full ^ ((1 << (2 * (j + 1))) - 1)
    return lhs & rhs


class Segment:
    """capKmers[n]: the counted k-mers of one bait, a slice of the merged list; exact lookups are binary searches in it"""

    def __init__(self, kmers, counts):
        self.kmers, self.counts = kmers, counts

    def _at(self, x):
        i = int(np.searchsorted(self.kmers, np.uint64(x)))
        return i if i < len(self.kmers) and int(self.kmers[i]) == x else -1

    def __contains__(self, x):
        return self._at(x) >= 0

    def __getitem__(self, x):
        i = self._at(x)
        if i < 0:
            raise KeyError(x)
        return int(self.counts[i])

    def get(self, x, default=0):
        i = self._at(x)
        return int(self.counts[i]) if i >= 0 else default


class Counted:
    """the merged counted list, ascending by (bait, k-mer), and where each bait's segment lies"""

    def __init__(self, baits, kmers, counts, n_baits):
        self.baits, self.kmers, self.counts = baits, kmers, counts
        self.offs = np.searchsorted(baits, np.arange(n_baits + 1, dtype=np.uint32))

    def segment(self, n):
        lo, hi = int(self.offs[n]), int(self.offs[n + 1])
        return Segment(self.kmers[lo:hi], self.counts[lo:hi])


# ---- the capture -------------------------------------------------------------------------------------------------------------
class Emitter:
    """zk_capture_kmers + zk_pileup_count over slices of a batch's pair list.  A call that would write more than `budget`
    entries writes nothing and says how many it needs: the slice is then cut into as many even parts as that takes."""

    def __init__(self, ctx, K, budget, pileup, stats):
        self.ctx, self.K, self.budget, self.pileup, self.stats = ctx, K, int(budget), pileup, stats
        self.bufs = None

    def _room(self, n):
        n = min(max(n, 1024), self.budget)
        if self.bufs is None or self.bufs[0].n < n:
            self.bufs = (self.ctx.empty(n, np.uint32), self.ctx.empty(n, np.uint64))

    def emit(self, pairs, texts, lines, r):
        ctx, st = self.ctx, self.stats
        todo = [(0, pairs.n)]
        self._room(1 << 20)
        while todo:
            lo, hi = todo.pop()
            t0 = time.perf_counter()
            n, fit = ctx.capture_kmers_into(pairs.view(hi - lo, lo), texts[0], lines[0], r, self.K, texts[1], lines[1], *self.bufs)
            if not fit and n <= self.budget:
                self._room(n + n // 8)
                n, fit = ctx.capture_kmers_into(pairs.view(hi - lo, lo), texts[0], lines[0], r, self.K, texts[1], lines[1], *self.bufs)
            st["emission_seconds"] += time.perf_counter() - t0
            if not fit:
                if hi - lo == 1:
                    raise InputError("one read pair has %d k-mers, more than a call takes (%d)" % (n, self.budget))
                parts = min(hi - lo, n // self.budget + 2)
                cuts = [lo + (hi - lo) * i // parts for i in range(parts + 1)]
                todo += [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
                continue
            st["entries"] += n
            st["slices"] += 1
            if n == 0:
                continue
            t0 = time.perf_counter()
            counted = ctx.pileup_count(self.bufs[0].view(n), self.bufs[1].view(n), self.K)
            st["count_seconds"] += time.perf_counter() - t0
            self.pileup.add_device(*counted)


def capture_inputs(ctx, table, K, inputs, batch, budget, pileup, read_counts, stats, verbose=False):
    """reads.reads(inputs, paired=True) (reads.py:56-124): the files in pairs (0,1), (2,3), ...  A pair ends with mate 1; if
    mate 2 ends first the warning is printed (the reference meant to, at reads.py:101) and the pair ends there."""
    emitter = Emitter(ctx, K, budget, pileup, stats)
    pairs_buf = None
    for i in range(0, len(inputs) - 1, 2):
        paths = inputs[i:i + 2]
        n_reads = 0
        with contextlib.closing(record_batches(ctx, paths, batch, warn_unequal=True)) as batches:
            for texts, lines, r, _ in batches:
                t0 = time.perf_counter()
                pairs_buf = ctx.capture_hits(table, K, texts[0], lines[0], r, texts[1], lines[1], out=whole(pairs_buf))
                stats["lookup_seconds"] += time.perf_counter() - t0
                stats["batches"] += 1
                if pairs_buf.n:
                    hit = (pairs_buf.to_host() >> np.uint64(32)).astype(np.int64)
                    read_counts += np.bincount(hit, minlength=len(read_counts))
                    emitter.emit(pairs_buf, texts, lines, r)
                n_reads += r
                if verbose:
                    sys.stderr.write("%s: %d read pairs\n" % (" & ".join(os.path.basename(p) for p in paths), n_reads))
        stats["read_pairs"] += n_reads


# ---- definite alleles --------------------------------------------------------------------------------------------------------
def allele_path(K, lhs, mid, rhs):
    """the expected k-mers of an allele between K - 1 bases of either flank (consAllele, hgvs-find.py:585-588, 626-627)"""
    return [x for x, _ in windows(K, lhs[-(K - 1):] + mid + rhs[:K - 1])]


def prune(K, Y):
    """fixed_path_finder.path_kmers, step 2 (debruijn.py:385-405): candidates without a de Bruijn neighbour at the next
    (previous) position go, until nothing changes -> Y, or None when a position empties"""
    m = (1 << (2 * (K - 1))) - 1
    done = False
    while not done:
        done = True
        for j in range(1, len(Y)):
            both = {x & m for x in Y[j - 1]} & {y >> 2 for y in Y[j]}
            vs = [x for x in Y[j - 1] if (x & m) in both]
            ws = [y for y in Y[j] if (y >> 2) in both]
            if not vs or not ws:
                return None
            if len(vs) != len(Y[j - 1]):
                Y[j - 1], done = vs, False
            if len(ws) != len(Y[j]):
                Y[j], done = ws, False
    return Y


def consensus(K, ys, cs):
    """consensus_kmer (hgvs-find.py:590-611): per base the majority weighted by the counts, the lowest base on a tie; and the
    smallest of the winning weights"""
    r, c = 0, None
    for i in range(K):
        w = [0, 0, 0, 0]
        for y, n in zip(ys, cs):
            w[(y >> (2 * i)) & 3] += n
        b = 0
        for q in range(1, 4):
            if w[q] > w[b]:
                b = q
        r |= b << (2 * i)
        c = w[b] if c is None else min(c, w[b])
    return r, c


def definite_allele(K, Y, mx):
    """findFairlySimpleAllele (hgvs-find.py:625-650) from the candidates per position -> an allele, or None"""
    if not Y or any(not ys for ys in Y):
        return None
    Y = prune(K, [list(ys) for ys in Y])
    if Y is None:
        return None
    path, cov = [], []
    for ys in Y:
        y, c = consensus(K, ys, [mx[v] for v in ys])
        path.append(y)
        cov.append(c)
    return {"allele": render_path(K, path), "covMin": min(cov), "path": path, "lhsPos": 0, "rhsPos": 0}


# ---- bridged alleles ---------------------------------------------------------------------------------------------------------
def follows(K, x, y):
    return (x & ((1 << (2 * (K - 1))) - 1)) == (y >> 2)


def anchor_threshold(K, seq, mx):
    """findAnchors' cut (hgvs-find.py:521-532): a tenth-ish (e^-1.5) of the best covered flank k-mer -> (the flank's windows,
    t), t None when no flank k-mer was seen"""
    xps = windows(K, seq)
    xc = max([mx.get(x, 0) for x, _ in xps] + [0])
    if xc == 0:
        return xps, None
    return xps, int(math.exp(math.log(xc) - 1.5))


def anchors_from(K, seq, xps, zs, is_lhs):
    """findAnchors, from the neighbours zs[p] of every flank position (hgvs-find.py:555-583): a neighbour that a neighbour of
    the next position towards the variant follows on is dropped -> sorted [(k-mer, distance from the variant)]"""
    res = set()
    step = -1 if is_lhs else 1
    for _, p in (xps if is_lhs else xps[::-1]):
        for s in zs.get(p, ()):
            res.add((s, p))
            for u in zs.get(p + step, ()):
                if follows(K, u, s) if is_lhs else follows(K, s, u):
                    res.discard((u, p + step))
    if is_lhs:
        last = len(seq) - K
        return sorted((x, last - p) for x, p in res)
    return sorted(res)


def paths(K, mx, xb, xe, n):
    """Interpolator.path for an exact length (debruijn.py:98-128): the paths of n k-mers of mx from xb to xe, grown from either
    end in turn.  The reference walks dicts; here the k-mers that end the partial paths are taken in ascending order."""
    full, top = (1 << (2 * K)) - 1, 2 * (K - 1)
    fwd, rev = {xb: [[xb]]}, {xe: [[xe]]}
    for i in range(1, n + 1):
        if i == n:
            for x in sorted(set(fwd) & set(rev)):
                for a in fwd[x]:
                    for b in rev[x]:
                        yield a + b[1:]
        nxt = {}
        if i & 1 == 0:
            for x in sorted(fwd):
                for q in range(4):
                    y = ((x << 2) & full) + q
                    if y in mx:
                        nxt.setdefault(y, []).extend(p + [y] for p in fwd[x])
            fwd = nxt
        else:
            for x in sorted(rev):
                for q in range(4):
                    y = (x >> 2) + (q << top)
                    if y in mx:
                        nxt.setdefault(y, []).extend([y] + p for p in rev[x])
            rev = nxt


def bridge(K, mx, lx, lxp, rx, rxp, z):
    """findAllele (hgvs-find.py:652-664)"""
    for pth in paths(K, mx, lx, rx, z + lxp + rxp + 1 + K):
        yield {"allele": render_path(K, pth)[lxp + K:-(rxp + K)], "covMin": min(mx[x] for x in pth[lxp + 1:-(rxp + 1)]),
               "path": pth[1:-1], "lhsPos": lxp, "rhsPos": rxp}


def bridging_alleles(K, mx, lhs_anchors, rhs_anchors, v, wt, mut, err):
    """AlleleFinder.bridgingAlleles (hgvs-find.py:758-798) -> [(kind, allele)] in the order of its loops"""
    out = []
    wtZ, mutZ, longest = len(wt), v.size(), 4 * K
    if len(lhs_anchors) * len(rhs_anchors) > 10:
        err.write("warning: highly ambiguous anchors for %s\n%d\tlhs anchors, and %d rhs anchors\n" % (v, len(lhs_anchors), len(rhs_anchors)))
    for lx, lxp in lhs_anchors:
        for rx, rxp in rhs_anchors:
            if wtZ == mutZ:
                if wtZ > longest:
                    err.write("warning: cannot bridge alleles because they are too long (%d) for %s\n" % (wtZ, v))
                    continue
                for a in bridge(K, mx, lx, lxp, rx, rxp, wtZ):
                    if a["allele"] == wt:
                        out.append(("wt", a))
                    elif mut is None or a["allele"] == mut:
                        out.append(("mut", a))
                continue
            if wtZ > longest:
                err.write("warning: cannot bridge wt allele because it is too long (%d) for %s\n" % (wtZ, v))
                continue
            for a in bridge(K, mx, lx, lxp, rx, rxp, wtZ):
                if a["allele"] == wt:
                    out.append(("wt", a))
            if mutZ > longest:
                err.write("warning: cannot bridge mut allele because it is too long (%d) for %s\n" % (mutZ, v))
                continue
            for a in bridge(K, mx, lx, lxp, rx, rxp, mutZ):
                if mut is None or a["allele"] == mut:
                    out.append(("mut", a))
    return out


# ---- scores ------------------------------------------------------------------------------------------------------------------
def _log_fac(n):
    """stats.logFac (stats.py:77-83)"""
    if n < 25:
        return math.log(math.factorial(n))
    return n * math.log(n) - n + math.log(n * (1 + 4 * n * (1 + 2 * n))) / 6.0 + math.log(math.pi) / 2.0


def _log_bin_eq(p, n, k):
    choose = 0 if k == 0 or k == n else _log_fac(n) - (_log_fac(n - k) + _log_fac(k))
    return choose + math.log(p) * k + math.log1p(-p) * (n - k)


def _log_bin_le(p, n, k):
    """stats.logBinLe (stats.py:199-212): the terms added from k downwards"""
    v = _log_bin_eq(p, n, k)
    for i in range(k - 1, -1, -1):
        w = _log_bin_eq(p, n, i)
        hi, lo = max(v, w), min(v, w)
        v = hi + math.log1p(math.exp(lo - hi))
    return v


def _cdf(pdf):
    """stats.pdf2cdf: P(X < i)"""
    t, out = 0, []
    for x in pdf:
        out.append(t)
        t += x
    return out


class Scorer:
    """Scorer (hgvs-find.py:679-711): the Hamming profile of an allele's path against the expected one, its one-sided
    Kolmogorov-Smirnov distance from the profile of random k-mers, the base-wise Hamming distance of the alleles, and the
    binomial score"""

    def __init__(self, K):
        self.K = K
        self.null_cdf = _cdf([math.exp(_log_bin_eq(0.25, K, j)) for j in range(K + 1)])
        self.bin_model = [1 - math.exp(_log_bin_le(0.25, K, d)) for d in range(K + 1)]

    def score(self, res, lhs, seq, rhs):
        K, xs = self.K, res["path"]
        prof = [0] * (K + 1)
        lp, rp = K - 1 + res["lhsPos"], K - 1 + res["rhsPos"]
        if seq is None:
            want = lhs[-lp:] + len(res["allele"]) * "N" + rhs[:rp]
            prof[0] += len(xs)
        else:
            want = lhs[-lp:] + seq + rhs[:rp]
            for x, (y, _) in zip(xs, windows(K, want)):
                prof[ham(x, y)] += 1
        total = max(1, sum(prof))
        cdf = _cdf([float(c) / total for c in prof])
        res["ksDist"] = max([0] + [a - b for a, b in zip(cdf, self.null_cdf)])
        got = render_path(K, xs)
        res["hamming"] = sum(1 for i in range(len(want)) if want[i] != got[i] and want[i] != "N" and got[i] != "N")
        p = 1.0
        for d in range(K + 1):
            p *= math.pow(self.bin_model[d], prof[d])
        res["binom"] = 1.0 - p


def best_allele(scorer, alleles, lhs, seq, rhs):
    """hgvs-find.py:1033-1053 with isBetter (713-720): more coverage wins, then fewer mismatches; the later one on a tie"""
    res = {"covMin": 0, "binom": 1.0, "ksDist": 0.0, "hamming": 0, "path": []}
    for a in alleles:
        scorer.score(a, lhs, seq, rhs)
        if a["covMin"] > res["covMin"] or (a["covMin"] == res["covMin"] and a["hamming"] <= res["hamming"]):
            res = a
    return res


def _median(mx, path):
    xs = sorted(mx.get(x, 0) for x in path) or [0]
    return xs[len(xs) // 2]


# ---- the scans ---------------------------------------------------------------------------------------------------------------
def scan(ctx, dev, K, wins):
    """one zk_path_scan -> per window the entry indices (into the merged list) of its matches, ascending"""
    if not wins or dev is None:
        return [np.empty(0, np.uint32)] * len(wins)
    w, e = ctx.path_scan(dev[0], dev[1], dev[2], K, wins)
    cuts = np.searchsorted(w, np.arange(len(wins) + 1, dtype=np.uint32))
    return [e[cuts[i]:cuts[i + 1]] for i in range(len(wins))]


def device_list(ctx, pileup, what):
    """the merged list of a DevicePileup as the entries after it take it: (baits, k-mers, counts u32) on the device, None if
    it is empty; a count beyond 32 bits is refused"""
    baits, kmers, counts = pileup.device_result()
    if baits.n == 0:
        return None
    narrow, mx = ctx.narrow_counts(counts)
    if mx >= 1 << 32:
        raise InputError("a k-mer was counted %d times, more than the %s's 32-bit counts hold" % (mx, what))
    return baits, kmers, narrow


def call_variants(ctx, items, variants, counted, read_counts, K, D, Q, V, fmt, out, err, stats, dev=None):
    """hgvs-find.py:969-1131 over the merged list.  dev: the list on the device (device_list), else it is uploaded"""
    t0 = time.perf_counter()
    if dev is None and len(counted.baits):
        if int(counted.counts.max()) >= 1 << 32:
            raise InputError("a k-mer was counted %d times, more than the scan's 32-bit counts hold" % int(counted.counts.max()))
        dev = (ctx.upload(counted.baits), ctx.upload(counted.kmers), ctx.upload(counted.counts.astype(np.uint32)))
    segs = [counted.segment(n) for n in range(len(items))]
    # every position of every definite path: one scan
    wins, owner = [], []
    for n, (itm, v) in enumerate(zip(items, variants)):
        if v.anonymous():
            continue
        for kind, mid in (("wt", itm["wtSeq"]), ("mut", itm["mutSeq"])):
            if mid is None:
                continue
            xs = allele_path(K, itm["lhsFlank"], mid, itm["rhsFlank"])
            owner.append((n, kind, len(wins), len(xs)))
            if D > 0:
                wins += [(n, x, get_mask(K, i, len(xs)), D - 1, 0) for i, x in enumerate(xs)]
    found = scan(ctx, dev, K, wins) if D > 0 else []
    stats["path_windows"] = len(wins)
    stats["path_matches"] = int(sum(len(f) for f in found))
    candidates = {}
    for n, kind, first, L in owner:
        candidates[(n, kind)] = [counted.kmers[found[first + i]].tolist() for i in range(L)] if D > 0 else None
    # the anchors of the anonymous variants: one more scan
    wins, flanks = [], {}
    for n, (itm, v) in enumerate(zip(items, variants)):
        if not v.anonymous():
            continue
        for is_lhs, seq in ((True, itm["lhsFlank"]), (False, itm["rhsFlank"])):
            xps, t = anchor_threshold(K, seq, segs[n])
            at = {}
            if t is not None and D >= 0:
                for x, p in xps:
                    if segs[n].get(x, -1) >= t:
                        at[p] = len(wins)
                        wins.append((n, x, 0, D, t))
            flanks[(n, is_lhs)] = (seq, xps, at)
    found = scan(ctx, dev, K, wins)
    stats["anchor_windows"] = len(wins)
    t1 = time.perf_counter()
    stats["path_scan_seconds"] += t1 - t0

    scorer = Scorer(K)
    header = False
    for n, (itm, v) in enumerate(zip(items, variants)):
        mx = segs[n]
        if "kmers" in fmt:
            for x, c in zip(mx.kmers.tolist(), mx.counts.tolist()):
                sys.stdout.write("%d\t%s\t%d\n" % (n, render(K, x), c))
        lhs, rhs, wt, mut = itm["lhsFlank"], itm["rhsFlank"], itm["wtSeq"], itm["mutSeq"]
        cs = np.sort(mx.counts[mx.counts >= np.uint64(max(Q, 0))]).tolist()
        nk = len(cs)
        cs = cs or [0]
        q10, q50, q90 = cs[len(cs) // 10], cs[5 * len(cs) // 10], cs[9 * len(cs) // 10]
        alleles = {"wt": [], "mut": []}
        if not v.anonymous():
            for kind in ("wt", "mut"):
                if (n, kind) in candidates:
                    a = definite_allele(K, candidates[(n, kind)], mx)
                    if a is not None:
                        alleles[kind].append(a)
        else:
            anc = []
            for is_lhs in (True, False):
                seq, xps, at = flanks[(n, is_lhs)]
                zs = {p: (set(counted.kmers[found[at[p]]].tolist()) if p in at else set()) for _, p in xps}
                anc.append(anchors_from(K, seq, xps, zs, is_lhs))
            for kind, a in bridging_alleles(K, mx, anc[0], anc[1], v, wt, mut, err):
                alleles[kind].append(a)
        w = best_allele(scorer, alleles["wt"], lhs, wt, rhs)
        m = best_allele(scorer, alleles["mut"], lhs, mut, rhs)
        wmed, mmed = _median(mx, w["path"]), _median(mx, m["path"])
        tot = max(1.0, float(wmed + mmed), float(q90))
        wvaf, mvaf = wmed / tot, mmed / tot
        res = 1 * (w["covMin"] > Q and w["hamming"] < 4 and wvaf > V) + 2 * (m["covMin"] > Q and m["hamming"] < 4 and mvaf > V)
        cols = [("n", "%d", n), ("res", "%s", ("null", "wt", "mut", "wt/mut")[res])]
        if "rds" in fmt:
            cols.append(("numReads", "%d", int(read_counts[n])))
        cols += [("numKmers", "%d", nk), ("covQ10", "%d", q10), ("covQ50", "%d", q50), ("covQ90", "%d", q90),
                 ("wtMin", "%d", w["covMin"]), ("mutMin", "%d", m["covMin"]), ("wtHam", "%d", w["hamming"]), ("mutHam", "%d", m["hamming"])]
        if "ks" in fmt:
            cols += [("wtD", "%g", w["ksDist"]), ("mutD", "%g", m["ksDist"])]
        if "binom" in fmt:
            cols += [("wtQ", "%g", w["binom"]), ("mutQ", "%g", m["binom"])]
        if "vaf" in fmt:
            cols += [("wtVaf", "%g", wvaf), ("mutVaf", "%g", mvaf)]
        cols.append(("hgvs", "%s", itm["hgvs"]))
        if not header:
            out.write("\t".join(c[0] for c in cols) + "\n")
            header = True
        out.write("\t".join(c[1] % c[2] for c in cols) + "\n")
        out.flush()
    stats["allele_seconds"] += time.perf_counter() - t1


def new_stats():
    return dict(read_pairs=0, batches=0, slices=0, entries=0, lookup_seconds=0.0, emission_seconds=0.0, count_seconds=0.0, merge_seconds=0.0,
                path_scan_seconds=0.0, allele_seconds=0.0, distinct_entries=0, path_windows=0, path_matches=0, anchor_windows=0)


def run(ctx, items, variants, inputs, K, D, Q, V, fmt, batch, out, budget=EMIT_BUDGET, verbose=False, err=None, stats=None, pileup=None):
    """the whole command behind its argument checks.  pileup: where the counted lists gather (None: a DevicePileup)"""
    err = err or sys.stderr
    stats = stats if stats is not None else new_stats()
    for k, v in new_stats().items():
        stats.setdefault(k, v)
    pileup = pileup if pileup is not None else DevicePileup(ctx)
    read_counts = np.zeros(len(items), dtype=np.int64)
    if items:
        if verbose:
            err.write("loading index.\n")
        table = capture.build_table(ctx, [(itm["hgvs"].encode(), bait_of(itm).encode("latin-1")) for itm in items], K)
        if verbose:
            err.write("done.\n")
        try:
            capture_inputs(ctx, table, K, inputs, batch, budget, pileup, read_counts, stats, verbose)
        finally:
            table.free()
    baits, kmers, counts = pileup.result()
    stats["merge_seconds"] = pileup.merge_seconds
    stats["merges"] = pileup.merges
    stats["distinct_entries"] = len(baits)
    counted = Counted(baits, kmers, counts, len(items))
    dev = device_list(ctx, pileup, "scan") if isinstance(pileup, DevicePileup) else None
    call_variants(ctx, items, variants, counted, read_counts, K, D, Q, V, fmt, out, err, stats, dev=dev)
    return 0
