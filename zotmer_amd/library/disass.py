"""
`zot disass` on the device (zotmer/commands/disass.py): the spectrum of k-mer multiplicities of every contig of an assembly,
and of the whole file.

The reference walks every record's k-mers (basics.kmersList, both strands unless -s, each kept iff basics.sub says so) through
a dict, and every record's dict through a second one for the file (disass.py:86-100); summarize (disass.py:27-64) then sorts
the dict's values.  Here whole records are packed into batches under a window budget, every batch is ONE zk_contig_spectra
(csrc/contig_spectra.hip): all its records' histograms in one array of record << 32 | count words, and the batch's counted key
list; the key lists are union-summed on a stack like a binary counter (strand.StrandTable, engine.KmerTable), and one
zk_count_spectrum at the end turns the file's table into the global histogram.  What summarize computes needs only the
histogram: summarize_bins works on the ascending (count, frequency) bins, on the host.
"""
import re

import numpy as np

from zotmer_amd.library import seqio
from zotmer_amd.library.timing import Phase

DEFAULTS = dict(K=25, C=5, P=1.0, Q=10, S=17)      # disass.py:8-13
WINDOW_BUDGET = 1 << 27         # windows per batch when nothing else is asked for
MAX_WINDOWS = (1 << 31) - 1     # of one zk_contig_spectra
BYTES_PER_WINDOW = 96           # workspace (72 B per stream byte), the outputs at their first capacities, the stream itself
WIDEN_AT = 1 << 32              # window total of a merge from which its counts are 64 bits wide (StrandTable's rule)


class TooLarge(ValueError):
    pass


# ---- summarize (host) -------------------------------------------------------------------------------------------------------

def _value_at(bins, i):
    """element i of the sorted list of counts that the bins stand for"""
    cum = 0
    for c, f in bins:
        cum += f
        if i < cum:
            return c
    raise IndexError(i)


def summarize_bins(bins, cut, Q):
    """summarize (disass.py:27-64) from the ascending (count, frequency) bins of the dict's values: the same float expressions
    in the same order.  Two differences: the quantile loop walks the bins in ascending count (the reference walks its dict's
    order), and exactly one value gives median = float(value) (the reference's cs[m + 1] raises IndexError)."""
    bins = [(int(c), int(f)) for c, f in bins]
    n = sum(f for _, f in bins)
    total = sum(c * f for c, f in bins)
    res = {}
    res["histogram"] = [[c, f] for c, f in bins]
    res["mean"] = float(total) / float(max(1, n))
    res["median"] = 0
    if n > 0:
        if (n & 1) == 0:
            res["median"] = _value_at(bins, n // 2)
        elif n == 1:
            res["median"] = float(bins[0][0])
        else:
            m = n // 2
            res["median"] = (_value_at(bins, m) + _value_at(bins, m + 1)) / 2.0
    res["low-count"] = 0
    res["high-count"] = 0
    t = float(n)
    q0 = t / Q
    q = q0
    quant = []
    cum = 0
    for c, f in bins:
        if c < cut:
            res["low-count"] += f
        else:
            res["high-count"] += f
        while cum + f > q:
            quant.append(c)
            q += q0
        cum += f
    res["quantiles"] = quant
    return res


# ---- YAML (host) ------------------------------------------------------------------------------------------------------------

_PLAIN = re.compile(r"^[A-Za-z_/][A-Za-z0-9_./+=@|-]*(?: [A-Za-z0-9_./+=@|][A-Za-z0-9_./+=@|-]*)*$")
_WORDS = {"y", "n", "yes", "no", "true", "false", "on", "off", "null"}      # what YAML 1.1 reads as something else


def _scalar(v):
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, int):
        return str(v)
    if isinstance(v, float):
        s = repr(v)
        if "." not in s and "e" in s:           # YAML 1.1 wants the point: 1e+16 would load as a string
            s = s.replace("e", ".0e", 1)
        return s
    s = str(v)
    if _PLAIN.match(s) and s.lower() not in _WORDS:
        return s
    out = ['"']
    for ch in s:
        o = ord(ch)
        if ch in '"\\':
            out.append("\\" + ch)
        elif ch == "\n":
            out.append("\\n")
        elif ch == "\t":
            out.append("\\t")
        elif o < 0x20 or 0x7f <= o <= 0xa0 or 0xd800 <= o <= 0xdfff or o in (0x2028, 0x2029, 0xfeff, 0xfffe, 0xffff):
            out.append("\\u%04x" % o)
        else:
            out.append(ch)
    out.append('"')
    return "".join(out)


def _is_leaf(v):
    return not isinstance(v, (list, tuple, dict))


def _flow(v):
    if isinstance(v, (list, tuple)):
        return "[" + ", ".join(_flow(x) for x in v) + "]"
    return _scalar(v)


def _emit(v, indent, out):
    """v, a non-empty block collection, at `indent` (lists sit at their parent key's indent, as PyYAML writes them)"""
    pad = " " * indent
    if isinstance(v, dict):
        for k in sorted(v):
            x = v[k]
            if _is_leaf(x) or not x or (isinstance(x, (list, tuple)) and all(_is_leaf(y) for y in x)):
                out.append("%s%s: %s\n" % (pad, _scalar(k), _flow(x) if not isinstance(x, dict) else "{}"))
            else:
                out.append("%s%s:\n" % (pad, _scalar(k)))
                _emit(x, indent if isinstance(x, (list, tuple)) else indent + 2, out)
    else:
        for x in v:
            if _is_leaf(x) or not x or (isinstance(x, (list, tuple)) and all(_is_leaf(y) for y in x)):
                out.append("%s- %s\n" % (pad, _flow(x) if not isinstance(x, dict) else "{}"))
            else:
                sub = []
                _emit(x, indent + 2, sub)
                out.append(pad + "- " + sub[0][indent + 2:])
                out.extend(sub[1:])


def dump_yaml(res):
    """yaml.safe_dump(res) for the structure disass.py:81-103 builds: keys sorted, block style except for the lists of
    scalars (flow style), strings plain where that is safe and double-quoted otherwise.  Flow lists are not wrapped."""
    if _is_leaf(res) or not res:
        return (_flow(res) if not isinstance(res, dict) else "{}") + "\n"
    if isinstance(res, (list, tuple)) and all(_is_leaf(y) for y in res):
        return _flow(res) + "\n"
    out = []
    _emit(res, 0, out)
    return "".join(out)


# ---- batches (host) ---------------------------------------------------------------------------------------------------------

def windows_of(length, K):
    return max(0, length - K + 1)


def pack_batches(records, K, budget, limit):
    """whole records (name, sequence) packed into batches of at most `budget` windows (a window bound: bases - K + 1); a record
    of more gets a batch of its own; one of more than `limit` windows cannot be counted -> lists of (name, sequence)"""
    batch, w = [], 0
    for nm, seq in records:
        n = windows_of(len(seq), K)
        if n > limit:
            raise TooLarge('record "%s" has %d windows of %d bases, the device takes %d in one batch' % (nm, n, K, limit))
        if batch and w + n > budget:
            yield batch
            batch, w = [], 0
        batch.append((nm, seq))
        w += n
    if batch:
        yield batch


def device_limit(ctx):
    """the windows one zk_contig_spectra can take on this device"""
    free, _ = ctx.mem_info()
    return max(1, min(MAX_WINDOWS, int(free * 0.6) // BYTES_PER_WINDOW))


# ---- the device path --------------------------------------------------------------------------------------------------------

class KeyTable:
    """The file's counted key list: the batches' lists on a stack, union-summed pairwise like a binary counter.  Counts stay
    32 bits wide while the windows counted into the two tables of a merge add up to less than WIDEN_AT."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.stack = []             # [(keys, counts, level, windows counted into it)]

    def add(self, keys, counts, windows):
        if keys.n == 0:
            return
        self.stack.append((self.ctx.copy_of(keys), self.ctx.copy_of(counts), 0, int(windows)))
        while len(self.stack) >= 2 and self.stack[-1][2] == self.stack[-2][2]:
            self._merge_top()

    def _merge_top(self):
        ctx = self.ctx
        bk, bc, lb, wb = self.stack.pop()
        ak, ac, la, wa = self.stack.pop()
        if wa + wb >= WIDEN_AT or ac.dtype.itemsize == 8 or bc.dtype.itemsize == 8:
            ac = ac if ac.dtype.itemsize == 8 else ctx.widen(ac)
            bc = bc if bc.dtype.itemsize == 8 else ctx.widen(bc)
        with Phase(ctx, "union_sum %d + %d" % (ak.n, bk.n)):
            mk, mc = ctx.union_sum(ak, ac, bk, bc)
            ctx.sync()
        self.stack.append((mk, mc, max(la, lb) + 1, wa + wb))

    def result(self):
        if not self.stack:
            return self.ctx.empty(0, np.uint64), self.ctx.empty(0, np.uint32)
        while len(self.stack) > 1:
            self._merge_top()
        return self.stack[0][0], self.stack[0][1]


def spectra(ctx, records, K, both=True, seed=17, p=1.0, budget=None):
    """records: (name, sequence bytes) of one file, in order -> (names, per record the ascending (count, frequency) bins of its
    dict, the bins of the file's dict)"""
    limit = device_limit(ctx)
    budget = min(limit, int(budget) if budget else WINDOW_BUDGET)
    names, bins = [], []
    table = KeyTable(ctx)
    for batch in pack_batches(records, K, budget, limit):
        first = len(names)
        names.extend(nm for nm, _ in batch)
        bins.extend([] for _ in batch)
        stream = b"".join(seq + b"\n" for _, seq in batch)
        with Phase(ctx, "upload (%d records)" % len(batch), len(stream)):
            d = ctx.upload_stream(stream)
        with Phase(ctx, "contig spectra", len(stream)):
            words, freq, keys, counts, st = ctx.contig_spectra(d, K, both, seed, p)
        assert st.n_records == len(batch)
        with Phase(ctx, "download bins", 16 * words.n):
            w, f = words.to_host(), freq.to_host()
        for rec, c, fr in zip((w >> np.uint64(32)).tolist(), (w & np.uint64(0xffffffff)).tolist(), f.tolist()):
            bins[first + rec].append((c, fr))
        table.add(keys, counts, st.n_windows)
        del d, words, freq, keys, counts
    gk, gc = table.result()
    with Phase(ctx, "global spectrum", gk.n * (8 + gc.dtype.itemsize)):
        glob = ctx.count_spectrum(gk, gc, K, both, seed, p)
    return names, bins, glob


def file_result(ctx, path, K, C, Q, both=True, seed=17, p=1.0, budget=None):
    """disass.py:83-101 for one file"""
    names, bins, glob = spectra(ctx, seqio.fasta_records(path), K, both, seed, p, budget)
    contigs = []
    for nm, b in zip(names, bins):
        s = summarize_bins(b, C, Q)
        s["name"] = nm
        contigs.append(s)
    return {"file": path, "contigs": contigs, "global": summarize_bins(glob, C, Q)}
