"""
`zot hgvs-index`: what the reference's `hgvs-find -X` and `-X -T` do (zotmer/commands/hgvs-find.py:838-915).

Indexing is host work.  Every `g.` HGVS string becomes an object with the range it replaces, the sequence it puts there and
its canonical spelling (library/hgvs.py:204-594); the chromosome is loaded (SequenceFactory, hgvs-find.py:800-818: the first
record of <home>/<stem>.fa.gz), and makeIndexedVariant / context (hgvs-find.py:479-511) cut the flanks and the wild-type
allele from it.  The index is the list of those dicts, written as yaml.safe_dump writes it (dump_yaml below: PyYAML is
optional in this project).

Testing (-T) asks how often the genome holds the k-mers of every allele: per distinct variant two records, lhs[-(K-1):] + wt +
rhs[:K-1] and the same around the mutant, whose K-mers of both strands are exactly a bait table (zk_bait_table_build).  The
reference then walks kmers(K, seq) over every chromosome and bumps a dict (hgvs-find.py:884-891): hours of Python.  Here the
sequence files stream through a zk_source in batches and every batch is one zk_sequence_tally (csrc/seq_tally.hip), which
adds to one u64 per key; inflating, the copies and the kernel overlap.  The fold over strands and the histograms per record
(hgvs-find.py:892-908) are numpy on a few hundred thousand keys.  What is printed does not depend on where the batches are cut.
"""
import os
import re
import sys
import time

import numpy as np

from zotmer_amd.library import hgvsfind
from zotmer_amd.library.hgvsfind import InputError

DEFAULT_BATCH = 64 << 20
_RC = {"A": "T", "C": "G", "G": "C", "T": "A"}       # align.rcDict: every other character stays


# ---- YAML --------------------------------------------------------------------------------------------------------------------
# yaml.safe_dump(x, default_flow_style=False) for lists and dicts of strings without blanks, ints and None: block style, keys
# sorted, a string plain unless PyYAML's emitter (analyze_scalar) or its YAML 1.1 resolver says otherwise, then single-quoted.
_NOT_STR = re.compile(
    r"^(?:yes|Yes|YES|no|No|NO|true|True|TRUE|false|False|FALSE|on|On|ON|off|Off|OFF"                                  # bool
    r"|~|null|Null|NULL"                                                                                               # null
    r"|[-+]?(?:[0-9][0-9_]*)\.[0-9_]*(?:[eE][-+][0-9]+)?|\.[0-9][0-9_]*(?:[eE][-+][0-9]+)?"                            # float
    r"|[-+]?[0-9][0-9_]*(?::[0-5]?[0-9])+\.[0-9_]*|[-+]?\.(?:inf|Inf|INF)|\.(?:nan|NaN|NAN)"
    r"|[-+]?0b[0-1_]+|[-+]?0[0-7_]+|[-+]?(?:0|[1-9][0-9_]*)|[-+]?0x[0-9a-fA-F_]+|[-+]?[1-9][0-9_]*(?::[0-5]?[0-9])+"   # int
    r"|[0-9][0-9][0-9][0-9]-[0-9][0-9]-[0-9][0-9]"                                                                     # timestamp
    r"|[0-9][0-9][0-9][0-9]-[0-9][0-9]?-[0-9][0-9]?[Tt][0-9][0-9]?:[0-9][0-9]:[0-9][0-9](?:\.[0-9]*)?(?:Z|[-+][0-9][0-9]?(?::[0-9][0-9])?)?"
    r"|<<|=|!|&|\*)$")                                                                                                 # merge, value, yaml
_SIMPLE_KEY = 123        # PyYAML writes a key as `? key` from this length on (128 less the 5 of its tag, '!!str')


def _plain(s):
    if not s or s.startswith("---") or s.startswith("..."):
        return False
    if s[0] in "#,[]{}&*!|>'\"%@`" or (s[0] in "?:-" and len(s) == 1) or s[-1] == ":":
        return False
    return _NOT_STR.match(s) is None


def scalar(v):
    if v is None:
        return "null"
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, (int, np.integer)):
        return str(int(v))
    if any(not "!" <= ch <= "~" for ch in v):
        raise ValueError("a string with a blank or a character outside ASCII: %r" % v)
    return v if _plain(v) else "'" + v.replace("'", "''") + "'"


def _emit(v, indent, out):
    """v, a non-empty list or dict, as block lines at `indent` (a list sits at its parent key's indent, as PyYAML writes it)"""
    pad = " " * indent
    if isinstance(v, dict):
        keys = sorted(v)
        for k in keys:
            x, ks = v[k], scalar(k)
            simple = not (isinstance(k, str) and (len(k) >= _SIMPLE_KEY or not k))
            if not isinstance(x, (list, dict)) or not x:
                val = scalar(x) if not isinstance(x, (list, dict)) else ("[]" if isinstance(x, list) else "{}")
                out.append("%s%s: %s\n" % (pad, ks, val) if simple else "%s? %s\n%s: %s\n" % (pad, ks, pad, val))
            elif simple:
                out.append("%s%s:\n" % (pad, ks))
                _emit(x, indent if isinstance(x, list) else indent + 2, out)
            else:
                sub = []
                _emit(x, indent + 2, sub)
                out.append("%s? %s\n" % (pad, ks))
                out.append(pad + ": " + sub[0][indent + 2:])
                out.extend(sub[1:])
    else:
        for x in v:
            if not isinstance(x, (list, dict)) or not x:
                out.append("%s- %s\n" % (pad, scalar(x) if not isinstance(x, (list, dict)) else ("[]" if isinstance(x, list) else "{}")))
            else:
                sub = []
                _emit(x, indent + 2, sub)
                out.append(pad + "- " + sub[0][indent + 2:])
                out.extend(sub[1:])


def dump_yaml(v):
    if not isinstance(v, (list, dict)):
        raise TypeError("dump_yaml takes a list or a dict")
    if not v:
        return "[]\n" if isinstance(v, list) else "{}\n"
    out = []
    _emit(v, 0, out)
    return "".join(out)


# ---- variants ----------------------------------------------------------------------------------------------------------------
class IndexVariant(hgvsfind.Variant):
    """hgvsfind.Variant with what indexing needs (library/hgvs.py:204-594): the accession, range() -- the 0-based half-open
    interval of the reference the variant replaces --, sequence(big) -- what it puts there, None for insALU -- and the
    canonical spelling as str()."""

    def __init__(self, text, kind, size, acc, fst, lst, arg):
        hgvsfind.Variant.__init__(self, text, kind, size)
        self.acc, self.fst, self.lst, self.arg = acc, fst, lst, arg

    def range(self):
        if self.kind in ("ins", "insN", "insALU"):
            return (self.lst, self.lst)             # bef = pos1 - 1: the reference takes the second position alone
        if self.kind == "sub":
            return (self.fst, self.fst + 1)
        return (self.fst, self.lst + 1)

    def cryptic(self):
        return self.kind == "insALU"

    def sequence(self, big):
        k = self.kind
        if k == "sub":
            return self.arg[1]
        if k == "del":
            return ""
        if k in ("ins", "delins"):
            return self.arg
        if k in ("insN", "delinsN"):
            return self.arg * "N"
        if k == "insALU":
            return None
        ref = big[self.fst:self.lst + 1].upper()
        if k == "dup":
            return 2 * ref
        if k == "repeat":
            return self.arg * ref
        return "".join(_RC.get(c, c) for c in ref)[::-1]      # inv: align.revComp

    def __str__(self):
        a, f, l, k = self.acc, self.fst + 1, self.lst + 1, self.kind
        if k == "sub":
            return "%s:g.%d%s>%s" % (a, f, self.arg[0], self.arg[1])
        if k in ("ins", "insN", "insALU"):
            return "%s:g.%d_%dins%s" % (a, self.lst, self.lst + 1, "ALU" if k == "insALU" else self.arg)
        if k == "inv":
            return "%s:g.%d_%dinv" % (a, f, l)
        tail = {"del": "del", "dup": "dup", "delins": "delins%s" % self.arg, "delinsN": "delins%s" % self.arg,
                "repeat": "[%s]" % self.arg}[k]
        return "%s:g.%d%s" % (a, f, tail) if f == l else "%s:g.%d_%d%s" % (a, f, l, tail)


_POS = re.compile(r"([^:]+):g\.([0-9]+)(?:_([0-9]+))?(.*)$", re.S)


def make_variant(text):
    """hgvs.makeHGVS (hgvs.py:609-712) on the grammar of hgvsfind.parse_hgvs -> IndexVariant, or None"""
    v = hgvsfind.parse_hgvs(text)
    m = _POS.match(text)
    if v is None or m is None:
        return None
    acc, pos0, pos1, tail = m.group(1), int(m.group(2)), m.group(3), m.group(4)
    kind = v.kind
    if kind == "sub":
        fst = lst = pos0 - 1
        arg = (tail[0], tail[2])
    elif kind == "repeat":
        bases = tail[:tail.index("[")]
        last = int(pos1) if pos1 is not None else (pos0 + len(bases) - 1 if bases else pos0)
        fst, lst, arg = pos0 - 1, last - 1, int(tail[tail.index("[") + 1:-1])
    else:
        fst, lst = pos0 - 1, (int(pos1) if pos1 is not None else pos0) - 1
        arg = None
        if kind in ("ins", "delins"):
            arg = tail[len(kind):]
        elif kind in ("insN", "delinsN"):
            arg = int(tail[len(kind) - 1:])
    size = v.size()
    if kind == "repeat":
        size = arg * (lst - fst + 1)          # Repeat.size from the positions the bases imply as well
    return IndexVariant(text, kind, size, acc, fst, lst, arg)


# ---- the reference sequences -------------------------------------------------------------------------------------------------
def read_names(path):
    """-n: 'accession  file-stem' per line -> {accession: stem}, in file order"""
    names = {}
    with open(path) as f:
        for n, line in enumerate(f, 1):
            w = line.split()
            if not w or w[0].startswith("#"):
                continue
            if len(w) != 2:
                raise InputError("%s, line %d: expected an accession and a file stem" % (path, n))
            names[w[0]] = w[1]
    return names


class Home:
    """SequenceFactory (hgvs-find.py:800-818): accession -> the first record of <home>/<stem>.fa.gz, else <stem>.fa, the stem
    being what -n names for the accession, else the accession itself.  Keeps the last one, as the reference does."""

    def __init__(self, home, names=None):
        self.home, self.names = home, dict(names or {})
        self.prev = (None, None)

    def path(self, acc):
        stem = os.path.join(self.home, self.names.get(acc, acc))
        for p in (stem + ".fa.gz", stem + ".fa"):
            if os.path.isfile(p):
                return p
        raise InputError("no sequence file for %s: neither %s.fa.gz nor %s.fa" % (acc, stem, stem))

    def __getitem__(self, acc):
        if self.prev[0] != acc:
            from zotmer_amd.library import seqio
            path = self.path(acc)
            for _, seq in seqio.fasta_records(path):
                if isinstance(seq, bytes):
                    seq = seq.decode("latin-1")
                self.prev = (acc, seq)
                break
            else:
                raise InputError("%s holds no FASTA record" % path)
        return self.prev[1]

    def files(self):
        """the files -T scans: with -n exactly the ones it names, in its order and each once; else every *.fa.gz / *.fa of the
        directory in name order (a stem with both takes the .fa.gz, as loading does)"""
        if self.names:
            out = []
            for acc in self.names:
                p = self.path(acc)
                if p not in out:
                    out.append(p)
            return out
        stems = set()
        for nm in os.listdir(self.home):
            for ext in (".fa.gz", ".fa"):
                if nm.endswith(ext) and len(nm) > len(ext):
                    stems.add(nm[:-len(ext)])
                    break
        return [os.path.join(self.home, s + (".fa.gz" if os.path.isfile(os.path.join(self.home, s + ".fa.gz")) else ".fa")) for s in sorted(stems)]


def context(rng, W, seq):
    """hgvs-find.py:479-489, slices as Python cuts them"""
    lhs = seq[max(0, rng[0] - W):rng[0]].upper()
    rhs = seq[rng[1]:min(rng[1] + W, len(seq))].upper()
    return lhs, rhs


def indexed_variant(v, W, seq):
    """makeIndexedVariant (hgvs-find.py:491-511)"""
    rng = v.range()
    lhs, rhs = context(rng, W, seq)
    mut = None if v.anonymous() or v.cryptic() else v.sequence(seq).upper()
    return {"hgvs": str(v), "lhsFlank": lhs, "rhsFlank": rhs, "wtSeq": seq[rng[0]:rng[1]].upper(), "mutSeq": mut}


def make_items(texts, home, W, err=None):
    """hgvs-find.py:847-868: the strings parsed (an unparsable one is reported and skipped), grouped by accession in order of
    first appearance, each made into its dict -> (items, variants)"""
    err = err or sys.stderr
    groups = {}
    for t in texts:
        v = make_variant(t)
        if v is None:
            err.write("unable to parse %s\n" % t)
            continue
        if any(not "!" <= ch <= "~" for ch in t):
            raise InputError("%r: a blank or a character outside ASCII in a variant" % t)
        groups.setdefault(v.acc, []).append(v)
    items, variants = [], []
    for acc, vs in groups.items():
        for v in vs:
            items.append(indexed_variant(v, W, home[acc]))
            variants.append(v)
    return items, variants


# ---- -T ----------------------------------------------------------------------------------------------------------------------
def test_records(items, K):
    """per distinct hgvs, in order of first appearance: (hgvs, wt record, mut record ('' where mutSeq is null))"""
    seen, out = set(), []
    for itm in items:
        if itm["hgvs"] in seen:
            continue
        seen.add(itm["hgvs"])
        lhs, rhs = itm["lhsFlank"][-(K - 1):], itm["rhsFlank"][:K - 1]
        out.append((itm["hgvs"], lhs + itm["wtSeq"] + rhs, lhs + itm["mutSeq"] + rhs if itm["mutSeq"] is not None else ""))
    return out


def rc_keys(K, x):
    """basics.rc on a uint64 array"""
    x = ~np.asarray(x, dtype=np.uint64)
    m2, m4 = np.uint64(0x3333333333333333), np.uint64(0x0F0F0F0F0F0F0F0F)
    x = ((x >> np.uint64(2)) & m2) | ((x & m2) << np.uint64(2))
    x = ((x >> np.uint64(4)) & m4) | ((x & m4) << np.uint64(4))
    x = x.byteswap()
    return x >> np.uint64(64 - 2 * K)


def fold(K, keys, offs, ids, counts, names):
    """hgvs-find.py:892-908: for every key x <= rc(x), c = counts[x] + counts[rc x] (a palindrome counts twice), and every
    record listing x takes one more k-mer seen c times.  Record 2 v is the wt record of names[v], 2 v + 1 its mut record.
    -> {hgvs: {'wt' | 'mut': {c: n}}}"""
    res = {}
    if len(keys) == 0:
        return res
    keys = np.asarray(keys, dtype=np.uint64)
    r = rc_keys(K, keys)
    j = np.searchsorted(keys, r)
    if np.any(j >= len(keys)) or np.any(keys[np.minimum(j, len(keys) - 1)] != r):
        raise InputError("the table does not hold both strands of a k-mer")
    c = np.asarray(counts, dtype=np.uint64) + np.asarray(counts, dtype=np.uint64)[j]
    lens = np.diff(np.asarray(offs, dtype=np.int64))
    keep = np.repeat(keys <= r, lens)
    rec = np.asarray(ids, dtype=np.int64)[keep]
    cs = np.repeat(c, lens)[keep]
    order = np.lexsort((cs, rec))
    rec, cs = rec[order], cs[order]
    first = np.ones(len(rec), dtype=bool)
    first[1:] = (rec[1:] != rec[:-1]) | (cs[1:] != cs[:-1])
    at = np.nonzero(first)[0]
    n = np.diff(np.append(at, len(rec)))
    for q, m in zip(at.tolist(), n.tolist()):
        res.setdefault(names[int(rec[q]) >> 1], {}).setdefault("mut" if int(rec[q]) & 1 else "wt", {})[int(cs[q])] = int(m)
    return res


_EOL = re.compile(rb"[\r\n]")


class RecordBody:
    """Where the body of a file's first FASTA record lies in the batches (file.readFasta, file.py:19-36): lines before the
    first header are ignored, the header line is the host's to skip, the body ends where zk_sequence_tally's first_gt says a
    line starts with '>'."""
    SEEK, HEADER, BODY, DONE = range(4)
    STEP = 1 << 16

    def __init__(self):
        self.phase, self.at_bol = self.SEEK, True

    def body_start(self, buf, n):
        """-> the offset in buf[0, n) where body bytes start (n: none in this batch)"""
        off = 0
        while off < n and self.phase < self.BODY:
            data = buf.view(min(self.STEP, n - off), off).to_host().tobytes()
            i = 0
            while i < len(data) and self.phase < self.BODY:
                if self.phase == self.SEEK and self.at_bol and data[i:i + 1] == b">":
                    self.phase = self.HEADER
                m = _EOL.search(data, i)
                if m is None:
                    self.at_bol = False
                    i = len(data)
                else:
                    i, self.at_bol = m.end(), True
                    if self.phase == self.HEADER:
                        self.phase = self.BODY
            off += i
        return off


def tally_file(ctx, table, path, counts, batch, stats):
    """the forward K-mers of the first record of one file, added to counts"""
    bufs = [ctx.empty(batch, np.uint8), ctx.empty(batch, np.uint8)]
    backup = ctx.empty(max(table.n_keys, 1), np.uint64)
    where, state, cur = RecordBody(), (0, 0), 0
    src = ctx.source_open(path)
    pending = False
    try:
        src.start(bufs[0], 0, batch)
        pending = True
        while True:
            t0 = time.perf_counter()
            n, eof = src.finish()
            pending = False
            stats["wait_seconds"] += time.perf_counter() - t0
            if not eof:
                src.start(bufs[1 - cur], 0, batch)           # the next batch streams in while this one is counted
                pending = True
            stats["batches"] += 1
            stats["bytes"] += n
            off = where.body_start(bufs[cur], n)
            t0 = time.perf_counter()
            while off < n:
                text = bufs[cur].view(n - off, off)
                ctx._check(ctx.lib.zk_copy(ctx.h, backup.ptr, counts.ptr, 8 * table.n_keys))
                after, nw, gt = ctx.sequence_tally(table, text, state, counts)
                if gt < text.n:                              # what was added includes bytes that are not the body's: count again
                    ctx._check(ctx.lib.zk_copy(ctx.h, counts.ptr, backup.ptr, 8 * table.n_keys))
                    if gt == 0 and not where.at_bol:         # a '>' inside a line that the batches cut: no header, it ends a run
                        off, state = off + 1, (0, 0)
                        continue
                    after, nw, gt = ctx.sequence_tally(table, text, state, counts, n=gt)      # a second record: up to its header
                    where.phase = where.DONE
                state = after
                stats["windows"] += nw
                where.at_bol = bufs[cur].view(1, n - 1).to_host()[0] in (10, 13)
                break
            stats["tally_seconds"] += time.perf_counter() - t0
            if eof or where.phase == where.DONE:
                break
            cur = 1 - cur
    finally:
        if pending:
            src.finish()
        src.close()


def new_stats():
    return dict(files=0, batches=0, bytes=0, windows=0, keys=0, wait_seconds=0.0, tally_seconds=0.0, fold_seconds=0.0)


def run_test(ctx, items, K, files, batch, out, verbose=False, err=None, stats=None):
    """-T behind its argument checks"""
    err = err or sys.stderr
    stats = stats if stats is not None else new_stats()
    for k, v in new_stats().items():
        stats.setdefault(k, v)
    recs = test_records(items, K)
    stream = "".join("%s\n%s\n" % (wt, mut) for _, wt, mut in recs).encode("latin-1")
    table = ctx.bait_table(ctx.upload_stream(stream), K) if recs else None
    res = {}
    if table is not None and table.n_keys:
        try:
            stats["keys"] = table.n_keys
            counts = ctx.upload(np.zeros(table.n_keys, dtype=np.uint64))
            for path in files:
                if verbose:
                    err.write("scanning %s\n" % path)
                tally_file(ctx, table, path, counts, batch, stats)
                stats["files"] += 1
            t0 = time.perf_counter()
            keys, offs, ids = (a.to_host() for a in table.arrays())
            res = fold(K, keys, offs, ids, counts.to_host(), [r[0] for r in recs])
            stats["fold_seconds"] += time.perf_counter() - t0
        finally:
            table.free()
    out.write(dump_yaml(res))
    return 0
