"""
`zot fizzle` (zotmer/commands/fizzle.py): the exon groups, and so the genes and gene pairs, that read pairs touch.

The reference's main dies in an `if True:` experiment; this is the path behind it.  -P (161-261) makes a BED file of numbered
exons from a refGene table, -X (272-306) cuts the exons from the reference sequences and writes one YAML document each, the
exon-tuple index (502-514) maps every K-mer of the exons to the ascending tuple of the exons that hold it, -T (516-553) reports
the k-mers shared between exons and the exons whose k-mers the genome holds elsewhere, and the scan (555-646) asks recHits
(354-414) for the exon groups of the two records of every read pair and prints a table.

-P, -X and the loader are plain Python.  The distinct tuples are numbered as classes, in ascending tuple order (ClassIndex, NumPy),
and go to the device as a bait table whose every key lists its class.  Read pairs stream through in batches
(fastq_batches.record_batches), one zk_fizzle_votes per batch (csrc/fizzle.hip): a record that hits one class is tallied on the
device, and recHits of it is that class's tuple with all its hits; the others (a pair whose mates lie in two exons is one) come
back as (record, class, hits) entries.  Steps 2 and 3 of recHits depend on the set of classes only, so the records are grouped by their class list
(Accumulator), each distinct list is evaluated once, and the hits of its kept components are summed over its records with
NumPy; only a record whose first round comes out empty needs its own counts and goes through the threshold loop alone.  -T's
genome counts are zk_sequence_tally over the keys and their reverse complements, as `zot hgvs-index -T` does.
"""
import contextlib
import gzip
import math
import os
import sys
import time

import numpy as np

from zotmer_amd.library import hgvsindex
from zotmer_amd.library.alufinder import kmers_with_pos
from zotmer_amd.library.hgvsindex import InputError, dump_yaml

FIELDS = ("chr", "en", "exon", "gene", "seq", "st", "strand")
HEADER = ("numReads", "numKmers", "kmersPerRead", "ggNumReads", "ggNumKmers", "ggKmersPerRead", "numExons", "numGenes", "geneGroup",
          "exonGroup")
FIRST_HIST = 1 << 12            # bins of the device histogram to start with; it grows when a record reaches its last bin
_RC = bytes.maketrans(b"ACGT", b"TGCA")


def open_text(path, mode="r"):
    """file.openFile for the small text inputs: gzip by suffix"""
    if path.endswith(".gz"):
        return gzip.open(path, mode + "t", encoding="latin-1", newline="")
    return open(path, mode, encoding="latin-1", newline="")


# ---- -P ----------------------------------------------------------------------------------------------------------------------
def _exons(t):
    ss = [int(s) for s in t[9].split(",") if s]
    ee = [int(e) for e in t[10].split(",") if e]
    return list(zip(ss, ee))


def _bed_lines(ch, exs, g, st):
    return ["%s\t%d\t%d\t%s/%02d\t%s\n" % (ch, s, e, g, i + 1, st) for i, (s, e) in enumerate(exs)]


def _fields(line, n, path, lineno):
    t = line.split()
    if t and len(t) < n:
        raise InputError("%s, line %d: %d columns, expected at least %d" % (path, lineno, len(t), n))
    return t


def prepare_gene(gene_list, ref_gene, err):
    """prepareBedFileGene (161-229): the exons of every transcript of the listed genes, merged where they overlap or touch,
    numbered along the strand -> the BED lines"""
    genes, strands = {}, {}
    with open_text(gene_list) as f:
        for n, l in enumerate(f, 1):
            t = _fields(l, 1, gene_list, n)
            if t:
                genes[t[0]] = set()
    with open_text(ref_gene) as f:
        for n, l in enumerate(f, 1):
            t = _fields(l, 13, ref_gene, n)
            if not t:
                continue
            tx, ch, st, g = t[1], t[2], t[3], t[12]
            if "_" in ch or g not in genes:              # chr6_cox_hap2 and friends
                continue
            if g in strands:
                if (ch, st) != strands[g]:
                    err.write("gene tx seen in multiple chromosomes: %s [%s] (%s%s, %s%s)\n" % (g, tx, strands[g][0], strands[g][1], ch, st))
                    continue
            else:
                strands[g] = (ch, st)
            genes[g].update(_exons(t))
    out = []
    for g in sorted(genes):
        if not genes[g]:
            err.write("no annotated transcripts for gene: %s\n" % (g,))
            continue
        exs = []
        for s, e in sorted(genes[g]):
            if exs and exs[-1][1] >= s:
                exs[-1] = (min(exs[-1][0], s), max(exs[-1][1], e))
            else:
                exs.append((s, e))
        ch, st = strands[g]
        out += _bed_lines(ch, exs[::-1] if st == "-" else exs, g, st)
    return out


def prepare_gene_tx(gene_list, ref_gene, err):
    """prepareBedFileGeneTx (231-261): the exons of the listed transcripts as they stand, in the table's order"""
    transcripts, found, out = {}, {}, []
    with open_text(gene_list) as f:
        for n, l in enumerate(f, 1):
            t = _fields(l, 2, gene_list, n)
            if t:
                transcripts[t[1]] = t[0]
    with open_text(ref_gene) as f:
        for n, l in enumerate(f, 1):
            t = _fields(l, 13, ref_gene, n)
            if not t or t[1] not in transcripts:
                continue
            found[t[1]] = t[12]
            exs = _exons(t)
            out += _bed_lines(t[2], exs[::-1] if t[3] == "-" else exs, t[12], t[3])
    for tx in sorted(set(transcripts) - set(found)):
        err.write("transcipt not found: %s\t(%s)\n" % (tx, transcripts[tx]))
    return out


def run_prepare(gene_list, ref_gene, bed, with_tx, err=None):
    err = err or sys.stderr
    try:
        lines = (prepare_gene_tx if with_tx else prepare_gene)(gene_list, ref_gene, err)
    except (ValueError, IndexError) as e:
        raise InputError("%s: %s" % (ref_gene, e))
    with open_text(bed, "w") as out:
        out.write("".join(lines))
    return 0


# ---- -X ----------------------------------------------------------------------------------------------------------------------
def index_items(bed, home, verbose=False, err=None):
    """indexBedFiles (272-306): one dict per BED line, the chromosomes in sorted order, the lines sorted within one"""
    err = err or sys.stderr
    idx = {}
    with open_text(bed) as f:
        for n, l in enumerate(f, 1):
            t = _fields(l, 5, bed, n)
            if not t:
                continue
            try:
                g, ex = t[3].split("/")
                idx.setdefault(t[0], []).append((int(t[1]), int(t[2]), t[4], g, ex))
            except ValueError:
                raise InputError("%s, line %d: expected chromosome, start, end, gene/exon, strand" % (bed, n))
    items = []
    for ch in sorted(idx):
        if verbose:
            err.write("processing %s\n" % (ch,))
        seq = home[ch].encode("latin-1")
        for s, e, st, g, ex in sorted(idx[ch]):
            ex_seq = seq[s:e].upper()
            if st == "-":
                ex_seq = ex_seq.translate(_RC)[::-1]
            items.append({"gene": g, "exon": ex, "chr": ch, "st": s, "en": e, "strand": st, "seq": ex_seq.decode("latin-1")})
    return items


def dump_all(items):
    """yaml.safe_dump_all(items, default_flow_style=False)"""
    try:
        return "---\n".join(dump_yaml(itm) for itm in items)
    except ValueError as e:
        raise InputError(str(e))


# ---- the loader ----------------------------------------------------------------------------------------------------------------
def _unquote(v, where):
    if v[:1] == "'":
        if len(v) < 2 or v[-1] != "'":
            raise InputError("%s: an unterminated quote" % where)
        return v[1:-1].replace("''", "'")
    if v[:1] in ('"', "[", "{", "|", ">", "&", "*", "!"):
        raise InputError("%s: a YAML form that -X does not write" % where)
    return v


def load_index(path):
    """the documents of an index as -X writes them (yaml.load_all with BaseLoader: every scalar a string); exon i is document i"""
    ref, cur, open_doc = [], {}, False
    with open_text(path) as f:
        for n, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            where = "%s, line %d" % (path, n)
            if line == "---" or line == "...":
                if open_doc:
                    ref.append(cur)
                cur, open_doc = {}, False
                continue
            if not line.strip() or line.lstrip().startswith("#"):
                continue
            key, sep, val = line.partition(":")
            if not sep or line[0] in " -\t" or (val and val[0] != " "):
                raise InputError("%s: expected `key: value`" % where)
            cur[_unquote(key.strip(), where)] = _unquote(val.strip(), where)
            open_doc = True
    if open_doc:
        ref.append(cur)
    for i, itm in enumerate(ref):
        for k in ("gene", "exon", "chr", "seq"):
            if k not in itm:
                raise InputError("%s: document %d has no `%s`" % (path, i, k))
    if not ref:
        raise InputError("%s holds no documents" % path)
    return ref


# ---- the exon-tuple index ----------------------------------------------------------------------------------------------------
class ClassIndex:
    """fizzle.py:502-514 with the distinct tuples numbered: keys (u64 ascending) = the K-mers of the exons' forward strands,
    key_class[j] = the class of keys[j], tuples[c] = the ascending exon tuple of class c (the tuples ascend with c), lens[i] =
    the windows of exon i, with repeats"""

    def __init__(self, K, ref):
        self.K, self.ref = K, ref
        xs, self.lens = [], []
        for itm in ref:
            x, _ = kmers_with_pos(K, itm["seq"].encode("latin-1"))
            xs.append(x)
            self.lens.append(len(x))
        x = np.concatenate(xs) if xs else np.empty(0, np.uint64)
        ex = np.repeat(np.arange(len(ref), dtype=np.int64), self.lens)
        order = np.lexsort((ex, x))
        x, ex = x[order], ex[order]
        keep = np.ones(len(x), dtype=bool)
        keep[1:] = (x[1:] != x[:-1]) | (ex[1:] != ex[:-1])
        x, ex = x[keep], ex[keep]
        head = np.ones(len(x), dtype=bool)
        head[1:] = x[1:] != x[:-1]
        at = np.flatnonzero(head)
        self.keys = x[at]
        self.offs = np.append(at, len(x)).astype(np.int64)      # ex[offs[j], offs[j + 1]) = the tuple of keys[j]
        self.exons = ex
        n = np.diff(self.offs)
        tuples = {(int(e),) for e in np.unique(ex[at[n == 1]]).tolist()}
        many = np.flatnonzero(n > 1)
        many_tuples = [tuple(ex[self.offs[j]:self.offs[j + 1]].tolist()) for j in many.tolist()]
        tuples.update(many_tuples)
        self.tuples = sorted(tuples)
        number = {t: c for c, t in enumerate(self.tuples)}
        self.key_class = np.zeros(len(self.keys), dtype=np.uint32)
        if len(self.tuples):
            single = np.full(len(ref), 0, dtype=np.uint32)
            for t, c in number.items():
                if len(t) == 1:
                    single[t[0]] = c
            one = n == 1
            self.key_class[one] = single[ex[at[one]]]
            self.key_class[many] = [number[t] for t in many_tuples]

    def name(self, i):
        return "%s/%s" % (self.ref[i]["gene"], self.ref[i]["exon"])

    def table(self, ctx):
        n = len(self.keys)
        return ctx.bait_table_from_arrays(self.K, ctx.upload(self.keys), ctx.upload(np.arange(n + 1, dtype=np.uint32)),
                                          ctx.upload(self.key_class), len(self.tuples))


# ---- recHits -----------------------------------------------------------------------------------------------------------------
def components(S):
    """step 2 of recHits: the tuples of S joined where they share an exon, transitively -> [(intersection, indices into S)]"""
    parent = list(range(len(S)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    first = {}
    for i, s in enumerate(S):
        for e in s:
            j = first.setdefault(e, i)
            if j != i:
                a, b = find(j), find(i)
                if a != b:
                    parent[b] = a
    groups = {}
    for i in range(len(S)):
        groups.setdefault(find(i), []).append(i)
    out = []
    for members in groups.values():
        inter = set(S[members[0]])
        for i in members[1:]:
            inter &= set(S[i])
        out.append((tuple(sorted(inter)), members))
    return out


def rec_hits(sdx):
    """recHits (354-414) from sdx = {tuple: windows} on -> (res, hitCount)"""
    n = sum(sdx.values())
    if n == 0:
        return {}, 0
    S = sorted(sdx)
    x_set = set(sdx.values())
    while True:
        res = {inter: sum(sdx[S[i]] for i in members) for inter, members in components(S) if inter}
        if res:
            return res, n
        x_set.remove(min(x_set))
        if not x_set:
            return res, n
        x_min = min(x_set)
        S = [s for s in S if sdx[s] >= x_min]


class Accumulator:
    """acc of fizzle.py:555-583 from what zk_fizzle_votes leaves: acc[key] = [records, k-mers], hist[h] = the records with a
    non-empty answer and h hits"""

    def __init__(self, tuples):
        self.tuples = tuples
        self.bits = max(1, (len(tuples) - 1).bit_length())
        self.acc, self.hist, self.plan = {}, {}, {}
        self.slow = self.multi = self.slow_seconds = 0

    def _count(self, key, reads, kmers):
        a = self.acc.setdefault(key, [0, 0])
        a[0] += int(reads)
        a[1] += int(kmers)

    def _hits(self, values):
        h = np.bincount(values)
        for v in np.flatnonzero(h).tolist():
            self.hist[v] = self.hist.get(v, 0) + int(h[v])

    def add_single(self, single, hist):
        """the device tallies: single[2 c], single[2 c + 1] = the records with class c alone and their hits; hist[h] = such
        records with h hits"""
        single = np.asarray(single, dtype=np.uint64)
        for c in np.flatnonzero(single[0::2]).tolist():
            self._count((self.tuples[c],), single[2 * c], single[2 * c + 1])
        for v in np.flatnonzero(hist).tolist():
            self.hist[v] = self.hist.get(v, 0) + int(hist[v])

    def _plan(self, classes):
        """steps 2 and 3 of recHits for a set of classes: (key of acc, the columns of its kept components), None when the first
        round comes out empty"""
        p = self.plan.get(classes, False)
        if p is False:
            kept = [(inter, members) for inter, members in components([self.tuples[c] for c in classes]) if inter]
            p = None
            if kept:
                p = (tuple(sorted(inter for inter, _ in kept)), np.array(sorted(i for _, m in kept for i in m), dtype=np.intp))
            self.plan[classes] = p
        return p

    def add_entries(self, rec, cls, cnt):
        """the entries of one call: ascending by record and, within a record, by class"""
        if len(rec) == 0:
            return
        cls, cnt = np.asarray(cls, dtype=np.int64), np.asarray(cnt, dtype=np.int64)
        head = np.ones(len(rec), dtype=bool)
        head[1:] = rec[1:] != rec[:-1]
        starts = np.flatnonzero(head)
        lens = np.diff(np.append(starts, len(rec)))
        self.multi += len(starts)
        for L in np.unique(lens).tolist():
            at = starts[lens == L][:, None] + np.arange(L)[None, :]
            sets, counts = cls[at], cnt[at]
            if L * self.bits <= 63:                            # a class list as one word: a flat unique, not a unique over rows
                word = np.zeros(len(sets), dtype=np.int64)
                for j in range(L):
                    word = (word << self.bits) | sets[:, j]
                _, first, inv = np.unique(word, return_index=True, return_inverse=True)
                uniq = sets[first]
            else:
                uniq, inv = np.unique(sets, axis=0, return_inverse=True)
            inv = inv.reshape(-1)
            order = np.argsort(inv, kind="stable")
            cuts = np.searchsorted(inv[order], np.arange(len(uniq) + 1))
            sums = np.add.reduceat(counts[order], cuts[:-1], axis=0)         # per distinct list, the hits of every class over its records
            rows = np.diff(cuts)
            answered = np.ones(len(uniq), dtype=bool)
            for u, classes in enumerate(map(tuple, uniq.tolist())):
                p = self._plan(classes)
                if p is not None:
                    self._count(p[0], rows[u], sums[u, p[1]].sum())
                    continue
                answered[u] = False
                t0 = time.perf_counter()
                for row in counts[order[cuts[u]:cuts[u + 1]]].tolist():      # the threshold loop needs the record's own counts
                    res, n = rec_hits({self.tuples[c]: k for c, k in zip(classes, row)})
                    self.slow += 1
                    if res:
                        self._count(tuple(sorted(res)), 1, sum(res.values()))
                        self.hist[n] = self.hist.get(n, 0) + 1
                self.slow_seconds += time.perf_counter() - t0
            self._hits(counts.sum(axis=1)[answered[inv]])


# ---- the table -----------------------------------------------------------------------------------------------------------------
class Filters:
    def __init__(self, min_gene_reads=1, min_exon_reads=1, min_gene_rate=1.0, min_exon_rate=1.0, gene_count=(0, 999999), exon_count=(0, 999999)):
        self.min_gene_reads, self.min_exon_reads, self.min_gene_rate, self.min_exon_rate = min_gene_reads, min_exon_reads, min_gene_rate, min_exon_rate
        self.gene_count, self.exon_count = gene_count, exon_count


def table_lines(ref, acc, flt=None):
    """fizzle.py:593-646: the header, then one line per key that passes the filters, ordered by the bytes of exonGroup"""
    flt = flt or Filters()
    genes = {k: tuple(sorted({ref[i]["gene"] for s in k for i in s})) for k in acc}
    gx_counts = {}
    for k, (reads, kmers) in acc.items():
        c = gx_counts.setdefault(genes[k], [0, 0])
        c[0] += reads
        c[1] += kmers
    rows = []
    for k, (reads, kmers) in acc.items():
        gx = genes[k]
        n_exons = len({i for s in k for i in s})
        if len(gx) < flt.gene_count[0] or len(gx) > flt.gene_count[1]:
            continue
        if n_exons < flt.exon_count[0] or n_exons > flt.exon_count[1]:
            continue
        if gx_counts[gx][0] < flt.min_gene_reads:
            continue
        if reads < flt.min_exon_reads:
            continue
        gx_rate = float(gx_counts[gx][1]) / float(gx_counts[gx][0])
        if gx_rate < flt.min_gene_rate:
            continue
        ex_rate = float(kmers) / float(reads)
        if ex_rate < flt.min_exon_rate:
            continue
        k_str = "--".join(sorted("|".join("%s/%s" % (ref[i]["gene"], ref[i]["exon"]) for i in s) for s in k))
        rows.append((k_str.encode("latin-1"), "%d\t%d\t%g\t%d\t%d\t%g\t%d\t%d\t%s\t%s" % (
            reads, kmers, ex_rate, gx_counts[gx][0], gx_counts[gx][1], gx_rate, len(k), len(gx), ":".join(gx), k_str)))
    rows.sort()
    return ["\t".join(HEADER)] + [r[1] for r in rows]


def verbose_lines(hist, pairs):
    """fizzle.py:585-591"""
    n = sum(hist.values())
    out = ["total read hits: %d" % n]
    if n:
        s, s2 = sum(h * c for h, c in hist.items()), sum(h * h * c for h, c in hist.items())
        mean = float(s) / float(n)
        out.append("total hits per read: %g (%g)" % (mean, math.sqrt(max(float(s2) / float(n) - mean * mean, 0.0))))
    out.append("total reads: %d" % pairs)
    return out + ["\t%d\t%d" % (h, hist[h]) for h in sorted(hist)]


# ---- the scan ----------------------------------------------------------------------------------------------------------------
def new_stats():
    return dict(pairs=0, batches=0, multi_records=0, slow_records=0, entries=0, hist_grown=0, kernel_seconds=0.0, d2h_seconds=0.0,
                group_seconds=0.0, slow_seconds=0.0, scan_seconds=0.0, format_seconds=0.0)


def scan_inputs(ctx, index, inputs, batch, accu, stats, verbose=False, err=None):
    """every pair of inputs in order -> the number of read pairs.  The tallies of the one-class records stay on the device until
    the end; the entries of the others come to the host batch by batch."""
    from zotmer_amd.library.fastq_batches import record_batches, whole
    err = err or sys.stderr
    n_classes = len(index.tuples)
    table = index.table(ctx)
    pairs = 0
    try:
        single = ctx.upload(np.zeros(2 * max(n_classes, 1), dtype=np.uint64))
        single_bak = ctx.empty(single.n, np.uint64)
        hist = ctx.upload(np.zeros(FIRST_HIST, dtype=np.uint64))
        hist_bak = ctx.empty(hist.n, np.uint64)
        bufs = None
        for p in range(0, len(inputs), 2):
            with contextlib.closing(record_batches(ctx, inputs[p:p + 2], batch)) as batches:
                for texts, lines, r, _ in batches:
                    while True:
                        # a record with more hits than the histogram has bins lands in the last one: undo, make room, count again
                        ctx._check(ctx.lib.zk_copy(ctx.h, single_bak.ptr, single.ptr, single.nbytes))
                        ctx._check(ctx.lib.zk_copy(ctx.h, hist_bak.ptr, hist.ptr, hist.nbytes))
                        t0 = time.perf_counter()
                        rec, cls, cnt = ctx.fizzle_votes(table, index.K, texts[0], lines[0], texts[1], lines[1], r, single, hist, out=bufs)
                        bufs = (whole(rec), whole(cls), whole(cnt))
                        stats["kernel_seconds"] += time.perf_counter() - t0
                        if int(hist.view(1, hist.n - 1).to_host()[0]) == 0:
                            break
                        ctx._check(ctx.lib.zk_copy(ctx.h, single.ptr, single_bak.ptr, single.nbytes))
                        bigger = ctx.upload(np.zeros(2 * hist.n, dtype=np.uint64))
                        ctx._check(ctx.lib.zk_copy(ctx.h, bigger.ptr, hist_bak.ptr, hist.nbytes))
                        hist, hist_bak = bigger, ctx.empty(bigger.n, np.uint64)
                        stats["hist_grown"] += 1
                    t0 = time.perf_counter()
                    h_rec, h_cls, h_cnt = rec.to_host(), cls.to_host(), cnt.to_host()
                    t1 = time.perf_counter()
                    accu.add_entries(h_rec, h_cls, h_cnt)
                    stats["d2h_seconds"] += t1 - t0
                    stats["group_seconds"] += time.perf_counter() - t1
                    stats["entries"] += len(h_rec)
                    stats["batches"] += 1
                    pairs += r
                    if verbose:
                        err.write("%s: %d read pairs processed\n" % (os.path.basename(inputs[p]), pairs))
        t0 = time.perf_counter()
        accu.add_single(single.to_host(), hist.to_host())
        stats["d2h_seconds"] += time.perf_counter() - t0
    finally:
        table.free()
    return pairs


def run_scan(ctx, index, inputs, batch, out, flt=None, verbose=False, err=None, stats=None):
    """the scan behind its argument checks"""
    err = err or sys.stderr
    stats = stats if stats is not None else new_stats()
    for k, v in new_stats().items():
        stats.setdefault(k, v)
    accu = Accumulator(index.tuples)
    t0 = time.perf_counter()
    pairs = scan_inputs(ctx, index, inputs, batch, accu, stats, verbose, err) if len(index.keys) else count_pairs(ctx, inputs, batch)
    stats["scan_seconds"] = time.perf_counter() - t0
    stats.update(pairs=pairs, multi_records=accu.multi, slow_records=accu.slow, slow_seconds=accu.slow_seconds)
    t0 = time.perf_counter()
    if verbose:
        err.write("".join(l + "\n" for l in verbose_lines(accu.hist, pairs)))
    out.write("".join(l + "\n" for l in table_lines(index.ref, accu.acc, flt)))
    stats["format_seconds"] = time.perf_counter() - t0
    return 0


def count_pairs(ctx, inputs, batch):
    """an index without a k-mer: the pairs are still read and counted"""
    from zotmer_amd.library.fastq_batches import record_batches
    pairs = 0
    for p in range(0, len(inputs), 2):
        with contextlib.closing(record_batches(ctx, inputs[p:p + 2], batch)) as batches:
            for _, _, r, _ in batches:
                pairs += r
    return pairs


# ---- -T ----------------------------------------------------------------------------------------------------------------------
def crosstalk_report(index, counts):
    """fizzle.py:516-553 from the genome counts of the exons"""
    from zotmer_amd.library.stopscan import render_all
    n = np.diff(index.offs)
    shared = np.flatnonzero(n > 1)
    ak = {}
    for j, text in zip(shared.tolist(), render_all(index.K, index.keys[shared]) if len(shared) else []):
        ak[text] = sorted(index.name(i) for i in index.exons[index.offs[j]:index.offs[j + 1]].tolist())
    gk = {}
    for i, (a, b) in enumerate(zip(index.lens, counts)):
        if int(a) != int(b):
            gk[index.name(i)] = {"indexed": int(a), "genomic": int(b)}
    return {"aliasing-within": ak, "aliasing-genomic": gk}


def genome_counts(index, keys2, tally):
    """counts[i] = the windows of both strands whose k-mer lists exon i; keys2 = the keys and their reverse complements,
    ascending, tally[j] = the forward windows of the genome equal to keys2[j]"""
    counts = np.zeros(len(index.ref), dtype=np.int64)
    if len(index.keys):
        tally = np.asarray(tally, dtype=np.int64)
        c = tally[np.searchsorted(keys2, index.keys)] + tally[np.searchsorted(keys2, hgvsindex.rc_keys(index.K, index.keys))]
        np.add.at(counts, index.exons, np.repeat(c, np.diff(index.offs)))
    return counts


def run_crosstalk(ctx, index, home, batch, out, verbose=False, err=None, stats=None):
    """-T behind its argument checks"""
    err = err or sys.stderr
    stats = stats if stats is not None else hgvsindex.new_stats()
    for k, v in hgvsindex.new_stats().items():
        stats.setdefault(k, v)
    chroms = sorted({itm["chr"] for itm in index.ref})
    files = [home.path(ch) for ch in chroms]
    keys2 = np.unique(np.concatenate((index.keys, hgvsindex.rc_keys(index.K, index.keys)))) if len(index.keys) else np.empty(0, np.uint64)
    tally = np.zeros(len(keys2), dtype=np.uint64)
    if len(keys2):
        n = len(keys2)
        table = ctx.bait_table_from_arrays(index.K, ctx.upload(keys2), ctx.upload(np.arange(n + 1, dtype=np.uint32)),
                                           ctx.upload(np.zeros(n, dtype=np.uint32)), 1)
        try:
            stats["keys"] = n
            d_counts = ctx.upload(tally)
            for ch, path in zip(chroms, files):
                if verbose:
                    err.write("processing %s\n" % (ch,))
                hgvsindex.tally_file(ctx, table, path, d_counts, batch, stats)
                stats["files"] += 1
            tally = d_counts.to_host()
        finally:
            table.free()
    out.write(dump_yaml(crosstalk_report(index, genome_counts(index, keys2, tally))))
    return 0
