"""`zot fizzle` restated in plain Python on ints: the loops of zotmer/commands/fizzle.py as they stand behind its dead `if True:`
experiment -- the exon-tuple index (502-514), recHits (354-414) without its print, the accumulation (555-583), the table
(593-646), -T (516-553), -X (272-306) and -P (161-261) -- with the things the port defines where the reference leaves them to
CPython 2: rows ordered by the bytes of exonGroup, -z tested on the row's own exons, a histogram as long as it needs to be.
Texts are str holding one character per byte (latin-1)."""
from tests._stop_restatement import WS, kmers_with_pos, read_fasta, read_fastq, render  # noqa: F401

_RC = {"A": "T", "C": "G", "G": "C", "T": "A"}


# ---- -P ----------------------------------------------------------------------------------------------------------------------
def _exons(t):
    ss = [int(s) for s in t[9].split(",") if len(s) > 0]
    ee = [int(e) for e in t[10].split(",") if len(e) > 0]
    return list(zip(ss, ee))


def prepare_gene(gene_list, ref_gene):
    """prepareBedFileGene on the two texts -> (bed text, warnings text)"""
    out, err = [], []
    genes = {}
    for l in gene_list.split("\n"):
        t = l.split()
        if t:
            genes[t[0]] = set()
    strands = {}
    for l in ref_gene.split("\n"):
        t = l.split()
        if not t:
            continue
        tx, ch, st, g = t[1], t[2], t[3], t[12]
        if "_" in ch:
            continue
        if g not in genes:
            continue
        if g in strands:
            if (ch, st) != strands[g]:
                err.append("gene tx seen in multiple chromosomes: %s [%s] (%s%s, %s%s)" % (g, tx, strands[g][0], strands[g][1], ch, st))
                continue
        else:
            strands[g] = (ch, st)
        for ex in _exons(t):
            genes[g].add(ex)
    for g in sorted(genes.keys()):
        if len(genes[g]) == 0:
            err.append("no annotated transcripts for gene: %s" % (g,))
            continue
        exs0 = sorted(genes[g])
        exs1 = [exs0[0]]
        for i in range(1, len(exs0)):
            if exs1[-1][1] >= exs0[i][0]:
                exs1[-1] = (min(exs1[-1][0], exs0[i][0]), max(exs1[-1][1], exs0[i][1]))
            else:
                exs1.append(exs0[i])
        if len(exs0) != len(exs1):
            genes[g] = exs1
    for g in sorted(genes.keys()):
        if len(genes[g]) == 0:
            continue
        ch, st = strands[g]
        exs = sorted(genes[g])
        if st == "-":
            exs = exs[::-1]
        for i in range(len(exs)):
            out.append("%s\t%d\t%d\t%s/%02d\t%s" % (ch, exs[i][0], exs[i][1], g, i + 1, st))
    return "".join(l + "\n" for l in out), "".join(l + "\n" for l in err)


def prepare_gene_tx(gene_list, ref_gene):
    """prepareBedFileGeneTx on the two texts -> (bed text, warnings text)"""
    out, err = [], []
    transcripts = {}
    for l in gene_list.split("\n"):
        t = l.split()
        if t:
            transcripts[t[1]] = t[0]
    found = {}
    for l in ref_gene.split("\n"):
        t = l.split()
        if not t:
            continue
        tx, ch, st, g = t[1], t[2], t[3], t[12]
        if tx not in transcripts:
            continue
        found[tx] = g
        exs = _exons(t)
        if st == "-":
            exs = exs[::-1]
        for i in range(len(exs)):
            out.append("%s\t%d\t%d\t%s/%02d\t%s" % (ch, exs[i][0], exs[i][1], g, i + 1, st))
    for tx in sorted(set(transcripts.keys()) - set(found.keys())):
        err.append("transcipt not found: %s\t(%s)" % (tx, transcripts[tx]))
    return "".join(l + "\n" for l in out), "".join(l + "\n" for l in err)


# ---- -X ----------------------------------------------------------------------------------------------------------------------
def rev_comp(seq):
    return "".join(_RC.get(c, c) for c in seq)[::-1]


def index_bed(bed, seq_of):
    """indexBedFiles: the items in the order it yields them; seq_of(chromosome) -> its sequence"""
    idx = {}
    for l in bed.split("\n"):
        t = l.split()
        if not t:
            continue
        g, ex = t[3].split("/")
        idx.setdefault(t[0], []).append((int(t[1]), int(t[2]), t[4], g, ex))
    items = []
    for ch in sorted(idx.keys()):
        seq = seq_of(ch)
        idx[ch].sort()
        for (s, e, st, g, ex) in idx[ch]:
            ex_seq = seq[s:e].upper()
            if st == "-":
                ex_seq = rev_comp(ex_seq)
            items.append({"gene": g, "exon": ex, "chr": ch, "st": s, "en": e, "strand": st, "seq": ex_seq})
    return items


def as_loaded(items):
    """what yaml.load_all(.., Loader=yaml.BaseLoader) makes of the written index: every scalar a string"""
    return [{k: str(v) for k, v in itm.items()} for itm in items]


# ---- the exon-tuple index ----------------------------------------------------------------------------------------------------
def tuple_index(K, ref):
    idx = {}
    lens = [0 for i in range(len(ref))]
    for i in range(len(ref)):
        for (x, _, p) in kmers_with_pos(K, ref[i]["seq"]):
            if x not in idx:
                idx[x] = set()
            idx[x].add(i)
            lens[i] += 1
    for x in idx:
        idx[x] = tuple(sorted(idx[x]))
    return idx, lens


# ---- recHits -----------------------------------------------------------------------------------------------------------------
class _UnionFind:
    def __init__(self):
        self.p = {}

    def find(self, x):
        self.p.setdefault(x, x)
        while self.p[x] != x:
            self.p[x] = self.p[self.p[x]]
            x = self.p[x]
        return x

    def union(self, a, b):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.p[b] = a


def rec_hits_sdx(sdx, drops=None):
    """recHits from sdx = {tuple: windows} on: (res, hitCount); drops (a list): one entry per turn of step 4"""
    n = sum(sdx.values())
    if n == 0:
        return {}, 0
    S = sorted(sdx)
    x_set = set(sdx.values())
    while True:
        u = _UnionFind()
        for i in range(len(S)):
            s0 = set(S[i])
            for j in range(i + 1, len(S)):
                if len(s0 & set(S[j])) > 0:
                    u.union(i, j)
        grps, cnts = {}, {}
        for i in range(len(S)):
            j = u.find(i)
            if j not in grps:
                grps[j] = set(S[i])
                cnts[j] = sdx[S[i]]
            else:
                grps[j] &= set(S[i])
                cnts[j] += sdx[S[i]]
        res = {}
        for j in grps.keys():
            if len(grps[j]) == 0:
                continue
            res[tuple(sorted(grps[j]))] = cnts[j]
        if len(res) > 0:
            return res, n
        x_set.remove(min(x_set))
        if drops is not None:
            drops.append(len(S))
        if len(x_set) == 0:
            return res, n
        x_min = min(x_set)
        S = [s for s in S if sdx[s] >= x_min]


def sdx_of(idx, xs):
    sdx = {}
    for x in xs:
        if x in idx:
            sdx[idx[x]] = sdx.get(idx[x], 0) + 1
    return sdx


def rec_hits(idx, xs):
    return rec_hits_sdx(sdx_of(idx, xs))


def records_of(K, seq1, seq2):
    """the two records of a pair: (lhsFwd + rhsRev, lhsRev + rhsFwd)"""
    w1, w2 = kmers_with_pos(K, seq1), kmers_with_pos(K, seq2)
    return ([x for x, _, _ in w1] + [xb for _, xb, _ in w2], [xb for _, xb, _ in w1] + [x for x, _, _ in w2])


# ---- the scan ----------------------------------------------------------------------------------------------------------------
def scan(K, idx, pairs):
    """fizzle.py:555-583 -> (acc {key: [reads, kmers]}, hit counts of the records that counted, pairs)"""
    acc, hit_counts, rn = {}, [], 0
    for seq1, seq2 in pairs:
        rn += 1
        for xs in records_of(K, seq1, seq2):
            hits, hit_count = rec_hits(idx, xs)
            if len(hits) > 0:
                k = tuple(sorted(hits.keys()))
                a = acc.setdefault(k, [0, 0])
                a[0] += 1
                a[1] += sum(hits.values())
                hit_counts.append(hit_count)
    return acc, hit_counts, rn


def pct_g(v):
    return "%g" % v


def table(ref, acc, min_gene_reads=1, min_exon_reads=1, min_gene_rate=1.0, min_exon_rate=1.0, gene_count=(0, 999999), exon_count=(0, 999999)):
    """fizzle.py:593-646 -> the lines, the header first; rows by the bytes of exonGroup"""
    def gex(s):
        return "|".join("%s/%s" % (ref[n]["gene"], ref[n]["exon"]) for n in s)

    gx_counts = {}
    for k in acc.keys():
        gx = set()
        for s in k:
            gx |= set(ref[i]["gene"] for i in s)
        c = gx_counts.setdefault(tuple(sorted(gx)), [0, 0])
        c[0] += acc[k][0]
        c[1] += acc[k][1]
    lines = ["\t".join(["numReads", "numKmers", "kmersPerRead", "ggNumReads", "ggNumKmers", "ggKmersPerRead", "numExons", "numGenes",
                        "geneGroup", "exonGroup"])]
    rows = []
    for k in acc.keys():
        nex = len(k)
        gx, ex = set(), set()
        for s in k:
            gx |= set(ref[i]["gene"] for i in s)
            ex |= set(s)
        k_str = "--".join(sorted(gex(s) for s in k))
        gx = tuple(sorted(gx))
        if len(gx) < gene_count[0] or len(gx) > gene_count[1]:
            continue
        if len(ex) < exon_count[0] or len(ex) > exon_count[1]:
            continue
        if gx_counts[gx][0] < min_gene_reads:
            continue
        if acc[k][0] < min_exon_reads:
            continue
        gx_rate = float(gx_counts[gx][1]) / float(gx_counts[gx][0])
        if gx_rate < min_gene_rate:
            continue
        ex_rate = float(acc[k][1]) / float(acc[k][0])
        if ex_rate < min_exon_rate:
            continue
        rows.append((k_str.encode("latin-1"), "%d\t%d\t%g\t%d\t%d\t%g\t%d\t%d\t%s\t%s" % (
            acc[k][0], acc[k][1], ex_rate, gx_counts[gx][0], gx_counts[gx][1], gx_rate, nex, len(gx), ":".join(gx), k_str)))
    rows.sort()
    return lines + [r[1] for r in rows]


def verbose_lines(hit_counts, rn):
    """fizzle.py:585-591, the histogram as long as it needs to be"""
    import math
    n, s, s2 = len(hit_counts), sum(hit_counts), sum(h * h for h in hit_counts)
    mean = float(s) / float(n)
    sd = math.sqrt(float(s2) / float(n) - mean * mean)
    out = ["total read hits: %d" % n, "total hits per read: %g (%g)" % (mean, sd), "total reads: %d" % rn]
    hist = {}
    for h in hit_counts:
        hist[h] = hist.get(h, 0) + 1
    return out + ["\t%d\t%d" % (i, hist[i]) for i in sorted(hist)]


# ---- -T ----------------------------------------------------------------------------------------------------------------------
def crosstalk(K, ref, seq_of):
    """fizzle.py:516-553 -> the report as a dict"""
    idx, lens = tuple_index(K, ref)
    ak = {}
    for x in sorted(idx.keys()):
        if len(idx[x]) == 1:
            continue
        ak[render(K, x)] = sorted("%s/%s" % (ref[i]["gene"], ref[i]["exon"]) for i in idx[x])
    counts = [0 for i in range(len(ref))]
    for ch in sorted(set(itm["chr"] for itm in ref)):
        for (x, xb, _) in kmers_with_pos(K, seq_of(ch)):
            for y in (x, xb):
                if y in idx:
                    for i in idx[y]:
                        counts[i] += 1
    gk = {}
    for i in range(len(ref)):
        if lens[i] == counts[i]:
            continue
        gk["%s/%s" % (ref[i]["gene"], ref[i]["exon"])] = {"indexed": lens[i], "genomic": counts[i]}
    return {"aliasing-within": ak, "aliasing-genomic": gk}
