"""A plain-Python restatement of `zot strand` without -r (zotmer/commands/strand.py:53-60,62-73,130-155 with
library/{basics,file}.py), written from the reference's semantics for the tests: the fixtures of
tests/golden/s1_strand.json must come out of it, and the device path must agree with it.  Slow (a dict probe per
window): small inputs only."""
from tests._capture_restatement import fastq_records, kmers

MASK64 = 0xFFFFFFFFFFFFFFFF
SEED = 17


def rc(k, x):
    """basics.rc (basics.py:115-121)"""
    y = 0
    for _ in range(k):
        y = (y << 2) | (3 - (x & 3))
        x >>= 2
    return y


def murmer(x, s):
    """basics.murmer (basics.py:191-229)"""
    k = (x * 0x87c37b91114253d5) & MASK64
    k = ((k << 31) | (k >> 33)) & MASK64
    k = (k * 0x4cf5ad432745937f) & MASK64
    h = s ^ k
    h = ((h << 27) | (h >> 37)) & MASK64
    h = (h * 5 + 0x52dce729) & MASK64
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & MASK64
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & MASK64
    h ^= h >> 33
    return h


def threshold(K, p):
    """strand.py:66,72-73: M = 4**K - 1, T = int(M * p)"""
    M = (1 << (2 * K)) - 1
    return M, int(M * p)


def read_kmers(K, inputs, single=False):
    """parseFiles (strand.py:39-60): per pair of reads, the forward k-mers of mate 1 and the reverse complements of those of
    mate 2; the files taken in pairs, a pair ending where the shorter file ends (`both`, strand.py:30-37).  single: the
    evident intent of -s (the reference's branch cannot run) -- the forward k-mers of every read of every file."""
    if single:
        for text in inputs:
            for rec in fastq_records(text):
                yield kmers(K, rec[1], False)
        return
    assert len(inputs) % 2 == 0          # pairs(), strand.py:24
    for i in range(0, len(inputs), 2):
        for fq1, fq2 in zip(fastq_records(inputs[i]), fastq_records(inputs[i + 1])):
            yield kmers(K, fq1[1], False) + [rc(K, x) for x in kmers(K, fq2[1], False)]


def count(K, p, inputs, single=False):
    """strand.py:130-140: kx[x] = occurrences of the ORIENTED k-mer x, for the k-mers whose canonical form passes the sample"""
    M, T = threshold(K, p)
    kx = {}
    for xs in read_kmers(K, inputs, single):
        for x in xs:
            if x in kx:
                kx[x] += 1
                continue
            y = rc(K, x)
            z = murmer(min(x, y), SEED)
            if (z & M) > T:
                continue
            kx[x] = 1
    return kx


def oriented(K, x, xc, yc):
    """strand.py:148-153"""
    return (xc, yc) if murmer(x, SEED) >= murmer(rc(K, x), SEED) else (yc, xc)


def lines_of(K, kx, orphans=False):
    """strand.py:142-155 -> ([(canonical x, ac, bc)] in dict order, stats).  orphans: also the k-mers seen only as the greater of
    {x, rc x}, with xc = 0 (the -a option of this port; the reference prints nothing for them)."""
    out = []
    st = dict(pairs=0, orphans=0, palindromes=0)
    for x in kx.keys():
        y = rc(K, x)
        if x > y:
            if y not in kx:
                st["orphans"] += 1
                if orphans:
                    out.append((y,) + oriented(K, y, 0, kx[x]))
            continue
        if x == y:
            st["palindromes"] += 1
        out.append((x,) + oriented(K, x, kx[x], kx.get(y, 0)))
    st["pairs"] = len(out)
    return out, st


def strand(K, p, inputs, single=False, orphans=False):
    """-> (the stdout lines in the reference's dict order, the same in ascending canonical k-mer order, stats)"""
    rows, st = lines_of(K, count(K, p, inputs, single), orphans)
    fmt = lambda rs: ["%d\t%d\n" % (a, b) for _, a, b in rs]
    return fmt(rows), fmt(sorted(rows)), st


# ---- the pieces the device entries are checked against ----------------------------------------------------------

def tagged_keys(K, seqs, reverse, T, seed=SEED, memo=None):
    """zk_strand_keys: the kept tagged keys (c << 1) | (oriented != c) of every window of every sequence, sorted.
    memo: a dict the caller keeps between calls with the same K and seed (x -> (rc x, hash of the canonical form))"""
    M = (1 << (2 * K)) - 1
    memo = {} if memo is None else memo
    out = []
    for s in seqs:
        for x in kmers(K, s, False):
            if x not in memo:
                y = rc(K, x)
                memo[x] = (y, murmer(min(x, y), seed) & M)
            y, h = memo[x]
            c = min(x, y)
            if h <= T:
                o = y if reverse else x
                out.append((c << 1) | (o != c))
    return sorted(out)


def pairs_of(K, keys, counts, orphans=False):
    """zk_strand_pairs over ascending distinct tagged keys: rebuild kx and walk it as the reference does -> (a[], b[] in
    ascending canonical k-mer order, stats)"""
    kx = {}
    for key, n in zip(keys, counts):
        c = int(key) >> 1
        kx[rc(K, c) if int(key) & 1 else c] = int(n)
    rows, st = lines_of(K, kx, orphans)
    rows.sort()
    return [r[1] for r in rows], [r[2] for r in rows], st
