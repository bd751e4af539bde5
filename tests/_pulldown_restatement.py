"""A plain-Python restatement of `zot pulldown -p` (zotmer/commands/pulldown.py with library/{basics,file}.py), written from
the reference's semantics for the tests: the fixtures of tests/golden/p1_pulldown.json must come out of it, and the device
path must agree with it.  Slow (a dict probe per window): small inputs only."""
import hashlib
import posixpath

from tests._capture_restatement import fasta_records, fastq_records, kmers

K = 25


def tables(baits_text, up_text):
    """-> (bait names, {25-mer of either strand of a bait: set of bait numbers}, set of the 25-mers of either strand of -U)"""
    names, idx = [], {}
    for n, (nm, seq) in enumerate(fasta_records(baits_text)):
        names.append(nm)
        for x in kmers(K, seq, True):
            idx.setdefault(x, set()).add(n)
    anti = set()
    for _, seq in fasta_records(up_text or ""):
        anti.update(kmers(K, seq, True))
    return names, idx, anti


def walk(idx, anti, text1, text2):
    """One file pair -> (per read pair: None when it is pushed up, else the set of baits it hits; the records of mate 1; of
    mate 2).  Pairs are drawn until either file ends."""
    r1, r2 = fastq_records(text1), fastq_records(text2)
    n = min(len(r1), len(r2))
    hits = []
    for r in range(n):
        xs = kmers(K, r1[r][1], False) + kmers(K, r2[r][1], False)
        if any(x in anti for x in xs):
            hits.append(None)
            continue
        h = set()
        for x in xs:
            h |= idx.get(x, set())
        hits.append(h)
    return hits, r1[:n], r2[:n]


def member_name(bait_name, fn):
    """'<p>/<fn>', p = the name's words joined by '/', normalised and without leading '/' (what ZipFile.write stores)"""
    return posixpath.normpath("/".join(bait_name.split()) + "/" + fn).lstrip("/")


def pulldown(baits_text, up_text, inputs, fns):
    """-> (hist {n: pairs with n baits} over all file pairs, members [(name, bytes)] of all file pairs in input order, pairs
    pushed up).  The reference keeps only the last file pair's members; with one file pair the two agree."""
    names, idx, anti = tables(baits_text, up_text)
    hist, members, vetoed = {}, [], 0
    for i in range(0, len(inputs), 2):
        hits, r1, r2 = walk(idx, anti, inputs[i], inputs[i + 1])
        per_bait = [[] for _ in names]
        for r, h in enumerate(hits):
            if h is None:
                vetoed += 1
                continue
            hist[len(h)] = hist.get(len(h), 0) + 1
            for b in h:
                per_bait[b].append(r)
        for b, rs in enumerate(per_bait):
            if rs:
                for recs, fn in ((r1, fns[i]), (r2, fns[i + 1])):
                    members.append((member_name(names[b], fn), "".join("%s\n%s\n%s\n%s\n" % recs[r] for r in rs).encode()))
    return hist, members, vetoed


def rows(hist):
    return "".join("%d\t%d\n" % (n, f) for n, f in sorted(hist.items()))


def digest(members):
    """[(name, sha256, size)] as the fixture holds them"""
    return [(nm, hashlib.sha256(b).hexdigest(), len(b)) for nm, b in members]
