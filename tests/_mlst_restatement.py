"""The reference's own route through `zot mlst` (zotmer/library/index.py:67-125, zotmer/commands/mlst.py:45-54, with
basics.kmers, basics.py:261-301, and file.readFasta, file.py:19-36), restated in plain Python 3 over lists and dictionaries:
no numpy, nothing of the project under test."""
import bisect

NUC = {"A": 0, "a": 0, "C": 1, "c": 1, "G": 2, "g": 2, "T": 3, "t": 3, "U": 3, "u": 3}


def read_fasta(text):
    """file.readFasta (file.py:19-36): (name, sequence) per record; lines stripped and joined, the name is the header
    without '>' and surrounding blanks, text before the first header is dropped"""
    out, name, parts = [], None, []
    for line in text.split("\n"):
        line = line.strip()
        if line[:1] == ">":
            if name is not None:
                out.append((name, "".join(parts)))
            name, parts = line[1:].strip(), []
        else:
            parts.append(line)
    if name is not None:
        out.append((name, "".join(parts)))
    return out


def kmers_both(K, seq):
    """basics.kmers(K, seq, True) (basics.py:261-301): x then its reverse complement for every window of K bases AaCcGgTtUu"""
    out, x, xb, run = [], 0, 0, 0
    msk, s = (1 << (2 * K)) - 1, 2 * (K - 1)
    for ch in seq:
        b = NUC.get(ch)
        if b is None:
            x = xb = run = 0
            continue
        x = ((x << 2) | b) & msk
        xb = (xb >> 2) | ((3 - b) << s)
        run += 1
        if run >= K:
            out.append(x)
            out.append(xb)
    return out


def kmers_forward(K, seq):
    return kmers_both(K, seq)[0::2]


def build_index(K, fasta_texts):
    """buildIndex (index.py:67-115) -> dict(K, names, lens, S, T, U)"""
    seqs = []
    for text in fasta_texts:
        seqs += read_fasta(text)
    names, lens, per_record, S = [], [], [], set()
    for nm, seq in seqs:
        xs = sorted(set(kmers_both(K, seq)))
        names.append(nm)
        lens.append(len(xs))
        per_record.append(xs)
        S.update(xs)
    S = sorted(S)
    T = [0] * (len(S) + 1)
    for xs in per_record:
        for x in xs:
            T[bisect.bisect_left(S, x)] += 1
    t0 = 0
    for i in range(len(T)):
        T[i], t0 = t0, t0 + T[i]
    fill = list(T)
    U = [0] * t0
    for i, xs in enumerate(per_record):
        for x in xs:
            r = bisect.bisect_left(S, x)
            U[fill[r]] = i
            fill[r] += 1
    return dict(K=K, names=names, lens=lens, S=S, T=T, U=U)


def lookup(idx, x):
    """KmerIndex.__getitem__ (index.py:49-56)"""
    r = bisect.bisect_left(idx["S"], x)
    if r == len(idx["S"]) or idx["S"][r] != x:
        return []
    return idx["U"][idx["T"][r]:idx["T"][r + 1]]


def complete(idx, xs):
    """mlst.py:45-54: the record numbers whose counter reaches zero"""
    cs = list(idx["lens"])
    for x in xs:
        for j in lookup(idx, x):
            cs[j] -= 1
    assert all(c >= 0 for c in cs)
    return [j for j in range(len(cs)) if cs[j] == 0]


def stdout(idx, inp, xs):
    return "".join("%s\t%d\t%s\n" % (inp, j, idx["names"][j]) for j in complete(idx, xs))
