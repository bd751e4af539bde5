"""Plain-Python restatements for the `zot hgvs-index` tests: what zk_sequence_tally computes (include/zotk.h) and the fold of
`-T` (zotmer/commands/hgvs-find.py:892-908).  Slow and obvious on purpose."""

CODE = {c: i for i, c in enumerate("ACGT")}
CODE["U"] = 3
CODE.update({c.lower(): v for c, v in list(CODE.items())})


def tally(K, text, keys, state=(0, 0)):
    """text: bytes, a piece of a FASTA record's body.  '\\n' and '\\r' vanish, any other byte outside AaCcGgTtUu ends the run.
    state = (the last min(run, K - 1) bases as a 2-bit value, that length).
    -> ({key: windows equal to it}, state after, windows met, first_gt)"""
    want = set(keys)
    counts = {}
    msk = (1 << (2 * K)) - 1
    x, run = state
    n_windows = 0
    first_gt = len(text)
    for i, b in enumerate(text):
        ch = chr(b)
        if ch == ">" and first_gt == len(text) and (i == 0 or text[i - 1] in b"\r\n"):
            first_gt = i
        if ch in "\r\n":
            continue
        if ch not in CODE:
            x, run = 0, 0
            continue
        x = ((x << 2) | CODE[ch]) & msk
        run += 1
        if run >= K:
            n_windows += 1
            if x in want:
                counts[x] = counts.get(x, 0) + 1
    keep = min(run, K - 1)
    return counts, (x & ((1 << (2 * keep)) - 1), keep), n_windows, first_gt


def kmers(K, seq, both=False):
    """basics.kmersList"""
    out, x, run, msk = [], 0, 0, (1 << (2 * K)) - 1
    for ch in seq:
        if ch not in CODE:
            x, run = 0, 0
            continue
        x = ((x << 2) | CODE[ch]) & msk
        run += 1
        if run >= K:
            out.append(x)
            if both:
                out.append(rc(K, x))
    return out


def rc(K, x):
    y = 0
    for _ in range(K):
        y = (y << 2) | (3 - (x & 3))
        x >>= 2
    return y


def table_of(K, records):
    """the bait table of the records: (ascending keys, per key the ascending records holding it)"""
    owners = {}
    for r, seq in enumerate(records):
        for x in kmers(K, seq, True):
            owners.setdefault(x, set()).add(r)
    keys = sorted(owners)
    return keys, [sorted(owners[x]) for x in keys]


def fold(K, keys, owners, counts, names):
    """for every key x <= rc(x): c = counts[x] + counts[rc x], and every record listing x takes one more k-mer seen c times;
    record 2 v is names[v]'s wt, 2 v + 1 its mut -> {hgvs: {allele: {c: n}}}"""
    at = {x: i for i, x in enumerate(keys)}
    res = {}
    for i, x in enumerate(keys):
        y = rc(K, x)
        if x > y:
            continue
        c = counts[i] + counts[at[y]]
        for r in owners[i]:
            h = res.setdefault(names[r >> 1], {}).setdefault("mut" if r & 1 else "wt", {})
            h[c] = h.get(c, 0) + 1
    return res
