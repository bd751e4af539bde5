"""A plain-Python restatement of `zot capture` (zotmer/commands/capture.py with library/{basics,file,reads}.py), written
from the reference's semantics for the tests: the fixtures of tests/golden/c1_capture.json must come out of it, and
the device path must agree with it on random cases.  Slow (a dict probe per window): small inputs only."""
_CODE = {c: i for i, c in enumerate("ACGT")}
_CODE.update({"U": 3})
_CODE.update({c.lower(): v for c, v in list(_CODE.items())})

READ_K = 25


def kmers(k, seq, both):
    """basics.kmersList (basics.py:303-347): every window of k bases in AaCcGgTtUu; x, then rc(x) if both"""
    out = []
    run = 0
    x = xb = 0
    msk = (1 << (2 * k)) - 1
    for ch in seq:
        b = _CODE.get(ch)
        if b is None:
            run, x, xb = 0, 0, 0
            continue
        x = ((x << 2) | b) & msk
        xb = (xb >> 2) | ((3 - b) << (2 * (k - 1)))
        run += 1
        if run >= k:
            out.append(x)
            if both:
                out.append(xb)
    return out


def fasta_records(text):
    """file.readFasta (file.py:19-36) over a str"""
    nm, seq = None, []
    for line in text.split("\n"):
        line = line.strip()
        if line[:1] == ">":
            if nm is not None:
                yield nm, "".join(seq)
            nm, seq = line[1:].strip(), []
        else:
            seq.append(line)
    if nm is not None:
        yield nm, "".join(seq)


def fastq_records(text):
    """file.readFastq (file.py:38-52): groups of four stripped lines; a trailing partial group is dropped"""
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    lines = [l.strip() for l in lines]
    return [tuple(lines[i:i + 4]) for i in range(0, len(lines) - 3, 4)]


def capture(baits_text, inputs, k, paired=False):
    """-> ({file name: bytes} as the prefix directory holds them after the run, stderr text with the prefix as '<P>',
    warnings).  inputs: FASTQ texts (str).  Baits that share a name share a file, written bait after bait (per batch in
    the device path; the restatement writes them as one batch)."""
    names, table = [], {}
    for n, (nm, seq) in enumerate(fasta_records(baits_text)):
        names.append(nm)
        for x in kmers(k, seq, True):
            table.setdefault(x, set()).add(n)
    per_bait = [[[] for _ in range(2 if paired else 1)] for _ in names]
    warnings = []
    step = 2 if paired else 1
    for i in range(0, len(inputs) - (step - 1), step):
        recs = [fastq_records(t) for t in inputs[i:i + step]]
        n = len(recs[0])
        if paired and len(recs[1]) < n:
            n = len(recs[1])
            warnings.append("warning: files had unequal length")
        for r in range(n):
            hits = set()
            for m in range(step):
                for x in kmers(READ_K, recs[m][r][1], False):
                    hits |= table.get(x, set())
            for b in hits:
                for m in range(step):
                    per_bait[b][m].append(recs[m][r])
    files = {}
    err = []
    for b, nm in enumerate(names):
        fns = ["%s_%d.fastq" % (nm, m + 1) for m in range(2)] if paired else ["%s.fastq" % nm]
        for m, fn in enumerate(fns):
            if per_bait[b][m]:
                files[fn] = files.get(fn, b"") + "".join("%s\n%s\n%s\n%s\n" % rd for rd in per_bait[b][m]).encode()
        err.append("<P>/%s: %d\n" % (fns[0], len(per_bait[b][0])))
    return files, "".join(err), warnings
