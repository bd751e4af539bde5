"""
What the reference's spikein tests call checkReads: does a record say where it comes from?  A record's header names the
fragment (u, fl, strand) and lists the errors put into the read; undoing them must give back the allele at that place.
Knows nothing of any generator.
"""
import re

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
_HEAD = re.compile(r"^@(\S+):(-?[0-9]+)-(-?[0-9]+) (\S+) ([0-9]+) ([0-9]+) ([+-]) (\S*)$")
_ERR = re.compile(r"^([0-9]+)(.)>([ACGT])$", re.S)


def split_records(text):
    lines = text.split("\n")
    assert lines[-1] == "" and (len(lines) - 1) % 4 == 0, "no whole number of four-line records"
    return [tuple(lines[i:i + 4]) for i in range(0, len(lines) - 1, 4)]


def parse_header(line):
    m = _HEAD.match(line)
    if m is None:
        raise ValueError("no spikein header: %r" % line)
    errs = []
    for e in (m.group(8).split(";") if m.group(8) else []):
        q = _ERR.match(e)
        if q is None:
            raise ValueError("no error entry: %r" % e)
        errs.append((int(q.group(1)), q.group(2), q.group(3)))
    return dict(ch=m.group(1), st=int(m.group(2)), en=int(m.group(3)), nm=m.group(4), u=int(m.group(5)), fl=int(m.group(6)),
                s=m.group(7), errors=errs)


def restore(read, errors):
    """the read before its errors, or None where an entry does not describe the read"""
    bases, seen = list(read), set()
    for p, c, d in errors:
        if p >= len(bases) or p in seen or bases[p] != d or c == d:
            return None
        seen.add(p)
        bases[p] = c
    return "".join(bases)


def expected(allele, u, fl, s, mate, L, upper_first=True):
    """mate 0 | 1 of the fragment allele[u:u + fl] on strand s.  upper_first False: complement, then upper-case, as the
    reference does (a lower-case base stays uncomplemented)"""
    if u < 0 or fl < L or u + fl > len(allele):
        return None
    frag = allele[u:u + fl]
    if upper_first:
        frag = frag.upper()
    if s == "-":
        frag = "".join(COMP.get(c, c) for c in frag)[::-1]
    return (frag[:L] if mate == 0 else frag[-L:]).upper()


def fits(record, mate, alleles, L, upper_first=True):
    """-> the indices of the alleles the record fits (empty: it fits none, or it is malformed)"""
    head, read, plus, qual = record
    if plus != "+" or qual != "I" * L or len(read) != L:
        return []
    try:
        h = parse_header(head)
    except ValueError:
        return []
    before = restore(read, h["errors"])
    if before is None:
        return []
    return [i for i, a in enumerate(alleles) if expected(a, h["u"], h["fl"], h["s"], mate, L, upper_first) == before]


def check_pairs(text1, text2, alleles_of, L, upper_first=True):
    """alleles_of(header dict) -> the alleles of the record's zone.  -> (per pair the set of alleles both mates fit, rejects)"""
    r1, r2 = split_records(text1), split_records(text2)
    assert len(r1) == len(r2)
    which, rejects = [], []
    for i, (a, b) in enumerate(zip(r1, r2)):
        try:
            ha, hb = parse_header(a[0]), parse_header(b[0])
        except ValueError:
            rejects.append(i)
            which.append(set())
            continue
        same = all(ha[k] == hb[k] for k in ("ch", "st", "en", "nm", "u", "fl", "s"))
        al = alleles_of(ha)
        both = set(fits(a, 0, al, L, upper_first)) & set(fits(b, 1, al, L, upper_first)) if same else set()
        which.append(both)
        if not both:
            rejects.append(i)
    return which, rejects
