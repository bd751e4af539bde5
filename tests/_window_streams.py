"""Streams for the window front end -- bytes of text become windows of K bases -- and the plain references they are checked against
(tests/test_window_streams_host.py on the CPU; tests/test_gpu_window_bytes.py and tests/test_gpu_record_lengths.py on the device).
Nothing here touches a device.

The rule (include/zotk.h, conventions): any byte outside AaCcGgTtUu ends the windows that touch it, 1 <= K <= 32, and an entry reads
[0, n) of its stream and nothing else.  The library states that rule in several classifiers, each with bit tricks of its own, so the
streams here hold what those tricks could get wrong:

    byte_phase_stream / byte_phase_fastq   every byte value 0..255 between two runs of bases, at every offset modulo 16 (its place in
                                           the 4-byte word and the 16-byte chunk of the SWAR classifiers)
    phantom_baits                          the k-mers a window would give if the byte WERE read as A, C, G or T
    embedded                               a payload inside an allocation whose every other byte is a base: a read past either end
                                           of the stream makes new k-mers instead of meeting a separator
    uniform_reads / near_uniform           streams of records of one length (the first pass lays its tiles along such records), and
                                           two spoiled forms that only a check of every separator can tell from them
    windows                                the one restatement the other references are checked against: a dict lookup per byte
"""
import functools

import numpy as np

U8, U64 = np.uint8, np.uint64
LETTERS = b"AaCcGgTtUu"
CODE = {c: i for c, i in zip(b"ACGT", range(4))}
CODE.update({ord("U"): 3})
CODE.update({c | 0x20: v for c, v in list(CODE.items())})
assert sorted(CODE) == sorted(LETTERS)
PHASES = 16

_CODES = np.full(256, -1, dtype=np.int64)
for _c, _v in CODE.items():
    _CODES[_c] = _v


def is_base(v):
    return v in CODE


def windows(data, K):
    """[(position of the window's first byte, k-mer)] for every run of K bytes of AaCcGgTtUu in data, by position"""
    out = []
    run, x = 0, 0
    msk = (1 << (2 * K)) - 1
    for p, ch in enumerate(bytes(data)):
        b = CODE.get(ch)
        if b is None:
            run, x = 0, 0
            continue
        x = ((x << 2) | b) & msk
        run += 1
        if run >= K:
            out.append((p - K + 1, x))
    return out


def revcomp(x, K):
    """of a Python int or a uint64 array"""
    if isinstance(x, (int, np.integer)):
        x, y = int(x), 0
        for _ in range(K):
            y = (y << 2) | (3 - (x & 3))
            x >>= 2
        return y
    x = np.asarray(x, dtype=U64)
    y = np.zeros_like(x)
    for i in range(K):
        y = (y << U64(2)) | (U64(3) - ((x >> U64(2 * i)) & U64(3)))
    return y


def kmers_both(data, K):
    """x, then rc(x), per window, in stream order: what zk_encode(both = 1) gives (uint64 array)"""
    fwd = np.array([x for _, x in windows(data, K)], dtype=U64)
    out = np.empty(2 * len(fwd), dtype=U64)
    out[0::2] = fwd
    out[1::2] = revcomp(fwd, K)
    return out


def counted(kmers):
    """(distinct ascending k-mers, counts u32) of a k-mer list: what zk_kmerize gives for the list of both strands"""
    k, c = np.unique(np.asarray(kmers, dtype=U64), return_counts=True)
    return k, c.astype(np.uint32)


def tagged_keys(K, seqs, reverse):
    """zk_strand_keys when every window is kept: (c << 1) | (oriented != c) per window of every sequence, c = min(x, rc x),
    oriented = rc x if reverse else x -> ascending uint64 array (K <= 31)"""
    xs = [x for s in seqs for _, x in windows(s, K)]
    x = np.array(xs, dtype=U64)
    y = revcomp(x, K)
    c = np.minimum(x, y)
    o = y if reverse else x
    return np.sort((c << U64(1)) | (o != c).astype(U64))


def acgt_of(kmers):
    k = np.asarray(kmers, dtype=U64)
    return [int(np.count_nonzero((k & U64(3)) == U64(b))) for b in range(4)]


def _letters(rng, n):
    return np.frombuffer(LETTERS, dtype=U8)[rng.integers(0, len(LETTERS), size=n)]


# ---- every byte value at every phase -------------------------------------------------------------------------------------------

def _piece(rng, K, v, s, start):
    """a piece that starts at stream offset `start` -> (uint8 array without a line end, where v lies in it): at least K + 1
    letters, lengthened so that v lands on an offset = s modulo 16, the byte v, K + 2 letters"""
    lead = K + 1
    lead += (s - (start + lead)) % PHASES
    return np.concatenate([_letters(rng, lead), np.array([v], dtype=U8), _letters(rng, K + 2)]), lead


@functools.lru_cache(maxsize=None)
def byte_phase_stream(K, seed):
    """-> (stream bytes, offsets int64[256, 16]): for every byte value v and every phase s a piece of at least K + 1 letters of
    AaCcGgTtUu, the byte v, K + 2 letters and '\\n'; offsets[v, s] = where that v lies, = s modulo 16."""
    rng = np.random.default_rng(seed)
    parts, offs, at = [], np.zeros((256, PHASES), dtype=np.int64), 0
    for v in range(256):
        for s in range(PHASES):
            piece, lead = _piece(rng, K, v, s, at)
            offs[v, s] = at + lead
            parts += [piece, np.array([10], dtype=U8)]
            at += len(piece) + 1
    offs.setflags(write=False)
    return np.concatenate(parts).tobytes(), offs


HEADER_LEN, PLUS_LEN = 11, 3          # lengths of the header and '+' lines of byte_phase_fastq (base letters only)


@functools.lru_cache(maxsize=None)
def byte_phase_fastq(K, seed, crlf=False):
    """-> (text bytes, offsets int64[256, 16], sequence lines as a tuple of bytes, without their line ends): the pieces of
    byte_phase_stream as the sequence lines of FASTQ records, without v = '\\n' (offsets[10] = -1).  The header, '+' and quality
    lines are base letters only (no '@', no '+'): the kernels go by line number, and one that took the wrong line would find
    windows.  crlf: every line ends with '\\r\\n'."""
    rng = np.random.default_rng(seed + 1000003)
    eol = np.frombuffer(b"\r\n" if crlf else b"\n", dtype=U8)
    parts, offs, seqs = [], np.full((256, PHASES), -1, dtype=np.int64), []
    at = 0
    rng_p = np.random.default_rng(seed)
    for v in range(256):
        if v == 10:
            continue
        for s in range(PHASES):
            head = _letters(rng, HEADER_LEN)
            start = at + HEADER_LEN + len(eol)
            piece, lead = _piece(rng_p, K, v, s, start)
            offs[v, s] = start + lead
            rec = [head, eol, piece, eol, _letters(rng, PLUS_LEN), eol, _letters(rng, len(piece)), eol]
            parts += rec
            seqs.append(piece.tobytes())
            at += sum(len(a) for a in rec)
    offs.setflags(write=False)
    return np.concatenate(parts).tobytes(), offs, tuple(seqs)


def phantom_baits(K, stream, offsets):
    """-> uint64[256, 16, K, 4, 2]: for the byte v at offsets[v, s], window j = the K bytes from offsets[v, s] - K + 1 + j on (it
    spans v), with v replaced by A, C, G, T in turn; the k-mer and its reverse complement.  For a v that is a base one of the four
    is a real window (the positive control); for any other v a hit on a phantom means the byte was read as a base.  Entries of an
    offset < 0 (a v that the stream leaves out) are zero and flagged in the second result, bool[256, 16]."""
    data = np.frombuffer(stream, dtype=U8)
    codes = _CODES[data]
    have = offsets >= 0
    p = np.where(have, offsets, K)                                             # [256, 16]
    idx = p[:, :, None, None] - (K - 1) + np.arange(K)[None, None, :, None] + np.arange(K)[None, None, None, :]     # [v, s, j, i]
    w = codes[idx]
    hole = (K - 1 - np.arange(K))                                              # where v lies in window j
    out = np.zeros(offsets.shape + (K, 4, 2), dtype=U64)
    for b in range(4):
        wb = w.copy()
        wb[:, :, np.arange(K), hole] = b
        assert (wb[have] >= 0).all(), "a window around v holds another byte that is not a base"
        x = np.zeros(wb.shape[:3], dtype=U64)
        for i in range(K):
            x = (x << U64(2)) | np.where(have[:, :, None], wb[:, :, :, i], 0).astype(U64)
        out[:, :, :, b, 0] = x
        out[:, :, :, b, 1] = revcomp(x, K)
    out[~have] = 0
    return out, have


def table_arrays(keys, records):
    """(key, record) pairs -> (keys u64 ascending distinct, offs u32[n + 1], ids u32 ascending within a key): the arrays of a
    bait table, as zk_bait_table_from_arrays takes them and zk_bait_table_arrays gives them"""
    keys, records = np.asarray(keys, dtype=U64), np.asarray(records, dtype=U64)
    order = np.lexsort((records, keys))
    k, r = keys[order], records[order]
    new = np.ones(len(k), dtype=bool)
    new[1:] = (k[1:] != k[:-1]) | (r[1:] != r[:-1])
    k, r = k[new], r[new]
    head = np.ones(len(k), dtype=bool)
    head[1:] = k[1:] != k[:-1]
    offs = np.concatenate([np.flatnonzero(head), [len(k)]]).astype(np.uint32)
    return k[head], offs, r.astype(np.uint32)


def phantom_table(phantoms, have, only=None):
    """the phantoms as a bait table of one record per byte value (only: of these byte values alone) -> (keys, offs, ids,
    n_records = 256)"""
    rec = np.broadcast_to(np.arange(256, dtype=np.int64)[:, None, None, None, None], phantoms.shape)
    mask = np.broadcast_to(have[:, :, None, None, None], phantoms.shape)
    if only is not None:
        mask = mask & np.isin(rec, list(only))
    return table_arrays(phantoms[mask], rec[mask]) + (256,)


def table_hits(table, xs):
    """-> (indices into xs, ids): one pair for every id the table lists under xs[i]"""
    keys, offs, ids = table[:3]
    xs = np.asarray(xs, dtype=U64)
    if not len(keys) or not len(xs):
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint32)
    at = np.minimum(np.searchsorted(keys, xs), len(keys) - 1)
    found = np.flatnonzero(keys[at] == xs)
    which, got = [], []
    for i in found:
        lo, hi = int(offs[at[i]]), int(offs[at[i] + 1])
        which += [int(i)] * (hi - lo)
        got += ids[lo:hi].tolist()
    return np.array(which, dtype=np.int64), np.array(got, dtype=np.uint32)


# ---- a payload among bases -----------------------------------------------------------------------------------------------------------

def embedded(payload, lead, tail=256, seed=5):
    """-> the allocation (uint8 array of lead + len(payload) + tail bytes): the payload at `lead`, every other byte from a random
    sequence over ACGTacgt (random, not periodic: a stray window is a new k-mer).  Leads that are multiples of 16 serve the entries
    that need a 16-byte stream, leads 1 and 7 the others."""
    pay = np.frombuffer(bytes(payload), dtype=U8)
    rng = np.random.default_rng(seed * 7919 + lead + 31 * len(pay))
    whole = np.frombuffer(b"ACGTacgt", dtype=U8)[rng.integers(0, 8, size=lead + len(pay) + tail)].copy()
    whole[lead:lead + len(pay)] = pay
    return whole


def base_run(n, seed):
    """n random letters of ACGT with no separator anywhere: windows start at byte 0 and reach byte n - 1"""
    rng = np.random.default_rng(seed)
    return np.frombuffer(b"ACGT", dtype=U8)[rng.integers(0, 4, size=n)].tobytes()


# ---- records of one length ----------------------------------------------------------------------------------------------------------------

def uniform_reads(L, K, seed, total=40_000):
    """ceil(total / (L + 1)) reads of exactly L characters sampled from a 2 000-base random genome (k-mers repeat), 0.2 % of them
    N and some reads in lower case -> a list of bytes.  K only varies the draw."""
    rng = np.random.default_rng([seed, K, L])
    n = -(-total // (L + 1))
    genome = np.frombuffer(b"ACGT", dtype=U8)[rng.integers(0, 4, size=2000)]
    start = rng.integers(0, len(genome) - L + 1, size=n)
    a = genome[start[:, None] + np.arange(L)[None, :]].copy()
    a[rng.random(a.shape) < 0.002] = ord("N")
    lower = rng.random(n) < 0.1
    a[lower] |= 0x20
    return [r.tobytes() for r in a]


def stream_of(reads):
    return b"".join(r + b"\n" for r in reads)


def near_uniform(reads):
    """two spoiled forms of stream_of(reads) -> (a, b).  a: the last read one base short, so n_bytes % rec != 0.  b: the length
    kept, one separator (not the first) an N and one base elsewhere a '\\n': the first newline and the length still look uniform."""
    assert len(reads) >= 4 and len(reads[0]) >= 2
    a = stream_of(reads[:-1] + [reads[-1][:-1]])
    rec = len(reads[0]) + 1
    b = bytearray(stream_of(reads))
    sep = (len(reads) // 2) * rec - 1
    assert b[sep] == 10
    b[sep] = ord("N")
    b[(len(reads) // 2 + 1) * rec + rec // 3] = 10
    assert len(b) == len(reads) * rec and b.index(10) == rec - 1
    return a, bytes(b)
