"""The window front end on the device: every entry that turns bytes of text into windows of K bases, on streams that hold every
byte value 0..255 at every offset modulo 16 (tests/_window_streams.py), and on payloads that lie among bases instead of behind a
separator or a guard word.

The rule is stated once (include/zotk.h): any byte outside AaCcGgTtUu ends the windows that touch it; an entry reads [0, n) of its
stream.  It is implemented several times -- encode_swar16 (stream_pass.hip), encode_words16 (encode_tile.hpp), base_code
(read_window.hpp) and seq_tally.hip's own -- and the other suites feed ACGT, acgtUu, N and line ends only.  Here a byte that shares
bits with a base ('@', 'E', 0xC1, 0x01, ...) sits between two runs of bases: read as a base it gives windows nobody else has, and
the phantom baits (the k-mers those windows would be) make the table entries see it.  Every comparison is exact; the references
are the C oracle and the plain restatements, which tests/test_window_streams_host.py holds against one another on these streams."""
import functools

import numpy as np
import pytest

from oracle import zkoracle as zo
from tests import _disass_restatement as DR
from tests import _hgvsindex_restatement as HR
from tests import _window_streams as W
from tests._core_cases import SEL_TILE
from tests._view_cases import fastq_mask_np
from zotmer_amd import native

pytestmark = pytest.mark.gpu

SEED = 1                     # the seed tests/test_window_streams_host.py checks the phantoms of
KS = (3, 25, 32)
PASS_TILES = (4096, 8192)    # positions a tile of the first pass takes (stream_pass.hip: 512 x 8 and 1024 x 8)
U64 = np.uint64


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


# ---- references, computed once --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ref(K):
    """the stream of every byte at every phase with its windows"""
    stream, offs = W.byte_phase_stream(K, SEED)
    both = W.kmers_both(stream, K)
    both.setflags(write=False)
    return stream, offs, both


@functools.lru_cache(maxsize=None)
def phantoms(K):
    stream, offs, _ = ref(K)
    ph, have = W.phantom_baits(K, stream, offs)
    return ph, have


@functools.lru_cache(maxsize=None)
def fastq_ref(crlf):
    """the FASTQ form at K = 25 -> (text, sequence lines, the phantom table's arrays, phantoms, have)"""
    text, offs, seqs = W.byte_phase_fastq(25, SEED, crlf)
    ph, have = W.phantom_baits(25, text, offs)
    return text, seqs, W.phantom_table(ph, have), ph, have


def summed(want):
    return dict(kmers=want["kmers"], counts=want["counts"], acgt=want["acgt"], n_windows=int(want["counts"].sum(dtype=U64)) // 2)


def check_kmerize(ctx, d, K, want, flags=native.KMERIZE_CANONICAL, label=None):
    k, c, st = ctx.kmerize(d, K, flags)
    assert np.array_equal(k.to_host(), want["kmers"]), label
    assert np.array_equal(c.to_host(), want["counts"]), label
    assert list(st.acgt) == want["acgt"], label
    assert st.n_windows == want["n_windows"] and st.n_instances == 2 * want["n_windows"] and st.n_unique == len(want["kmers"]), label


def table_on_device(ctx, K, arrays, n_records):
    keys, offs, ids = arrays[:3]
    return ctx.bait_table_from_arrays(K, ctx.upload(keys), ctx.upload(offs), ctx.upload(ids), n_records)


# ---- base-stream entries on every byte at every phase -----------------------------------------------------------------------------

@pytest.mark.parametrize("K", KS)
def test_encode_every_byte(ctx, K):
    stream, _, both = ref(K)
    d = ctx.upload_stream(stream)
    out, acgt = ctx.encode(d, K, True)
    assert np.array_equal(out.to_host(), both) and acgt == W.acgt_of(both)
    out, acgt = ctx.encode(d, K, False)
    assert np.array_equal(out.to_host(), both[0::2]) and acgt == W.acgt_of(both[0::2])


@pytest.mark.parametrize("K", KS)
def test_stream_checksum_every_byte(ctx, K):
    stream, _, both = ref(K)
    M = (1 << 64) - 1
    want = [len(both), int(both.sum(dtype=U64)), sum(zo.murmer(int(x), 0) for x in both) & M] + W.acgt_of(both)
    d = ctx.upload_stream(stream)
    assert [int(v) for v in ctx.stream_checksum(d, K)] + ctx.stream_acgt(d, K) == want


@pytest.mark.parametrize("K", KS)
def test_kmerize_every_byte(ctx, K):
    """every first-pass route: the ranged pass in its three forms (encode_swar16), the look-back pipeline and the pass kernel of
    ZK_KMERIZE_BOTH (encode_words16), 8 K-key tiles, and at K = 25 the forced block dedupe with tags and with whole keys"""
    stream, _, both = ref(K)
    want = summed(zo.kmerize(K, [stream]))
    assert want["n_windows"] == len(both) // 2
    d = ctx.upload_stream(stream)
    try:
        for sp in (1, 2, 3, 0):
            ctx.tune(stream_pass=sp)
            check_kmerize(ctx, d, K, want, label=("stream_pass", sp))
        ctx.tune(stream_pass=1)
        check_kmerize(ctx, d, K, want, native.KMERIZE_BOTH, label="both")
        ctx.tune(wide_tiles=0)
        check_kmerize(ctx, d, K, want, label="wide_tiles=0")
        check_kmerize(ctx, d, K, want, native.KMERIZE_BOTH, label="wide_tiles=0 both")
        ctx.tune(wide_tiles=1)
        if K == 25:
            for tw in (1, 0):
                ctx.tune(dedupe_bits=18, tag_words=tw)
                check_kmerize(ctx, d, K, want, label=("dedupe_bits=18 tag_words", tw))
    finally:
        ctx.tune(stream_pass=1, wide_tiles=1, dedupe_bits=0, tag_words=native.DEFAULT_TAG_WORDS)


def filter_want(stream, K, baits):
    """zk_capture_filter restated: a '\\n'-terminated piece is kept iff one of its windows is a bait, else every byte of it is 'N'"""
    data = np.frombuffer(stream, dtype=np.uint8)
    ends = np.flatnonzero(data == 10)
    win = W.windows(stream, K)
    pos = np.array([p for p, _ in win], dtype=np.int64)
    hit = np.isin(np.array([x for _, x in win], dtype=U64), np.asarray(baits, dtype=U64))
    kept = np.unique(np.searchsorted(ends, pos[hit]))                      # read = the terminators before the window
    read_of = np.searchsorted(ends, np.arange(len(data)))
    blank = (data != 10) & (read_of < len(ends)) & ~np.isin(read_of, kept)  # bytes behind the last terminator belong to no read
    return np.where(blank, np.uint8(ord("N")), data).tobytes(), len(ends), len(kept)


@pytest.mark.parametrize("K", [25, 32])
def test_capture_filter_every_byte(ctx, K):
    stream, offs, _ = ref(K)
    ph, _ = phantoms(K)
    baits = np.unique(ph)
    want, n_reads, n_kept = filter_want(stream, K, baits)
    # kept: the pieces whose byte is a base and nothing else (v = '\n' cuts its piece in two, neither half holds a bait)
    assert n_reads == 4096 + 16 and n_kept == 10 * 16
    out, nr, nk = ctx.capture_filter(ctx.upload_stream(stream), K, ctx.upload(baits))
    assert (nr, nk) == (n_reads, n_kept)
    assert out.to_host().tobytes() == want


def bait_table_want(stream, K):
    """zk_bait_table_build restated (capture.py:85-95): every K-mer of both strands of every '\\n'-terminated record -> the
    ascending records that hold it"""
    data = np.frombuffer(stream, dtype=np.uint8)
    ends = np.flatnonzero(data == 10)
    win = W.windows(stream, K)
    pos = np.array([p for p, _ in win], dtype=np.int64)
    x = np.array([v for _, v in win], dtype=U64)
    rec = np.searchsorted(ends, pos)
    return W.table_arrays(np.concatenate([x, W.revcomp(x, K)]), np.concatenate([rec, rec])) + (len(ends),)


@pytest.mark.parametrize("K", KS)
def test_bait_table_build_every_byte(ctx, K):
    stream, _, _ = ref(K)
    keys, offs, ids, n_records = bait_table_want(stream, K)
    t = ctx.bait_table(ctx.upload_stream(stream), K)
    try:
        assert (t.n_keys, t.n_ids, t.n_records) == (len(keys), len(ids), n_records)
        gk, go, gi = (a.to_host() for a in t.arrays())
        assert np.array_equal(gk, keys) and np.array_equal(go, offs) and np.array_equal(gi, ids)
    finally:
        t.free()


def bins_of(d):
    h = {}
    for c in d.values():
        h[c] = h.get(c, 0) + 1
    return sorted(h.items())


def spectra_want(stream, K, both, seed=17, p=1.0):
    """zk_contig_spectra by the definition (disass.py:91-99): per record the dict of the k-mers of kmersList(K, seq, both) that
    pass sub(seed, p, .), as (record << 32 | count, frequency) words; the counted key list; the stats"""
    recs = stream.split(b"\n")[:-1]
    keep, keys, words, n_windows = {}, {}, [], 0
    for r, seq in enumerate(recs):
        d = {}
        for _, x in W.windows(seq, K):
            y = W.revcomp(x, K)
            for z in ((x, y) if both else (x,)):
                if z not in keep:
                    keep[z] = DR.sub(seed, p, z)
                if keep[z]:
                    d[z] = d.get(z, 0) + 1
            k = min(x, y) if both else x
            keys[k] = keys.get(k, 0) + 1
            n_windows += 1
        words += [((r << 32) | c, f) for c, f in bins_of(d)]
    return words, sorted(keys.items()), (len(recs), n_windows)


@pytest.mark.parametrize("both", [0, 1])
@pytest.mark.parametrize("K", KS)
def test_contig_spectra_every_byte(ctx, K, both):
    stream, _, _ = ref(K)
    want_words, want_keys, (n_records, n_windows) = spectra_want(stream, K, both)
    words, freq, keys, counts, st = ctx.contig_spectra(ctx.upload_stream(stream), K, both, 17, 1.0)
    assert (st.n_records, st.n_windows, st.n_keys, st.n_bins) == (n_records, n_windows, len(want_keys), len(want_words))
    assert list(zip(keys.to_host().tolist(), counts.to_host().tolist())) == want_keys
    assert list(zip(words.to_host().tolist(), freq.to_host().tolist())) == want_words


# ---- FASTQ-text entries on every byte at every phase ---------------------------------------------------------------------------------

EOLS = [False, True]
EOL_IDS = ["lf", "crlf"]


@pytest.mark.parametrize("crlf", EOLS, ids=EOL_IDS)
def test_line_ends_and_fastq_mask_every_byte(ctx, crlf):
    text, seqs, _, _, _ = fastq_ref(crlf)
    d = ctx.upload_stream(text)
    data = np.frombuffer(text, dtype=np.uint8)
    assert np.array_equal(ctx.line_ends(d).to_host(), np.flatnonzero(data == 10).astype(U64))
    masked, n_nl = ctx.fastq_mask(d)
    want_mask, want_nl = fastq_mask_np(text, 0)
    assert n_nl == want_nl == 4 * len(seqs) and np.array_equal(masked.to_host(), want_mask)
    # the masked stream holds the windows of the sequence lines and no others
    K = 25
    want = summed(zo.kmerize(K, list(seqs)))
    try:
        for sp in (1, 0):
            ctx.tune(stream_pass=sp)
            check_kmerize(ctx, masked, K, want, label=("masked", sp))
    finally:
        ctx.tune(stream_pass=1)


@functools.lru_cache(maxsize=None)
def read_windows(crlf, K):
    """the forward windows of every sequence line -> (read numbers int64, k-mers u64), in read order"""
    _, seqs, _, _, _ = fastq_ref(crlf)
    rd, xs = [], []
    for r, s in enumerate(seqs):
        w = [x for _, x in W.windows(s, K)]
        rd += [r] * len(w)
        xs += w
    return np.array(rd, dtype=np.int64), np.array(xs, dtype=U64)


@functools.lru_cache(maxsize=None)
def hits_want(crlf, veto_values=()):
    """zk_capture_hits / zk_pulldown_hits restated (capture.py:97-116, pulldown.py:77-99) on the phantom table: a read hits record
    v iff one of its forward 25-mers is a phantom of v; a read with a window among the phantoms of veto_values is pushed up
    -> (pairs ascending, hist[257], vetoed reads)"""
    _, seqs, table, ph, have = fastq_ref(crlf)
    rd, xs = read_windows(crlf, 25)
    which, ids = W.table_hits(table, xs)
    vetoed = set()
    if veto_values:
        vw, _ = W.table_hits(W.phantom_table(ph, have, only=veto_values), xs)
        vetoed = set(rd[vw].tolist())
    per_read = {}
    for r, v in zip(rd[which].tolist(), ids.tolist()):
        if r not in vetoed:
            per_read.setdefault(r, set()).add(v)
    pairs = np.array(sorted((v << 32) | r for r, vs in per_read.items() for v in vs), dtype=U64)
    hist = np.zeros(257, dtype=U64)
    for r in range(len(seqs)):
        if r not in vetoed:
            hist[len(per_read.get(r, ()))] += 1
    return pairs, hist, len(vetoed)


NOT_BASES = tuple(v for v in range(256) if not W.is_base(v))
VETO = NOT_BASES + (ord("A"), ord("c"))          # the reads around 'A' and 'c' are pushed up; any other means a misread byte


@pytest.mark.parametrize("crlf", EOLS, ids=EOL_IDS)
def test_capture_and_pulldown_hits_every_byte(ctx, crlf):
    text, seqs, table, ph, have = fastq_ref(crlf)
    pairs, hist, vetoed = hits_want(crlf)
    # the reads around a base hit the record of that base, one each, and no other read hits anything
    assert vetoed == 0 and len(pairs) == 10 * 16 and hist[1] == 160 and hist[0] == len(seqs) - 160
    assert sorted(set((pairs >> U64(32)).tolist())) == sorted(W.CODE)
    vpairs, vhist, vvetoed = hits_want(crlf, VETO)
    assert vvetoed == 32 and len(vpairs) == 8 * 16
    d = ctx.upload_stream(text)
    lines = ctx.line_ends(d)
    t = table_on_device(ctx, 25, table, 256)
    veto = table_on_device(ctx, 25, W.phantom_table(ph, have, only=VETO), 256)
    try:
        n = len(seqs)
        assert np.array_equal(ctx.capture_hits(t, 25, d, lines, n).to_host(), pairs)
        gp, gh, gv = ctx.pulldown_hits(t, 25, d, lines, n)
        assert np.array_equal(gp.to_host(), pairs) and np.array_equal(gh, hist) and gv == 0
        assert np.array_equal(ctx.capture_hits(t, 25, d, lines, n, veto=veto).to_host(), vpairs)
        gp, gh, gv = ctx.pulldown_hits(t, 25, d, lines, n, veto=veto)
        assert np.array_equal(gp.to_host(), vpairs) and np.array_equal(gh, vhist) and gv == vvetoed
        # both mates: the same text twice gives the same pairs
        assert np.array_equal(ctx.capture_hits(t, 25, d, lines, n, d, lines).to_host(), pairs)
    finally:
        t.free()
        veto.free()


@pytest.mark.parametrize("crlf", EOLS, ids=EOL_IDS)
@pytest.mark.parametrize("K", [25, 31])
def test_strand_keys_every_byte(ctx, K, crlf):
    text, seqs, _, _, _ = fastq_ref(crlf)
    d = ctx.upload_stream(text)
    lines = ctx.line_ends(d)
    T = (1 << (2 * K)) - 1                       # the largest hash: every window is kept
    for reverse in (0, 1):
        want = W.tagged_keys(K, seqs, reverse)
        out = ctx.empty(len(want) + 64, np.uint64)
        n, fit = ctx.strand_keys(d, lines, len(seqs), K, reverse, T, out)
        assert fit and n == len(want)
        assert np.array_equal(np.sort(out.to_host()[:n]), want), reverse


def pileup_want(K, table, seqs, strip=bytes.strip):
    """zk_anchor_pileup by its definition (include/zotk.h) -> the sorted (coordinate, k-mer) pairs"""
    out = []
    for s in seqs:
        s = strip(s)
        wins = W.windows(s, K)
        if not wins:
            continue
        for lst in ([(x, p) for p, x in wins], [(W.revcomp(x, K), len(s) - p - K) for p, x in wins]):
            which, anchors = W.table_hits(table, np.array([x for x, _ in lst], dtype=U64))
            D = {int(a) - lst[i][1] for i, a in zip(which.tolist(), anchors.tolist())}
            out += [(d + p, x) for d in D for x, p in lst]
    return sorted(out)


@pytest.mark.parametrize("crlf", EOLS, ids=EOL_IDS)
def test_anchor_pileup_every_byte(ctx, crlf):
    K, pad = 25, 128
    text, seqs, table, _, _ = fastq_ref(crlf)
    assert max(len(s) for s in seqs) + 1 <= pad
    anchors = (table[0], table[1], table[2] + np.uint32(pad))              # record v -> the anchor pad + v
    want = pileup_want(K, anchors, seqs)
    assert len(want) >= 160 * 2 * 42
    d = ctx.upload_stream(text)
    lines = ctx.line_ends(d)
    t = table_on_device(ctx, K, anchors, 256 + 2 * pad)
    try:
        oc, ok = ctx.anchor_pileup(t, d, lines, len(seqs), K, pad)
        assert sorted(zip(oc.to_host().tolist(), ok.to_host().tolist())) == want
    finally:
        t.free()


@pytest.mark.parametrize("crlf", EOLS, ids=EOL_IDS)
@pytest.mark.parametrize("K", [25, 32])
def test_capture_kmers_every_byte(ctx, K, crlf):
    """every read against one bait (all reads, not only those that hit: the entry takes the pairs it is given)"""
    text, seqs, _, _, _ = fastq_ref(crlf)
    d = ctx.upload_stream(text)
    lines = ctx.line_ends(d)
    n = len(seqs)
    pairs = (U64(3) << U64(32)) | np.arange(n, dtype=U64)
    want = np.sort(np.concatenate([W.kmers_both(s, K) for s in seqs]))
    ob, ok = ctx.capture_kmers(ctx.upload(pairs), d, lines, n, K)
    assert ob.n == len(want) and np.all(ob.to_host() == 3)
    assert np.array_equal(np.sort(ok.to_host()), want)


def test_sequence_tally_every_byte(ctx):
    """the genome tally's own classifier ('\\n' and '\\r' vanish, any other byte outside the bases ends the run): the whole stream,
    and at every phase in two pieces cut at the byte v and just behind it"""
    K = 25
    stream, offs, both = ref(K)
    ph, have = phantoms(K)
    # keys: the phantoms and every 40th real window, so that the counts are not only those around the ten bases
    keys = np.unique(np.concatenate([ph.reshape(-1), both[0::80]]))
    table = (keys, np.arange(len(keys) + 1, dtype=np.uint32), np.zeros(len(keys), dtype=np.uint32))
    got, wst, wnw, wgt = HR.tally(K, stream, set(keys.tolist()))
    want = np.array([got.get(int(x), 0) for x in keys], dtype=U64)
    assert wnw > len(both) // 2 and want.sum() > 160 * K          # windows that bridge a '\n' or '\r' count too
    t = table_on_device(ctx, K, table, 1)
    d = ctx.upload_stream(stream)
    try:
        counts = ctx.upload(np.zeros(len(keys), dtype=U64))
        st, nw, gt = ctx.sequence_tally(t, d, (0, 0), counts)
        assert np.array_equal(counts.to_host(), want) and (st, nw, gt) == (wst, wnw, wgt)
        for s in range(W.PHASES):
            for v in (ord("N"), ord("\r"), ord("G"), 0xC7, 0x07, ord(">")):
                for cut in (int(offs[v, s]), int(offs[v, s]) + 1):
                    counts = ctx.upload(np.zeros(len(keys), dtype=U64))
                    st, nw_a, _ = ctx.sequence_tally(t, d.view(cut), (0, 0), counts)
                    st, nw_b, _ = ctx.sequence_tally(t, d.view(len(stream) - cut, cut), st, counts)
                    assert np.array_equal(counts.to_host(), want) and st == wst and nw_a + nw_b == wnw, (s, v, cut)
    finally:
        t.free()


# ---- strip semantics: every byte first and last on its line -------------------------------------------------------------------------------

STRIP_LEN = 40


@functools.lru_cache(maxsize=None)
def strip_case():
    """FASTQ text of two records per byte value v != '\\n', with v the first and the last byte of the sequence line, around 40
    (a blank v) or 39 (any other) bases that every read shares: bytes.strip() leaves 40 bytes of every line
    -> (text, the sequence lines, the 40 bases)"""
    body = W.base_run(STRIP_LEN, 77)
    seqs = []
    for v in range(256):
        if v != 10:
            b = bytes([v])
            seqs += [b + body, body + b] if b.strip() == b"" else [b + body[1:], body[:-1] + b]
    assert all(len(s.strip()) == STRIP_LEN for s in seqs) and sum(len(s) > STRIP_LEN for s in seqs) == 2 * 5
    text = b"".join(b"CATG\n" + s + b"\nTTG\n" + b"G" * len(s) + b"\n" for s in seqs)
    return text, seqs, body


def test_strip_anchor_pileup(ctx):
    """The line is stripped as bytes.strip() strips it before it is measured.  The pairs themselves do not move with the line (a
    diagonal and a position shift together), so the length is what shows: pad is the stripped length of every line here, and a
    line with a hit that is longer than pad is ZK_ERANGE -- a blank that stayed on its line would make it so."""
    K, pad = 25, STRIP_LEN
    text, seqs, body = strip_case()
    # zones: the body, then its reverse complement (so that both orientations hit), 2 * pad apart
    n_win = len(body) - K + 1
    fwd = np.array([x for _, x in W.windows(body, K)], dtype=U64)
    keys = np.concatenate([fwd, W.revcomp(fwd, K)[::-1]])
    anchors = np.concatenate([pad + np.arange(n_win), n_win + 3 * pad + np.arange(n_win)])
    table = W.table_arrays(keys, anchors)
    want = pileup_want(K, table, seqs)
    assert len(want) >= len(seqs) * 2 * (n_win - 1)
    d = ctx.upload_stream(text)
    lines = ctx.line_ends(d)
    t = table_on_device(ctx, K, table, 2 * n_win + 4 * pad)
    try:
        oc, ok = ctx.anchor_pileup(t, d, lines, len(seqs), K, pad)
        assert sorted(zip(oc.to_host().tolist(), ok.to_host().tolist())) == want
        # the bound is live: one base more on a line is refused
        long = ctx.upload_stream(b"CATG\n" + body + b"A\nTTG\n" + b"G" * (STRIP_LEN + 1) + b"\n")
        with pytest.raises(native.ZotkError) as e:
            ctx.anchor_pileup(t, long, ctx.line_ends(long), 1, K, pad)
        assert e.value.code == native.ZK_ERANGE
        oc, ok = ctx.anchor_pileup(t, d, lines, len(seqs), K, pad)                  # (and the context is fine afterwards)
        assert oc.n == len(want)
    finally:
        t.free()


def test_strip_capture_gather(ctx):
    text, seqs, _ = strip_case()
    d = ctx.upload_stream(text)
    lines = ctx.line_ends(d)
    n = len(seqs)
    pairs = np.arange(n, dtype=U64)                                        # every read, bait 0
    want = b"".join(b"CATG\n" + s.strip() + b"\nTTG\n" + b"G" * len(s) + b"\n" for s in seqs)
    out, first_pair, first_byte = ctx.capture_gather(ctx.upload(pairs), 1, d, lines)
    assert out.to_host().tobytes() == want
    assert first_pair.tolist() == [0, n] and first_byte.tolist() == [0, len(want)]


# ---- sequence lines around the 64-window step of the one-wave-per-read walk -----------------------------------------------------------

WALK_K = 25


@functools.lru_cache(maxsize=None)
def walk_case():
    """FASTQ records whose sequence lines are K - 1, K, K + 1, 62 + K .. 65 + K, 127 + K and 128 + K letters long: no window, one, two;
    the last window in lanes 62 and 63 of the first step, the first windows of the second step; and the same one step on
    -> (text, the sequence lines)"""
    K = WALK_K
    lens = [K - 1, K, K + 1, 62 + K, 63 + K, 64 + K, 65 + K, 127 + K, 128 + K]
    seqs = [W.base_run(n, 900 + n) for n in lens]
    assert [len(W.windows(s, K)) for s in seqs] == [0, 1, 2, 63, 64, 65, 66, 128, 129]
    text = b"".join(b"CATG\n" + s + b"\nTTG\n" + b"G" * len(s) + b"\n" for s in seqs)
    return text, seqs


def walk_table(seqs, pad=0):
    """the LAST window of every line as a key: record (anchor) pad + the line's number"""
    K = WALK_K
    last = [(W.windows(s, K)[-1][1], pad + r) for r, s in enumerate(seqs) if len(s) >= K]
    return W.table_arrays([x for x, _ in last], [r for _, r in last])


def test_walk_lengths_capture_and_pulldown_hits(ctx):
    K = WALK_K
    text, seqs = walk_case()
    table = walk_table(seqs)
    d = ctx.upload_stream(text)
    lines = ctx.line_ends(d)
    n = len(seqs)
    want = np.array(sorted((r << 32) | r for r in range(1, n)), dtype=U64)          # every line but the short one hits its own record
    t = table_on_device(ctx, K, table, n)
    veto = table_on_device(ctx, K, W.table_arrays([W.windows(seqs[5], K)[-1][1]], [0]), 1)    # the window in lane 0 of the second step
    try:
        assert np.array_equal(ctx.capture_hits(t, K, d, lines, n).to_host(), want)
        assert np.array_equal(ctx.capture_hits(t, K, d, lines, n, d, lines).to_host(), want)
        gp, gh, gv = ctx.pulldown_hits(t, K, d, lines, n)
        assert np.array_equal(gp.to_host(), want) and gh[0] == 1 and gh[1] == n - 1 and gv == 0
        assert np.array_equal(ctx.capture_hits(t, K, d, lines, n, veto=veto).to_host(), want[want != U64((5 << 32) | 5)])
        gp, gh, gv = ctx.pulldown_hits(t, K, d, lines, n, veto=veto)
        assert gv == 1 and gh[1] == n - 2
    finally:
        t.free()
        veto.free()


def test_walk_lengths_strand_keys(ctx):
    K = WALK_K
    text, seqs = walk_case()
    d = ctx.upload_stream(text)
    lines = ctx.line_ends(d)
    for reverse in (0, 1):
        want = W.tagged_keys(K, seqs, reverse)
        out = ctx.empty(len(want) + 64, np.uint64)
        n, fit = ctx.strand_keys(d, lines, len(seqs), K, reverse, (1 << (2 * K)) - 1, out)
        assert fit and n == len(want) == 518
        assert np.array_equal(np.sort(out.to_host()[:n]), want), reverse


def test_walk_lengths_capture_kmers(ctx):
    K = WALK_K
    text, seqs = walk_case()
    d = ctx.upload_stream(text)
    lines = ctx.line_ends(d)
    n = len(seqs)
    pairs = (U64(3) << U64(32)) | np.arange(n, dtype=U64)
    want = np.concatenate([W.kmers_both(s, K) for s in seqs])
    for mates, reps in (((), 1), ((d, lines), 2)):
        ob, ok = ctx.capture_kmers(ctx.upload(pairs), d, lines, n, K, *mates)
        assert ob.n == reps * len(want) and np.all(ob.to_host() == 3)
        assert np.array_equal(np.sort(ok.to_host()), np.sort(np.tile(want, reps)))


def test_walk_lengths_anchor_pileup(ctx):
    K, pad = WALK_K, 256
    text, seqs = walk_case()
    table = walk_table(seqs, pad)
    want = pileup_want(K, table, seqs)
    assert len(want) == 518                      # one diagonal per line, from its last window, in the forward list only
    d = ctx.upload_stream(text)
    lines = ctx.line_ends(d)
    t = table_on_device(ctx, K, table, 3 * pad)
    try:
        oc, ok = ctx.anchor_pileup(t, d, lines, len(seqs), K, pad)
        assert sorted(zip(oc.to_host().tolist(), ok.to_host().tolist())) == want
    finally:
        t.free()


# ---- stream ends and surroundings ----------------------------------------------------------------------------------------------------------------

def lengths(K, tiles):
    """n from K - 1 to K + 40 (every residue modulo 16 at least twice; n < K gives nothing), and around the tiles of the kernel"""
    out = list(range(K - 1, K + 41))
    for t in tiles:
        out += [t - 1, t, t + 1, 2 * t + 5]
    return out


def embedded_view(ctx, payload, lead):
    whole = W.embedded(payload, lead)
    dw = ctx.upload(whole)
    return dw, whole, dw.view(len(payload), lead)


STREAM16_LEADS = (16, 112, 48)        # the entries that need a 16-byte stream: tests/_frames.py's placements
ANY_LEADS = (1, 7, 16)
ENTRIES = ["encode", "stream_checksum", "kmerize", "capture_filter", "bait_table_build", "contig_spectra", "fastq_text"]


def fastq_payload():
    """five records whose sequence lines are cut from one genome (lengths around the 64 window starts of a chunk), every other line
    base letters; it ends with its last '\\n' -> (text, sequence lines, genome)"""
    g = W.base_run(600, 91)
    seqs = [g[10:10 + 25], g[40:40 + 88], g[100:100 + 89], g[150:150 + 24], g[200:200 + 153]]
    text = b"".join(g[300 + r:311 + r] + b"\n" + s + b"\n" + g[320:323] + b"\n" + g[330 + r:330 + r + len(s)] + b"\n" for r, s in enumerate(seqs))
    return text, seqs, g


@pytest.mark.parametrize("entry", ENTRIES)
def test_streams_embedded_in_bases(ctx, entry):
    """The payload starts with a window at byte 0 and lies among random bases: a kernel that reads in front of its pointer or past
    n_bytes and takes what it finds for text gives one k-mer too many (behind a guard word or zeros it would meet a separator).
    zk_encode, zk_stream_checksum and zk_kmerize take a run of bases without a separator, so windows reach byte n - 1; the entries
    whose records are '\\n'-terminated by contract take the run followed by its '\\n'.  The bytes around the payload are compared
    afterwards: inputs are not changed."""
    K = 25
    if entry == "fastq_text":
        return embedded_fastq(ctx, K)
    tiles = dict(encode=(SEL_TILE,), kmerize=PASS_TILES).get(entry, (SEL_TILE, 4096))
    terminated = entry in ("capture_filter", "bait_table_build", "contig_spectra")
    leads = ANY_LEADS if entry in ("bait_table_build", "contig_spectra") else STREAM16_LEADS
    try:
        for n in lengths(K, tiles):
            payload = W.base_run(n - 1, n) + b"\n" if terminated else W.base_run(n, n)
            both = W.kmers_both(payload, K)
            assert len(both) == 2 * max(0, n - terminated - K + 1)
            if entry == "stream_checksum":
                want = (len(both), int(both.sum(dtype=U64)), sum(zo.murmer(int(x), 0) for x in both) & ((1 << 64) - 1))
            elif entry == "kmerize":
                k, c = W.counted(both)
                want = dict(kmers=k, counts=c, acgt=W.acgt_of(both), n_windows=len(both) // 2)
            elif entry == "bait_table_build":
                keys, offs, ids, n_records = bait_table_want(payload, K)
            elif entry == "contig_spectra":
                want = [spectra_want(payload, K, b) for b in (0, 1)]
            for lead in leads:
                dw, whole, d = embedded_view(ctx, payload, lead)
                tag = (entry, n, lead)
                if entry == "encode":
                    out, acgt = ctx.encode(d, K, True)
                    assert np.array_equal(out.to_host(), both) and acgt == W.acgt_of(both), tag
                    out, _ = ctx.encode(d, K, False)
                    assert np.array_equal(out.to_host(), both[0::2]), tag
                elif entry == "stream_checksum":
                    assert ctx.stream_checksum(d, K) == want and ctx.stream_acgt(d, K) == W.acgt_of(both), tag
                elif entry == "kmerize":
                    for sp in (1, 0):
                        ctx.tune(stream_pass=sp)
                        check_kmerize(ctx, d, K, want, label=tag + (sp,))
                elif entry == "capture_filter":
                    # baits: the second half of the payload's windows and every window that crosses an end of the payload
                    at = int(lead)
                    cross = [x for p, x in W.windows(bytes(whole), K) if p < at or p + K > at + n]
                    baits = np.unique(np.concatenate([both[len(both) // 4 * 2:], np.array(cross, dtype=U64)]))
                    want, n_reads, n_kept = filter_want(payload, K, baits)
                    out, nr, nk = ctx.capture_filter(d, K, ctx.upload(baits))
                    assert (nr, nk) == (n_reads, n_kept) == (1, int(n - 1 >= K)) and out.to_host().tobytes() == want, tag
                elif entry == "bait_table_build":
                    t = ctx.bait_table(d, K)
                    try:
                        assert (t.n_keys, t.n_ids, t.n_records) == (len(keys), len(ids), 1), tag
                        if t.n_keys:
                            gk, go, gi = (a.to_host() for a in t.arrays())
                            assert np.array_equal(gk, keys) and np.array_equal(go, offs) and np.array_equal(gi, ids), tag
                    finally:
                        t.free()
                else:
                    for both_strands in (0, 1):
                        want_words, want_keys, (n_records, n_windows) = want[both_strands]
                        words, freq, keys, counts, st = ctx.contig_spectra(d, K, both_strands, 17, 1.0)
                        assert (st.n_records, st.n_windows, st.n_keys, st.n_bins) == (1, n_windows, len(want_keys), len(want_words)), tag
                        assert list(zip(keys.to_host().tolist(), counts.to_host().tolist())) == want_keys, tag
                        assert list(zip(words.to_host().tolist(), freq.to_host().tolist())) == want_words, tag
                assert np.array_equal(dw.to_host(), whole), tag
    finally:
        ctx.tune(stream_pass=1)


def embedded_fastq(ctx, K):
    """the text entries on a FASTQ payload that ends with its last '\\n', at leads 1 and 7 (any address) and, for zk_fastq_mask, 16"""
    text, seqs, g = fastq_payload()
    n = len(seqs)
    data = np.frombuffer(text, dtype=np.uint8)
    ends = np.flatnonzero(data == 10).astype(U64)
    # the table: records = pieces of the genome, so that reads 0, 1, 2 and 4 hit (read 3 has no window), some of them two records
    recs = [g[0:120], g[90:260], g[255:400]]
    win = [(r, x) for r, s in enumerate(recs) for x in W.kmers_both(s, K).tolist()]
    table = W.table_arrays([x for _, x in win], [r for r, _ in win])
    rd, xs = [], []
    for r, s in enumerate(seqs):
        w = [x for _, x in W.windows(s, K)]
        rd += [r] * len(w)
        xs += w
    which, ids = W.table_hits(table, np.array(xs, dtype=U64))
    pairs = np.unique(np.array([(int(v) << 32) | rd[i] for i, v in zip(which.tolist(), ids.tolist())], dtype=U64))
    assert sorted(set((pairs & U64(0xFFFFFFFF)).tolist())) == [0, 1, 2, 4] and len(pairs) > 4
    hist = np.bincount(np.bincount((pairs & U64(0xFFFFFFFF)).astype(np.int64), minlength=n), minlength=4).astype(U64)
    pad = 256
    anchors = W.table_arrays(table[0], pad + np.arange(len(table[0])))      # one anchor per key
    want_pile = pileup_want(K, anchors, seqs)
    want_kmers = sorted((int(w) >> 32, x) for w in pairs for x in W.kmers_both(seqs[int(w) & 0xFFFFFFFF], K).tolist())
    t = table_on_device(ctx, K, table, len(recs))
    ta = table_on_device(ctx, K, anchors, len(table[0]) + 2 * pad)
    try:
        for lead in (1, 7, 16):
            dw, whole, d = embedded_view(ctx, text, lead)
            lines = ctx.line_ends(d)
            assert np.array_equal(lines.to_host(), ends), lead
            assert np.array_equal(ctx.capture_hits(t, K, d, lines, n).to_host(), pairs), lead
            gp, gh, gv = ctx.pulldown_hits(t, K, d, lines, n)
            assert np.array_equal(gp.to_host(), pairs) and np.array_equal(gh, hist) and gv == 0, lead
            for reverse in (0, 1):
                want = W.tagged_keys(K, seqs, reverse)
                out = ctx.empty(len(want) + 8, np.uint64)
                got, fit = ctx.strand_keys(d, lines, n, K, reverse, (1 << (2 * K)) - 1, out)
                assert fit and got == len(want) and np.array_equal(np.sort(out.to_host()[:got]), want), lead
            oc, ok = ctx.anchor_pileup(ta, d, lines, n, K, pad)
            assert sorted(zip(oc.to_host().tolist(), ok.to_host().tolist())) == want_pile, lead
            ob, ok = ctx.capture_kmers(ctx.upload(pairs), d, lines, n, K)
            assert sorted(zip(ob.to_host().tolist(), ok.to_host().tolist())) == want_kmers, lead
            if lead % 16 == 0:
                masked, n_nl = ctx.fastq_mask(d)
                want_mask, want_nl = fastq_mask_np(text, 0)
                assert n_nl == want_nl and np.array_equal(masked.to_host(), want_mask), lead
            assert np.array_equal(dw.to_host(), whole), lead
    finally:
        t.free()
        ta.free()
