"""Every kernel family returns its small results (a total, a flag, a few sums) through the context's zk_scalars block
(csrc/internal.hpp) and its pinned mirror.  What can go wrong there is a field wired to the wrong reader, or a word left
by one entry point read as the fresh result of another.  So: ONE context, every entry point that reads scalars back, on
inputs just past one tile of its scheme, each result against numpy / the host restatements -- and then the same list
again in reverse order, when every host word holds what some other call left there."""
import random

import numpy as np
import pytest

from oracle import zkoracle as zo
from tests import _contigs_restatement as CR
from tests import _ksnp_brute as KB
from tests import _ksnp_cases as KC
from tests import _spectrum_host as H
from tests import _spikein_restatement as SR
from tests import _stop_cases as SC
from tests import _stop_restatement as ST
from tests import _strand_restatement as R
from tests import _vardyger_cases as VC
from tests import _vardyger_restatement as VR
from tests._spikein_cases import allele_text, tables as spike_tables
from zotmer_amd import native, synth

pytestmark = pytest.mark.gpu

N_RLE = 8192 + 1 + 100          # csrc/select.hip RLE_TILE: 8 192 keys
N_CP = 4096 + 1 + 50            # csrc/compact.hpp CP_TILE, select / merge tiles: 4 096 items
N_SCAN = 2048 + 1 + 60          # csrc/codec.hip SCAN_TILE: 2 048 items
M64 = (1 << 64) - 1


def distinct_sorted(rng, n, bits):
    k = np.unique(rng.integers(0, 1 << bits, size=2 * n, dtype=np.uint64))
    return np.sort(rng.choice(k, size=n, replace=False))


def union_np(sets):
    """(keys, u64 sums, acgt weighted by the sums) of the union of (keys, counts) lists"""
    k = np.concatenate([s[0] for s in sets])
    c = np.concatenate([s[1].astype(np.uint64) for s in sets])
    u, inv = np.unique(k, return_inverse=True)
    s = np.zeros(len(u), dtype=np.uint64)
    np.add.at(s, inv, c)
    return u, s, [int(s[(u & np.uint64(3)) == np.uint64(b)].sum()) for b in range(4)]


def checksum_np(keys, counts):
    c = [int(v) for v in counts]
    return (sum(c), sum(int(k) * w for k, w in zip(keys, c)) & M64, sum(R.murmer(int(k), 0) * w for k, w in zip(keys, c)) & M64)


def tagged_table(K, n, rng):
    """n ascending distinct tagged keys (canonical << 1 | tag) with orphans, pairs and palindromes mixed"""
    keys = []
    c = 0
    while len(keys) < n:
        y = R.rc(K, c)
        if c == y:
            keys.append(c << 1)
        elif c < y:
            kind = rng.integers(0, 3)
            keys += [c << 1] if kind == 0 else [(c << 1) | 1] if kind == 1 else [c << 1, (c << 1) | 1]
        c += 1
    return keys[:n]


def make_cases():
    """[(name, run)]: run(ctx) calls the entry point(s) and asserts; every expected value is computed here, once, on the host"""
    rng = np.random.default_rng(20261)
    cases = []

    def case(f):
        cases.append((f.__name__, f))
        return f

    # ---- sort_count, rle: repeats over more than one 8 192-key tile
    rk = np.sort(rng.integers(0, 3000, size=N_RLE, dtype=np.uint64))
    rk_shuffled = rng.permutation(rk)
    ru, rc = np.unique(rk, return_counts=True)

    @case
    def sort_count(ctx):
        k, c = ctx.sort_count(ctx.upload(rk_shuffled), 12)
        assert np.array_equal(k.to_host(), ru) and np.array_equal(c.to_host(), rc.astype(np.uint32))

    @case
    def rle(ctx):
        k, c = ctx.rle(ctx.upload(rk))
        assert np.array_equal(k.to_host(), ru) and np.array_equal(c.to_host(), rc.astype(np.uint32))

    # ---- kmerize: a few thousand bases, reads that repeat their k-mers
    reads = synth.read_strings(11, 0, 40, 100, genome=700, sub_thr=synth.frac32(0.01), n_thr=synth.frac32(0.002))
    stream = ("".join(r + "\n" for r in reads)).encode()
    want_km = {K: zo.kmerize(K, reads) for K in (24, 25)}

    def check_kmerize(ctx, K):
        k, c, st = ctx.kmerize(ctx.upload_stream(stream), K)
        w = want_km[K]
        assert np.array_equal(k.to_host(), w["kmers"]) and np.array_equal(c.to_host(), w["counts"])
        assert st.n_unique == len(w["kmers"]) and list(st.acgt) == w["acgt"]

    @case
    def kmerize_even(ctx):
        check_kmerize(ctx, 24)

    @case
    def kmerize_odd(ctx):
        check_kmerize(ctx, 25)

    @case
    def kmerize_odd_strand_blocks(ctx):
        try:
            ctx.tune(dedupe_bits=18)          # the block dedupe whatever the size: csrc/strand_blocks.hip builds the strands
            check_kmerize(ctx, 25)
        finally:
            ctx.tune(dedupe_bits=0)

    # ---- the compactions and merges: more than one 4 096-item tile
    A, B, D = (distinct_sorted(rng, n, 30) for n in (N_CP, N_CP - 30, N_CP + 11))
    B[:2000] = A[:2000]          # shared keys
    B = np.unique(B)
    cA, cB, cD = (rng.integers(1, 10, size=len(x), dtype=np.uint64) for x in (A, B, D))
    cA[[5, 4100]] = [4096, 70000]          # counts >= 4096: the side list of the histogram

    @case
    def trim(ctx):
        k, c = ctx.trim(ctx.upload(A), ctx.upload(cA.astype(np.uint32)), 3, 8)
        keep = (cA >= 3) & (cA <= 8)
        assert np.array_equal(k.to_host(), A[keep]) and np.array_equal(c.to_host(), cA[keep].astype(np.uint32))

    @case
    def project_dedupe(ctx):
        assert np.array_equal(ctx.project_dedupe(ctx.upload(A), 12).to_host(), np.unique(A >> np.uint64(12)))

    @case
    def split(ctx):
        shared = len(np.intersect1d(A, B))
        assert ctx.split(ctx.upload(A), ctx.upload(B)) == (shared, len(A) - shared, len(B) - shared)

    want_union = union_np([(A, cA), (B, cB)])
    want_merge = union_np([(A, cA), (B, cB), (D, cD)])

    @case
    def union_sum(ctx):
        k, c, acgt = ctx.union_sum(ctx.upload(A), ctx.upload(cA.astype(np.uint32)), ctx.upload(B), ctx.upload(cB.astype(np.uint32)),
                                   want_acgt=True)
        assert np.array_equal(k.to_host(), want_union[0]) and np.array_equal(c.to_host().astype(np.uint64), want_union[1])
        assert acgt == want_union[2]

    def check_merge(ctx):
        k, c, acgt = ctx.merge_n([(ctx.upload(x), ctx.upload(y)) for x, y in ((A, cA), (B, cB), (D, cD))])
        assert np.array_equal(k.to_host(), want_merge[0]) and np.array_equal(c.to_host(), want_merge[1]) and acgt == want_merge[2]

    @case
    def merge_n(ctx):
        check_merge(ctx)

    @case
    def merge_n_kway(ctx):
        try:
            ctx.tune(kway=2)          # csrc/kway.hip at any size
            check_merge(ctx)
        finally:
            ctx.tune(kway=1)

    # ---- project_sum + spectrum_sums
    want_pa, want_pb = H.host_project_sum(A, cA, 8), H.host_project_sum(B, cB, 8)
    want_sp = H.host_spectrum_sums(want_pa[0], want_pa[1], want_pb[0], want_pb[1])

    @case
    def project_sum_spectrum(ctx):
        pa = ctx.project_sum(ctx.upload(A), ctx.upload(cA), 8)
        pb = ctx.project_sum(ctx.upload(B), ctx.upload(cB.astype(np.uint32)), 8)
        for got, want in ((pa, want_pa), (pb, want_pb)):
            assert np.array_equal(got[0].to_host(), want[0]) and np.array_equal(got[1].to_host(), want[1]) and got[2] == want[2]
        got = ctx.spectrum_sums(pa[0], pa[1], pa[2], pb[0], pb[1], pb[2])
        for f in ("cx", "cy", "n_shared", "S_min", "X_shared", "Y_shared", "S_xy"):
            assert got[f] == want_sp[f], f
        # the two doubles: n_shared roundings of a sum taken in any order and the few inside a term (tests/test_gpu_dist_spectrum.py)
        eps = (want_sp["n_shared"] + 8) * 2.0 ** -52
        assert abs(got["S_sqrt"] - want_sp["S_sqrt"]) <= eps * want_sp["sqrt_abs"]
        assert abs(got["S_js"] - want_sp["S_js"]) <= eps * want_sp["js_abs"]

    # ---- hist, the checksums, first_descent
    hv, hf = np.unique(cA, return_counts=True)
    want_hist = {int(v): int(f) for v, f in zip(hv, hf)}
    assert max(want_hist) >= 4096

    @case
    def hist(ctx):
        assert ctx.hist(ctx.upload(cA.astype(np.uint32))) == want_hist

    want_cs = checksum_np(A, cA)

    @case
    def checksum(ctx):
        assert ctx.checksum(ctx.upload(A), ctx.upload(cA.astype(np.uint32))) == want_cs
        assert ctx.checksum_counts(ctx.upload(A), ctx.upload(cA)) == want_cs

    xs = np.concatenate([zo.kmers_list(25, r, True) for r in reads])
    want_scs = (len(xs), int(xs.sum(dtype=np.uint64)), sum(R.murmer(int(x), 0) for x in xs) & M64)
    want_acgt = [int(np.sum((xs & np.uint64(3)) == np.uint64(b))) for b in range(4)]

    @case
    def stream_checksum(ctx):
        d = ctx.upload_stream(stream)
        assert ctx.stream_checksum(d, 25) == want_scs and ctx.stream_acgt(d, 25) == want_acgt

    descent = A.copy()
    descent[4099] = descent[4098]

    @case
    def first_descent(ctx):
        assert ctx.first_descent(ctx.upload(A)) == len(A)
        assert ctx.first_descent(ctx.upload(descent)) == 4099

    # ---- the codec
    want_words = zo.codec64_encode(zo.delta(A))

    @case
    def codec(ctx):
        words = ctx.codec_encode(ctx.upload(A), True)
        assert np.array_equal(words.to_host(), want_words)
        assert np.array_equal(ctx.codec_decode(words, True).to_host(), A)
        assert np.array_equal(ctx.codec_decode(words, True, len(A)).to_host(), A)

    # ---- line_ends, strand_pairs + format_pairs
    text = np.frombuffer(synth.fastq_text(11, 0, 30, 70).encode(), dtype=np.uint8)
    assert len(text) > N_CP

    @case
    def line_ends(ctx):
        assert np.array_equal(ctx.line_ends(ctx.upload(text)).to_host(), np.flatnonzero(text == 10).astype(np.uint64))

    SK = 8
    tk = tagged_table(SK, N_CP, rng)
    tc = [int(v) for v in rng.integers(1, 1000, size=len(tk))]
    wa, wb, wst = R.pairs_of(SK, tk, tc, True)
    assert len({wst["pairs"], wst["orphans"], wst["palindromes"], 0}) == 4          # non-zero and distinct
    want_lines = "".join("%d\t%d\n" % p for p in zip(wa, wb)).encode()

    @case
    def strand_pairs_format(ctx):
        a, b, st = ctx.strand_pairs(ctx.upload(np.array(tk, dtype=np.uint64)), ctx.upload(np.array(tc, dtype=np.uint32)), SK, orphans=True)
        assert (st.n_pairs, st.n_orphans, st.n_palindromes) == (wst["pairs"], wst["orphans"], wst["palindromes"])
        assert np.array_equal(a.to_host(), np.array(wa, dtype=np.uint64)) and np.array_equal(b.to_host(), np.array(wb, dtype=np.uint64))
        assert ctx.format_pairs(a, b).to_host().tobytes() == want_lines

    # ---- the entries whose total lands in the one shared word (csrc/codec.hip scan_total): sizes just past one 2 048-item scan tile
    totals = dict(line_ends=int((text == 10).sum()), strand_pairs=wst["pairs"], format_pairs=len(want_lines),
                  project_sum_a=len(want_pa[0]), project_sum_b=len(want_pb[0]))

    # spike_pairs: the only entry with two landings
    a1, a2 = allele_text(1, 3000), allele_text(2, 3100)
    sp_zones = [("chr1:100-900 a ", 1000, [(a1, 100, 900), (a2, 100, 905)]), ("chr1:901-901 None ", 0, [(a1, 901, 901), (a2, 901, 901)]),
                ("chr2:1000-2999 b ", N_SCAN - 1000, [(a2, 1000, 2999), (a1, 1000, 2899)])]
    sp_scalars = (77, 20, 60, SR.sd_q(60, 0.1), SR.frac32(0.3), SR.frac32(0.05))
    sp_tables = spike_tables(sp_zones)
    want_m1, want_m2, _ = SR.records(*sp_scalars, sp_zones)
    totals.update(spike_mate1=len(want_m1), spike_mate2=len(want_m2))

    @case
    def spike_pairs(ctx):
        o1, o2 = ctx.spike_pairs(*[ctx.upload(t) for t in sp_tables], *sp_scalars, 0, N_SCAN)
        assert (o1.n, o2.n) == (len(want_m1), len(want_m2))
        assert o1.to_host().tobytes() == want_m1.encode("latin-1") and o2.to_host().tobytes() == want_m2.encode("latin-1")

    # contig_render: one offset more than a scan tile of contigs of one to three nodes
    CK = 25
    cr_keys = distinct_sorted(rng, 3000, 2 * CK)
    cr_paths = [rng.integers(0, len(cr_keys), size=1 + i % 3).tolist() for i in range(N_SCAN)]
    want_fasta = CR.text_of(CK, cr_keys.tolist(), cr_paths).encode()
    totals.update(contig_render=len(want_fasta))

    @case
    def contig_render(ctx):
        nodes = np.array([j for p in cr_paths for j in p], dtype=np.uint32)
        offs = np.cumsum([0] + [len(p) for p in cr_paths]).astype(np.uint64)
        assert ctx.contig_render(ctx.upload(cr_keys), CK, ctx.upload(nodes), ctx.upload(offs)).to_host().tobytes() == want_fasta

    # ksnp: groups of one, a group for the workgroup kernel and one past ZK_KSNP_LDS_GROUP for the tile-pair kernel (its tile pairs are scanned too)
    KK = 13
    ks = sum((KC.group(KK, p, KC.random_lows(KK, 1, 50 + p)) for p in range(1100)), [])
    ks += KC.group(KK, 1100, KC.planted_lows(KK, native.KSNP_LDS_GROUP + 6, 3)) + KC.group(KK, 1101, KC.planted_lows(KK, 40, 4))
    ks = np.array(sorted(ks), dtype=np.uint64)
    assert len(ks) > N_SCAN
    want_snps = KB.run(KK, KC.HAMMING, 1, ks)
    # (the entry scans twice more on its way: the groups of two or more, and the tile pairs of the groups past ZK_KSNP_LDS_GROUP)
    ks_sizes = [b - a for a, b in KB.group_slices(KK, ks) if b - a >= 2]
    ks_tiles = [-(-s // native.KSNP_PAIR_TILE) for s in ks_sizes if s > native.KSNP_LDS_GROUP]
    totals.update(ksnp=len(want_snps), ksnp_groups=len(ks_sizes), ksnp_tile_pairs=sum(t * (t + 1) // 2 for t in ks_tiles))

    @case
    def ksnp_components(ctx):
        assert np.array_equal(ctx.ksnp(ctx.upload(ks), KK, native.KSNP_HAMMING, 1).to_host(), want_snps)

    # dup_join: more entries than a scan tile, a duplication in every sequence
    from zotmer_amd.library import vardyger
    DK = 8
    py = random.Random(9)
    dj_records, dj_counts = [], []
    for r in range(24):
        seq = VC.rand_seq(py, 70 + r % 13)
        dj_records.append(("s%03d" % r, seq))
        dj_counts.append({x: py.choice((9, 10, 40)) for x in VR.kmers_list(DK, VC.duplicated(seq, 20, 5 + r % 9), True)})
    dj_index = vardyger.Index(DK, dj_records)
    dj_lists = VC.counted_from(dj_counts)
    dj_tables = [np.asarray(t) for t in (dj_index.rseq, dj_index.rkmer, dj_index.rpos, dj_index.by_second)]
    assert len(dj_lists[0]) > N_SCAN
    want_cover, want_rows = VC.join_by_its_contract(*dj_lists, *[t.tolist() for t in dj_tables], DK, 10)
    totals.update(dup_join=len(want_rows))

    @case
    def dup_join(ctx):
        lists = [ctx.upload(np.array(a, dtype=dt)) for a, dt in zip(dj_lists, (np.uint32, np.uint64, np.uint32))]
        cover, e, i, j = ctx.dup_join(*lists, *[ctx.upload(t) for t in dj_tables], DK, 10)
        assert cover.tolist() == want_cover and list(zip(e.tolist(), i.tolist(), j.tolist())) == want_rows

    # stop_frames: more reads than a scan tile, cut from transcripts with a stop codon every few bases
    from zotmer_amd.library import stopscan
    TK, PAD, SEED = 25, 128, 17
    sf_records = [("tx%d" % t, "".join(VC.rand_seq(py, py.randrange(2, 9)) + py.choice(("TAA", "TAG", "TGA", "TTA", "CTA", "TCA")) for _ in range(40)))
                  for t in range(3)]
    sf_reads = []
    for g in range(N_SCAN):
        seq = sf_records[g % 3][1]
        p = py.randrange(0, len(seq) - 60)
        sf_reads.append(seq[p:p + 60] if g % 2 else SC.rc(seq[p:p + 60]))
    sf_ref = ST.Index(TK, sf_records)
    sf_index = stopscan.Index(TK, [(nm, seq.encode("latin-1")) for nm, seq in sf_records])
    t_of = {nm: t for t, nm in enumerate(sf_index.names)}
    want_stops = sorted((t_of[nm], x) for g, seq in enumerate(sf_reads) for nm, x in ST.read_stops(sf_ref, seq, SEED, g)[0])
    sf_fastq = np.frombuffer(SC.fastq_text(sf_reads).encode(), dtype=np.uint8)
    totals.update(stop_frames=len(want_stops), stop_lines=int((sf_fastq == 10).sum()))          # (the case calls line_ends on its text)

    @case
    def stop_frames(ctx):
        layout = stopscan.layout_of(sf_index, PAD)
        table = stopscan.anchor_table(ctx, sf_index, layout)
        try:
            d = ctx.upload(sf_fastq)
            tx, kmers = ctx.stop_frames(table, ctx.upload(stopscan.starts_of(layout)), d, ctx.line_ends(d), N_SCAN, TK, PAD, SEED, 0)
            assert sorted(zip(tx.to_host().tolist(), kmers.to_host().tolist())) == want_stops
        finally:
            table.free()

    # a word left in the shared landing by one entry can pass for the total of another only if the two totals are equal
    assert len(set(totals.values()) | {0}) == len(totals) + 1, totals
    return cases


def test_scalar_fields_forward_and_reverse():
    import __graft_entry__ as ge
    ge.build()
    cases = make_cases()
    with native.Context(0) as ctx:
        for order in (cases, cases[::-1]):
            for name, run in order:
                print(name)
                run(ctx)
