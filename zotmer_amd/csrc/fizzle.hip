// fizzle.hip -- `zot fizzle` (zotmer/commands/fizzle.py:555-583): which classes of exon tuples do the windows of a read pair hit?
//
// The reference indexes every K-mer of its exons by the tuple of exons that hold it, and per read pair builds two records:
// orientation 0 = the forward windows of mate 1 and the reverse-complement windows of mate 2, orientation 1 the other way
// round.  recHits (fizzle.py:354-414) starts from sdx = {tuple: windows of the record that have it}.  zk_fizzle_votes computes
// sdx for every record of a batch, with the distinct tuples numbered as classes by the host:
//   * One wave per pair, 64 windows per step, cut from the stripped sequence lines (read_window.hpp) and looked up in a bait
//     table whose every key lists one id, its class (bait_table.hpp).  The table is not canonical -- an exon has a strand -- so
//     a window is looked up once for each orientation, as x and as rc(x).
//   * A wave keeps the (class, windows) list of the record it is on in LDS, ZK_FIZZLE_CLASSES entries at most: the classes of
//     a step are taken one after the other (the lowest lane that has one left names it, a ballot counts its lanes), and the
//     list is searched 64 entries at a time.  A record with more distinct classes is done by a path that keeps no list: the
//     classes ascend, and the next one -- the smallest above the last -- and its windows come from walking the record again
//     (slow, exact, and only ever taken by reads laid across hundreds of tuples).
//   * fizzle_count_kernel leaves per record its hits, its class if it has one only, and the entries it will write (its distinct
//     classes if two or more); scan64_inclusive turns those into offsets and the host decides whether they fit.  Only then
//     fizzle_single_kernel adds the one-class records to d_single and d_hist (64-bit integer atomics: totals that do not depend
//     on the order) and fizzle_emit_kernel writes the others' entries, each record's ascending by class at its own offset.
//     A refused call has added and written nothing.  No float.
#include "internal.hpp"
#include "bait_table.hpp"
#include "read_window.hpp"

namespace zk {

constexpr int FZ_CLASSES = ZK_FIZZLE_CLASSES, FZ_BLOCK = 256, FZ_WAVES = FZ_BLOCK / 64;
static_assert(FZ_CLASSES >= 64 && FZ_CLASSES % 64 == 0 && FZ_CLASSES * 8 * FZ_WAVES <= 64 * 1024, "a wave's class list lives in LDS");

__device__ __forceinline__ void fz_wave_fence() {      // what one lane of the wave stored in LDS, the others read after this
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// f(hit, cls) for every step of 64 windows of record 2 p + o: the windows of mate 1 and then of mate 2, forward in mate o and
// reverse-complemented in the other; lane l holds the window that starts at byte l of the step, hit = it is in the table, cls its
// class.  Called by the whole wave.
template <class F>
__device__ __forceinline__ void fz_walk(const BaitView& bt, const Mate& m1, const Mate& m2, u64 p, int K, int o, int lane, F f) {
    for (int m = 0; m < 2; m++) {
        const Mate mt = m ? m2 : m1;
        u64 s, e;
        seq_line(mt.lines, p, s, e);
        strip(mt.text, s, e);
        if (e - s < (u64)K) continue;
        const bool rc = (m ^ o) != 0;
        for_each_chunk(mt.text, s, e, K, lane, [&](u64, bool valid, u64 x) {
            u32 lo = 0, hi = 0;
            const bool hit = valid && bait_find(bt, rc ? revcomp(K, x) : x, lo, hi);
            f(hit, hit ? bt.ids[lo] : 0u);
            return false;
        });
    }
}

// The (class, windows) list of record 2 p + o into lcls / lcnt, in the order the classes are met: nd entries, hits = the windows
// in the table.  False when the record has more than FZ_CLASSES distinct classes (the list is then of no use; hits is whole).
__device__ __forceinline__ bool fz_collect(const BaitView& bt, const Mate& m1, const Mate& m2, u64 p, int K, int o, int lane, u32* lcls,
                                           u32* lcnt, u32& nd, u32& hits) {
    u32 n = 0, h = 0;
    bool over = false;
    fz_walk(bt, m1, m2, p, K, o, lane, [&](bool hit, u32 cls) {
        u64 pend = __ballot(hit);
        h += (u32)__popcll(pend);
        while (pend && !over) {
            const u32 c = __shfl(cls, __ffsll((long long)pend) - 1, 64);
            const u64 same = __ballot(hit && cls == c);
            pend &= ~same;
            u64 found = 0;
            u32 j0 = 0;
            for (; j0 < n; j0 += 64) {
                found = __ballot(j0 + lane < n && lcls[j0 + lane] == c);
                if (found) break;
            }
            if (found) {
                if (lane == 0) lcnt[j0 + (u32)__ffsll((long long)found) - 1] += (u32)__popcll(same);
            } else if (n < (u32)FZ_CLASSES) {
                if (lane == 0) { lcls[n] = c; lcnt[n] = (u32)__popcll(same); }
                n++;
                fz_wave_fence();
            } else {
                over = true;
            }
        }
    });
    fz_wave_fence();
    nd = n;
    hits = h;
    return !over;
}

// The smallest class of record 2 p + o above `after` (any class when first), and the windows that have it, by walking the
// record.  False when there is none.
__device__ __forceinline__ bool fz_next_class(const BaitView& bt, const Mate& m1, const Mate& m2, u64 p, int K, int o, int lane, bool first,
                                              u32 after, u32& c, u32& k) {
    u32 best = 0, mine = 0;
    bool any = false;
    fz_walk(bt, m1, m2, p, K, o, lane, [&](bool hit, u32 cls) {
        if (hit && (first || cls > after)) {
            if (!any || cls < best) { best = cls; mine = 1; any = true; }
            else if (cls == best) mine++;
        }
    });
    if (!__ballot(any)) return false;
    c = wave_min_u32(any ? best : 0xffffffffu);
    k = wave_sum_u32(any && best == c ? mine : 0u);
    return true;
}

// per record 2 p + o: ent = the entries it will write (its distinct classes if there are two or more, else 0), hits = its
// windows in the table, one = its class if it has exactly one
__global__ __launch_bounds__(FZ_BLOCK) void fizzle_count_kernel(BaitView bt, Mate m1, Mate m2, u64 n_pairs, int K, u64* __restrict__ ent,
                                                                u32* __restrict__ one, u32* __restrict__ hits_out) {
    __shared__ u32 s_cls[FZ_WAVES][FZ_CLASSES];
    __shared__ u32 s_cnt[FZ_WAVES][FZ_CLASSES];
    const WaveIds w = wave_ids();
    const int lane = w.lane, wv = (threadIdx.x >> 6) & (FZ_WAVES - 1);
    u32 *lcls = s_cls[wv], *lcnt = s_cnt[wv];
    for (u64 p = w.wave; p < n_pairs; p += w.nw)
        for (int o = 0; o < 2; o++) {
            u32 nd, hits;
            if (!fz_collect(bt, m1, m2, p, K, o, lane, lcls, lcnt, nd, hits)) {
                nd = 0;
                u32 c = 0, k;
                while (fz_next_class(bt, m1, m2, p, K, o, lane, nd == 0, c, c, k)) nd++;
            }
            const u32 c0 = nd == 1 ? lcls[0] : 0u;
            if (lane == 0) { ent[2 * p + o] = nd >= 2 ? nd : 0; one[2 * p + o] = c0; hits_out[2 * p + o] = hits; }
            fz_wave_fence();                         // the next record's list comes after these reads
        }
}

// the records with one class: a thread each
__global__ __launch_bounds__(FZ_BLOCK) void fizzle_single_kernel(const u64* __restrict__ incl, const u32* __restrict__ one,
                                                                 const u32* __restrict__ hits, u64 n_rec, u64 n_classes, u64* __restrict__ single,
                                                                 u64* __restrict__ hist, u64 n_hist) {
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += (u64)gridDim.x * blockDim.x) {
        const u64 h = hits[r];
        if (h == 0 || incl[r] != (r ? incl[r - 1] : 0)) continue;
        const u64 c = one[r];
        if (c >= n_classes) continue;                // (the table's ids are below its record count)
        atomicAdd((unsigned long long*)&single[2 * c], 1ull);
        atomicAdd((unsigned long long*)&single[2 * c + 1], (unsigned long long)h);
        atomicAdd((unsigned long long*)&hist[h < n_hist - 1 ? h : n_hist - 1], 1ull);
    }
}

// the records with two classes or more: entries [incl[r - 1], incl[r]) ascending by class
__global__ __launch_bounds__(FZ_BLOCK) void fizzle_emit_kernel(BaitView bt, Mate m1, Mate m2, u64 n_pairs, int K, const u64* __restrict__ incl,
                                                               u32* __restrict__ out_rec, u32* __restrict__ out_cls, u32* __restrict__ out_cnt,
                                                               u64 cap) {
    __shared__ u32 s_cls[FZ_WAVES][FZ_CLASSES];
    __shared__ u32 s_cnt[FZ_WAVES][FZ_CLASSES];
    const WaveIds w = wave_ids();
    const int lane = w.lane, wv = (threadIdx.x >> 6) & (FZ_WAVES - 1);
    u32 *lcls = s_cls[wv], *lcnt = s_cnt[wv];
    for (u64 p = w.wave; p < n_pairs; p += w.nw)
        for (int o = 0; o < 2; o++) {
            const u64 r = 2 * p + o;
            u64 at = r ? incl[r - 1] : 0;
            const u64 want = incl[r] - at;
            if (want == 0) continue;
            if (want <= (u64)FZ_CLASSES) {
                u32 nd, hits;
                fz_collect(bt, m1, m2, p, K, o, lane, lcls, lcnt, nd, hits);
                nd = nd < (u32)want ? nd : (u32)want;            // (they are equal: the count pass saw the same text)
                for (u32 j = (u32)lane; j < nd; j += 64) {
                    const u32 cj = lcls[j];
                    u32 rank = 0;
                    for (u32 i = 0; i < nd; i++) rank += lcls[i] < cj ? 1u : 0u;
                    const u64 pos = at + rank;
                    if (pos < cap) { out_rec[pos] = (u32)r; out_cls[pos] = cj; out_cnt[pos] = lcnt[j]; }
                }
                fz_wave_fence();
            } else {
                u32 c = 0, k;
                const u64 end = at + want;
                for (bool first = true; at < end && fz_next_class(bt, m1, m2, p, K, o, lane, first, c, c, k); first = false, at++)
                    if (lane == 0 && at < cap) { out_rec[at] = (u32)r; out_cls[at] = c; out_cnt[at] = k; }
            }
        }
}

static int fizzle_votes(zk_ctx* c, const zk_bait_table* classes, int K, Mate m1, Mate m2, uint64_t n_reads, uint64_t n_classes, u64* single,
                        u64* hist, uint64_t n_hist, u32* out_rec, u32* out_cls, u32* out_cnt, uint64_t cap, uint64_t* n_out) {
    *n_out = 0;
    if (n_reads == 0 || classes->n_keys == 0) return ZK_OK;
    const BaitView bt = view_of(classes);
    const uint64_t n_rec = 2 * n_reads;
    const uint64_t room = 16 * n_rec + (4 << 20);
    ZK_TRY(arena_require(c, room, room));
    u64* ent;
    u32 *one, *hits;
    ZK_TRY(arena_alloc(c, 8 * n_rec, (void**)&ent));
    ZK_TRY(arena_alloc(c, 4 * n_rec, (void**)&one));
    ZK_TRY(arena_alloc(c, 4 * n_rec, (void**)&hits));
    const u32 grid = grid_cap(c, div_up(n_reads, FZ_WAVES), 16);
    uint64_t tb1 = 0, tb2 = 0;
    if (c->profile) {
        ZK_HIP(c, hipMemcpy(&tb1, m1.lines + 4 * n_reads - 1, sizeof(u64), hipMemcpyDeviceToHost));
        ZK_HIP(c, hipMemcpy(&tb2, m2.lines + 4 * n_reads - 1, sizeof(u64), hipMemcpyDeviceToHost));
    }
    prof_begin(c, ZK_PROF_FIZZLE_COUNT, tb1 + tb2 + 16 * n_rec);
    hipLaunchKernelGGL(fizzle_count_kernel, dim3(grid), dim3(FZ_BLOCK), 0, c->stream, bt, m1, m2, (u64)n_reads, K, ent, one, hits);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(scan_total(c, ent, n_rec, n_out));
    const uint64_t total = *n_out;
    if (total > cap) return no_room(c, "zk_fizzle_votes", "entries", total, cap);
    prof_begin(c, ZK_PROF_FIZZLE_EMIT, 16 * n_rec + 12 * total);
    hipLaunchKernelGGL(fizzle_single_kernel, dim3(grid_cap(c, div_up(n_rec, FZ_BLOCK), 16)), dim3(FZ_BLOCK), 0, c->stream, ent, one, hits, (u64)n_rec,
                       (u64)n_classes, single, hist, (u64)n_hist);
    if (total)
        hipLaunchKernelGGL(fizzle_emit_kernel, dim3(grid), dim3(FZ_BLOCK), 0, c->stream, bt, m1, m2, (u64)n_reads, K, ent, out_rec, out_cls, out_cnt,
                           (u64)cap);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    return check_device_error(c);
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_fizzle_votes(zk_ctx* c, const zk_bait_table* classes, int K, const uint8_t* d_text1, const uint64_t* d_lines1, const uint8_t* d_text2,
                    const uint64_t* d_lines2, uint64_t n_reads, uint64_t n_classes, uint64_t* d_single, uint64_t* d_hist, uint64_t n_hist,
                    uint32_t* d_rec, uint32_t* d_cls, uint32_t* d_cnt, uint64_t cap, uint64_t* n_out) {
    ZK_ARGS(c, classes && n_out && (n_reads == 0 || (d_text1 && d_lines1 && d_text2 && d_lines2 && d_hist && n_hist > 0)) &&
                   (n_reads == 0 || n_classes == 0 || d_single) && (cap == 0 || (d_rec && d_cls && d_cnt)));
    if (K < 1 || K > 32) return fail(c, ZK_EINVAL, "zk_fizzle_votes: K = %d, 1 <= K <= 32", K);
    if (classes->K != K) return fail(c, ZK_EINVAL, "zk_fizzle_votes: K = %d, the class table was built with K = %d", K, classes->K);
    if (classes->n_records != n_classes)
        return fail(c, ZK_EINVAL, "zk_fizzle_votes: n_classes = %llu, the class table has %llu records", (unsigned long long)n_classes,
                    (unsigned long long)classes->n_records);
    if (n_reads >= (1ull << 31))
        return fail(c, ZK_ERANGE, "zk_fizzle_votes: %llu pairs in one batch (record numbers are 32 bits wide: fewer than 2^31)",
                    (unsigned long long)n_reads);
    arena_reset(c);
    return fizzle_votes(c, classes, K, Mate{d_text1, (const u64*)d_lines1}, Mate{d_text2, (const u64*)d_lines2}, n_reads, n_classes,
                        (u64*)d_single, (u64*)d_hist, n_hist, d_rec, d_cls, d_cnt, cap, n_out);
}

}  // extern "C"
