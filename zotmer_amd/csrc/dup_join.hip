// dup_join.hip -- `zot vardyger` (zotmer/commands/vardyger.py:82-133, 403-431): candidate tandem duplications, joined.
//
// With J = K / 2 a K-mer is two J-mers, a first half and a second.  The reference keeps, per sequence, the halves of its own
// K-mers (wtFst, wtLst) and of the K-mers counted from the reads (fst, lst); findDup names (a, b, c, d) with ab and cd K-mers of
// the sequence, cb and cd counted, a != c and b != d, and positions places ab and cd on the sequence and keeps the placements
// with cd more than J behind ab.  Every half comes from a K-mer of the sequence, so positions' search by Hamming distance finds
// the exact J-mers only, and a row is a counted entry cb with two occurrences of K-mers of its sequence:
//   * The occurrence table lists every window of every sequence, ascending by (sequence, K-mer, position): the occurrences whose
//     first half is c are a run of it.  d_by_second is the same table ascending by (sequence, second half, first half,
//     position): the occurrences whose second half is b are a run of that.
//   * dup_cover_kernel looks every occurrence up in its own sequence's segment of the counted list: one search each.
//   * dup_join_kernel<false> takes an entry per lane: the first place of either run (two searches; an entry that has no run
//     ends there), their ends (a few steps, a search when a run is long), and the pairs of the two runs that make rows.  A lane
//     walks a product of up to ZK_DUP_WAVE_PAIRS pairs itself; a larger one is done by the wave, 64 pairs a step in the order of
//     the rows, a ballot counting them.  scan64_inclusive turns the counts into offsets, the host decides whether the rows fit, and
//     dup_join_kernel<true> walks the entries that have rows again and writes them, ranked by the same ballots.
// No atomics, no float: the same call leaves the same bytes.
#include "internal.hpp"
#include "search.hpp"

namespace zk {

constexpr int DJ_BLOCK = 256;
constexpr u32 DJ_WAVE_PAIRS = ZK_DUP_WAVE_PAIRS;

struct DupList { const u32* baits; const u64* kmers; const u32* counts; u32 n; };              // ascending by (bait, k-mer)
struct DupOcc { const u32* seq; const u64* kmer; const u32* pos; const u32* by_second; u32 m; };   // ascending by (sequence, k-mer, position)
struct DupGroup { u32 i0, ni, j0, nj; };   // by_second[i0, i0 + ni): the second half is b; occurrences [j0, j0 + nj): the first half is c

// the occurrence at place k of the by-second order (a value that is no index reads the last occurrence: wrong rows for a wrong
// table, no access outside it)
__device__ __forceinline__ u32 dj_by(const DupOcc& R, u32 k) {
    const u32 i = R.by_second[k];
    return i < R.m ? i : R.m - 1;
}

// the end of the run that starts at lo: same() holds on a prefix of [lo, hi) that lo belongs to.  Runs are short (a half-mer occurs
// once in a sequence, but for repeats): a few steps, then a search.
template <class P>
__device__ __forceinline__ u32 dj_run_end(u32 lo, u32 hi, P same) {
    u32 e = lo + 1;
    for (int t = 0; t < 3 && e < hi && same(e); t++) e++;
    if (e < hi && same(e)) e = partition_point(e + 1, hi, same);
    return e;
}

// the two runs of the entry (s, x); ni * nj == 0 when either is empty
__device__ __forceinline__ DupGroup dj_group(const DupOcc& R, u32 s, u64 x, int K) {
    const u64 low = (1ull << K) - 1;                 // K = 2 J bits a half: K <= 32, no shift by 64
    const u64 c = x >> K, b = x & low;
    DupGroup g = {0, 0, 0, 0};
    const u32 m = R.m;
    const u32 i0 = partition_point(0u, m, [&](u32 k) {
        const u32 i = dj_by(R, k);
        const u32 rs = R.seq[i];
        return rs < s || (rs == s && (R.kmer[i] & low) < b);
    });
    auto same_b = [&](u32 k) { const u32 i = dj_by(R, k); return R.seq[i] == s && (R.kmer[i] & low) == b; };
    if (i0 == m || !same_b(i0)) return g;
    const u32 j0 = partition_point(0u, m, [&](u32 j) {
        const u32 rs = R.seq[j];
        return rs < s || (rs == s && (R.kmer[j] >> K) < c);
    });
    auto same_c = [&](u32 j) { return R.seq[j] == s && (R.kmer[j] >> K) == c; };
    if (j0 == m || !same_c(j0)) return g;
    g.i0 = i0;
    g.ni = dj_run_end(i0, m, same_b) - i0;
    g.j0 = j0;
    g.nj = dj_run_end(j0, m, same_c) - j0;
    return g;
}

// is (place ii of the first run, place jj of the second) a row of the entry x = cb?  -> the two occurrences
__device__ __forceinline__ bool dj_pair(const DupOcc& R, const u32* __restrict__ cover, const DupGroup& g, u32 ii, u32 jj, u64 x, int K,
                                        u32 min_count, u32& i, u32& j) {
    i = dj_by(R, g.i0 + ii);
    j = g.j0 + jj;
    return (R.kmer[i] >> K) != (x >> K) && R.kmer[j] != x && cover[j] >= min_count && (u64)R.pos[j] > (u64)R.pos[i] + (u64)(K / 2);
}

// cover[i] = the count of occurrence i's k-mer among the entries of its own sequence, 0 if it has none
__global__ __launch_bounds__(DJ_BLOCK) void dup_cover_kernel(DupList L, DupOcc R, u32* __restrict__ cover) {
    for (u64 i = (u64)blockIdx.x * DJ_BLOCK + threadIdx.x; i < R.m; i += (u64)gridDim.x * DJ_BLOCK) {
        const u32 s = R.seq[i];
        const u64 x = R.kmer[i];
        const u32 k = partition_point(0u, L.n, [&](u32 e) {
            const u32 b = L.baits[e];
            return b < s || (b == s && L.kmers[e] < x);
        });
        cover[i] = k < L.n && L.baits[k] == s && L.kmers[k] == x ? L.counts[k] : 0u;
    }
}

// EMIT false: cells[e] = the rows of entry e.  EMIT true: cells holds the inclusive scan of those, and the rows are written:
// entry e's at [cells[e - 1], cells[e]), ascending by the place of ab in the by-second order and then by cd.
template <bool EMIT>
__global__ __launch_bounds__(DJ_BLOCK) void dup_join_kernel(DupList L, DupOcc R, const u32* __restrict__ cover, int K, u32 min_count,
                                                            u64* __restrict__ cells, u32* __restrict__ out_e, u32* __restrict__ out_i,
                                                            u32* __restrict__ out_j, u64 cap) {
    const int lane = threadIdx.x & 63;
    const u64 wave = ((u64)blockIdx.x * DJ_BLOCK + threadIdx.x) >> 6, nw = ((u64)gridDim.x * DJ_BLOCK) >> 6;
    for (u64 base = wave * 64; base < L.n; base += nw * 64) {          // the whole wave stays in the loop: the ballots below
        const u64 e64 = base + (u64)lane;
        const bool in = e64 < L.n;
        const u32 e = (u32)e64;
        DupGroup g = {0, 0, 0, 0};
        u64 x = 0, at = 0, mine = 0;
        if (in) {
            bool live;
            if (EMIT) {                               // an entry without rows is not searched again
                at = e ? cells[e - 1] : 0;
                live = cells[e] != at;
            } else {
                live = L.counts[e] >= min_count;
            }
            if (live) {
                x = L.kmers[e];
                g = dj_group(R, L.baits[e], x, K);
            }
        }
        const u64 prod = (u64)g.ni * g.nj;
        const bool big = prod > (u64)DJ_WAVE_PAIRS;
        if (prod != 0 && !big) {
            for (u32 ii = 0; ii < g.ni; ii++)
                for (u32 jj = 0; jj < g.nj; jj++) {
                    u32 i, j;
                    if (!dj_pair(R, cover, g, ii, jj, x, K, min_count, i, j)) continue;
                    if (EMIT) {
                        if (at < cap) { out_e[at] = e; out_i[at] = i; out_j[at] = j; }
                        at++;
                    } else {
                        mine++;
                    }
                }
        }
        // the large products, one after the other, by the whole wave: pair p = ii * nj + jj of lane l is p0 + l
        u64 pend = __ballot(big);
        while (pend) {
            const int src = __ffsll((long long)pend) - 1;
            pend &= pend - 1;
            DupGroup gs;
            gs.i0 = __shfl(g.i0, src, 64); gs.ni = __shfl(g.ni, src, 64); gs.j0 = __shfl(g.j0, src, 64); gs.nj = __shfl(g.nj, src, 64);
            const u64 xs = (u64)__shfl((u32)x, src, 64) | (u64)__shfl((u32)(x >> 32), src, 64) << 32;
            const u64 ats = (u64)__shfl((u32)at, src, 64) | (u64)__shfl((u32)(at >> 32), src, 64) << 32;
            const u32 es = (u32)(base + (u64)src);
            const u64 prods = (u64)gs.ni * gs.nj;
            const u32 step_i = 64u / gs.nj, step_j = 64u % gs.nj;
            u32 ii = (u32)lane / gs.nj, jj = (u32)lane % gs.nj;
            u64 pos = ats;
            for (u64 p0 = 0; p0 < prods; p0 += 64) {
                u32 i = 0, j = 0;
                const bool ok = ii < gs.ni && dj_pair(R, cover, gs, ii, jj, xs, K, min_count, i, j);
                const u64 hm = __ballot(ok);
                if (EMIT && ok) {
                    const u64 p = pos + popc_below(hm);
                    if (p < cap) { out_e[p] = es; out_i[p] = i; out_j[p] = j; }
                }
                pos += (u64)__popcll(hm);
                ii += step_i;
                jj += step_j;
                if (jj >= gs.nj) { jj -= gs.nj; ii++; }
            }
            if (lane == src) mine = pos - ats;
        }
        if (!EMIT && in) cells[e] = mine;
    }
}

static int dup_join(zk_ctx* c, const DupList& L, const DupOcc& R, int K, u32 min_count, u32* cover, u32* out_e, u32* out_i, u32* out_j,
                    uint64_t cap, uint64_t* n_out) {
    *n_out = 0;
    const uint64_t n = L.n, m = R.m;
    if (m == 0) return ZK_OK;
    prof_begin(c, ZK_PROF_DUP_COVER, 16 * m);
    hipLaunchKernelGGL(dup_cover_kernel, dim3(grid_cap(c, div_up(m, DJ_BLOCK), 16)), dim3(DJ_BLOCK), 0, c->stream, L, R, cover);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    if (n == 0) return check_device_error(c);
    const uint64_t room = 8 * n + (4 << 20);
    ZK_TRY(arena_require(c, room, room));
    u64* cells;
    ZK_TRY(arena_alloc(c, 8 * n, (void**)&cells));
    const u32 grid = grid_cap(c, div_up(n, DJ_BLOCK), 16);
    prof_begin(c, ZK_PROF_DUP_JOIN, 16 * n);
    hipLaunchKernelGGL(dup_join_kernel<false>, dim3(grid), dim3(DJ_BLOCK), 0, c->stream, L, R, (const u32*)cover, K, min_count, cells,
                       (u32*)nullptr, (u32*)nullptr, (u32*)nullptr, (u64)0);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(scan_total(c, cells, n, n_out));
    const uint64_t total = *n_out;
    if (total > cap) return no_room(c, "zk_dup_join", "rows", total, cap);
    if (total == 0) return ZK_OK;
    prof_begin(c, ZK_PROF_DUP_JOIN, 16 * n + 12 * total);
    hipLaunchKernelGGL(dup_join_kernel<true>, dim3(grid), dim3(DJ_BLOCK), 0, c->stream, L, R, (const u32*)cover, K, min_count, cells, out_e,
                       out_i, out_j, (u64)cap);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    return check_device_error(c);
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_dup_join(zk_ctx* c, const uint32_t* d_baits, const uint64_t* d_kmers, const uint32_t* d_counts, uint64_t n, const uint32_t* d_rseq,
                const uint64_t* d_rkmer, const uint32_t* d_rpos, const uint32_t* d_by_second, uint64_t m, int K, uint32_t min_count,
                uint32_t* d_cover, uint32_t* d_entry, uint32_t* d_left, uint32_t* d_right, uint64_t cap, uint64_t* n_out) {
    ZK_ARGS(c, n_out && (n == 0 || (d_baits && d_kmers && d_counts)) && (m == 0 || (d_rseq && d_rkmer && d_rpos && d_by_second && d_cover)) &&
                   (cap == 0 || (d_entry && d_left && d_right)));
    if (K < 2 || K > 32 || (K & 1)) return fail(c, ZK_EINVAL, "zk_dup_join: K = %d, even and 2 <= K <= 32", K);
    if (n >= (1ull << 32) || m >= (1ull << 32))
        return fail(c, ZK_EINVAL, "zk_dup_join: %llu entries, %llu occurrences (indices are 32 bits wide: fewer than 2^32 of either)",
                    (unsigned long long)n, (unsigned long long)m);
    arena_reset(c);
    return dup_join(c, DupList{d_baits, (const u64*)d_kmers, d_counts, (u32)n}, DupOcc{d_rseq, (const u64*)d_rkmer, d_rpos, d_by_second, (u32)m}, K,
                    min_count, d_cover, d_entry, d_left, d_right, cap, n_out);
}

}  // extern "C"
