// vars_scan.hip -- `zot vars -r` (zotmer/commands/vars.py:85-119): the sample contexts in which some next base is enriched over
// the reference set beyond chance.
//
// The reference walks two sorted (k-mer, count) lists group by group (a group = the entries sharing x >> 2) and evaluates
// logBinGe(p, n, k) -- an O(n) log-sum -- for every base of every sample group.  Here one pass over both lists hands back only the
// groups that can print, as an exact superset; the host evaluates the reference's formulas on those rows.
//   * vars_join_kernel: the merge-path cut of setops.hip (A = the reference list, B = the sample list, ties A first), a tile's two
//     slices staged in LDS with the halo of include/zotk.h.  A thread walks VS_ITEMS merged elements; on a sample entry that
//     starts a group it has the A cursor i of that entry, and the reference group of the same context lies in A[i - 4, i + 2]:
//     the A entries not above the sample entry are the (at most 4) just before the cursor, the ones above it the (at most 3)
//     just after.  The thread owns the group: it gathers both groups into scalars, tests the four lanes and, for a row, sets
//     the bit of the group's first sample entry in a mask.  The workgroups stride over the tiles and add their tallies once.
//   * the rows leave through compact.hpp over the mask (count, scan, write): the write pass gathers a row's two groups again,
//     the reference group by binary search -- per ROW, not per group; nothing waits on another workgroup.
#include <cmath>

#include "internal.hpp"
#include "compact.hpp"
#include "search.hpp"

namespace zk {

constexpr int VS_BLOCK = 512;
constexpr int VS_ITEMS = 8;
constexpr int VS_TILE = VS_BLOCK * VS_ITEMS;
static_assert(VS_TILE == MERGE_TILE && VS_TILE == ZK_VARS_TILE, "the tiles are make_partition's; include/zotk.h exports their size");
constexpr int VS_NW = VS_BLOCK / 64;
constexpr int VS_HALO_A = 4;       // reference entries staged before a tile's slice (and as many after it: 3 are read)
constexpr int VS_HALO_B = 1;       // sample entries before the slice (is the first entry a group's head?); 3 after it
constexpr int VS_SLOTS = VS_TILE + 2 * VS_HALO_A + VS_HALO_B + 3;

// ---------------------------------------------------------------------------------------
// the first term of logBinGe in the reference's order of operations (library/stats.py:77-84, 121-128, 214-222)
// ---------------------------------------------------------------------------------------
__device__ const double VS_LOG_SMALL_FAC[25] = {
    0, 0, 0.69314718055994529, 1.791759469228055, 3.1780538303479458,
    4.7874917427820458, 6.5792512120101012, 8.5251613610654147, 10.604602902745251, 12.801827480081469,
    15.104412573075516, 17.502307845873887, 19.987214495661885, 22.552163853123425, 25.19122118273868,
    27.89927138384089, 30.671860106080672, 33.505073450136891, 36.395445208033053, 39.339884187199495,
    42.335616460753485, 45.380138898476908, 48.471181351835227, 51.606675567764377, 54.784729398112319};
constexpr double VS_HALF_LOG_PI = 0.5723649429247001;      // log(pi) / 2
constexpr double VS_GUARD_UNIT = 0x1p-47;                  // 64 roundings of 2^-53

// log(m!) and, in mag, the sum of the magnitudes of the terms it is made of
__device__ __forceinline__ double vs_log_fac(u64 m, double& mag) {
#pragma clang fp contract(off)
    if (m < 25) { mag = 64.0; return VS_LOG_SMALL_FAC[m]; }
    const double x = (double)m, lx = log(x);
    mag = x * lx + x + 64.0;
    return x * lx - x + log(x * (1.0 + 4.0 * x * (1.0 + 2.0 * x))) / 6.0 + VS_HALF_LOG_PI;
}

// one lane: count k of n in the sample, g of gt in the reference.  Candidate = can have logBinGe(g / gt, n, k) < threshold.
__device__ __forceinline__ bool vs_candidate(u64 k, u64 n, u64 g, u64 gt, double threshold) {
#pragma clang fp contract(off)
    if (g == 0 || g >= gt) return false;
    // k / n > g / gt exactly
    const u64 lhi = __umul64hi(k, gt), llo = k * gt, rhi = __umul64hi(n, g), rlo = n * g;
    if (!(lhi > rhi || (lhi == rhi && llo > rlo))) return false;
    const double p = (double)g / (double)gt;
    if (!(0.0 < p && p < 1.0)) return false;          // the reference's own test, on its own double
    const double lp = log(p), l1mp = log1p(-p);
    double mag = 0.0, lc = 0.0;
    if (k != 0 && k != n) {
        double m0, m1, m2;
        const double f0 = vs_log_fac(n, m0), f1 = vs_log_fac(n - k, m1), f2 = vs_log_fac(k, m2);
        lc = f0 - (f1 + f2);
        mag = m0 + m1 + m2;
    }
    const double dk = (double)k, dr = (double)(n - k);
    const double F = lc + lp * dk + l1mp * dr;
    mag += dk * fabs(lp) + dr * fabs(l1mp);
    return F < threshold + mag * VS_GUARD_UNIT;
}

__device__ __forceinline__ u64 vs_count(const void* c, int bits, u64 i) {
    return bits == 32 ? (u64)((const u32*)c)[i] : ((const u64*)c)[i];
}

struct VarsLists {
    const u64* rk; const void* rc; int rbits; u64 n_ref;
    const u64* sk; const void* sc; int sbits; u64 n_sam;
};

// tallies[0..3] = sample groups, groups whose context is not in the reference, joined groups whose reference group has >= 2
// entries, the smallest missing context (starts at ~0)
__global__ __launch_bounds__(VS_BLOCK) void vars_join_kernel(VarsLists L, const u64* __restrict__ part, u32 tiles, double threshold,
                                                             u32* __restrict__ mask, u64* __restrict__ tallies, u32* __restrict__ err) {
    __shared__ u64 keys[VS_SLOTS];
    __shared__ u64 cnts[VS_SLOTS];
    __shared__ u64 scratch[VS_NW];
    const int tid = threadIdx.x;
    const u64 nA = L.n_ref, nB = L.n_sam;
    u64 n_groups = 0, n_missing = 0, n_mixed = 0, first_missing = ~0ull;
    for (u32 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const u64 a0 = part[tile], a1 = part[tile + 1];
        u64 d0 = (u64)tile * VS_TILE, d1 = d0 + VS_TILE;
        if (d1 > nA + nB) d1 = nA + nB;
        const u64 b0 = d0 - a0, b1 = d1 - a1;
        const int nAt = (int)(a1 - a0), nBt = (int)(b1 - b0);
        // ka[p] = A[a0 - 4 + p], p < nAt + 8;  kb[q] = B[b0 - 1 + q], q < nBt + 4.  Slots past either list hold 0 and are never
        // taken for entries: validity is always the global index.  All loads of a thread before its first LDS write (setops.hip).
        u64* const ka = keys;
        u64* const kb = keys + nAt + 2 * VS_HALO_A;
        u64* const ca = cnts;
        u64* const cb = cnts + nAt + 2 * VS_HALO_A;
        {
            constexpr int R = (VS_SLOTS + VS_BLOCK - 1) / VS_BLOCK;
            const int slots = nAt + nBt + 2 * VS_HALO_A + VS_HALO_B + 3;
            u64 kv[R], cv[R];
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int sl = tid + r * VS_BLOCK;
                const bool isA = sl < nAt + 2 * VS_HALO_A;
                const u64 g = isA ? a0 + (u64)sl - VS_HALO_A : b0 + (u64)(sl - nAt - 2 * VS_HALO_A) - VS_HALO_B;     // wraps below 0: >= n
                const bool ok = sl < slots && g < (isA ? nA : nB);
                // a slot without an entry loads the sample's first one (n_sam > 0) and keeps 0: no load sits in a branch of its own
                const u64 at = ok ? g : 0;
                const bool fromA = ok && isA;
                kv[r] = (fromA ? L.rk : L.sk)[at];
                cv[r] = vs_count(fromA ? L.rc : L.sc, fromA ? L.rbits : L.sbits, at);
                if (!ok) { kv[r] = 0; cv[r] = 0; }
            }
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int sl = tid + r * VS_BLOCK;
                if (sl < slots) { keys[sl] = kv[r]; cnts[sl] = cv[r]; }
            }
        }
        __syncthreads();

        const int total = nAt + nBt;
        int d = tid * VS_ITEMS;
        if (d > total) d = total;
        int i = partition_point(d > nBt ? d - nBt : 0, d < nAt ? d : nAt,
                                [&](int mid) { return ka[VS_HALO_A + mid] <= kb[VS_HALO_B + d - mid - 1]; });
        int j = d - i;
#pragma unroll 1
        for (int s = 0; s < VS_ITEMS; s++) {
            if (d + s >= total) break;
            const bool hasA = i < nAt, hasB = j < nBt;
            const u64 ak = ka[VS_HALO_A + i], bk = kb[VS_HALO_B + j];
            if (hasA && (!hasB || ak <= bk)) { i++; continue; }
            // the sample entry b0 + j, with i reference entries of the tile merged before it
            const u64 ctx = bk >> 2;
            const bool head = (b0 + (u64)j == 0) || (kb[j] >> 2) != ctx;          // kb[j] = the entry before it
            if (head) {
                n_groups++;
                u64 s0 = 0, s1 = 0, s2 = 0, s3 = 0, st = 0;
                bool over = false;
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const u64 key = kb[VS_HALO_B + j + t];
                    if (b0 + (u64)(j + t) < nB && (key >> 2) == ctx) {
                        const u64 c = cb[VS_HALO_B + j + t];
                        const u32 b = (u32)key & 3u;
                        s0 = b == 0 ? c : s0; s1 = b == 1 ? c : s1; s2 = b == 2 ? c : s2; s3 = b == 3 ? c : s3;
                        st += c;
                        over |= st < c;
                    }
                }
                u64 g0 = 0, g1 = 0, g2 = 0, g3 = 0, gt = 0;
                int n_in_ref = 0;
#pragma unroll
                for (int t = 0; t < 2 * VS_HALO_A - 1; t++) {          // A[a0 + i - 4 .. a0 + i + 2]
                    const u64 key = ka[i + t];
                    if (a0 + (u64)(i + t) - VS_HALO_A < nA && (key >> 2) == ctx) {
                        const u64 c = ca[i + t];
                        const u32 b = (u32)key & 3u;
                        g0 = b == 0 ? c : g0; g1 = b == 1 ? c : g1; g2 = b == 2 ? c : g2; g3 = b == 3 ? c : g3;
                        gt += c;
                        over |= gt < c;
                        n_in_ref++;
                    }
                }
                if (over) atomicOr(err, ZK_DERR_COUNT_OVERFLOW);
                if (n_in_ref == 0) {
                    n_missing++;
                    first_missing = ctx < first_missing ? ctx : first_missing;
                } else if (n_in_ref >= 2) {
                    n_mixed++;
                    bool row = false;
#pragma unroll 1
                    for (int b = 0; b < 4 && !over; b++) {
                        const u64 k = b == 0 ? s0 : b == 1 ? s1 : b == 2 ? s2 : s3;
                        const u64 g = b == 0 ? g0 : b == 1 ? g1 : b == 2 ? g2 : g3;
                        row |= vs_candidate(k, st, g, gt, threshold);
                    }
                    if (row) { const u64 e = b0 + (u64)j; atomicOr(&mask[e >> 5], 1u << (e & 31)); }
                }
            }
            j++;
        }
        __syncthreads();        // the next tile restages the slices
    }
    n_groups = block_sum_u64(n_groups, scratch);
    n_missing = block_sum_u64(n_missing, scratch);
    n_mixed = block_sum_u64(n_mixed, scratch);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u64 t = __shfl_xor(first_missing, o, 64); first_missing = t < first_missing ? t : first_missing; }
    if ((tid & 63) == 0 && first_missing != ~0ull) atomicMin((unsigned long long*)&tallies[3], (unsigned long long)first_missing);
    if (tid == 0) {
        if (n_groups) atomicAdd((unsigned long long*)&tallies[0], (unsigned long long)n_groups);
        if (n_missing) atomicAdd((unsigned long long*)&tallies[1], (unsigned long long)n_missing);
        if (n_mixed) atomicAdd((unsigned long long*)&tallies[2], (unsigned long long)n_mixed);
    }
}

// item e = sample entry e; kept = the mask says it starts a row (compact.hpp)
struct VarsRows {
    VarsLists L; const u32* mask; u64* ctx; u64* rows;
    __device__ bool flag(u64 e) const { return (mask[e >> 5] >> (e & 31)) & 1u; }
    __device__ void store(u64 pos, u64 e) const {
        const u64 c = L.sk[e] >> 2;
        u64* const row = rows + 8 * pos;
        for (int t = 0; t < 8; t++) row[t] = 0;
        ctx[pos] = c;
        for (u64 q = e; q < L.n_sam && q < e + 4 && (L.sk[q] >> 2) == c; q++) row[L.sk[q] & 3] = vs_count(L.sc, L.sbits, q);
        const u64 lo = partition_point(0ull, L.n_ref, [&](u64 i) { return (L.rk[i] >> 2) < c; });          // the first reference entry of the context
        for (u64 q = lo; q < L.n_ref && q < lo + 4 && (L.rk[q] >> 2) == c; q++) row[4 + (L.rk[q] & 3)] = vs_count(L.rc, L.rbits, q);
    }
};

static int vars_scan(zk_ctx* c, const VarsLists& L, double threshold, u64* d_ctx, u64* d_rows, uint64_t cap_rows, zk_vars_stats* st) {
    if (L.n_sam == 0) return ZK_OK;
    const uint64_t tiles64 = div_up(L.n_ref + L.n_sam, VS_TILE);
    if (tiles64 >= (1ull << 32) - 1) return fail(c, ZK_ERANGE, "vars scan: %llu entries in the two lists (fewer than 2^44)",
                                                 (unsigned long long)(L.n_ref + L.n_sam));
    // the mask (a bit per sample entry), the cuts, the tile counts of the compaction and their scan
    const uint64_t need = L.n_sam / 8 + 8 * tiles64 + 16 * div_up(L.n_sam, CP_TILE) + (1 << 20);
    ZK_TRY(arena_require(c, need, need));
    u32* mask;
    const uint64_t mask_bytes = 4 * (L.n_sam / 32 + 1);
    ZK_TRY(arena_alloc(c, mask_bytes, (void**)&mask));
    ZK_HIP(c, hipMemsetAsync(mask, 0, mask_bytes, c->stream));
    u64* tallies = c->d_scalars->vars;
    ZK_HIP(c, hipMemsetAsync(tallies, 0, 3 * sizeof(u64), c->stream));
    ZK_HIP(c, hipMemsetAsync(tallies + 3, 0xff, sizeof(u64), c->stream));
    u64* part; u32 tiles;
    const u64* A = L.n_ref ? L.rk : L.sk;          // (an empty list is never read)
    ZK_TRY(make_partition(c, A, L.n_ref, L.sk, L.n_sam, &part, &tiles));
    prof_begin(c, ZK_PROF_VARS_SCAN, (8 + L.rbits / 8) * L.n_ref + (8 + L.sbits / 8) * L.n_sam);
    hipLaunchKernelGGL(vars_join_kernel, dim3(grid_cap(c, tiles, 2)), dim3(VS_BLOCK), 0, c->stream, L, part, tiles, threshold, mask, tallies,
                       c->d_err);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(fetch(c, &c->h_scalars->vars));
    u64* cnt;
    uint64_t n_rows = 0;
    VarsRows vr{L, mask, d_ctx, d_rows};
    ZK_TRY(compact_count(c, vr, L.n_sam, &cnt, &n_rows));          // synchronises; reports a group sum that wrapped
    const u64* h = c->h_scalars->vars;
    st->n_groups = h[0];
    st->n_missing = h[1];
    st->n_mixed = h[2];
    st->first_missing = h[1] ? h[3] : 0;
    st->n_rows = n_rows;
    if (n_rows > cap_rows) return no_room(c, "vars scan", "rows", n_rows, cap_rows);
    ZK_TRY(compact_write(c, vr, L.n_sam, cnt));
    return check_device_error(c);
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_vars_scan(zk_ctx* c, const uint64_t* d_ref_keys, const void* d_ref_counts, int ref_count_bits, uint64_t n_ref,
                 const uint64_t* d_sam_keys, const void* d_sam_counts, int sam_count_bits, uint64_t n_sam, int K, double threshold,
                 uint64_t* d_ctx, uint64_t* d_row_counts, uint64_t cap_rows, zk_vars_stats* stats) {
    ZK_ARGS(c, stats && K >= 1 && K <= 32 && std::isfinite(threshold) && (ref_count_bits == 32 || ref_count_bits == 64) &&
                   (sam_count_bits == 32 || sam_count_bits == 64) && (n_ref == 0 || (d_ref_keys && d_ref_counts)) &&
                   (n_sam == 0 || (d_sam_keys && d_sam_counts)) && (cap_rows == 0 || (d_ctx && d_row_counts)));
    *stats = zk_vars_stats{0, 0, 0, 0, 0};
    arena_reset(c);
    const VarsLists L{(const u64*)d_ref_keys, d_ref_counts, ref_count_bits, (u64)n_ref, (const u64*)d_sam_keys, d_sam_counts, sam_count_bits,
                      (u64)n_sam};
    return vars_scan(c, L, threshold, (u64*)d_ctx, (u64*)d_row_counts, cap_rows, stats);
}

}  // extern "C"
