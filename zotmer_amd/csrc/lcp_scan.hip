// lcp_scan.hip -- `zot scan` (zotmer/commands/scan.py): for every k-mer of a gene index the sample k-mer with the longest
// common prefix, as the reference's resolveAll leaves it (scan.py:95-120), and the placement of those k-mers on the positions
// of the genes (scan.py:281-304).
//
// resolveAll is two sequential loops.  Pass 1 compares S[i] with the first x >= S[i] of the sample X (the last x where there
// is none) and keeps (lcp, x) where the lcp is above 0; pass 2 offers every entry the Y of the entry before it, as already
// updated.  So after pass 2 entry i holds either its own pass-1 value (a "start") or the value carried from the last start
// before it, and a carried value v = Y1[j] survives at i iff lcp(v, S[i]) > L1[i].  With nb(j) = the first i > j where Y1[j]
// does not survive, the starts are the orbit of 0 under nb (DESIGN.md section 6m has the argument).
//   * lcp_pass1_kernel: one thread per S[i], a lower bound in X.  The workgroup also keeps the largest L1 of its ZK_LCP_TILE
//     entries; lcp_max_kernel folds 256 of those into one.
//   * lcp_next_kernel: nb(j).  A value that survives at j + 1 is below S[j + 1], so its lcp with S[i] does not grow with i: a
//     whole tile (256 tiles) whose largest L1 is below the lcp with its LAST entry cannot stop it and is stepped over.  A tile
//     that is walked without a stop is one over which the lcp fell, which happens at most K times: no walk is longer than
//     512 (K + 2) + nS / 65536 steps, whatever the input.
//   * lcp_jump_kernel: pointer doubling.  Round r marks nb^(2^r)(j) for every marked j and squares the jump; nb(j) > j, so
//     ceil(log2 nS) rounds mark the whole orbit.  Marks are bytes set by plain stores of 1.
//   * lcp_last_kernel / lcp_max_kernel / lcp_prev_kernel: the last start in every tile, in every 256 tiles, before every tile.
//   * lcp_fill_kernel: an entry that is no start takes the Y1 of the last start before it -- by ballot within its wave, the
//     waves' last starts within the tile, lcp_prev_kernel's word before it -- and the lcp of that value with its own S.  Starts
//     are not written again, so L and Y hold pass 1's values in place until they are replaced.
// No atomics, no wait on another workgroup, all integer work.
//
// The placement: scan_check_kernel proves the arrays (nothing is written before it has passed); scan_best_kernel finds the
// S index of every entry in T, counts it under (record, L) and offers (L << 32 | ~entry) to its slot with a 64-bit max -- the
// largest L wins, among equals the first entry; scan_gather_kernel turns a slot's winner into (P, Q).
#include <algorithm>

#include "internal.hpp"
#include "search.hpp"

namespace zk {

constexpr int LCP_BLOCK = 256;          // lcp_next_kernel shifts by 8
static_assert(LCP_BLOCK == ZK_LCP_TILE, "the tile include/zotk.h publishes");
constexpr int LCP_NW = LCP_BLOCK / 64;
constexpr int LCP_SUPER_SHIFT = 16;          // 256 tiles of 256 entries

// basics.lcp (zotmer/library/basics.py:160-170)
__device__ __forceinline__ u32 lcp_of(int K, u64 x, u64 y) {
    const u64 z = x ^ y;
    return z ? (u32)(K - 1 - ((63 - __clzll((long long)z)) >> 1)) : (u32)K;
}

__global__ __launch_bounds__(LCP_BLOCK) void lcp_pass1_kernel(const u64* __restrict__ S, u32 nS, const u64* __restrict__ X, u64 nX, int K,
                                                              u8* __restrict__ L, u64* __restrict__ Y, u32* __restrict__ tmax) {
    __shared__ u32 s_w[LCP_NW];
    const u64 i = (u64)blockIdx.x * LCP_BLOCK + threadIdx.x;
    u32 l = 0;
    if (i < nS) {
        const u64 s = S[i];
        const u64 lo = lower_bound(X, 0ull, nX, s);
        u64 x = X[lo < nX ? lo : nX - 1];
        l = lcp_of(K, x, s);
        if (l == 0) x = 0;          // scan.py:102-104: L and Y are touched only where the lcp is above 0
        L[i] = (u8)l;
        Y[i] = x;
    }
    const u32 m = block_max_u32<LCP_NW>(l, s_w);
    if (threadIdx.x == 0) tmax[blockIdx.x] = m;
}

// out[g] = the largest of in[256 g .. 256 g + 255]
__global__ __launch_bounds__(LCP_BLOCK) void lcp_max_kernel(const u32* __restrict__ in, u32 n, u32* __restrict__ out) {
    __shared__ u32 s_w[LCP_NW];
    const u64 i = (u64)blockIdx.x * LCP_BLOCK + threadIdx.x;
    const u32 m = block_max_u32<LCP_NW>(i < n ? in[i] : 0u, s_w);
    if (threadIdx.x == 0) out[blockIdx.x] = m;
}

__global__ __launch_bounds__(LCP_BLOCK) void lcp_next_kernel(const u64* __restrict__ S, u32 nS, int K, const u8* __restrict__ L,
                                                             const u64* __restrict__ Y, const u32* __restrict__ tmax,
                                                             const u32* __restrict__ smax, u32* __restrict__ nb) {
    const u64 j = (u64)blockIdx.x * LCP_BLOCK + threadIdx.x;
    if (j >= nS) return;
    const u64 v = Y[j], n = nS;
    u64 i = j + 1;
    while (i < n) {
        // entry by entry to the end of the tile; the first of these is j + 1 itself, and what survives there is below S[j + 1]
        u64 end = ((i >> 8) + 1) << 8;
        if (end > n) end = n;
        bool stop = false;
        for (; i < end; i++)
            if (lcp_of(K, v, S[i]) <= (u32)L[i]) { stop = true; break; }
        if (stop) break;
        // i is the first entry of a tile: whole tiles, and from the first of 256 tiles on whole groups of them
        while (i < n) {
            if ((i & ((1ull << LCP_SUPER_SHIFT) - 1)) == 0) {
                u64 se = i + (1ull << LCP_SUPER_SHIFT);
                if (se > n) se = n;
                if (smax[i >> LCP_SUPER_SHIFT] < lcp_of(K, v, S[se - 1])) { i = se; continue; }
            }
            u64 te = i + LCP_BLOCK;
            if (te > n) te = n;
            if (tmax[i >> 8] < lcp_of(K, v, S[te - 1])) { i = te; continue; }
            break;
        }
    }
    nb[j] = (u32)i;
}

__global__ __launch_bounds__(LCP_BLOCK) void lcp_jump_kernel(const u32* __restrict__ jin, u32* __restrict__ jout, u8* mark, u32 nS) {
    const u64 i = (u64)blockIdx.x * LCP_BLOCK + threadIdx.x;
    if (i >= nS) return;
    const u32 a = jin[i];
    // a mark that another thread of this launch has just set may or may not be seen: what it leads to is in the orbit either way
    if (a < nS && mark[i]) mark[a] = 1;
    jout[i] = a < nS ? jin[a] : nS;
}

// last[t] = 1 + the last marked index of tile t, 0 if it has none
__global__ __launch_bounds__(LCP_BLOCK) void lcp_last_kernel(const u8* __restrict__ mark, u32 nS, u32* __restrict__ last) {
    __shared__ u32 s_w[LCP_NW];
    const u64 i = (u64)blockIdx.x * LCP_BLOCK + threadIdx.x;
    const u32 m = block_max_u32<LCP_NW>(i < nS && mark[i] ? (u32)i + 1u : 0u, s_w);
    if (threadIdx.x == 0) last[blockIdx.x] = m;
}

// prev[t] = 1 + the last marked index before tile t (0 only for tile 0: index 0 is always marked)
__global__ __launch_bounds__(LCP_BLOCK) void lcp_prev_kernel(const u32* __restrict__ last, const u32* __restrict__ slast, u32 tiles,
                                                             u32* __restrict__ prev) {
    const u64 t = (u64)blockIdx.x * LCP_BLOCK + threadIdx.x;
    if (t >= tiles) return;
    u32 r = 0;
    const u64 first = (t >> 8) << 8;
    for (u64 u = t; u > first && r == 0; u--) r = last[u - 1];
    for (u64 s = t >> 8; s > 0 && r == 0; s--) r = slast[s - 1];
    prev[t] = r;
}

__global__ __launch_bounds__(LCP_BLOCK) void lcp_fill_kernel(const u64* __restrict__ S, u32 nS, int K, const u8* __restrict__ mark,
                                                             const u32* __restrict__ prev, u8* L, u64* Y) {
    __shared__ u32 s_w[LCP_NW];
    const u64 i = (u64)blockIdx.x * LCP_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool in = i < nS;
    const bool m = in && mark[i];
    const u64 bal = __ballot(m);
    const u64 wave0 = (u64)blockIdx.x * LCP_BLOCK + (u64)wave * 64;
    if (lane == 0) s_w[wave] = bal ? (u32)(wave0 + (u64)(63 - __clzll((long long)bal))) + 1u : 0u;
    __syncthreads();
    if (!in || m) return;
    const u64 below = bal & ((2ull << lane) - 1);          // lane 63: 2 << 63 wraps to 0, the mask is all ones
    u32 s1 = below ? (u32)(wave0 + (u64)(63 - __clzll((long long)below))) + 1u : 0u;
    for (int w = wave; w > 0 && s1 == 0; w--) s1 = s_w[w - 1];
    if (s1 == 0) s1 = prev[blockIdx.x];
    if (s1 == 0) return;          // cannot happen: index 0 is marked
    const u64 v = Y[s1 - 1];          // a start: nobody writes it
    Y[i] = v;
    L[i] = (u8)lcp_of(K, v, S[i]);
}

static int lcp_resolve(zk_ctx* c, const u64* S, uint64_t nS, const u64* X, uint64_t nX, int K, u8* L, u64* Y) {
    const u32 n = (u32)nS;
    const u32 tiles = (u32)div_up(nS, LCP_BLOCK), supers = (u32)div_up(tiles, 256);
    const uint64_t need = 9 * nS + 16 * (uint64_t)tiles + 8 * (uint64_t)supers + (1 << 20);
    ZK_TRY(arena_require(c, need, need));
    u32 *ja, *jb, *tmax, *smax, *last, *slast, *prev;
    u8* mark;
    ZK_TRY(arena_alloc(c, 4 * nS, (void**)&ja));
    ZK_TRY(arena_alloc(c, 4 * nS, (void**)&jb));
    ZK_TRY(arena_alloc(c, nS, (void**)&mark));
    ZK_TRY(arena_alloc(c, 4 * (uint64_t)tiles, (void**)&tmax));
    ZK_TRY(arena_alloc(c, 4 * (uint64_t)supers, (void**)&smax));
    ZK_TRY(arena_alloc(c, 4 * (uint64_t)tiles, (void**)&last));
    ZK_TRY(arena_alloc(c, 4 * (uint64_t)supers, (void**)&slast));
    ZK_TRY(arena_alloc(c, 4 * (uint64_t)tiles, (void**)&prev));
    ZK_HIP(c, hipMemsetAsync(mark, 0, nS, c->stream));
    ZK_HIP(c, hipMemsetAsync(mark, 1, 1, c->stream));
    int rounds = 0;
    while ((1ull << rounds) < nS) rounds++;
    prof_begin(c, ZK_PROF_LCP_RESOLVE, (48 + 12 * (uint64_t)rounds) * nS);          // the searches in X are not in it
    hipLaunchKernelGGL(lcp_pass1_kernel, dim3(tiles), dim3(LCP_BLOCK), 0, c->stream, S, n, X, (u64)nX, K, L, Y, tmax);
    hipLaunchKernelGGL(lcp_max_kernel, dim3(supers), dim3(LCP_BLOCK), 0, c->stream, (const u32*)tmax, tiles, smax);
    hipLaunchKernelGGL(lcp_next_kernel, dim3(tiles), dim3(LCP_BLOCK), 0, c->stream, S, n, K, (const u8*)L, (const u64*)Y, (const u32*)tmax,
                       (const u32*)smax, ja);
    for (int r = 0; r < rounds; r++) {
        hipLaunchKernelGGL(lcp_jump_kernel, dim3(tiles), dim3(LCP_BLOCK), 0, c->stream, (const u32*)ja, jb, mark, n);
        u32* t = ja; ja = jb; jb = t;
    }
    hipLaunchKernelGGL(lcp_last_kernel, dim3(tiles), dim3(LCP_BLOCK), 0, c->stream, (const u8*)mark, n, last);
    hipLaunchKernelGGL(lcp_max_kernel, dim3(supers), dim3(LCP_BLOCK), 0, c->stream, (const u32*)last, tiles, slast);
    hipLaunchKernelGGL(lcp_prev_kernel, dim3((u32)div_up(tiles, LCP_BLOCK)), dim3(LCP_BLOCK), 0, c->stream, (const u32*)last, (const u32*)slast,
                       tiles, prev);
    hipLaunchKernelGGL(lcp_fill_kernel, dim3(tiles), dim3(LCP_BLOCK), 0, c->stream, S, n, K, (const u8*)mark, (const u32*)prev, L, Y);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    return check_device_error(c);
}

// ---------------------------------------------------------------------------------------
// zk_scan_place
// ---------------------------------------------------------------------------------------
struct PlaceArgs {
    const u8* L; const u64* Y; u32 nS;
    const u32* T; const u32* U; const int* V; u32 n_entries;
    const u64* rec_off; u32 n_rec; int K;
};

// the S index of entry j: the last i with T[i] <= j (T ascends from 0 to n_entries > j, so 0 <= i < nS)
__device__ __forceinline__ u32 place_owner(const u32* __restrict__ T, u32 nS, u32 j) {
    return upper_bound(T, 0u, nS + 1, j) - 1;
}
// the slot within its record that position p names (scan.py:297-300): p - 1, on the reverse strand -(p + 1)
__device__ __forceinline__ u64 place_q(int p) { const long long q = p; return (u64)(q > 0 ? q : -q) - 1; }

// most = 1 + the longest of the arrays
__global__ __launch_bounds__(LCP_BLOCK) void scan_check_kernel(PlaceArgs a, u64 most, u64* __restrict__ bad) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < most; i += (u64)gridDim.x * blockDim.x) {
        if (i < a.nS && (a.T[i] > a.T[i + 1] || (int)a.L[i] > a.K)) *bad = 1;
        if (i == 0 && (a.T[0] != 0 || a.T[a.nS] != a.n_entries || a.rec_off[0] != 0)) *bad = 1;
        if (i < a.n_rec && a.rec_off[i] > a.rec_off[i + 1]) *bad = 1;
        if (i < a.n_entries) {
            const u32 r = a.U[i];
            const int p = a.V[i];
            if (r >= a.n_rec || p == 0) *bad = 1;
            else if (place_q(p) >= a.rec_off[r + 1] - a.rec_off[r]) *bad = 1;
        }
    }
}

__global__ __launch_bounds__(LCP_BLOCK) void scan_best_kernel(PlaceArgs a, u64* __restrict__ best, u32* __restrict__ cnt) {
    const u64 j = (u64)blockIdx.x * LCP_BLOCK + threadIdx.x;
    if (j >= a.n_entries) return;
    const u32 i = place_owner(a.T, a.nS, (u32)j);
    const u32 l = a.L[i], r = a.U[j];
    atomicAdd(&cnt[(u64)r * (u64)(a.K + 1) + l], 1u);
    if (l == 0) return;          // scan.py:302: never above the 0 a slot starts with
    const u64 slot = a.rec_off[r] + place_q(a.V[j]);
    atomicMax((unsigned long long*)&best[slot], ((unsigned long long)l << 32) | (unsigned long long)(0xFFFFFFFFu - (u32)j));
}

__global__ __launch_bounds__(LCP_BLOCK) void scan_gather_kernel(PlaceArgs a, const u64* __restrict__ best, u64 n_slots, u64* __restrict__ P,
                                                                u8* __restrict__ Q) {
    for (u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x; s < n_slots; s += (u64)gridDim.x * blockDim.x) {
        const u64 b = best[s];
        u64 y = 0;
        if (b) {
            const u32 j = 0xFFFFFFFFu - (u32)b;
            y = a.Y[place_owner(a.T, a.nS, j)];
            if (a.V[j] < 0) y = revcomp(a.K, y);
        }
        P[s] = y;
        Q[s] = (u8)(b >> 32);
    }
}

static int scan_place(zk_ctx* c, const PlaceArgs& a, u64* P, u8* Q, u32* cnt) {
    u64* bad = &c->d_scalars->place_bad;
    ZK_HIP(c, hipMemsetAsync(bad, 0, sizeof(u64), c->stream));
    const uint64_t most = std::max<uint64_t>(std::max<uint64_t>(a.n_entries, a.nS), a.n_rec) + 1;
    hipLaunchKernelGGL(scan_check_kernel, dim3(grid_cap(c, div_up(most, LCP_BLOCK), 16)), dim3(LCP_BLOCK), 0, c->stream, a, (u64)most, bad);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(fetch(c, &c->h_scalars->place_bad));
    ZK_TRY(fetch(c, &c->h_scalars->place_slots, a.rec_off + a.n_rec));
    ZK_TRY(check_device_error(c));
    if (c->h_scalars->place_bad)
        return fail(c, ZK_EINVAL, "zk_scan_place: T does not ascend from 0 to n_entries, the record offsets do not ascend from 0, an L is above K, "
                                  "or an entry names a record >= %u, position 0 or a position outside its record", a.n_rec);
    const uint64_t n_slots = c->h_scalars->place_slots;
    const uint64_t cnt_bytes = 4ull * a.n_rec * (uint64_t)(a.K + 1);
    if (cnt_bytes) ZK_HIP(c, hipMemsetAsync(cnt, 0, cnt_bytes, c->stream));
    if (n_slots == 0) return stream_sync(c);
    if (!P || !Q) return fail(c, ZK_EINVAL, "zk_scan_place: %llu slots and no P or Q", (unsigned long long)n_slots);
    const uint64_t need = 8 * n_slots + (1 << 20);
    ZK_TRY(arena_require(c, need, need));
    u64* best;
    ZK_TRY(arena_alloc(c, 8 * n_slots, (void**)&best));
    ZK_HIP(c, hipMemsetAsync(best, 0, 8 * n_slots, c->stream));
    prof_begin(c, ZK_PROF_SCAN_PLACE, 8ull * a.n_entries + 17 * n_slots);
    if (a.n_entries)
        hipLaunchKernelGGL(scan_best_kernel, dim3((u32)div_up(a.n_entries, LCP_BLOCK)), dim3(LCP_BLOCK), 0, c->stream, a, best, cnt);
    hipLaunchKernelGGL(scan_gather_kernel, dim3(grid_cap(c, div_up(n_slots, LCP_BLOCK), 16)), dim3(LCP_BLOCK), 0, c->stream, a, (const u64*)best,
                       (u64)n_slots, P, Q);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    return check_device_error(c);
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_lcp_resolve(zk_ctx* c, const uint64_t* d_S, uint64_t nS, const uint64_t* d_X, uint64_t nX, int K, uint8_t* d_L, uint64_t* d_Y) {
    ZK_ARGS(c, K >= 1 && K <= 32 && (nS == 0 || (d_S && d_L && d_Y)) && (nX == 0 || d_X));
    if (nS == 0) return ZK_OK;
    if (nS >= (1ull << 32)) return fail(c, ZK_ERANGE, "zk_lcp_resolve: %llu index k-mers (fewer than 2^32)", (unsigned long long)nS);
    if (nX == 0) return fail(c, ZK_EINVAL, "zk_lcp_resolve: the sample is empty");
    arena_reset(c);
    return lcp_resolve(c, (const u64*)d_S, nS, (const u64*)d_X, nX, K, (u8*)d_L, (u64*)d_Y);
}

int zk_scan_place(zk_ctx* c, const uint8_t* d_L, const uint64_t* d_Y, uint64_t nS, const uint32_t* d_T, const uint32_t* d_U, const int32_t* d_V,
                  uint64_t n_entries, const uint64_t* d_rec_off, uint64_t n_rec, int K, uint64_t* d_P, uint8_t* d_Q, uint32_t* d_cnt) {
    ZK_ARGS(c, K >= 1 && K <= 32 && d_T && d_rec_off && (nS == 0 || (d_L && d_Y)) && (n_entries == 0 || (d_U && d_V && d_P && d_Q)) &&
                   (n_rec == 0 || d_cnt));
    if (nS >= (1ull << 32) || n_entries >= (1ull << 32) || n_rec >= (1ull << 32))
        return fail(c, ZK_ERANGE, "zk_scan_place: %llu k-mers, %llu entries, %llu records (each fewer than 2^32)", (unsigned long long)nS,
                    (unsigned long long)n_entries, (unsigned long long)n_rec);
    arena_reset(c);
    const PlaceArgs a{(const u8*)d_L, (const u64*)d_Y, (u32)nS, (const u32*)d_T, (const u32*)d_U, (const int*)d_V, (u32)n_entries,
                      (const u64*)d_rec_off, (u32)n_rec, K};
    return scan_place(c, a, (u64*)d_P, (u8*)d_Q, (u32*)d_cnt);
}

}  // extern "C"
