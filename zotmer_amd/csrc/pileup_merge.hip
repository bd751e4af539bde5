// pileup_merge.hip -- the counted lists of zk_pileup_count made one on the device: zk_pileup_merge, and zk_narrow_counts for the
// entries that take the merged list with 32-bit counts.
//
// A list is three arrays (u32 coordinate or bait, u64 k-mer, count), strictly ascending by (coordinate, k-mer).  The merged
// order of two of them -- A before B on ties -- is cut on diagonals into tiles of PM_TILE merged inputs (pm_partition_kernel: one
// binary search per tile boundary over the 96-bit keys in global memory).  A tile then holds the slices A[a0, a1) and
// B[b0, b1), a1 - a0 + b1 - b0 = PM_TILE, and both passes over it are one kernel body (pm_tile_kernel):
//   * the slices go into LDS as two arrays, one element of halo on each side of each;
//   * a thread finds where its PM_ITEMS merged inputs start (a second merge-path search, in LDS) and walks them;
//   * every A element survives; its count takes the B element of the same key, which is the next merged input: B[j] of the walk,
//     the right halo B[b1] when the A element is the tile's last input;
//   * a B element survives unless the A element before it has its key: A[i - 1] of the walk, the left halo A[a0 - 1] for the
//     tile's first input.  So a pair of equal keys is written by the tile that holds its A element and by nobody else.
// The count pass reads the keys only and leaves the tile's survivors in counts[t]; one workgroup scans the counts
// (pm_scan_kernel: the tiles are few, 16 bytes of work space each); the emit pass reads the counts too, parks the survivors in
// LDS at their rank and writes them as one run from out[incl[t - 1]].  Nothing waits on another workgroup, nothing is added
// atomically.  Lists that are not ascending give partitions that need not ascend: a tile clamps its slices to what its
// diagonals allow, so that every index stays inside the arrays whatever the keys are.
#include "internal.hpp"

namespace zk {

constexpr int PM_BLOCK = 256, PM_ITEMS = 8, PM_TILE = PM_BLOCK * PM_ITEMS, PM_NW = PM_BLOCK / 64;
constexpr int PM_SLOTS = PM_TILE + 4;            // both slices and their four halo elements
static_assert(ZK_PILEUP_MERGE_TILE == PM_TILE, "ZK_PILEUP_MERGE_TILE is the tile of pm_tile_kernel");

struct PmLists { const u32* ac; const u64* ak; u64 na; const u32* bc; const u64* bk; u64 nb; };

// (c1, k1) <= (c2, k2): coordinate first, then k-mer, both unsigned
__device__ __forceinline__ bool pm_le(u32 c1, u64 k1, u32 c2, u64 k2) { return c1 < c2 || (c1 == c2 && k1 <= k2); }

// part[t] = the A elements among the first min(t * PM_TILE, na + nb) merged inputs, t = 0 .. tiles
__global__ __launch_bounds__(256) void pm_partition_kernel(PmLists l, u64 tiles, u64* __restrict__ part) {
    for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t <= tiles; t += (u64)gridDim.x * blockDim.x) {
        const u64 total = l.na + l.nb;
        const u64 d = t * PM_TILE < total ? t * PM_TILE : total;
        u64 lo = d > l.nb ? d - l.nb : 0, hi = d < l.na ? d : l.na;
        while (lo < hi) {                        // lo <= mid < na, 0 <= d - 1 - mid < nb
            const u64 mid = lo + (hi - lo) / 2, j = d - 1 - mid;
            if (pm_le(l.ac[mid], l.ak[mid], l.bc[j], l.bk[j])) lo = mid + 1; else hi = mid;
        }
        part[t] = lo;
    }
}

// MODE 0: the count pass (counts[t] = the tile's survivors); 1 and 2: the emit pass with B's counts 32 and 64 bits wide
template <int MODE>
__global__ __launch_bounds__(PM_BLOCK) void pm_tile_kernel(PmLists l, const u64* __restrict__ an, const void* __restrict__ bn, u64 tiles,
                                                           const u64* __restrict__ part, u64* __restrict__ counts, u32* __restrict__ oc,
                                                           u64* __restrict__ ok, u64* __restrict__ on) {
    constexpr bool EMIT = MODE != 0;
    __shared__ u32 sC[PM_SLOTS];
    __shared__ u64 sK[PM_SLOTS];
    __shared__ u64 sN[EMIT ? PM_SLOTS : 1];
    __shared__ u32 wtot[PM_NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (u64 t = blockIdx.x; t < tiles; t += gridDim.x) {
        const u64 total = l.na + l.nb;
        const u64 d0 = t * PM_TILE, d1 = d0 + PM_TILE < total ? d0 + PM_TILE : total;
        const u32 L = (u32)(d1 - d0);
        const u64 a0 = part[t];
        u64 a1 = part[t + 1];
        a1 = a1 < a0 ? a0 : (a1 > a0 + L ? a0 + L : a1);       // ascending lists never need it
        const u64 b0 = d0 - a0, b1 = d1 - a1;
        const u32 na_t = (u32)(a1 - a0), nb_t = L - na_t;
        const bool left_a = a0 > 0, right_b = b1 < l.nb;
        // LDS: A's slice at [1, na_t], its halo at 0 and na_t + 1; B's the same from slot bo on
        const u32 bo = na_t + 2;
        for (u32 x = tid; x < na_t + 2; x += PM_BLOCK) {
            const u64 g = a0 + x - 1;                           // x == 0 && a0 == 0 wraps: not below na
            const bool in = (x > 0 || left_a) && g < l.na;
            sC[x] = in ? l.ac[g] : 0u;
            sK[x] = in ? l.ak[g] : 0ull;
            if (EMIT) sN[x] = in ? an[g] : 0ull;
        }
        for (u32 x = tid; x < nb_t + 2; x += PM_BLOCK) {
            const u64 g = b0 + x - 1;
            const bool in = (x > 0 || b0 > 0) && g < l.nb;
            sC[bo + x] = in ? l.bc[g] : 0u;
            sK[bo + x] = in ? l.bk[g] : 0ull;
            if (EMIT) sN[bo + x] = !in ? 0ull : MODE == 2 ? ((const u64*)bn)[g] : (u64)((const u32*)bn)[g];
        }
        __syncthreads();
        // where this thread's inputs start: i A elements and j B elements of the tile lie before them
        const u32 p0 = (u32)tid * PM_ITEMS < L ? (u32)tid * PM_ITEMS : L;
        u32 lo = p0 > nb_t ? p0 - nb_t : 0, hi = p0 < na_t ? p0 : na_t;
        while (lo < hi) {
            const u32 mid = (lo + hi) / 2, j = p0 - 1 - mid;
            if (pm_le(sC[1 + mid], sK[1 + mid], sC[bo + 1 + j], sK[bo + 1 + j])) lo = mid + 1; else hi = mid;
        }
        u32 i = lo, j = p0 - lo, keep = 0;
        u32 rc[PM_ITEMS];
        u64 rk[PM_ITEMS], rn[PM_ITEMS];
#pragma unroll
        for (int s = 0; s < PM_ITEMS; s++) {
            rc[s] = 0; rk[s] = 0; rn[s] = 0;
            if (p0 + s < L) {
                // i <= na_t and j <= nb_t: the slots read are the slices' or their right halos
                const u32 ca = sC[1 + i], cb = sC[bo + 1 + j];
                const u64 ka = sK[1 + i], kb = sK[bo + 1 + j];
                const bool take_a = i < na_t && (j >= nb_t || pm_le(ca, ka, cb, kb));
                if (take_a) {
                    const bool twin = (j < nb_t || right_b) && ca == cb && ka == kb;
                    rc[s] = ca; rk[s] = ka;
                    if (EMIT) rn[s] = sN[1 + i] + (twin ? sN[bo + 1 + j] : 0ull);
                    keep |= 1u << s;
                    i++;
                } else {
                    const bool twin = (i > 0 || left_a) && sC[i] == cb && sK[i] == kb;       // slot i = A element i - 1
                    rc[s] = cb; rk[s] = kb;
                    if (EMIT) rn[s] = sN[bo + 1 + j];
                    if (!twin) keep |= 1u << s;
                    j++;
                }
            }
        }
        const u32 k = (u32)__popc(keep);
        const u32 incl = wave_incl_scan_u32(k);
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();                                        // ... and every thread has read its inputs from LDS
        u32 rank = incl - k, all = 0;
#pragma unroll
        for (int w = 0; w < PM_NW; w++) { if (w < wave) rank += wtot[w]; all += wtot[w]; }
        if (!EMIT) {
            if (tid == 0) counts[t] = all;
        } else {
#pragma unroll
            for (int s = 0; s < PM_ITEMS; s++)
                if ((keep >> s) & 1u) { sC[rank] = rc[s]; sK[rank] = rk[s]; sN[rank] = rn[s]; rank++; }      // all <= L slots
            __syncthreads();
            const u64 base = t ? counts[t - 1] : 0;            // counts: scanned, inclusive
            for (u32 x = tid; x < all; x += PM_BLOCK) { oc[base + x] = sC[x]; ok[base + x] = sK[x]; on[base + x] = sN[x]; }
        }
        __syncthreads();
    }
}

// v[0, n) -> its inclusive sums, in place, by one workgroup; *total = the last of them
__global__ __launch_bounds__(1024) void pm_scan_kernel(u64* __restrict__ v, u64 n, u64* __restrict__ total) {
    __shared__ u64 wsum[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 carry = 0;
    for (u64 base = 0; base < n; base += 1024) {
        const u64 i = base + threadIdx.x;
        const u64 x = i < n ? v[i] : 0ull;
        const u64 incl = wave_incl_scan_u64(x);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        u64 before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) { if (w < wave) before += wsum[w]; all += wsum[w]; }
        if (i < n) v[i] = carry + before + incl;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

static int pileup_merge(zk_ctx* c, const PmLists& l, const u64* an, const void* bn, int b_bits, u32* oc, u64* ok, u64* on, uint64_t cap,
                        uint64_t* n_out) {
    *n_out = 0;
    const uint64_t total = l.na + l.nb;
    if (total == 0) return ZK_OK;
    const uint64_t tiles = div_up(total, PM_TILE);
    u64 *part, *counts;
    ZK_TRY(arena_alloc(c, 8 * (tiles + 1), (void**)&part));
    ZK_TRY(arena_alloc(c, 8 * tiles, (void**)&counts));
    const u32 grid = (u32)(tiles < (1ull << 30) ? tiles : (1ull << 30));
    prof_begin(c, ZK_PROF_PILEUP_MERGE, 12 * total);
    hipLaunchKernelGGL(pm_partition_kernel, dim3(grid_cap(c, div_up(tiles + 1, 256), 16)), dim3(256), 0, c->stream, l, (u64)tiles, part);
    // MODE 0 compiles every use of an, bn, oc, ok and on away: the count pass reads keys and writes counts[], so a refusal below has written nothing
    hipLaunchKernelGGL((pm_tile_kernel<0>), dim3(grid), dim3(PM_BLOCK), 0, c->stream, l, an, bn, (u64)tiles, part, counts, oc, ok, on);
    hipLaunchKernelGGL(pm_scan_kernel, dim3(1), dim3(1024), 0, c->stream, counts, (u64)tiles, &c->d_scalars->merge_total);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(fetch(c, &c->h_scalars->merge_total));
    ZK_TRY(check_device_error(c));
    const uint64_t m = c->h_scalars->merge_total;
    *n_out = m;
    if (m > cap) return no_room(c, "zk_pileup_merge", "pairs in the union", m, cap);
    prof_add_bytes(c, ZK_PROF_PILEUP_MERGE, 20 * l.na + (b_bits == 64 ? 24 : 16) * l.nb + 20 * m);
    if (b_bits == 64)
        hipLaunchKernelGGL((pm_tile_kernel<2>), dim3(grid), dim3(PM_BLOCK), 0, c->stream, l, an, bn, (u64)tiles, part, counts, oc, ok, on);
    else
        hipLaunchKernelGGL((pm_tile_kernel<1>), dim3(grid), dim3(PM_BLOCK), 0, c->stream, l, an, bn, (u64)tiles, part, counts, oc, ok, on);
    prof_end(c);                                 // the record's end moves behind the emit pass
    ZK_HIP(c, hipGetLastError());
    return check_device_error(c);
}

// ---------------------------------------------------------------------------------------
// zk_narrow_counts
// ---------------------------------------------------------------------------------------
constexpr int NC_BLOCK = 256;

__global__ __launch_bounds__(NC_BLOCK) void narrow_kernel(const u64* __restrict__ in, u32* __restrict__ out, u64 n, u64* __restrict__ block_max) {
    __shared__ u64 wmax[NC_BLOCK / 64];
    u64 m = 0;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 v = in[i];
        out[i] = v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)v;
        m = v > m ? v : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u64 t = __shfl_xor(m, o, 64); m = t > m ? t : m; }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NC_BLOCK / 64; w++) m = wmax[w] > m ? wmax[w] : m;
        block_max[blockIdx.x] = m;
    }
}

// the largest of v[0, n), by one wave
__global__ __launch_bounds__(64) void narrow_max_kernel(const u64* __restrict__ v, u32 n, u64* __restrict__ out) {
    u64 m = 0;
    for (u32 i = threadIdx.x; i < n; i += 64) m = v[i] > m ? v[i] : m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u64 t = __shfl_xor(m, o, 64); m = t > m ? t : m; }
    if (threadIdx.x == 0) *out = m;
}

static int narrow_counts(zk_ctx* c, const u64* in, u32* out, uint64_t n, uint64_t* max_in) {
    *max_in = 0;
    if (n == 0) return ZK_OK;
    const u32 grid = grid_cap(c, div_up(n, NC_BLOCK), 8);
    u64* block_max;
    ZK_TRY(arena_alloc(c, 8 * (uint64_t)grid, (void**)&block_max));
    hipLaunchKernelGGL(narrow_kernel, dim3(grid), dim3(NC_BLOCK), 0, c->stream, in, out, (u64)n, block_max);
    hipLaunchKernelGGL(narrow_max_kernel, dim3(1), dim3(64), 0, c->stream, block_max, grid, &c->d_scalars->narrow_max);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(fetch(c, &c->h_scalars->narrow_max));
    ZK_TRY(check_device_error(c));
    *max_in = c->h_scalars->narrow_max;
    return ZK_OK;
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_pileup_merge(zk_ctx* c, const uint32_t* d_ac, const uint64_t* d_ak, const uint64_t* d_an, uint64_t na, const uint32_t* d_bc,
                    const uint64_t* d_bk, const void* d_bn, int b_count_bits, uint64_t nb, uint32_t* d_oc, uint64_t* d_ok, uint64_t* d_on,
                    uint64_t cap, uint64_t* n_out) {
    ZK_ARGS(c, n_out && na < (1ull << 62) && nb < (1ull << 62) && (na == 0 || (d_ac && d_ak && d_an)) && (nb == 0 || (d_bc && d_bk && d_bn)) &&
                   (cap == 0 || (d_oc && d_ok && d_on)));
    if (b_count_bits != 32 && b_count_bits != 64) return fail(c, ZK_EINVAL, "zk_pileup_merge: b_count_bits = %d, 32 or 64", b_count_bits);
    arena_reset(c);
    const PmLists l{d_ac, (const u64*)d_ak, na, d_bc, (const u64*)d_bk, nb};
    return pileup_merge(c, l, (const u64*)d_an, d_bn, b_count_bits, d_oc, (u64*)d_ok, (u64*)d_on, cap, n_out);
}

int zk_narrow_counts(zk_ctx* c, const uint64_t* d_in, uint32_t* d_out, uint64_t n, uint64_t* max_in) {
    ZK_ARGS(c, max_in && (n == 0 || (d_in && d_out)));
    arena_reset(c);
    return narrow_counts(c, (const u64*)d_in, d_out, n, max_in);
}

}  // extern "C"
