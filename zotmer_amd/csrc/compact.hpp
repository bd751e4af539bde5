// compact.hpp -- the order-preserving compaction and the predicates that more than one command feeds it.
// Users: capture.hip, contig_spectra.hip, pileup.hip, strand_bias.hip, vars_scan.hip.
#pragma once
#include "internal.hpp"

namespace zk {

// ---------------------------------------------------------------------------------------
// shared predicates (flag / store: below)
// ---------------------------------------------------------------------------------------
struct NewlinePos {      // positions of the '\n' bytes
    const u8* text; u64* out;
    __device__ bool flag(u64 i) const { return text[i] == '\n'; }
    __device__ void store(u64 pos, u64 i) const { out[pos] = i; }
};

// Run heads of a sorted array: item i is kept when it is the first of a run of equal keys, or of equal (key, value) in a
// key-sorted, value-stable array.  What a head stores is its user's: derive, and add store.
struct KeyRunHead {
    const u64* k;
    __device__ bool flag(u64 i) const { return i == 0 || k[i] != k[i - 1]; }
};
struct PairRunHead {
    const u64* k; const u32* v;
    __device__ bool flag(u64 i) const { return i == 0 || k[i] != k[i - 1] || v[i] != v[i - 1]; }
};

// ---------------------------------------------------------------------------------------
// Order-preserving compaction: a count pass over tiles of 4096 items, an inclusive scan of the tile counts
// (scan64_inclusive), a write pass.  Every workgroup owns one tile; nothing waits on another workgroup.
// P::flag(i) says whether item i is kept, P::store(pos, i) writes it at its rank.
// ---------------------------------------------------------------------------------------
constexpr int CP_BLOCK = 256, CP_ITEMS = 16, CP_TILE = CP_BLOCK * CP_ITEMS;

template <class P>
__global__ __launch_bounds__(CP_BLOCK) void compact_count_kernel(P p, u64 n, u64* __restrict__ tile_counts) {
    __shared__ u32 part[CP_BLOCK / 64];
    const u64 base = (u64)blockIdx.x * CP_TILE + (u64)threadIdx.x * CP_ITEMS;
    u32 k = 0;
    for (int i = 0; i < CP_ITEMS; i++) k += (base + i < n && p.flag(base + i)) ? 1u : 0u;
    k = wave_sum_u32(k);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = k;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 t = 0;
        for (int w = 0; w < CP_BLOCK / 64; w++) t += part[w];
        tile_counts[blockIdx.x] = t;
    }
}

template <class P>
__global__ __launch_bounds__(CP_BLOCK) void compact_write_kernel(P p, u64 n, const u64* __restrict__ tile_incl) {
    __shared__ u32 part[CP_BLOCK / 64];
    const u64 base = (u64)blockIdx.x * CP_TILE + (u64)threadIdx.x * CP_ITEMS;
    u32 keep = 0;
    for (int i = 0; i < CP_ITEMS; i++)
        if (base + i < n && p.flag(base + i)) keep |= 1u << i;
    const u32 k = (u32)__popc(keep);
    const u32 incl = wave_incl_scan_u32(k);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) part[wave] = incl;
    __syncthreads();
    u64 pos = blockIdx.x ? tile_incl[blockIdx.x - 1] : 0;
    for (int w = 0; w < wave; w++) pos += part[w];
    pos += incl - k;
    for (int i = 0; i < CP_ITEMS; i++)
        if ((keep >> i) & 1u) p.store(pos++, base + i);
}

// the count pass: *total = kept items; tile_incl (arena, valid until the next arena_reset) feeds compact_write
template <class P>
static int compact_count(zk_ctx* c, const P& p, uint64_t n, u64** tile_incl, uint64_t* total) {
    *total = 0;
    *tile_incl = nullptr;
    if (n == 0) return ZK_OK;
    const u64 tiles = div_up(n, CP_TILE);
    u64* cnt;
    ZK_TRY(arena_alloc(c, 8 * tiles, (void**)&cnt));
    hipLaunchKernelGGL((compact_count_kernel<P>), dim3((u32)tiles), dim3(CP_BLOCK), 0, c->stream, p, (u64)n, cnt);
    ZK_HIP(c, hipGetLastError());
    *tile_incl = cnt;
    return scan_total(c, cnt, tiles, total);
}

template <class P>
static int compact_write(zk_ctx* c, const P& p, uint64_t n, const u64* tile_incl) {
    if (n == 0) return ZK_OK;
    hipLaunchKernelGGL((compact_write_kernel<P>), dim3((u32)div_up(n, CP_TILE)), dim3(CP_BLOCK), 0, c->stream, p, (u64)n, tile_incl);
    ZK_HIP(c, hipGetLastError());
    return ZK_OK;
}

}  // namespace zk
