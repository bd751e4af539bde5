// search.hpp -- the binary search of the command kernels, and the bucket directory that shortens it over a sorted key list
// (bait_table.hpp's lookup and debruijn.hip's link searches start from it; every one-sided search of capture.hip,
// contig_spectra.hip, debruijn.hip, pileup.hip, lcp_scan.hip, hgvs_find.hip, vars_scan.hip, spikein.hip, allele_tally.hip,
// capi.hip and select.hip is partition_point, but spike_geo's, which measured slower with it).  The two-sided diagonal searches
// of the merge paths stay where they are.
#pragma once
#include "internal.hpp"

namespace zk {

// The first i of [lo, hi) for which pred(i) is false, hi if there is none; pred is true on a prefix of the range and false
// after it.  I is u32 or u64; the midpoint lo + (hi - lo) / 2 does not wrap, whatever lo + hi is.
template <class I, class P>
__device__ __forceinline__ I partition_point(I lo, I hi, P pred) {
    while (lo < hi) { const I mid = lo + ((hi - lo) >> 1); if (pred(mid)) lo = mid + 1; else hi = mid; }
    return lo;
}
// the first i of [lo, hi) with a[i] >= q (a ascending)
template <class T, class I, class Q>
__device__ __forceinline__ I lower_bound(const T* a, I lo, I hi, Q q) {
    return partition_point(lo, hi, [=](I i) { return a[i] < q; });
}
// the first i of [lo, hi) with a[i] > q
template <class T, class I, class Q>
__device__ __forceinline__ I upper_bound(const T* a, I lo, I hi, Q q) {
    return partition_point(lo, hi, [=](I i) { return a[i] <= q; });
}

// ---------------------------------------------------------------------------------------
// Key directory: the keys whose top bits x >> shift equal b are k[dir[b], dir[b + 1]), b = 0 .. nb - 1 (fewer than 2^32 keys)
// ---------------------------------------------------------------------------------------
struct KeyDir { const u32* dir; int shift; };

// the bucket of q (q >> shift < nb): two adjacent words of the directory
__device__ __forceinline__ void dir_bucket(const KeyDir& d, u64 q, u32& lo, u32& hi) {
    const u64 b = q >> d.shift;
    lo = d.dir[b]; hi = d.dir[b + 1];
}
// the number of keys < q
__device__ __forceinline__ u32 dir_lower(const u64* k, const KeyDir& d, u64 q) {
    u32 lo, hi;
    dir_bucket(d, q, lo, hi);
    return lower_bound(k, lo, hi, q);
}
// the number of keys <= q
__device__ __forceinline__ u32 dir_upper(const u64* k, const KeyDir& d, u64 q) {
    u32 lo, hi;
    dir_bucket(d, q, lo, hi);
    return upper_bound(k, lo, hi, q);
}

// dir[b] = the number of keys below b << shift, dir[nb] = n
template <class N>
__global__ __launch_bounds__(256) void key_dir_fill_kernel(const u64* __restrict__ k, N n, int shift, u64 nb, u32* __restrict__ dir) {
    for (u64 b = (u64)blockIdx.x * blockDim.x + threadIdx.x; b <= nb; b += (u64)gridDim.x * blockDim.x)
        dir[b] = b == nb ? (u32)n : (u32)lower_bound(k, (N)0, n, b << shift);
}
// N: the index type of the searches (u32 where the caller's n is below 2^32 by its own contract, u64 otherwise)
template <class N>
static int key_dir_build(zk_ctx* c, const u64* k, N n, int shift, u64 nb, u32* dir) {
    hipLaunchKernelGGL(key_dir_fill_kernel<N>, dim3(grid_cap(c, div_up(nb + 1, 256), 16)), dim3(256), 0, c->stream, k, n, shift, nb, dir);
    ZK_HIP(c, hipGetLastError());
    return ZK_OK;
}

}  // namespace zk
