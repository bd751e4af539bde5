// probe_scan.hip -- `zot spoligo` (zotmer/commands/spoligo.py:50-84): is a probe present in a k-mer set, up to two
// substituted bases?
//
// The reference answers per probe window (J bases, value v) by enumerating the substitution neighbours of v -- neigh(J, v, d)
// for d = 1, 2: exactly the values at Hamming distance d, 3J and 9 J (J - 1) / 2 of them -- and asking the sorted set, once
// per neighbour y, whether it holds an entry in [y << s, (y + 1) << s), s = 2 (K - J) (findApprox, spoligo.py:50-67).  That is
// the question "does the set hold an entry x with ham(x >> s, v) <= D", ham being basics.ham (basics.py:123-133): a base that
// differs in one bit or in both is one mismatch.  zk_probe_scan answers it for every window of a panel in ONE streaming pass
// over the set and returns, per window, how many entries lie at distance 0, 1 and 2.
//
//   * Workgroups stride over tiles of ZK_PROBE_TILE entries; a thread holds 16 entries of a tile, entry = round * 256 + thread
//     (the coalesced layout of project_sum_kernel).
//   * The windows are staged once per workgroup in LDS, as the value moved up to the window's place (v << s) and the mask of
//     the low bit of every base of the window: ham = popcount(((z | z >> 1) & mask)) on z = x ^ (v << s), with no shift that
//     depends on the window (and none by 64: s <= 62).  The loop over the windows is uniform across the wave.
//   * Matches are rare: one ballot of (d <= 2) per wave, window and round; only a non-zero ballot resolves the three classes
//     and adds their popcounts to the workgroup's u32 tally in LDS.  At its end a workgroup adds every non-zero tally to the
//     zeroed device tallies with one 64-bit integer atomic: integer adds commute, a repeated call returns the same bits.
//
// Algorithmic bytes: 8 read per entry and call, whatever the number of windows.
#include <vector>

#include "internal.hpp"

namespace zk {

constexpr int PB_BLOCK = 256, PB_ROUNDS = 16, PB_TILE = PB_BLOCK * PB_ROUNDS;
static_assert(PB_TILE == ZK_PROBE_TILE, "the tile include/zotk.h publishes");
constexpr u64 PB_LOW_BITS = 0x5555555555555555ull;          // bits.m1: the low bit of every base

// FULL: every entry of the tile exists (all tiles but the last one)
template <bool FULL>
__device__ __forceinline__ void probe_tile(const u64* __restrict__ k, u64 base, u64 n, u32 W, const u64* s_value, const u64* s_mask,
                                           u32* s_tally) {
    const int tid = threadIdx.x, lane = tid & 63;
    u64 x[PB_ROUNDS];
    u32 valid = 0;
#pragma unroll
    for (int r = 0; r < PB_ROUNDS; r++) {
        const u64 i = base + (u64)r * PB_BLOCK + tid;
        const bool in = FULL || i < n;
        x[r] = in ? k[i] : 0;
        valid |= in ? 1u << r : 0u;
    }
    for (u32 w = 0; w < W; w++) {
        const u64 v = s_value[w], m = s_mask[w];
#pragma unroll
        for (int r = 0; r < PB_ROUNDS; r++) {
            const u64 z = x[r] ^ v;
            const u64 y = (z | (z >> 1)) & m;
            const u32 d = (u32)__builtin_popcount((u32)y) + (u32)__builtin_popcount((u32)(y >> 32));
            const bool near = d <= 2 && (FULL || ((valid >> r) & 1u));
            if (__ballot(near) == 0) continue;
            const u64 b0 = __ballot(near && d == 0), b1 = __ballot(near && d == 1), b2 = __ballot(near && d == 2);
            if (lane == 0) {
                if (b0) atomicAdd(&s_tally[3 * w + 0], (u32)__popcll(b0));
                if (b1) atomicAdd(&s_tally[3 * w + 1], (u32)__popcll(b1));
                if (b2) atomicAdd(&s_tally[3 * w + 2], (u32)__popcll(b2));
            }
        }
    }
}

// params: [W] values moved up, then [W] masks.  Dynamic LDS: the two, then the [W][3] u32 tally -- 28 bytes per window.
__global__ __launch_bounds__(PB_BLOCK) void probe_scan_kernel(const u64* __restrict__ k, u64 n, u64 tiles, const u64* __restrict__ params,
                                                              u32 W, u64* __restrict__ tallies) {
    extern __shared__ __attribute__((aligned(16))) u64 pb_lds[];
    u64* s_value = pb_lds;
    u64* s_mask = pb_lds + W;
    u32* s_tally = (u32*)(pb_lds + 2 * (u64)W);
    for (u32 s = threadIdx.x; s < 2 * W; s += PB_BLOCK) pb_lds[s] = params[s];
    for (u32 s = threadIdx.x; s < 3 * W; s += PB_BLOCK) s_tally[s] = 0;
    __syncthreads();
    for (u64 t = blockIdx.x; t < tiles; t += gridDim.x) {
        const u64 base = t * PB_TILE;
        if (base + PB_TILE <= n) probe_tile<true>(k, base, n, W, s_value, s_mask, s_tally);
        else probe_tile<false>(k, base, n, W, s_value, s_mask, s_tally);
    }
    __syncthreads();
    for (u32 s = threadIdx.x; s < 3 * W; s += PB_BLOCK) {
        const u32 v = s_tally[s];
        if (v) atomicAdd((unsigned long long*)&tallies[s], (unsigned long long)v);
    }
}

static int probe_scan(zk_ctx* c, const u64* keys, uint64_t n, int K, const zk_probe_window* win, uint32_t W, uint64_t* tallies) {
    for (uint32_t s = 0; s < 3 * W; s++) tallies[s] = 0;
    if (n == 0 || W == 0) return ZK_OK;
    std::vector<u64> params(2 * (size_t)W);
    for (uint32_t w = 0; w < W; w++) {
        const int shift = 2 * (K - win[w].J);                         // 0 .. 62
        params[w] = (u64)win[w].value << shift;
        params[W + w] = PB_LOW_BITS & ~((1ull << shift) - 1);          // bits above 2K are zero in every entry and every value
    }
    const u64 tiles = div_up(n, PB_TILE);
    const u64 grid = grid_cap(c, tiles, 8);
    // the LDS tally is 32 bits wide: a workgroup must see fewer than 2^32 entries in one launch
    if (div_up(tiles, grid) * PB_TILE >= 1ull << 32)
        return fail(c, ZK_EINVAL, "zk_probe_scan: %llu entries are more than one launch can tally", (unsigned long long)n);
    u64 *d_params, *d_tallies;
    ZK_TRY(arena_alloc(c, 16ull * W, (void**)&d_params));
    ZK_TRY(arena_alloc(c, 24ull * W, (void**)&d_tallies));
    ZK_HIP(c, hipMemcpyAsync(d_params, params.data(), 16ull * W, hipMemcpyHostToDevice, c->stream));
    ZK_HIP(c, hipMemsetAsync(d_tallies, 0, 24ull * W, c->stream));
    prof_begin(c, ZK_PROF_PROBE_SCAN, 8 * n);
    hipLaunchKernelGGL(probe_scan_kernel, dim3((u32)grid), dim3(PB_BLOCK), 28u * W, c->stream, keys, (u64)n, tiles, d_params, (u32)W,
                       d_tallies);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    ZK_HIP(c, hipMemcpyAsync(tallies, d_tallies, 24ull * W, hipMemcpyDeviceToHost, c->stream));
    ZK_HIP(c, hipStreamSynchronize(c->stream));          // (params is read until here)
    return check_device_error(c);
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_probe_scan(zk_ctx* c, const uint64_t* d_kmers, uint64_t n, int K, const zk_probe_window* windows, uint32_t n_windows,
                  uint64_t* tallies) {
    if (!c) return ZK_EINVAL;
    zk::enter(c);
    if ((n != 0 && !d_kmers) || (n_windows != 0 && (!windows || !tallies)))
        return fail(c, ZK_EINVAL, "zk_probe_scan: a null array");
    if (K < 1 || K > 32) return fail(c, ZK_EINVAL, "zk_probe_scan: K = %d, 1 <= K <= 32", K);
    if (n_windows > ZK_PROBE_MAX_WINDOWS)
        return fail(c, ZK_EINVAL, "zk_probe_scan: %u windows, at most %d a call", n_windows, ZK_PROBE_MAX_WINDOWS);
    for (uint32_t w = 0; w < n_windows; w++) {
        const int J = windows[w].J;
        if (J < 1 || J > K) return fail(c, ZK_EINVAL, "zk_probe_scan: window %u has J = %d, 1 <= J <= K = %d", w, J, K);
        if (J < 32 && (windows[w].value >> (2 * J)) != 0)
            return fail(c, ZK_EINVAL, "zk_probe_scan: window %u has bits above its %d bases", w, J);
    }
    arena_reset(c);
    return probe_scan(c, (const u64*)d_kmers, n, K, windows, n_windows, tallies);
}

}  // extern "C"
