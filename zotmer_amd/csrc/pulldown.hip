// pulldown.hip -- `zot pulldown` (zotmer/commands/pulldown.py): read pairs binned by the baits they touch, those with a k-mer of
// the -U sequences left out, and the histogram of the number of baits a pair hits (pulldown.py:77-99, 139-142).
//
// zk_pulldown_hits is zk_capture_hits (capture.hip: the window lookup, one wave per read, then the sort and the cut of the
// repeats) with two small passes behind it:
//   * the lookup also marks every vetoed read (capture_hits_kernel<true>), since "hit no bait" and "pushed up" both leave no pair;
//   * tally: one thread per distinct (bait, read) pair adds 1 to its read's counter -- the pairs are distinct, so the counter ends
//     as the number of distinct baits; within a bait the reads ascend, so neighbouring lanes add to neighbouring words;
//   * histogram: a grid-stride pass over the reads skips the marked ones and bins the counters, the bins below PD_LDS_BINS in the
//     workgroup's LDS (flushed with one global add per non-zero bin and workgroup), the rare ones above straight in global memory.
// All adds are integer adds: the result does not depend on the order the workgroups run in.
#include "internal.hpp"
#include "bait_table.hpp"

namespace zk {

constexpr int PD_LDS_BINS = 1024;    // 4 KiB of LDS a workgroup: sixteen 256-thread workgroups a CU keep 64 of its 160 KiB

__global__ __launch_bounds__(256) void pulldown_tally_kernel(const u64* __restrict__ pairs, u64 n, u64 n_reads, u32* __restrict__ cnt) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (u64)gridDim.x * blockDim.x) {
        const u64 r = pairs[j] & 0xffffffffull;
        if (r < n_reads) atomicAdd(&cnt[r], 1u);
    }
}

// hist[b] += the unmarked reads with cnt == b (b < n_bins; a larger counter is a damaged table: ZK_DERR_CAPACITY, nothing
// written); *n_vetoed += the marked reads.  Whole waves walk the reads (the loop bound is the workgroup's), so the ballot is
// taken by all 64 lanes.
__global__ __launch_bounds__(256) void pulldown_hist_kernel(const u32* __restrict__ cnt, const u8* __restrict__ mark, u64 n_reads, u64 n_bins,
                                                            u64* __restrict__ hist, u64* n_vetoed, u32* err) {
    __shared__ u32 bins[PD_LDS_BINS];
    __shared__ u32 vetoed;
    for (int i = threadIdx.x; i < PD_LDS_BINS; i += 256) bins[i] = 0;
    if (threadIdx.x == 0) vetoed = 0;
    __syncthreads();
    for (u64 base = (u64)blockIdx.x * 256; base < n_reads; base += (u64)gridDim.x * 256) {
        const u64 r = base + threadIdx.x;
        const bool in = r < n_reads;
        const bool v = in && mark[r] != 0;
        const u64 bal = __ballot(v);
        if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&vetoed, (u32)__popcll(bal));
        if (in && !v) {
            const u32 b = cnt[r];
            if (b >= n_bins) atomicOr(err, ZK_DERR_CAPACITY);
            else if (b < (u32)PD_LDS_BINS) atomicAdd(&bins[b], 1u);
            else atomicAdd(&hist[b], 1ull);
        }
    }
    __syncthreads();
    for (u32 i = threadIdx.x; i < (u32)PD_LDS_BINS && i < n_bins; i += 256)
        if (bins[i]) atomicAdd(&hist[i], (u64)bins[i]);
    if (threadIdx.x == 0 && vetoed) atomicAdd(n_vetoed, (u64)vetoed);
}

static int pulldown_hits(zk_ctx* c, const zk_bait_table* baits, const zk_bait_table* veto, int RK, Mate m1, Mate m2, uint64_t n_reads,
                         u64* pairs, uint64_t cap, uint64_t* n_pairs, u64* hist, uint64_t* n_vetoed) {
    *n_pairs = 0;
    *n_vetoed = 0;
    const uint64_t n_bins = baits->n_records + 1;
    ZK_HIP(c, hipMemsetAsync(hist, 0, 8 * n_bins, c->stream));
    if (n_reads == 0) return stream_sync(c);
    // The marks and the counters live from the lookup to the histogram, the sort's work space is known only after the lookup,
    // and the arena grows only while nothing is handed out: when it proves too small for both, it is grown and the lookup is
    // repeated (the same input gives the same number of pairs, so at most once -- and only until the arena has the batch's size).
    const uint64_t side = 5 * n_reads + (1 << 20);
    uint64_t room = side, raw = 0;
    u8* mark = nullptr;
    u32* cnt = nullptr;
    for (int attempt = 0;; attempt++) {
        arena_reset(c);
        ZK_TRY(arena_require(c, room, room));
        ZK_TRY(arena_alloc(c, n_reads, (void**)&mark));
        ZK_TRY(arena_alloc(c, 4 * n_reads, (void**)&cnt));
        ZK_HIP(c, hipMemsetAsync(mark, 0, n_reads, c->stream));
        ZK_TRY(capture_lookup(c, baits, veto, RK, m1, m2, n_reads, pairs, cap, mark, &raw));
        if (raw > cap) {
            *n_pairs = raw;
            return no_room(c, "pulldown", "(bait, read) pairs before deduplication", raw, cap);
        }
        room = side + capture_sort_bytes(raw);
        if (raw == 0 || room <= c->arena_size) break;
        if (attempt) return fail(c, ZK_EINTERNAL, "pulldown: the lookup gave %llu pairs the second time", (unsigned long long)raw);
    }
    uint64_t n = 0;
    if (raw) ZK_TRY(capture_sort_dedupe(c, baits, pairs, raw, &n));
    ZK_HIP(c, hipMemsetAsync(cnt, 0, 4 * n_reads, c->stream));
    if (n) {
        prof_begin(c, ZK_PROF_PULLDOWN_TALLY, 8 * n);
        hipLaunchKernelGGL(pulldown_tally_kernel, dim3(grid_cap(c, div_up(n, 256), 16)), dim3(256), 0, c->stream, pairs, (u64)n, (u64)n_reads, cnt);
        prof_end(c);
        ZK_HIP(c, hipGetLastError());
    }
    u64* d_vetoed = &c->d_scalars->pulldown_vetoed;
    ZK_HIP(c, hipMemsetAsync(d_vetoed, 0, sizeof(u64), c->stream));
    prof_begin(c, ZK_PROF_PULLDOWN_TALLY, 5 * n_reads);
    hipLaunchKernelGGL(pulldown_hist_kernel, dim3(grid_cap(c, div_up(n_reads, 256), 16)), dim3(256), 0, c->stream, cnt, mark, (u64)n_reads, (u64)n_bins,
                       hist, d_vetoed, c->d_err);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(fetch(c, &c->h_scalars->pulldown_vetoed));
    ZK_TRY(check_device_error(c));
    *n_pairs = n;
    *n_vetoed = c->h_scalars->pulldown_vetoed;
    return ZK_OK;
}

}  // namespace zk

using namespace zk;

extern "C" int zk_pulldown_hits(zk_ctx* c, const zk_bait_table* baits, const zk_bait_table* veto, int read_K, const uint8_t* d_text1,
                                const uint64_t* d_lines1, const uint8_t* d_text2, const uint64_t* d_lines2, uint64_t n_reads, uint64_t* d_pairs,
                                uint64_t cap, uint64_t* n_pairs, uint64_t* d_hist, uint64_t hist_cap, uint64_t* n_vetoed) {
    ZK_ARGS(c, baits && n_pairs && n_vetoed && d_hist && read_K >= 1 && read_K <= 32 && n_reads < (1ull << 32) && (!d_text2 == !d_lines2) &&
                   (n_reads == 0 || (d_text1 && d_lines1)) && (cap == 0 || d_pairs) && hist_cap >= baits->n_records + 1);
    arena_reset(c);
    return pulldown_hits(c, baits, veto, read_K, Mate{d_text1, (const u64*)d_lines1}, Mate{d_text2, (const u64*)d_lines2}, n_reads, (u64*)d_pairs, cap,
                         n_pairs, (u64*)d_hist, n_vetoed);
}
