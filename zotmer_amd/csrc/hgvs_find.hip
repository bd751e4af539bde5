// hgvs_find.hip -- `zot hgvs-find` (zotmer/commands/hgvs-find.py:917-1131): the k-mers of the captured read pairs per bait, and
// the Hamming neighbours of expected k-mer paths among them.
//
// The reference adds, for every read pair and every bait n that holds one of its k-mers, all of kmersList(K, mate, True) of
// both mates to capKmers[n] (library/capture.py:99-135), and later asks capKmers[n], window by window, for the k-mers that agree
// with an expected one under a mask and lie within a Hamming distance (library/debruijn.py:364-383, hgvs-find.py:534-553).
// Two entries of include/zotk.h:
//   * zk_capture_kmers: behind zk_capture_hits.  capkmers_mark_kernel flags the reads the pairs name (and refuses a read that
//     is no record of the batch); capkmers_count_kernel counts the valid windows of the flagged reads, one wave per read, once
//     however many baits hit it; capkmers_len_kernel + scan64_inclusive give every pair the end of its entries; and
//     capkmers_emit_kernel, one wave per pair, cuts 64 window starts per step (read_window.hpp) and writes the step's v valid
//     windows to v neighbouring entries and their reverse complements to the v after them.
//   * zk_path_scan: the host asks the device where every window's bait lies in the entries (path_seg_kernel: two binary
//     searches), lays the (window, tile) cells out window-major and uploads that plan.  path_scan_kernel<false> counts, one
//     workgroup per tile of ZK_PATH_TILE entries: a wave holds a quarter of the tile in registers, 16 rounds of 64
//     neighbouring entries, the tile's windows pass through LDS ZK_PATH_CHUNK at a time, and a wave's matches per window are
//     ballot popcounts stored (not added) to its own LDS word.  scan64_inclusive turns the cells into offsets.
//     path_scan_kernel<true> repeats the comparison: a match's place is its cell's offset + the matches of the waves before
//     its own (LDS) + those of the rounds before its own (a wave-uniform register) + the lanes below it (mbcnt).
// No atomics anywhere; nothing waits on another workgroup but inside scan64_inclusive.
#include <vector>

#include "internal.hpp"
#include "bait_table.hpp"
#include "read_window.hpp"

namespace zk {

// ---------------------------------------------------------------------------------------
// zk_capture_kmers
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void capkmers_mark_kernel(const u64* __restrict__ pairs, u64 n, u64 n_reads, u8* __restrict__ need, u64* bad) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (u64)gridDim.x * blockDim.x) {
        const u64 r = pairs[j] & 0xffffffffull;
        if (r < n_reads) need[r] = 1;
        else *bad = 1;
    }
}

// wcount[r] = the valid windows of the sequence lines of a needed record r
__global__ __launch_bounds__(256) void capkmers_count_kernel(Mate m1, Mate m2, u64 n_reads, int K, const u8* __restrict__ need,
                                                             u32* __restrict__ wcount) {
    const WaveIds w = wave_ids();
    for (u64 r = w.wave; r < n_reads; r += w.nw) {
        if (!need[r]) continue;
        u32 n = 0;
        for_each_mate_chunk(m1, m2, r, K, w.lane, [&](u64, bool valid, u64) { n += (u32)__popcll(__ballot(valid)); return false; });
        if (w.lane == 0) wcount[r] = n;
    }
}

// len[j] = entries of pair j: every valid window and its reverse complement
__global__ __launch_bounds__(256) void capkmers_len_kernel(const u64* __restrict__ pairs, u64 n, const u32* __restrict__ wcount, u64* __restrict__ len) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (u64)gridDim.x * blockDim.x)
        len[j] = 2ull * wcount[pairs[j] & 0xffffffffull];
}

__global__ __launch_bounds__(256) void capkmers_emit_kernel(const u64* __restrict__ pairs, u64 n, Mate m1, Mate m2, int K,
                                                            const u64* __restrict__ incl, u32* __restrict__ baits, u64* __restrict__ kmers, u64 cap) {
    const WaveIds w = wave_ids();
    for (u64 j = w.wave; j < n; j += w.nw) {
        const u64 word = pairs[j];
        const u64 r = word & 0xffffffffull;
        const u32 bait = (u32)(word >> 32);
        u64 o = j ? incl[j - 1] : 0;
        for_each_mate_chunk(m1, m2, r, K, w.lane, [&](u64, bool valid, u64 x) {
            const u64 vm = __ballot(valid);
            const u32 v = (u32)__popcll(vm);
            const u64 p = o + popc_below(vm);
            if (valid && p + v < cap) {           // (the host has checked the total against cap: never false)
                baits[p] = bait; kmers[p] = x;
                baits[p + v] = bait; kmers[p + v] = revcomp(K, x);
            }
            o += 2ull * v;
            return false;
        });
    }
}

static int capture_kmers(zk_ctx* c, const u64* pairs, uint64_t n, Mate m1, Mate m2, uint64_t n_reads, int K, u32* baits, u64* kmers,
                         uint64_t cap, uint64_t* n_out) {
    *n_out = 0;
    if (n == 0) return ZK_OK;
    const uint64_t room = 5 * n_reads + 8 * n + (4 << 20);
    ZK_TRY(arena_require(c, room, room));
    u8* need;
    u32* wcount;
    u64* len;
    ZK_TRY(arena_alloc(c, n_reads, (void**)&need));
    ZK_TRY(arena_alloc(c, 4 * n_reads, (void**)&wcount));
    ZK_TRY(arena_alloc(c, 8 * n, (void**)&len));
    u64* d_bad = &c->d_scalars->capkmers_bad;
    ZK_HIP(c, hipMemsetAsync(d_bad, 0, sizeof(u64), c->stream));
    ZK_HIP(c, hipMemsetAsync(need, 0, n_reads, c->stream));
    ZK_HIP(c, hipMemsetAsync(wcount, 0, 4 * n_reads, c->stream));
    const u32 gp = grid_cap(c, div_up(n, 256), 16);
    hipLaunchKernelGGL(capkmers_mark_kernel, dim3(gp), dim3(256), 0, c->stream, pairs, (u64)n, (u64)n_reads, need, d_bad);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(fetch(c, &c->h_scalars->capkmers_bad));
    ZK_TRY(stream_sync(c));
    if (c->h_scalars->capkmers_bad)
        return fail(c, ZK_EINVAL, "zk_capture_kmers: a pair names a read that is none of the batch's %llu", (unsigned long long)n_reads);
    hipLaunchKernelGGL(capkmers_count_kernel, dim3(grid_cap(c, div_up(n_reads, 4), 16)), dim3(256), 0, c->stream, m1, m2, (u64)n_reads, K, need, wcount);
    ZK_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(capkmers_len_kernel, dim3(gp), dim3(256), 0, c->stream, pairs, (u64)n, wcount, len);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(scan_total(c, len, n, n_out));
    const uint64_t total = *n_out;
    if (total >= (1ull << 32))
        return fail(c, ZK_ERANGE, "zk_capture_kmers: %llu entries in one call (at most 2^32 - 1); pass fewer pairs", (unsigned long long)total);
    if (total > cap) return no_room(c, "zk_capture_kmers", "entries", total, cap);
    if (total == 0) return ZK_OK;
    prof_begin(c, ZK_PROF_CAPTURE_KMERS, 12 * total);
    hipLaunchKernelGGL(capkmers_emit_kernel, dim3(grid_cap(c, div_up(n, 4), 16)), dim3(256), 0, c->stream, pairs, (u64)n, m1, m2, K, len, baits, kmers,
                       (u64)cap);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    return check_device_error(c);
}

// ---------------------------------------------------------------------------------------
// zk_path_scan
// ---------------------------------------------------------------------------------------
constexpr int PS_BLOCK = 256, PS_WAVES = PS_BLOCK / 64, PS_ROUNDS = 16, PS_WAVE_TILE = 64 * PS_ROUNDS, PS_TILE = PS_WAVES * PS_WAVE_TILE;
constexpr int PS_CHUNK = ZK_PATH_CHUNK;
static_assert(PS_TILE == ZK_PATH_TILE, "the tile include/zotk.h publishes");
constexpr u64 PS_LOW_BITS = 0x5555555555555555ull;          // bits.m1: the low bit of every base

// A window as the kernels read it: what the caller gave and where its cells are.  The entries of its bait lie in the tiles
// t0 .. t0 + nt - 1 (nt == 0: the bait has none); cell (w, t) is word cell0 + (t - t0) of the cell array.
struct PathWin { u64 value, mask, cell0; u32 bait, max_ham, min_count, t0, nt, pad; };

// seg[2w], seg[2w + 1] = the entries [lo, hi) whose bait is that of window w
__global__ __launch_bounds__(256) void path_seg_kernel(const u32* __restrict__ baits, u64 n, const u32* __restrict__ wbait, u32 W, u32* __restrict__ seg) {
    for (u32 w = blockIdx.x * blockDim.x + threadIdx.x; w < W; w += gridDim.x * blockDim.x) {
        const u32 b = wbait[w];
        const u64 lo = lower_bound(baits, 0ull, n, b);
        seg[2 * w] = (u32)lo;
        seg[2 * w + 1] = (u32)upper_bound(baits, lo, n, b);
    }
}

// first window whose bait is >= b (UPPER: > b)
template <bool UPPER>
__device__ __forceinline__ u32 ps_window_bound(const PathWin* __restrict__ win, u32 W, u32 b) {
    return partition_point(0u, W, [&](u32 i) { return UPPER ? win[i].bait <= b : win[i].bait < b; });
}

// EMIT false: cells[cell(w, t)] = the matches of window w in tile t.  EMIT true: cells holds the inclusive scan of those, and
// the matches are written.
template <bool EMIT>
__global__ __launch_bounds__(PS_BLOCK) void path_scan_kernel(const u32* __restrict__ baits, const u64* __restrict__ kmers, const u32* __restrict__ counts,
                                                             u64 n, const PathWin* __restrict__ win, u32 W, u64* __restrict__ cells,
                                                             u32* __restrict__ out_w, u32* __restrict__ out_e, u64 cap) {
    __shared__ u64 s_value[PS_CHUNK], s_mask[PS_CHUNK];
    __shared__ u32 s_bait[PS_CHUNK], s_ham[PS_CHUNK], s_min[PS_CHUNK];
    __shared__ u32 s_cnt[PS_CHUNK][PS_WAVES];
    __shared__ u32 s_range[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32 t = blockIdx.x;
    const u64 tile0 = (u64)t * PS_TILE;
    const u64 tile_end = tile0 + PS_TILE < n ? tile0 + PS_TILE : n;
    if (tid == 0) {        // the windows of the baits between the tile's first entry and its last
        s_range[0] = ps_window_bound<false>(win, W, baits[tile0]);
        s_range[1] = ps_window_bound<true>(win, W, baits[tile_end - 1]);
    }
    // the wave's quarter of the tile: entry = base + round * 64 + lane
    const u64 base = tile0 + (u64)wave * PS_WAVE_TILE;
    u64 x[PS_ROUNDS];
    u32 eb[PS_ROUNDS], ec[PS_ROUNDS];
    u32 valid = 0;
#pragma unroll
    for (int r = 0; r < PS_ROUNDS; r++) {
        const u64 i = base + (u64)r * 64 + lane;
        const bool in = i < n;
        x[r] = in ? kmers[i] : 0;
        eb[r] = in ? baits[i] : 0;
        ec[r] = in ? counts[i] : 0;
        valid |= in ? 1u << r : 0u;
    }
    // the baits of the wave's entries (ascending): a window of another bait has no match here
    const bool wave_any = base < n;
    const u64 last = base + PS_WAVE_TILE <= n ? base + PS_WAVE_TILE - 1 : n - 1;
    const u32 wb0 = wave_any ? baits[base] : 1u, wb1 = wave_any ? baits[last] : 0u;
    __syncthreads();
    const u32 wlo = s_range[0], whi = s_range[1];
    for (u32 c0 = wlo; c0 < whi; c0 += PS_CHUNK) {
        const u32 nc = whi - c0 < (u32)PS_CHUNK ? whi - c0 : (u32)PS_CHUNK;
        __syncthreads();               // the chunk before is done with
        for (u32 s = tid; s < nc; s += PS_BLOCK) {
            const PathWin pw = win[c0 + s];
            s_value[s] = pw.value; s_mask[s] = pw.mask; s_bait[s] = pw.bait; s_ham[s] = pw.max_ham; s_min[s] = pw.min_count;
        }
        __syncthreads();
        // a wave's matches per window
        for (u32 s = 0; s < nc; s++) {
            const u32 b = s_bait[s];
            u32 k = 0;
            if (b >= wb0 && b <= wb1) {
                const u64 v = s_value[s], m = s_mask[s];
                const u32 hmax = s_ham[s], cmin = s_min[s];
#pragma unroll
                for (int r = 0; r < PS_ROUNDS; r++) {
                    const u64 z = x[r] ^ v;
                    const u64 y = (z | (z >> 1)) & PS_LOW_BITS;
                    const u32 d = (u32)__builtin_popcount((u32)y) + (u32)__builtin_popcount((u32)(y >> 32));
                    const bool hit = ((valid >> r) & 1u) && eb[r] == b && (z & m) == 0 && d <= hmax && ec[r] >= cmin;
                    k += (u32)__popcll(__ballot(hit));
                }
            }
            if (lane == 0) s_cnt[s][wave] = k;
        }
        __syncthreads();
        if (!EMIT) {
            for (u32 s = tid; s < nc; s += PS_BLOCK) {
                const PathWin pw = win[c0 + s];
                const u32 dt = t - pw.t0;
                if (dt < pw.nt) {
                    u32 k = 0;
#pragma unroll
                    for (int q = 0; q < PS_WAVES; q++) k += s_cnt[s][q];
                    cells[pw.cell0 + dt] = k;
                }
            }
        } else {
            for (u32 s = 0; s < nc; s++) {
                if (s_cnt[s][wave] == 0) continue;           // wave-uniform
                const PathWin pw = win[c0 + s];
                const u32 dt = t - pw.t0;
                if (dt >= pw.nt) continue;                   // (the entries are not ascending by bait: no cell, nothing written)
                const u64 cell = pw.cell0 + dt;
                u64 pos = cell ? cells[cell - 1] : 0;
                for (int q = 0; q < wave; q++) pos += s_cnt[s][q];
                const u64 v = s_value[s], m = s_mask[s];
                const u32 b = s_bait[s], hmax = s_ham[s], cmin = s_min[s];
#pragma unroll
                for (int r = 0; r < PS_ROUNDS; r++) {
                    const u64 z = x[r] ^ v;
                    const u64 y = (z | (z >> 1)) & PS_LOW_BITS;
                    const u32 d = (u32)__builtin_popcount((u32)y) + (u32)__builtin_popcount((u32)(y >> 32));
                    const bool hit = ((valid >> r) & 1u) && eb[r] == b && (z & m) == 0 && d <= hmax && ec[r] >= cmin;
                    const u64 hm = __ballot(hit);
                    if (hm == 0) continue;
                    const u64 p = pos + popc_below(hm);
                    if (hit && p < cap) { out_w[p] = c0 + s; out_e[p] = (u32)(base + (u64)r * 64 + lane); }
                    pos += (u64)__popcll(hm);
                }
            }
        }
    }
}

static int path_scan(zk_ctx* c, const u32* baits, const u64* kmers, const u32* counts, uint64_t n, const zk_path_window* windows, uint32_t W,
                     u32* out_w, u32* out_e, uint64_t cap, uint64_t* n_out) {
    *n_out = 0;
    if (n == 0 || W == 0) return ZK_OK;
    // where every window's bait lies in the entries
    std::vector<u32> wbait(W), seg(2 * (size_t)W);
    for (uint32_t w = 0; w < W; w++) wbait[w] = windows[w].bait;
    u32 *d_wbait, *d_seg;
    ZK_TRY(arena_alloc(c, 4ull * W, (void**)&d_wbait));
    ZK_TRY(arena_alloc(c, 8ull * W, (void**)&d_seg));
    ZK_HIP(c, hipMemcpyAsync(d_wbait, wbait.data(), 4ull * W, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(path_seg_kernel, dim3(grid_cap(c, div_up(W, 256), 16)), dim3(256), 0, c->stream, baits, (u64)n, d_wbait, (u32)W, d_seg);
    ZK_HIP(c, hipGetLastError());
    ZK_HIP(c, hipMemcpyAsync(seg.data(), d_seg, 8ull * W, hipMemcpyDeviceToHost, c->stream));
    ZK_TRY(stream_sync(c));
    // the cells, window-major: their scan is the order of the output
    std::vector<PathWin> plan(W);
    uint64_t n_cells = 0;
    for (uint32_t w = 0; w < W; w++) {
        const u32 lo = seg[2 * (size_t)w], hi = seg[2 * (size_t)w + 1];
        PathWin& p = plan[w];
        p.value = windows[w].value; p.mask = windows[w].mask; p.bait = windows[w].bait;
        p.max_ham = windows[w].max_ham; p.min_count = windows[w].min_count;
        p.cell0 = n_cells; p.pad = 0;
        p.t0 = hi > lo ? lo / PS_TILE : 0;
        p.nt = hi > lo ? (hi - 1) / PS_TILE - p.t0 + 1 : 0;
        n_cells += p.nt;
    }
    if (n_cells == 0) return ZK_OK;
    arena_reset(c);                       // (d_wbait and d_seg are done with: the stream is idle)
    const uint64_t room = sizeof(PathWin) * (uint64_t)W + 8 * n_cells + (1 << 20);
    ZK_TRY(arena_require(c, room, room));
    PathWin* d_plan;
    u64* cells;
    ZK_TRY(arena_alloc(c, sizeof(PathWin) * (uint64_t)W, (void**)&d_plan));
    ZK_TRY(arena_alloc(c, 8 * n_cells, (void**)&cells));
    ZK_HIP(c, hipMemcpyAsync(d_plan, plan.data(), sizeof(PathWin) * (uint64_t)W, hipMemcpyHostToDevice, c->stream));
    ZK_HIP(c, hipMemsetAsync(cells, 0, 8 * n_cells, c->stream));
    const u32 tiles = (u32)div_up(n, PS_TILE);
    prof_begin(c, ZK_PROF_PATH_SCAN, 16 * n);
    hipLaunchKernelGGL(path_scan_kernel<false>, dim3(tiles), dim3(PS_BLOCK), 0, c->stream, baits, kmers, counts, (u64)n, d_plan, (u32)W, cells,
                       (u32*)nullptr, (u32*)nullptr, (u64)0);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(scan_total(c, cells, n_cells, n_out));               // (plan is read until here)
    const uint64_t total = *n_out;
    if (total > cap) return no_room(c, "zk_path_scan", "matches", total, cap);
    if (total == 0) return ZK_OK;
    prof_begin(c, ZK_PROF_PATH_SCAN, 16 * n + 8 * total);
    hipLaunchKernelGGL(path_scan_kernel<true>, dim3(tiles), dim3(PS_BLOCK), 0, c->stream, baits, kmers, counts, (u64)n, d_plan, (u32)W, cells, out_w,
                       out_e, (u64)cap);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    return check_device_error(c);
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_capture_kmers(zk_ctx* c, const uint64_t* d_pairs, uint64_t n_pairs, const uint8_t* d_text1, const uint64_t* d_lines1,
                     const uint8_t* d_text2, const uint64_t* d_lines2, uint64_t n_reads, int K, uint32_t* d_baits, uint64_t* d_kmers,
                     uint64_t cap, uint64_t* n_out) {
    ZK_ARGS(c, n_out && n_reads < (1ull << 32) && (!d_text2 == !d_lines2) &&
                   (n_pairs == 0 || (d_pairs && d_text1 && d_lines1)) && (cap == 0 || (d_baits && d_kmers)));
    if (K < 1 || K > 32) return fail(c, ZK_EINVAL, "zk_capture_kmers: K = %d, 1 <= K <= 32", K);
    arena_reset(c);
    return capture_kmers(c, (const u64*)d_pairs, n_pairs, Mate{d_text1, (const u64*)d_lines1}, Mate{d_text2, (const u64*)d_lines2}, n_reads, K,
                         d_baits, (u64*)d_kmers, cap, n_out);
}

int zk_path_scan(zk_ctx* c, const uint32_t* d_baits, const uint64_t* d_kmers, const uint32_t* d_counts, uint64_t n, int K,
                 const zk_path_window* windows, uint32_t n_windows, uint32_t* d_win, uint32_t* d_entry, uint64_t cap, uint64_t* n_out) {
    ZK_ARGS(c, n_out && n < (1ull << 32) && (n == 0 || (d_baits && d_kmers && d_counts)) && (n_windows == 0 || windows) &&
                   (cap == 0 || (d_win && d_entry)));
    if (K < 1 || K > 32) return fail(c, ZK_EINVAL, "zk_path_scan: K = %d, 1 <= K <= 32", K);
    for (uint32_t w = 0; w < n_windows; w++) {
        if (w && windows[w].bait < windows[w - 1].bait)
            return fail(c, ZK_EINVAL, "zk_path_scan: window %u has bait %u after bait %u: the windows ascend by bait", w, windows[w].bait,
                        windows[w - 1].bait);
        if (K < 32 && ((windows[w].value >> (2 * K)) != 0 || (windows[w].mask >> (2 * K)) != 0))
            return fail(c, ZK_EINVAL, "zk_path_scan: window %u has value or mask bits above its %d bases", w, K);
    }
    arena_reset(c);
    return path_scan(c, d_baits, (const u64*)d_kmers, d_counts, n, windows, n_windows, d_win, d_entry, cap, n_out);
}

}  // extern "C"
