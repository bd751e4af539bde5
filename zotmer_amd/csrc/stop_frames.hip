// stop_frames.hip -- `zot stop` (zotmer/commands/stop.py): the in-frame stop codons of reads placed on transcripts.
//
// The reference indexes every K-mer of its transcripts by (name, position), lets every window of a read vote for the frames
// (name, q - p, orientation) that its anchors (name, q) name, draws one frame with probability votes / n, and collects the
// windows of that orientation that end in frame with TAA, TAG or TGA (stop.py:112-150).  Two entries of include/zotk.h:
//   * zk_stop_frames: one wave per read, 64 windows per step, cut from the raw FASTQ text (read_window.hpp) and looked up in a
//     bait table whose ids are anchors on one u32 axis (bait_table.hpp), the transcripts laid out in name order, so that a
//     frame's sort key is (diagonal << 1) | orientation.  stop_long_kernel runs first (a line longer than pad that hits:
//     ZK_ERANGE).  stop_pick_kernel counts a read's votes n, takes their smallest and largest key and keeps the first
//     ZK_STOP_VOTES keys in LDS; the vote of rank r = mulhi64(rnd(seed, T_STOP, g) & ~2047, n) is the smallest key k with
//     #(votes <= k) > r, found by bisecting [smallest, largest] -- counting over the keys in LDS, or, for a read with more
//     votes than that, by walking its windows again for every probe (slow, exact, and only ever taken by reads on tandem
//     repeats).  One distinct key (the common read) needs no search.  The kernel leaves the key drawn and the number of
//     stops per read; scan64_inclusive turns the numbers into offsets; stop_emit_kernel walks the drawn orientation once more
//     and writes.  No atomics, no float; what a read gives depends on its text and its ordinal alone.
//   * zk_stop_nearest: for every counted (transcript, k-mer) the nearest k-mer of the transcript under ham(x >> 3, y >> 3),
//     the smallest among ties, and whether the k-mer is a known stop.  A workgroup takes ZK_STOP_NEAR_ENTRIES entries, one per
//     lane in a register, and streams the k-mers of each transcript they name through LDS in coalesced tiles of
//     ZK_STOP_NEAR_TILE; each of its waves compares a quarter of a tile (every lane reads the same word: a broadcast), and the
//     waves' (distance, k-mer) are reduced lexicographically.  No atomics.
#include "internal.hpp"
#include "bait_table.hpp"
#include "read_window.hpp"

namespace zk {

constexpr int SF_VOTES = ZK_STOP_VOTES, SF_BLOCK = 256, SF_WAVES = SF_BLOCK / 64;
constexpr u64 SF_T_STOP = 24;                    // synth.py: T_STOP
constexpr u64 SF_NONE = ~0ull;                   // no frame drawn (keys have 33 bits)
static_assert(SF_VOTES >= 64 && SF_VOTES % 64 == 0 && SF_VOTES * 8 * SF_WAVES <= 64 * 1024, "a wave's vote keys live in LDS");

__device__ __host__ __forceinline__ u64 sf_mix64(u64 z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ u64 wave_min_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u64 t = __shfl_xor(v, o, 64); v = t < v ? t : v; }
    return v;
}
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u64 t = __shfl_xor(v, o, 64); v = t > v ? t : v; }
    return v;
}

// window i of a line of L bytes as the list of orientation o holds it (stop.py:28-37)
__device__ __forceinline__ void sf_orient(int K, int o, u64 L, u64 i, u64 x, u64& key, u32& p) {
    key = o ? revcomp(K, x) : x;
    p = o ? (u32)(L - i - (u64)K) : (u32)i;
}

__device__ __forceinline__ u64 sf_vote(u32 a, u32 p, int o) { return ((u64)(a - p) << 1) | (u64)o; }

__device__ __forceinline__ bool sf_is_stop(u64 x) {
    const u32 y = (u32)x & 63u;
    return y == 48u || y == 50u || y == 56u;         // TAA, TAG, TGA
}

// the stripped sequence line of record r
__device__ __forceinline__ void sf_line(const u8* __restrict__ text, const u64* __restrict__ lines, u64 r, u64& s, u64& e) {
    seq_line(lines, r, s, e);
    strip(text, s, e);
}

// a line longer than pad that has a hit: its diagonals could reach the coordinates of another transcript
__global__ __launch_bounds__(SF_BLOCK) void stop_long_kernel(BaitView bt, const u8* __restrict__ text, const u64* __restrict__ lines, u64 n_reads, int K,
                                                             u64 pad, u64* __restrict__ bad) {
    const WaveIds w = wave_ids();
    for (u64 r = w.wave; r < n_reads; r += w.nw) {
        u64 s, e;
        sf_line(text, lines, r, s, e);
        if (e - s <= pad) continue;
        const bool hit = for_each_chunk(text, s, e, K, w.lane, [&](u64, bool valid, u64 x) {
            u32 lo, hi;
            return __ballot(valid && (bait_find(bt, x, lo, hi) || bait_find(bt, revcomp(K, x), lo, hi))) != 0;
        });
        if (hit && w.lane == 0) *bad = 1;
    }
}

// the votes of the line with a key <= k, both orientations, by walking the windows again
__device__ __forceinline__ u64 sf_count_walk(const BaitView& bt, const u8* __restrict__ text, u64 s, u64 e, int K, int lane, u64 k) {
    const u64 L = e - s;
    u64 below = 0;
    for (int o = 0; o < 2; o++)
        for_each_chunk(text, s, e, K, lane, [&](u64 c0, bool valid, u64 x) {
            u64 key;
            u32 p, t = 0, te = 0;
            sf_orient(K, o, L, c0 - s + lane, x, key, p);
            if (!(valid && bait_find(bt, key, t, te))) t = te = 0;
            // a window's anchors ascend, and so do its keys
            const u32 cut = partition_point(t, te, [&](u32 j) { return sf_vote(bt.ids[j], p, o) <= k; });
            below += cut - t;
            return false;
        });
    return wave_sum_u64(below);
}

// sel[r] = the key of the frame drawn for read first + r (SF_NONE: no vote), cnt[r] = the stops it gives
__global__ __launch_bounds__(SF_BLOCK) void stop_pick_kernel(BaitView bt, const u32* __restrict__ starts, u32 n_tx, const u8* __restrict__ text,
                                                             const u64* __restrict__ lines, u64 n_reads, int K, u32 pad, u64 s_stop, u64 first,
                                                             u64* __restrict__ sel, u64* __restrict__ cnt) {
    __shared__ u64 s_votes[SF_WAVES][SF_VOTES];
    const WaveIds w = wave_ids();
    const int lane = w.lane;
    u64* votes = s_votes[(threadIdx.x >> 6) & (SF_WAVES - 1)];
    for (u64 r = w.wave; r < n_reads; r += w.nw) {
        u64 s, e;
        sf_line(text, lines, r, s, e);
        const u64 L = e - s;
        u64 n = 0, lo = SF_NONE, hi = 0;
        if (L >= (u64)K) {
            for (int o = 0; o < 2; o++)
                for_each_chunk(text, s, e, K, lane, [&](u64 c0, bool valid, u64 x) {
                    u64 key;
                    u32 p, t = 0, te = 0;
                    sf_orient(K, o, L, c0 - s + lane, x, key, p);
                    if (!(valid && bait_find(bt, key, t, te))) t = te = 0;
                    const u32 mine = te - t;
                    const u32 upto = wave_incl_scan_u32(mine);
                    u64 pos = n + (upto - mine);
                    for (u32 j = t; j < te; j++, pos++) {
                        const u64 k = sf_vote(bt.ids[j], p, o);
                        lo = k < lo ? k : lo;
                        hi = k > hi ? k : hi;
                        if (pos < (u64)SF_VOTES) votes[pos] = k;
                    }
                    n += (u64)__shfl(upto, 63, 64);
                    return false;
                });
        }
        u64 key = SF_NONE, stops = 0;
        if (n) {
            lo = wave_min_u64(lo);
            hi = wave_max_u64(hi);
            if (lo != hi) {
                const u64 R = sf_mix64(s_stop + first + r);
                const u64 rank = __umul64hi(R & ~2047ull, n);            // ((R >> 11) * n) >> 53
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // the keys the other lanes of the wave stored
                __builtin_amdgcn_wave_barrier();
                // the smallest k of [lo, hi] with #(votes <= k) > rank
                while (lo < hi) {
                    const u64 mid = lo + ((hi - lo) >> 1);
                    u64 below;
                    if (n <= (u64)SF_VOTES) {
                        u32 b = 0;
                        for (u32 j = (u32)lane; j < (u32)n; j += 64) b += votes[j] <= mid ? 1u : 0u;
                        below = wave_sum_u32(b);
                    } else {
                        below = sf_count_walk(bt, text, s, e, K, lane, mid);
                    }
                    if (below > rank) hi = mid; else lo = mid + 1;
                }
                __builtin_amdgcn_wave_barrier();                         // the next read's keys come after these reads
            }
            key = lo;
            // the windows of the drawn orientation that end in frame with a stop
            const int o = (int)(key & 1u);
            const u32 d = (u32)(key >> 1);
            const u32 t = upper_bound(starts, 0u, n_tx, (u64)d + pad) - 1u;        // d + pad >= starts[0]: the layout
            const long long off = (long long)d - (long long)starts[t < n_tx ? t : 0u];
            u32 k3 = 0;
            for_each_chunk(text, s, e, K, lane, [&](u64 c0, bool valid, u64 x) {
                u64 xo;
                u32 p;
                sf_orient(K, o, L, c0 - s + lane, x, xo, p);
                const long long v = ((long long)p + off + K - 3) % 3;
                k3 += (u32)__popcll(__ballot(valid && v == 0 && sf_is_stop(xo)));     // v == 0 whatever the sign of the remainder
                return false;
            });
            stops = k3;
        }
        if (lane == 0) { sel[r] = key; cnt[r] = stops; }
    }
}

__global__ __launch_bounds__(SF_BLOCK) void stop_emit_kernel(const u32* __restrict__ starts, u32 n_tx, const u8* __restrict__ text,
                                                             const u64* __restrict__ lines, u64 n_reads, int K, u32 pad, const u64* __restrict__ sel,
                                                             const u64* __restrict__ incl, u32* __restrict__ tx, u64* __restrict__ kmers, u64 cap) {
    const WaveIds w = wave_ids();
    const int lane = w.lane;
    for (u64 r = w.wave; r < n_reads; r += w.nw) {
        u64 at = r ? incl[r - 1] : 0;
        if (incl[r] == at) continue;
        const u64 key = sel[r];
        u64 s, e;
        sf_line(text, lines, r, s, e);
        const u64 L = e - s;
        const int o = (int)(key & 1u);
        const u32 d = (u32)(key >> 1);
        const u32 t = upper_bound(starts, 0u, n_tx, (u64)d + pad) - 1u;
        const long long off = (long long)d - (long long)starts[t < n_tx ? t : 0u];
        for_each_chunk(text, s, e, K, lane, [&](u64 c0, bool valid, u64 x) {
            u64 xo;
            u32 p;
            sf_orient(K, o, L, c0 - s + lane, x, xo, p);
            const bool hit = valid && ((long long)p + off + K - 3) % 3 == 0 && sf_is_stop(xo);
            const u64 hm = __ballot(hit);
            const u64 pos = at + popc_below(hm);
            if (hit && pos < cap) { tx[pos] = t; kmers[pos] = xo; }
            at += (u64)__popcll(hm);
            return false;
        });
    }
}

static int stop_frames(zk_ctx* c, const zk_bait_table* anchors, const u32* starts, uint64_t n_tx, const u8* text, const u64* lines,
                       uint64_t n_reads, int K, u32 pad, uint64_t seed, uint64_t first, u32* tx, u64* kmers, uint64_t cap, uint64_t* n_out) {
    *n_out = 0;
    if (n_reads == 0 || anchors->n_keys == 0 || n_tx == 0) return ZK_OK;
    const BaitView bt = view_of(anchors);
    const uint64_t room = 16 * n_reads + (4 << 20);
    ZK_TRY(arena_require(c, room, room));
    u64 *sel, *cnt;
    ZK_TRY(arena_alloc(c, 8 * n_reads, (void**)&sel));
    ZK_TRY(arena_alloc(c, 8 * n_reads, (void**)&cnt));
    const u32 grid = grid_cap(c, div_up(n_reads, SF_WAVES), 16);
    u64* d_long = &c->d_scalars->stop_long;
    ZK_HIP(c, hipMemsetAsync(d_long, 0, sizeof(u64), c->stream));
    hipLaunchKernelGGL(stop_long_kernel, dim3(grid), dim3(SF_BLOCK), 0, c->stream, bt, text, lines, (u64)n_reads, K, (u64)pad, d_long);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(fetch(c, &c->h_scalars->stop_long));
    ZK_TRY(check_device_error(c));
    if (c->h_scalars->stop_long)
        return fail(c, ZK_ERANGE, "zk_stop_frames: a sequence line longer than pad = %u has a hit: its frames could name another transcript", pad);
    uint64_t text_bytes = 0;
    if (c->profile) ZK_HIP(c, hipMemcpy(&text_bytes, lines + 4 * n_reads - 1, sizeof(u64), hipMemcpyDeviceToHost));
    prof_begin(c, ZK_PROF_STOP_FRAMES, text_bytes + 16 * n_reads);
    hipLaunchKernelGGL(stop_pick_kernel, dim3(grid), dim3(SF_BLOCK), 0, c->stream, bt, starts, (u32)n_tx, text, lines, (u64)n_reads, K, pad,
                       sf_mix64(seed + SF_T_STOP), (u64)first, sel, cnt);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(scan_total(c, cnt, n_reads, n_out));
    const uint64_t total = *n_out;
    if (total >= (1ull << 32))
        return fail(c, ZK_ERANGE, "zk_stop_frames: %llu stops in one batch (at most 2^32 - 1); use smaller batches", (unsigned long long)total);
    if (total > cap) return no_room(c, "zk_stop_frames", "stops", total, cap);
    if (total == 0) return ZK_OK;
    prof_begin(c, ZK_PROF_STOP_EMIT, 16 * n_reads + 12 * total);
    hipLaunchKernelGGL(stop_emit_kernel, dim3(grid), dim3(SF_BLOCK), 0, c->stream, starts, (u32)n_tx, text, lines, (u64)n_reads, K, pad, sel, cnt, tx,
                       kmers, (u64)cap);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    return check_device_error(c);
}

// ---------------------------------------------------------------------------------------
// zk_stop_nearest
// ---------------------------------------------------------------------------------------
constexpr int SN_BLOCK = 256, SN_WAVES = SN_BLOCK / 64, SN_ENTRIES = ZK_STOP_NEAR_ENTRIES, SN_TILE = ZK_STOP_NEAR_TILE, SN_PART = SN_TILE / SN_WAVES;
static_assert(SN_ENTRIES == 64, "an entry per lane");
static_assert(SN_TILE % SN_BLOCK == 0 && SN_PART % 64 == 0, "whole waves load and compare a tile");
constexpr u64 SN_LOW_BITS = 0x5555555555555555ull;          // bits.m1: the low bit of every base

__global__ __launch_bounds__(SN_BLOCK) void stop_nearest_kernel(const u32* __restrict__ tx, const u64* __restrict__ kmers, u64 m, int K,
                                                                const u64* __restrict__ tk, const u64* __restrict__ tk_offs, u32 n_tx,
                                                                const u64* __restrict__ known, u64 n_known, u32* __restrict__ dist,
                                                                u64* __restrict__ near, u8* __restrict__ flags) {
    __shared__ u64 s_y[SN_TILE];
    __shared__ u64 s_best[SN_WAVES][SN_ENTRIES];
    __shared__ u32 s_d[SN_WAVES][SN_ENTRIES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (u64 e0 = (u64)blockIdx.x * SN_ENTRIES; e0 < m; e0 += (u64)gridDim.x * SN_ENTRIES) {
        const u64 e1 = e0 + SN_ENTRIES < m ? e0 + SN_ENTRIES : m;
        const u64 i = e0 + lane;
        const bool in = i < e1;
        const u64 x = in ? kmers[i] : 0;
        const u32 mt = in ? tx[i] : 0xffffffffu;
        const u64 xs = x >> 3;
        u32 best_d = (u32)K + 1u;          // nearest3's initial values (stop.py:69-77)
        u64 best_y = x;
        // the transcripts of the tile's entries, one after the other (the entries ascend by transcript)
        u64 a = e0;
        while (a < e1) {
            const u32 t = tx[a];
            const u64 lo = t < n_tx ? tk_offs[t] : 0, hi = t < n_tx ? tk_offs[t + 1] : 0;
            for (u64 b0 = lo; b0 < hi; b0 += SN_TILE) {
                const u32 nb = hi - b0 < (u64)SN_TILE ? (u32)(hi - b0) : (u32)SN_TILE;
                __syncthreads();                   // the tile before is done with
                for (u32 j = (u32)tid; j < nb; j += SN_BLOCK) s_y[j] = tk[b0 + j];
                __syncthreads();
                const u32 j0 = (u32)wave * SN_PART, j1 = j0 + SN_PART < nb ? j0 + SN_PART : nb;
                if (mt == t)
                    for (u32 j = j0; j < j1; j++) {
                        const u64 y = s_y[j];
                        const u64 z = xs ^ (y >> 3);
                        const u64 v = (z | (z >> 1)) & SN_LOW_BITS;
                        const u32 d = (u32)__builtin_popcount((u32)v) + (u32)__builtin_popcount((u32)(v >> 32));
                        if (d < best_d || (d == best_d && y < best_y)) { best_d = d; best_y = y; }
                    }
            }
            a = upper_bound(tx, a, e1, t);
        }
        __syncthreads();                           // s_best / s_d of the round before are read
        s_best[wave][lane] = best_y;
        s_d[wave][lane] = best_d;
        __syncthreads();
        if (wave == 0 && in) {
            u32 d = s_d[0][lane];
            u64 y = s_best[0][lane];
#pragma unroll
            for (int q = 1; q < SN_WAVES; q++) {
                const u32 dq = s_d[q][lane];
                const u64 yq = s_best[q][lane];
                if (dq < d || (dq == d && yq < y)) { d = dq; y = yq; }
            }
            dist[i] = d;
            near[i] = y;
            const u64 at = lower_bound(known, 0ull, n_known, x);
            flags[i] = (at < n_known && known[at] == x) ? 1 : 0;
        }
    }
}

static int stop_nearest(zk_ctx* c, const u32* tx, const u64* kmers, uint64_t m, int K, const u64* tk, const u64* tk_offs, uint64_t n_tx,
                        const u64* known, uint64_t n_known, u32* dist, u64* near, u8* flags) {
    if (m == 0) return ZK_OK;
    prof_begin(c, ZK_PROF_STOP_NEAREST, 25 * m);
    hipLaunchKernelGGL(stop_nearest_kernel, dim3(grid_cap(c, div_up(m, SN_ENTRIES), 16)), dim3(SN_BLOCK), 0, c->stream, tx, kmers, (u64)m, K, tk, tk_offs,
                       (u32)n_tx, known, (u64)n_known, dist, near, flags);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    return check_device_error(c);
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_stop_frames(zk_ctx* c, const zk_bait_table* anchors, const uint32_t* d_starts, uint64_t n_tx, const uint8_t* d_text, const uint64_t* d_lines,
                   uint64_t n_reads, int K, uint32_t pad, uint64_t seed, uint64_t first, uint32_t* d_tx, uint64_t* d_kmers, uint64_t cap,
                   uint64_t* n_out) {
    ZK_ARGS(c, anchors && n_out && n_reads < (1ull << 32) && n_tx < (1ull << 32) && (n_tx == 0 || d_starts) &&
                   (n_reads == 0 || (d_text && d_lines)) && (cap == 0 || (d_tx && d_kmers)));
    if (K < 3 || K > 32) return fail(c, ZK_EINVAL, "zk_stop_frames: K = %d, 3 <= K <= 32", K);
    if (anchors->K != K) return fail(c, ZK_EINVAL, "zk_stop_frames: K = %d, the anchor table was built with K = %d", K, anchors->K);
    arena_reset(c);
    return stop_frames(c, anchors, d_starts, n_tx, d_text, (const u64*)d_lines, n_reads, K, pad, seed, first, d_tx, (u64*)d_kmers, cap, n_out);
}

int zk_stop_nearest(zk_ctx* c, const uint32_t* d_tx, const uint64_t* d_kmers, uint64_t m, int K, const uint64_t* d_tk, const uint64_t* d_tk_offs,
                    uint64_t n_tx, const uint64_t* d_known, uint64_t n_known, uint32_t* d_dist, uint64_t* d_near, uint8_t* d_flags) {
    ZK_ARGS(c, n_tx < (1ull << 32) && (m == 0 || (d_tx && d_kmers && d_dist && d_near && d_flags)) && (n_tx == 0 || d_tk_offs) &&
                   (n_known == 0 || d_known));
    if (K < 3 || K > 32) return fail(c, ZK_EINVAL, "zk_stop_nearest: K = %d, 3 <= K <= 32", K);
    arena_reset(c);
    return stop_nearest(c, d_tx, (const u64*)d_kmers, m, K, (const u64*)d_tk, (const u64*)d_tk_offs, n_tx, (const u64*)d_known, n_known, d_dist,
                        (u64*)d_near, d_flags);
}

}  // extern "C"
