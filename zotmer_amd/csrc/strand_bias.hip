// strand_bias.hip -- `zot strand` (zotmer/commands/strand.py, the paired mode without -r): per-k-mer counts with the
// orientation kept, for a hash-sampled fraction of the canonical k-mers.
//
// A window becomes one TAGGED KEY (c << 1) | (oriented != c): c = min(x, rc x), oriented = x for mate 1 and rc x for mate 2
// (strand.py:59).  The key is 2K + 1 bits wide (K <= 31).  Sorted and counted (zk_sort_count), merged over the batches
// (zk_union_sum), the two orientations of a k-mer are neighbours: (c, tag 0) and then (c, tag 1).  Three entries of
// include/zotk.h:
//   * zk_strand_keys: one wave per read, 64 windows per step, cut from the raw FASTQ text as capture.hip's lookup cuts them
//     (read_window.hpp); the windows that pass the sample test (murmer(c, seed) & M) <= T (strand.py:136-139) are appended
//     to the output with one atomic per wave and step;
//   * zk_strand_pairs: the output loop of strand.py:142-155 as a neighbour test over the sorted table, compacted in
//     ascending c by count / scan / write over tiles that own their output range (compact.hpp);
//   * zk_format_pairs: the "%d\t%d\n" lines of strand.py:155 -- line lengths, a scan, the write.
#include "internal.hpp"
#include "compact.hpp"
#include "read_window.hpp"

namespace zk {

// ---------------------------------------------------------------------------------------
// zk_strand_keys
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void strand_keys_kernel(const u8* __restrict__ text, const u64* __restrict__ lines, u64 n_reads, int K,
                                                          int reverse, u64 seed, u64 M, u64 T, u64* __restrict__ keys, u64 cap,
                                                          u64* cursor) {
    const WaveIds w = wave_ids();
    const int lane = w.lane;
    for (u64 r = w.wave; r < n_reads; r += w.nw) {
        u64 b, e;
        seq_line(lines, r, b, e);
        for_each_chunk(text, b, e, K, lane, [&](u64, bool valid, u64 x) {
            const u64 y = revcomp(K, x);
            const u64 c = x < y ? x : y;
            const u64 oriented = reverse ? y : x;
            const bool keep = valid && (murmer(c, seed) & M) <= T;
            const u64 kept = __ballot(keep);
            if (kept == 0) return false;
            // the kept keys of the step take consecutive places: one atomic for the wave, a ballot rank for the lane
            u64 base = 0;
            if (lane == 0) base = atomicAdd((unsigned long long*)cursor, (unsigned long long)__popcll(kept));
            base = __shfl(base, 0, 64);
            const u64 q = base + popc_below(kept);
            if (keep && q < cap) keys[q] = (c << 1) | (oriented != c ? 1ull : 0ull);
            return false;
        });
    }
}

static int strand_keys(zk_ctx* c, const u8* text, const u64* lines, uint64_t n_reads, int K, int reverse, u64 seed, u64 T, u64* keys,
                       uint64_t cap, uint64_t* n_keys) {
    *n_keys = 0;
    if (n_reads == 0) return ZK_OK;
    u64* d_cur = &c->d_scalars->strand_cursor;
    ZK_HIP(c, hipMemsetAsync(d_cur, 0, sizeof(u64), c->stream));
    const u64 M = (1ull << (2 * K)) - 1;
    prof_begin(c, ZK_PROF_STRAND_KEYS, 0);
    hipLaunchKernelGGL(strand_keys_kernel, dim3(grid_cap(c, div_up(n_reads, 4), 16)), dim3(256), 0, c->stream, text, lines, (u64)n_reads, K, reverse,
                       seed, M, T, keys, (u64)cap, d_cur);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(fetch(c, &c->h_scalars->strand_cursor));
    ZK_TRY(check_device_error(c));
    *n_keys = c->h_scalars->strand_cursor;
    prof_add_bytes(c, ZK_PROF_STRAND_KEYS, 8 * (*n_keys < cap ? *n_keys : cap));
    if (*n_keys > cap) return no_room(c, "zk_strand_keys", "keys", *n_keys, cap);
    return ZK_OK;
}

// ---------------------------------------------------------------------------------------
// zk_strand_pairs
// ---------------------------------------------------------------------------------------
// Entry i of the sorted distinct tagged list.  Tag 0 (the k-mer seen as the smaller of {x, rc x}) always prints a line; its
// partner, if seen, is entry i + 1.  Tag 1 prints only as an orphan (entry i - 1 is not its partner) and only when asked.
template <typename CT>
struct StrandLines {
    const u64* k; const CT* cnt; u64 n; int K; u64 seed; bool orphans; u64* a; u64* b;
    __device__ bool orphan(u64 i) const { return (k[i] & 1ull) && !(i > 0 && k[i - 1] == k[i] - 1); }
    __device__ bool flag(u64 i) const { return !(k[i] & 1ull) || (orphans && orphan(i)); }
    __device__ void store(u64 pos, u64 i) const {
        const u64 key = k[i], x = key >> 1, y = revcomp(K, x);
        u64 xc, yc;
        if (key & 1ull) { xc = 0; yc = (u64)cnt[i]; }
        else {
            xc = (u64)cnt[i];
            yc = (x == y) ? xc : ((i + 1 < n && k[i + 1] == key + 1) ? (u64)cnt[i + 1] : 0);   // kx.get(y, 0); y is x for a palindrome
        }
        const bool x_first = murmer(x, seed) >= murmer(y, seed);      // strand.py:148-153
        a[pos] = x_first ? xc : yc;
        b[pos] = x_first ? yc : xc;
    }
};

// the count pass of compact.hpp with the two tallies of the statistics: sums[0] += orphans, sums[1] += palindromes
__global__ __launch_bounds__(CP_BLOCK) void strand_count_kernel(const u64* __restrict__ k, u64 n, int K, int orphans, u64* __restrict__ tile_counts,
                                                                u64* sums) {
    __shared__ u32 part[3][CP_BLOCK / 64];
    const u64 base = (u64)blockIdx.x * CP_TILE + (u64)threadIdx.x * CP_ITEMS;
    u32 lines = 0, orph = 0, pal = 0;
    for (int j = 0; j < CP_ITEMS; j++) {
        const u64 i = base + j;
        if (i >= n) break;
        const u64 key = k[i];
        if (key & 1ull) {
            const bool o = !(i > 0 && k[i - 1] == key - 1);
            orph += o ? 1u : 0u;
            lines += (o && orphans) ? 1u : 0u;
        } else {
            lines++;
            pal += (revcomp(K, key >> 1) == (key >> 1)) ? 1u : 0u;
        }
    }
    lines = wave_sum_u32(lines); orph = wave_sum_u32(orph); pal = wave_sum_u32(pal);
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = lines; part[1][threadIdx.x >> 6] = orph; part[2][threadIdx.x >> 6] = pal; }
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 tl = 0, to = 0, tp = 0;
        for (int w = 0; w < CP_BLOCK / 64; w++) { tl += part[0][w]; to += part[1][w]; tp += part[2][w]; }
        tile_counts[blockIdx.x] = tl;
        if (to) atomicAdd((unsigned long long*)&sums[0], (unsigned long long)to);
        if (tp) atomicAdd((unsigned long long*)&sums[1], (unsigned long long)tp);
    }
}

static int strand_pairs(zk_ctx* c, const u64* keys, const void* cnts, int count_bits, uint64_t n, int K, u64 seed, int flags, u64* a, u64* b,
                        uint64_t cap, zk_strand_stats* st) {
    st->n_pairs = st->n_orphans = st->n_palindromes = 0;
    if (n == 0) return ZK_OK;
    const bool orphans = (flags & ZK_STRAND_ORPHANS) != 0;
    const u64 tiles = div_up(n, CP_TILE);
    u64* cnt;
    ZK_TRY(arena_alloc(c, 8 * tiles, (void**)&cnt));
    u64* d_sums = c->d_scalars->strand_sums;
    ZK_HIP(c, hipMemsetAsync(d_sums, 0, 2 * sizeof(u64), c->stream));
    prof_begin(c, ZK_PROF_STRAND_PAIRS, 8 * n);
    hipLaunchKernelGGL(strand_count_kernel, dim3((u32)tiles), dim3(CP_BLOCK), 0, c->stream, keys, (u64)n, K, (int)orphans, cnt, d_sums);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(fetch(c, &c->h_scalars->strand_sums));
    ZK_TRY(scan_total(c, cnt, tiles, &st->n_pairs));
    st->n_orphans = c->h_scalars->strand_sums[0];
    st->n_palindromes = c->h_scalars->strand_sums[1];
    if (st->n_pairs > cap) return no_room(c, "zk_strand_pairs", "lines", st->n_pairs, cap);
    prof_begin(c, ZK_PROF_STRAND_PAIRS, (8 + count_bits / 8) * n + 16 * st->n_pairs);
    if (count_bits == 32) {
        StrandLines<u32> p{keys, (const u32*)cnts, (u64)n, K, seed, orphans, a, b};
        ZK_TRY(compact_write(c, p, n, cnt));
    } else {
        StrandLines<u64> p{keys, (const u64*)cnts, (u64)n, K, seed, orphans, a, b};
        ZK_TRY(compact_write(c, p, n, cnt));
    }
    prof_end(c);
    return check_device_error(c);
}

// ---------------------------------------------------------------------------------------
// zk_format_pairs
// ---------------------------------------------------------------------------------------
// (dec_digits, put_dec: common.hpp)
__global__ __launch_bounds__(256) void line_len_kernel(const u64* __restrict__ a, const u64* __restrict__ b, u64 n, u64* __restrict__ len) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x)
        len[i] = dec_digits(a[i]) + dec_digits(b[i]) + 2;
}

// line i ends at incl[i]: written backwards from there -- '\n', b, '\t', a
__global__ __launch_bounds__(256) void line_write_kernel(const u64* __restrict__ a, const u64* __restrict__ b, u64 n, const u64* __restrict__ incl,
                                                         u8* __restrict__ out) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        u8* p = out + incl[i];
        *--p = '\n';
        p = put_dec(p, b[i]);
        *--p = '\t';
        put_dec(p, a[i]);
    }
}

static int format_pairs(zk_ctx* c, const u64* a, const u64* b, uint64_t n, u8* out, uint64_t cap, uint64_t* n_bytes) {
    *n_bytes = 0;
    if (n == 0) return ZK_OK;
    ZK_TRY(arena_require(c, 8 * n + n / 32 + (1 << 20), 8 * n + n / 32 + (1 << 20)));
    u64* len;
    ZK_TRY(arena_alloc(c, 8 * n, (void**)&len));
    const u32 g = grid_cap(c, div_up(n, 256), 16);
    prof_begin(c, ZK_PROF_FORMAT_PAIRS, 24 * n);
    hipLaunchKernelGGL(line_len_kernel, dim3(g), dim3(256), 0, c->stream, a, b, (u64)n, len);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(scan_total(c, len, n, n_bytes));
    if (*n_bytes > cap) return no_room(c, "zk_format_pairs", "bytes of lines", *n_bytes, cap);
    prof_begin(c, ZK_PROF_FORMAT_PAIRS, 24 * n + *n_bytes);
    hipLaunchKernelGGL(line_write_kernel, dim3(g), dim3(256), 0, c->stream, a, b, (u64)n, len, out);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    return check_device_error(c);
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_strand_keys(zk_ctx* c, const uint8_t* d_text, const uint64_t* d_lines, uint64_t n_reads, int K, int reverse, uint64_t seed, uint64_t T,
                   uint64_t* d_keys, uint64_t cap, uint64_t* n_keys) {
    ZK_ARGS(c, n_keys && (n_reads == 0 || (d_text && d_lines)) && (cap == 0 || d_keys));
    if (K < 1 || K > 31)
        return fail(c, ZK_EINVAL, "zk_strand_keys: K = %d; a tagged key is 2K + 1 bits wide, so 1 <= K <= 31", K);
    arena_reset(c);
    return strand_keys(c, d_text, (const u64*)d_lines, n_reads, K, reverse != 0, seed, T, (u64*)d_keys, cap, n_keys);
}

int zk_strand_pairs(zk_ctx* c, const uint64_t* d_keys, const void* d_counts, int count_bits, uint64_t n, int K, uint64_t seed, int flags,
                    uint64_t* d_a, uint64_t* d_b, uint64_t cap, zk_strand_stats* stats) {
    ZK_ARGS(c, stats && (count_bits == 32 || count_bits == 64) && (n == 0 || (d_keys && d_counts)) && (cap == 0 || (d_a && d_b)) &&
                   (flags & ~ZK_STRAND_ORPHANS) == 0);
    if (K < 1 || K > 31)
        return fail(c, ZK_EINVAL, "zk_strand_pairs: K = %d; a tagged key is 2K + 1 bits wide, so 1 <= K <= 31", K);
    arena_reset(c);
    return strand_pairs(c, (const u64*)d_keys, d_counts, count_bits, n, K, seed, flags, (u64*)d_a, (u64*)d_b, cap, stats);
}

int zk_format_pairs(zk_ctx* c, const uint64_t* d_a, const uint64_t* d_b, uint64_t n, uint8_t* d_out, uint64_t cap, uint64_t* n_bytes) {
    ZK_ARGS(c, n_bytes && (n == 0 || (d_a && d_b)) && (cap == 0 || d_out));
    arena_reset(c);
    return format_pairs(c, (const u64*)d_a, (const u64*)d_b, n, d_out, cap, n_bytes);
}

}  // extern "C"
