// spectrum.hip -- the k-mer SPECTRUM measures of `zot dist` (the "quant" / "ab" / jensen.shannon rows of
// zotmer/commands/dist.py:59-92; formulas zotmer/library/dist.py, the vec=True branches) without the dense vector of 4**K
// counters the reference builds: every term of every formula is zero unless the k-mer occurs in both sets, so the sums over
// the 4**K positions are sums over the matches of two sorted (prefix, count) lists.
//
//   zk_project_sum   Measure.prep, vector mode (commands/dist.py:35-41): v[x >> S] += c, as the sorted distinct prefixes
//                    and the u64 sum of the counts under each.  Count / scan / write over tiles of 4096 entries, as the
//                    order-preserving compaction of capture.hip: no workgroup waits on another.  Segments are reduced inside
//                    the tile (a segmented scan per wave, then LDS adds); a segment that lies inside one tile is stored, the
//                    piece of one that crosses a tile border is added to the zeroed output with one integer atomic per
//                    (tile, segment) -- integer adds give the same sums in whatever order they land.
//   zk_spectrum_sums one merge-path pass over two such lists (the partition of setops.hip, ties A before B, so an equal pair
//                    is adjacent), structured like intersect_kernel: everything the nine measures need, the integers exact.
//   zk_spectrum_sums_row  the same pass for one list against m others -- a row of a distance matrix -- in three launches, one
//                    read-back and one synchronise whatever m is: one launch cuts all m merges, one runs over the tile groups of
//                    all pairs (the tile body is spectrum_kernel's), one adds each pair's slots in index order.
//
// Algorithmic bytes: zk_project_sum reads 8 per entry in the count pass, 8 + cb in the write pass (cb = 4 or 8 count bytes)
// and writes 16 per distinct prefix; zk_spectrum_sums reads 16 per entry and writes nothing but its few words.
//
// Precondition of both: the counts of a set add up to less than 2^64 (then every sum here fits its word, and the 128 bits
// of S_xy <= cx * cy).
#include <math.h>
#include <string.h>

#include "internal.hpp"

// The Jensen-Shannon terms keep the reference's operation order, one rounding per operation: a fused multiply-add
// (cy*x + cx*y in one rounding) would be a different number.
#pragma clang fp contract(off)

namespace zk {

// ---------------------------------------------------------------------------------------
// zk_project_sum
// ---------------------------------------------------------------------------------------
constexpr int PS_BLOCK = 256, PS_ROUNDS = 16, PS_TILE = PS_BLOCK * PS_ROUNDS, PS_NW = PS_BLOCK / 64;
constexpr int PS_CHUNKS = PS_TILE / 64;          // a chunk = the 64 consecutive entries one wave takes in one round

__device__ __forceinline__ bool ps_head(const u64* __restrict__ k, u64 i, int shift) {
    return i == 0 || (k[i] >> shift) != (k[i - 1] >> shift);
}

// tile_counts[t] = entries of tile t that start a segment (a new value of k >> shift)
__global__ __launch_bounds__(PS_BLOCK) void project_count_kernel(const u64* __restrict__ k, u64 n, int shift, u64* __restrict__ tile_counts) {
    __shared__ u64 scratch[PS_NW];
    const u64 base = (u64)blockIdx.x * PS_TILE;
    u64 heads = 0;
#pragma unroll
    for (int r = 0; r < PS_ROUNDS; r++) {
        const u64 i = base + (u64)r * PS_BLOCK + threadIdx.x;
        heads += (i < n && ps_head(k, i, shift)) ? 1u : 0u;
    }
    heads = block_sum_u64(heads, scratch);
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = heads;
}

// Entry i of the tile belongs to the tile's segment number idx = (heads among the tile's entries up to and including i):
// 0 = the segment that came in from the tile before, 1 .. H = the segments that start here.  Segment idx of tile t is
// output entry tile_incl[t - 1] + idx - 1.
template <typename CT>
__global__ __launch_bounds__(PS_BLOCK) void project_sum_kernel(const u64* __restrict__ k, const CT* __restrict__ cnt, u64 n, int shift,
                                                               const u64* __restrict__ tile_incl, u64* __restrict__ out_k,
                                                               u64* __restrict__ out_s, u64* __restrict__ tile_total) {
    __shared__ u64 sums[PS_TILE + 1];
    __shared__ u32 chunk_heads[PS_CHUNKS];
    __shared__ u64 scratch[PS_NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 base = (u64)blockIdx.x * PS_TILE;
    for (int s = tid; s < PS_TILE + 1; s += PS_BLOCK) sums[s] = 0;

    // every load of a thread before anything depends on one
    u64 key[PS_ROUNDS], c[PS_ROUNDS];
    u64 hmask[PS_ROUNDS];
    u32 isheads = 0;
#pragma unroll
    for (int r = 0; r < PS_ROUNDS; r++) {
        const u64 i = base + (u64)r * PS_BLOCK + tid;
        const bool in = i < n;
        key[r] = in ? k[i] >> shift : 0;
        c[r] = in ? (u64)cnt[i] : 0;
        if (in && ps_head(k, i, shift)) isheads |= 1u << r;
    }
#pragma unroll
    for (int r = 0; r < PS_ROUNDS; r++) {
        hmask[r] = __ballot((isheads >> r) & 1u);
        if (lane == 0) chunk_heads[r * PS_NW + wave] = (u32)__popcll(hmask[r]);
    }
    __syncthreads();          // chunk_heads complete, sums zeroed
    // heads in the chunks before each of this wave's chunks (chunk q = r * PS_NW + wave is in tile order)
    const u32 incl = wave_incl_scan_u32(chunk_heads[lane]);          // PS_CHUNKS == 64: one chunk per lane
    const u32 H = (u32)__shfl(incl, 63, 64);
    const u64 first = blockIdx.x ? tile_incl[blockIdx.x - 1] : 0;    // output entries before this tile's segment 1

    u64 total = 0;
#pragma unroll
    for (int r = 0; r < PS_ROUNDS; r++) {
        const int q = r * PS_NW + wave;
        const u32 before = (u32)__shfl(incl, q, 64) - (u32)__popcll(hmask[r]);
        const u64 upto = hmask[r] & (~0ull >> (63 - lane));          // heads at lanes <= this one
        const u32 idx = before + (u32)__popcll(upto);
        if ((isheads >> r) & 1u) out_k[first + idx - 1] = key[r];
        // segmented inclusive scan of the counts over the chunk: a lane adds what lies `o` lanes below only while that
        // lane is not before the start of its own segment
        const int start = upto ? 63 - __clzll((long long)upto) : 0;
        u64 v = c[r];
        total += v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const u64 t = __shfl_up(v, o, 64);
            if (lane - o >= start) v += t;
        }
        // the last lane of each segment of the chunk holds the segment's sum over the chunk
        const bool tail = lane == 63 || (((hmask[r] >> lane) >> 1) & 1ull);
        if (tail && v) atomicAdd(&sums[idx], v);
    }
    total = block_sum_u64(total, scratch);          // (its barriers also end the LDS adds)
    if (tid == 0) tile_total[blockIdx.x] = total;
    // A segment that starts here and ends here is stored; the piece of one that crosses a border of the tile is added.
    const u64 end = base + PS_TILE;
    const bool last_closed = end >= n || ps_head(k, end, shift);
    for (u32 s = tid; s <= H; s += PS_BLOCK) {
        const u64 v = sums[s];
        if (s == 0) {
            if (v) atomicAdd(&out_s[first - 1], v);          // v != 0 only when entry 0 of the tile is no head: first >= 1
        } else if (s < H || last_closed) out_s[first + s - 1] = v;
        else if (v) atomicAdd(&out_s[first + s - 1], v);
    }
}

int project_sum(zk_ctx* c, const u64* keys, const void* cnts, int count_bits, uint64_t n, int shift, u64* out_k, u64* out_s,
                uint64_t cap, uint64_t* n_out, uint64_t* total) {
    *n_out = 0;
    *total = 0;
    if (n == 0) return ZK_OK;
    const u64 tiles = div_up(n, PS_TILE);
    u64 *heads, *tot;
    ZK_TRY(arena_alloc(c, 8 * tiles, (void**)&heads));
    ZK_TRY(arena_alloc(c, 8 * tiles, (void**)&tot));
    prof_begin(c, ZK_PROF_PROJECT_SUM, 8 * n);
    hipLaunchKernelGGL(project_count_kernel, dim3((u32)tiles), dim3(PS_BLOCK), 0, c->stream, keys, (u64)n, shift, heads);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(scan_total(c, heads, tiles, n_out));
    const uint64_t m = *n_out;
    if (m > cap) return no_room(c, "zk_project_sum", "distinct prefixes", m, cap);
    ZK_HIP(c, hipMemsetAsync(out_s, 0, 8 * m, c->stream));
    prof_begin(c, ZK_PROF_PROJECT_SUM, (8 + count_bits / 8) * n + 16 * m);
    if (count_bits == 32)
        hipLaunchKernelGGL((project_sum_kernel<u32>), dim3((u32)tiles), dim3(PS_BLOCK), 0, c->stream, keys, (const u32*)cnts, (u64)n, shift,
                           heads, out_k, out_s, tot);
    else
        hipLaunchKernelGGL((project_sum_kernel<u64>), dim3((u32)tiles), dim3(PS_BLOCK), 0, c->stream, keys, (const u64*)cnts, (u64)n, shift,
                           heads, out_k, out_s, tot);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(column_sum(c, tot, tiles, 1, &c->d_scalars->project_total));
    ZK_TRY(fetch(c, &c->h_scalars->project_total));
    ZK_TRY(stream_sync(c));
    *total = c->h_scalars->project_total;
    return ZK_OK;
}

// ---------------------------------------------------------------------------------------
// zk_spectrum_sums
// ---------------------------------------------------------------------------------------
constexpr int SP_BLOCK = 512, SP_ITEMS = 8, SP_TILE = SP_BLOCK * SP_ITEMS, SP_NW = SP_BLOCK / 64;
static_assert(SP_TILE == MERGE_TILE, "the tiles of make_partition");

// result words (device): 0 n_shared, 1 S_min, 2 X_shared, 3 Y_shared, 4 / 5 S_xy low / high, 6 S_sqrt, 7 S_js (doubles)
constexpr int SP_WORDS = 8;

// What a thread has met so far: the six integers and the two doubles of zk_spectrum.
struct SpAcc {
    u64 n_shared = 0, s_min = 0, x_sh = 0, y_sh = 0, xy_lo = 0, xy_hi = 0;
    double s_sqrt = 0, s_js = 0;
};

// The LDS of a workgroup.  The A slice and the B slice of a tile add up to SP_TILE entries, so they share one buffer (as
// MergeSmem of setops.hip):
//   ka = keys           : [0] = left halo A[a0 - 1], [1 .. nAt] = the A slice
//   kb = keys + nAt + 1 : [0 .. nBt - 1] = the B slice; [nBt] is read (never used) when the B cursor stands at its end
// Keys and sums of a tile: 64 KiB, two workgroups per CU -- what intersect_kernel takes for the keys alone.
struct SpSmem {
    alignas(16) u64 keys[SP_TILE + 2];          // aligned as arrays of their own would be: the merge steps read them 16 bytes at a time
    alignas(16) u64 sums[SP_TILE + 2];
    u64 scratch[SP_NW];
    double fscratch[SP_NW];
};

// One tile of the merge of (A, sA) and (B, sB): part[tile], part[tile + 1] = its cut (make_partition).  The body of
// spectrum_kernel and of spectrum_row_kernel; every workgroup thread calls it.  A key counts as shared when both sums are
// non-zero (a count of zero is an absent k-mer in the reference's vector).
__device__ __forceinline__ void spectrum_tile(SpSmem& sm, const u64* __restrict__ A, const u64* __restrict__ sA, u64 nA,
                                              const u64* __restrict__ B, const u64* __restrict__ sB, u64 nB,
                                              const u64* __restrict__ part, u32 tile, double cx, double cy, double cx2, double cy2,
                                              SpAcc& acc) {
    u64* const keys = sm.keys;
    u64* const sums = sm.sums;
    const int tid = threadIdx.x;
    u64 n_shared = acc.n_shared, s_min = acc.s_min, x_sh = acc.x_sh, y_sh = acc.y_sh, xy_lo = acc.xy_lo, xy_hi = acc.xy_hi;
    double s_sqrt = acc.s_sqrt, s_js = acc.s_js;
    {
        const u64 a0 = part[tile], a1 = part[tile + 1];
        u64 d0 = (u64)tile * SP_TILE, d1 = d0 + SP_TILE;
        if (d1 > nA + nB) d1 = nA + nB;
        const u64 b0 = d0 - a0, b1 = d1 - a1;
        const int nAt = (int)(a1 - a0), nBt = (int)(b1 - b0);
        {
            // all loads of a thread before its first LDS write (see union_sum_kernel)
            constexpr int R = (SP_TILE + 1 + SP_BLOCK - 1) / SP_BLOCK;
            u64 kv[R], sv[R];
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int sl = tid + r * SP_BLOCK;
                const bool isA = sl <= nAt;
                const u64 g = isA ? a0 + (u64)sl : b0 + (u64)(sl - nAt - 1);          // A side: element index + 1
                const bool ok = (sl < nAt + 1 + nBt) && (isA ? g >= 1 : true);
                kv[r] = *(ok ? (isA ? A + (g - 1) : B + g) : A);
                sv[r] = *(ok ? (isA ? sA + (g - 1) : sB + g) : sA);
                if (!ok) { kv[r] = 0; sv[r] = 0; }
            }
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int sl = tid + r * SP_BLOCK;
                if (sl < nAt + 1 + nBt) { keys[sl] = kv[r]; sums[sl] = sv[r]; }
            }
        }
        __syncthreads();
        const u64* const ka = keys;
        const u64* const kb = keys + nAt + 1;
        const u64* const ca = sums;
        const u64* const cb = sums + nAt + 1;
        const bool have_left = a0 > 0;
        const int total = nAt + nBt;
        int d = tid * SP_ITEMS;
        if (d > total) d = total;
        int lo = d > nBt ? d - nBt : 0, hi = d < nAt ? d : nAt;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ka[1 + mid] <= kb[d - mid - 1]) lo = mid + 1; else hi = mid;
        }
        int i = lo, j = d - lo;
#pragma unroll
        for (int s = 0; s < SP_ITEMS; s++) {
            if (d + s < total) {
                const bool hasA = i < nAt, hasB = j < nBt;
                if (hasA && (!hasB || ka[1 + i] <= kb[j])) i++;
                else {
                    // a B entry: its equal, if any, is the A entry just before the A cursor (possibly the left halo)
                    const bool avalid = (i > 0) || have_left;
                    const u64 x = ca[i], y = cb[j];
                    if (avalid && ka[i] == kb[j] && x && y) {
                        n_shared++;
                        s_min += x < y ? x : y;
                        x_sh += x;
                        y_sh += y;
                        const u64 pl = x * y, ph = __umul64hi(x, y);
                        xy_lo += pl;
                        xy_hi += ph + (xy_lo < pl ? 1 : 0);
                        const double fx = (double)x, fy = (double)y;
                        // library/dist.py:90: sqrt(x*y).  fx * fy is the correctly rounded product while x, y < 2^53
                        s_sqrt += sqrt(fx * fy);
                        // library/dist.py:138-139, operation by operation
                        const double cyx = cy * fx, cxy = cx * fy;
                        s_js += fx / cx * log(cy2 * fx / (cyx + cxy));
                        s_js += fy / cy * log(cx2 * fy / (cxy + cyx));
                    }
                    j++;
                }
            }
        }
        __syncthreads();        // the next tile restages keys / sums
    }
    acc.n_shared = n_shared; acc.s_min = s_min; acc.x_sh = x_sh; acc.y_sh = y_sh; acc.xy_lo = xy_lo; acc.xy_hi = xy_hi;
    acc.s_sqrt = s_sqrt; acc.s_js = s_js;
}

// The workgroup's sums of what its threads met: the integers with one atomic each into res[0 .. 5] (S_xy: 128 bits), the two
// doubles into the workgroup's own slot.
__device__ __forceinline__ void spectrum_flush(SpSmem& sm, const SpAcc& acc, u64* __restrict__ res, double* __restrict__ slot) {
    u64* const scratch = sm.scratch;
    double* const fscratch = sm.fscratch;
    const int tid = threadIdx.x;
    u64 n_shared = acc.n_shared, s_min = acc.s_min, x_sh = acc.x_sh, y_sh = acc.y_sh, xy_lo = acc.xy_lo, xy_hi = acc.xy_hi;
    double s_sqrt = acc.s_sqrt, s_js = acc.s_js;
    // S_xy: the low words as two 32-bit halves, so that the workgroup's sum of each fits 64 bits
    n_shared = block_sum_u64(n_shared, scratch);
    s_min = block_sum_u64(s_min, scratch);
    x_sh = block_sum_u64(x_sh, scratch);
    y_sh = block_sum_u64(y_sh, scratch);
    const u64 l0 = block_sum_u64(xy_lo & 0xffffffffull, scratch);
    const u64 l1 = block_sum_u64(xy_lo >> 32, scratch);
    xy_hi = block_sum_u64(xy_hi, scratch);
    s_sqrt = block_sum_f64<SP_NW>(s_sqrt, fscratch);
    s_js = block_sum_f64<SP_NW>(s_js, fscratch);
    if (tid == 0) {
        slot[0] = s_sqrt;
        slot[1] = s_js;
        if (n_shared) {
            atomicAdd(&res[0], n_shared);
            atomicAdd(&res[1], s_min);
            atomicAdd(&res[2], x_sh);
            atomicAdd(&res[3], y_sh);
            // l0 + 2^32 * l1 as 128 bits, then the add with the carry out of the low word (the returned old value tells it)
            u64 low = l0 + (l1 << 32);
            u64 high = xy_hi + (l1 >> 32) + (low < l0 ? 1 : 0);
            const u64 old = atomicAdd(&res[4], low);
            high += (old + low < old) ? 1 : 0;
            if (high) atomicAdd(&res[5], high);
        }
    }
}

// Workgroups stride over the tiles and add their integers ONCE at the end (intersect_kernel's comment has the cost of an atomic
// per tile); the two doubles go to the workgroup's own slot, partial[2 * blockIdx.x], and are added up in slot order by
// spectrum_combine_kernel: the same inputs give the same bits.
__global__ __launch_bounds__(SP_BLOCK) void spectrum_kernel(const u64* __restrict__ A, const u64* __restrict__ sA, u64 nA,
                                                            const u64* __restrict__ B, const u64* __restrict__ sB, u64 nB,
                                                            const u64* __restrict__ part, u32 tiles, double cx, double cy,
                                                            u64* __restrict__ res, double* __restrict__ partial) {
    __shared__ SpSmem sm;
    SpAcc acc;
    const double cy2 = 2 * cy, cx2 = 2 * cx;
    for (u32 tile = blockIdx.x; tile < tiles; tile += gridDim.x) spectrum_tile(sm, A, sA, nA, B, sB, nB, part, tile, cx, cy, cx2, cy2, acc);
    spectrum_flush(sm, acc, res, partial + 2 * blockIdx.x);
}

// the workgroups' doubles in slot order: one wave, lane l takes slots l, l + 64, ..., then the xor tree
__global__ __launch_bounds__(64) void spectrum_combine_kernel(const double* __restrict__ partial, u32 slots, u64* __restrict__ res) {
    double a = 0, b = 0;
    for (u32 s = threadIdx.x; s < slots; s += 64) { a += partial[2 * s]; b += partial[2 * s + 1]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
    if (threadIdx.x == 0) {
        res[6] = (u64)__double_as_longlong(a);
        res[7] = (u64)__double_as_longlong(b);
    }
}

int spectrum_sums(zk_ctx* c, const u64* A, const u64* sA, u64 nA, const u64* B, const u64* sB, u64 nB, double cx, double cy,
                  zk_spectrum* out) {
    *out = zk_spectrum{};
    if (nA == 0 || nB == 0) return ZK_OK;
    u64* part; u32 tiles;
    ZK_TRY(make_partition(c, A, nA, B, nB, &part, &tiles));
    const u32 grid = grid_cap(c, tiles, 8);
    u64* res; double* partial;
    ZK_TRY(arena_alloc(c, sizeof(u64) * SP_WORDS, (void**)&res));
    ZK_TRY(arena_alloc(c, 2 * sizeof(double) * grid, (void**)&partial));
    ZK_HIP(c, hipMemsetAsync(res, 0, sizeof(u64) * SP_WORDS, c->stream));
    prof_begin(c, ZK_PROF_SPECTRUM, 16 * (nA + nB));
    hipLaunchKernelGGL(spectrum_kernel, dim3(grid), dim3(SP_BLOCK), 0, c->stream, A, sA, nA, B, sB, nB, part, tiles, cx, cy, res, partial);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(spectrum_combine_kernel, dim3(1), dim3(64), 0, c->stream, partial, grid, res);
    ZK_HIP(c, hipGetLastError());
    static_assert(sizeof(zk_scalars::spectrum) == sizeof(u64) * SP_WORDS, "the landing holds every word of res");
    ZK_TRY(fetch(c, &c->h_scalars->spectrum, res));
    ZK_TRY(stream_sync(c));
    const u64* h = c->h_scalars->spectrum;
    out->n_shared = h[0]; out->s_min = h[1]; out->x_shared = h[2]; out->y_shared = h[3]; out->s_xy_lo = h[4]; out->s_xy_hi = h[5];
    memcpy(&out->s_sqrt, &h[6], sizeof(double));
    memcpy(&out->s_js, &h[7], sizeof(double));
    return ZK_OK;
}

// ---------------------------------------------------------------------------------------
// zk_spectrum_sums_row: one spectrum against m others in three launches, one read-back and one synchronise
// ---------------------------------------------------------------------------------------
// Pair j = (x, y_j) has tiles_j = ceil((nx + ny_j) / SP_TILE) tiles.  A workgroup takes one GROUP of consecutive tiles of one
// pair; the group size is a function of the pair's tile count alone, so which terms a workgroup's doubles hold, and the slot
// order they are added in, do not depend on the rest of the row or on the device: the same pair gives the same bits wherever
// it stands.  No workgroup reads what another wrote.
constexpr u32 SPR_GROUP_MIN = 4;        // tiles per workgroup of a short pair
constexpr u32 SPR_GROUPS_MAX = 2048;    // a long pair has at most this many groups (and slots)
static inline u32 spr_group_tiles(u32 tiles) {
    const u32 g = (u32)div_up(tiles, SPR_GROUPS_MAX);
    return g < SPR_GROUP_MIN ? SPR_GROUP_MIN : g;
}

struct SprPair {            // one per pair, made on the host; an empty pair has tiles == 0
    const u64* yk;
    const u64* ys;
    u64 ny;
    double cy;
    u32 tiles, group;       // group = tiles a workgroup takes
};
static_assert(sizeof(SprPair) == 40, "SprPair: five words");

// the pair a flat index belongs to: the last j with pre[j] <= i (pre[0] = 0, pre[m] > i; pairs of width 0 are skipped)
template <typename T>
__device__ __forceinline__ u32 spr_find(const T* __restrict__ pre, u32 m, T i) {
    u32 lo = 0, hi = m;               // the answer lies in [lo, hi)
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (pre[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// Thread i of dpre[m] = the diagonals of all pairs (tiles_j + 1 each): the merge-path search of merge_partition_kernel, ties A
// before B; pair j's cuts start at part[dpre[j]].
__global__ __launch_bounds__(256) void spectrum_row_partition_kernel(const u64* __restrict__ A, u64 nA, const SprPair* __restrict__ pairs,
                                                                     const u64* __restrict__ dpre, u32 m, u64* __restrict__ part) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= dpre[m]) return;
    const u32 j = spr_find<u64>(dpre, m, i);
    const u64* __restrict__ B = pairs[j].yk;
    const u64 nB = pairs[j].ny;
    u64 D = (i - dpre[j]) * SP_TILE;
    if (D > nA + nB) D = nA + nB;
    u64 lo = D > nB ? D - nB : 0, hi = D < nA ? D : nA;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (A[mid] <= B[D - mid - 1]) lo = mid + 1; else hi = mid;
    }
    part[i] = lo;
}

// Workgroup b of gpre[m] = the tile groups of all pairs.  Its integers go to its pair's words res[8 j ..], its doubles to
// partial[2 b]: pair j's slots are partial[2 gpre[j]] .. partial[2 gpre[j + 1]).
__global__ __launch_bounds__(SP_BLOCK) void spectrum_row_kernel(const u64* __restrict__ A, const u64* __restrict__ sA, u64 nA, double cx,
                                                                const SprPair* __restrict__ pairs, const u64* __restrict__ dpre,
                                                                const u32* __restrict__ gpre, u32 m, const u64* __restrict__ part,
                                                                u64* __restrict__ res, double* __restrict__ partial) {
    __shared__ SpSmem sm;
    const u32 j = spr_find<u32>(gpre, m, blockIdx.x);
    const SprPair p = pairs[j];
    const u32 t0 = (blockIdx.x - gpre[j]) * p.group;
    const u32 t1 = t0 + p.group < p.tiles ? t0 + p.group : p.tiles;
    const u64* __restrict__ pp = part + dpre[j];
    SpAcc acc;
    const double cy = p.cy, cy2 = 2 * cy, cx2 = 2 * cx;
    for (u32 tile = t0; tile < t1; tile++) spectrum_tile(sm, A, sA, nA, p.yk, p.ys, p.ny, pp, tile, cx, cy, cx2, cy2, acc);
    spectrum_flush(sm, acc, res + (u64)SP_WORDS * j, partial + 2 * (u64)blockIdx.x);
}

// a wave per pair adds the pair's slots in index order: lane l takes slots l, l + 64, ..., then the xor tree
__global__ __launch_bounds__(256) void spectrum_row_combine_kernel(const double* __restrict__ partial, const u32* __restrict__ gpre, u32 m,
                                                                   u64* __restrict__ res) {
    const u32 j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= m) return;
    const u32 s0 = gpre[j], s1 = gpre[j + 1];
    double a = 0, b = 0;
    for (u32 s = s0 + lane; s < s1; s += 64) { a += partial[2 * (u64)s]; b += partial[2 * (u64)s + 1]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
    if (lane == 0) {
        res[(u64)SP_WORDS * j + 6] = (u64)__double_as_longlong(a);
        res[(u64)SP_WORDS * j + 7] = (u64)__double_as_longlong(b);
    }
}

// the pinned block the descriptors go up through and the results land in; kept by the context, sized for a full row
static int row_stage(zk_ctx* c, char** up, u64** down) {
    constexpr size_t UP = ZK_SPECTRUM_ROW_MAX * sizeof(SprPair) + (ZK_SPECTRUM_ROW_MAX + 1) * (sizeof(u64) + sizeof(u32)) + 64;
    constexpr size_t DOWN = (size_t)ZK_SPECTRUM_ROW_MAX * SP_WORDS * sizeof(u64);
    if (!c->row_stage) ZK_HIP(c, hipHostMalloc(&c->row_stage, UP + DOWN, hipHostMallocDefault));
    *down = (u64*)c->row_stage;
    *up = (char*)c->row_stage + DOWN;
    return ZK_OK;
}

int spectrum_sums_row(zk_ctx* c, const u64* A, const u64* sA, u64 nA, double cx, u32 m, const u64* const* yk, const u64* const* ys,
                      const uint64_t* ny, const double* cy, zk_spectrum* out) {
    for (u32 j = 0; j < m; j++) out[j] = zk_spectrum{};
    if (m == 0 || nA == 0) return ZK_OK;
    char* up; u64* down;
    ZK_TRY(row_stage(c, &up, &down));
    // layout of the descriptor block (host and device): pairs[m], dpre[m + 1], gpre[m + 1]
    const size_t off_d = (size_t)m * sizeof(SprPair), off_g = off_d + ((size_t)m + 1) * sizeof(u64);
    const size_t up_bytes = off_g + ((size_t)m + 1) * sizeof(u32);
    SprPair* hp = (SprPair*)up;
    u64* hd = (u64*)(up + off_d);
    u32* hg = (u32*)(up + off_g);
    u64 diags = 0, groups = 0, bytes = 0;
    for (u32 j = 0; j < m; j++) {
        hd[j] = diags;
        hg[j] = (u32)groups;
        const u64 total = ny[j] ? nA + ny[j] : 0;
        const u64 tiles = div_up(total, SP_TILE);
        if (tiles > 0xfffffffeull) return fail(c, ZK_EINVAL, "zk_spectrum_sums_row: pair %u is too long", j);
        const u32 g = spr_group_tiles((u32)tiles);
        hp[j] = SprPair{yk[j], ys[j], ny[j], cy[j], (u32)tiles, g};
        if (tiles) { diags += tiles + 1; groups += div_up(tiles, g); bytes += 16 * total; }
    }
    hd[m] = diags;
    hg[m] = (u32)groups;
    if (groups == 0) return ZK_OK;
    char* dev; u64 *part, *res; double* partial;
    // a long row of long lists needs more than the arena's floor: size it before the first allocation
    const uint64_t want = up_bytes + sizeof(u64) * diags + sizeof(u64) * SP_WORDS * m + 2 * sizeof(double) * groups + 4 * 256;
    ZK_TRY(arena_require(c, want, want));
    ZK_TRY(arena_alloc(c, up_bytes, (void**)&dev));
    ZK_TRY(arena_alloc(c, sizeof(u64) * diags, (void**)&part));
    ZK_TRY(arena_alloc(c, sizeof(u64) * SP_WORDS * m, (void**)&res));
    ZK_TRY(arena_alloc(c, 2 * sizeof(double) * groups, (void**)&partial));
    ZK_HIP(c, hipMemcpyAsync(dev, up, up_bytes, hipMemcpyHostToDevice, c->stream));
    ZK_HIP(c, hipMemsetAsync(res, 0, sizeof(u64) * SP_WORDS * m, c->stream));
    const SprPair* dp = (const SprPair*)dev;
    const u64* dd = (const u64*)(dev + off_d);
    const u32* dg = (const u32*)(dev + off_g);
    hipLaunchKernelGGL(spectrum_row_partition_kernel, dim3((u32)div_up(diags, 256)), dim3(256), 0, c->stream, A, nA, dp, dd, m, part);
    ZK_HIP(c, hipGetLastError());
    prof_begin(c, ZK_PROF_SPECTRUM, bytes);
    hipLaunchKernelGGL(spectrum_row_kernel, dim3((u32)groups), dim3(SP_BLOCK), 0, c->stream, A, sA, nA, cx, dp, dd, dg, m, part, res, partial);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(spectrum_row_combine_kernel, dim3((u32)div_up(m, 4)), dim3(256), 0, c->stream, partial, dg, m, res);
    ZK_HIP(c, hipGetLastError());
    ZK_HIP(c, hipMemcpyAsync(down, res, sizeof(u64) * SP_WORDS * m, hipMemcpyDeviceToHost, c->stream));
    ZK_TRY(stream_sync(c));
    for (u32 j = 0; j < m; j++) {
        const u64* h = down + (size_t)SP_WORDS * j;
        zk_spectrum* o = out + j;
        o->n_shared = h[0]; o->s_min = h[1]; o->x_shared = h[2]; o->y_shared = h[3]; o->s_xy_lo = h[4]; o->s_xy_hi = h[5];
        memcpy(&o->s_sqrt, &h[6], sizeof(double));
        memcpy(&o->s_js, &h[7], sizeof(double));
    }
    return ZK_OK;
}

}  // namespace zk
