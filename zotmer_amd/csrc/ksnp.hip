// ksnp.hip -- `zot ksnp` (zotmer/commands/ksnp.py: ksnp, hamming, levenshtein): the k-mers of a set that are candidate SNPs.
//
// With J = (K - 1) / 2 a k-mer x is cut into a prefix x >> 2(J + 1) (the top K - J - 1 bases), a middle base (x >> 2J) & 3 and a
// tail of J bases.  The set is ascending, so the k-mers of one prefix -- a group -- are one contiguous range of it.
//   * zk_ksnp_flank (the default mode): x is kept iff one of its three middle-base variants x ^ (b << 2J) is in the set.
//     ksnp_flank_kernel makes the three searches from the key directory of search.hpp and writes one ballot word per wave; the
//     kept entries leave through compact.hpp.  No atomics.
//   * zk_ksnp_components (-H, -L): inside each group every pair at distance <= d is joined, and a connected component is kept
//     iff its members carry two different middle bases.  The reference tests all pairs of a group; so does this, every
//     unordered pair ONCE, by group size:
//        1                      never looked at (ksnp_init_kernel leaves it its own component);
//        2 .. KS_WAVE_MAX       one wave per group, members and parents in LDS (ksnp_group_kernel<64, 64>);
//        .. KS_LDS_MAX          one workgroup per group, the same kernel (ksnp_group_kernel<256, 1024>);
//        above                  cut into tiles of KS_PAIR_TILE members, one workgroup per (i-tile <= j-tile) pair over all large
//                               groups at once, parents in global memory (ksnp_pair_kernel).
//     In the LDS kernels member i meets the members i + 1 .. i + s / 2 (cyclically; at an even size the last offset belongs to
//     the lower half only): s (s - 1) / 2 tests, the same number for every member.
//     Joins are lock-free unions on a u32 parent array: the larger root is hooked under the smaller by compare-and-swap.  Only
//     roots are ever swapped, so a parent changes once, a stale read of "i is a root" fails its swap and learns the real
//     parent, and every retry starts lower than the last.  The root of a finished component is its smallest member whatever
//     the schedule.  Then ksnp_mask_kernel points every member at its root and ORs its middle-base bit into the root's mask,
//     and the members whose root has two bits leave through compact.hpp.  Nothing waits on another workgroup.
//   * basics.lev of two k-mers of one group is that of their low J + 1 <= 16 bases (a common prefix changes nothing).  It is
//     computed bit-parallel (Myers 1999, one 32-bit word a column): a thread keeps the four match masks of its own member in
//     registers and advances one column per base of the other.  basics.lev is NOT symmetric (see KsPattern): the member that
//     comes first in the list is the pattern, so where the cyclic order of an LDS kernel meets a member from above, the
//     masks are built from the other one.
#include "internal.hpp"
#include "compact.hpp"
#include "search.hpp"

namespace zk {

constexpr int KS_WAVE_MAX = 64, KS_LDS_MAX = 1024, KS_PAIR_TILE = 256;
static_assert(KS_WAVE_MAX == ZK_KSNP_WAVE_GROUP && KS_LDS_MAX == ZK_KSNP_LDS_GROUP && KS_PAIR_TILE == ZK_KSNP_PAIR_TILE,
              "the sizes include/zotk.h publishes");

// ---------------------------------------------------------------------------------------
// the default mode
// ---------------------------------------------------------------------------------------
// word w of `kept` = the ballot of the entries [64 w, 64 w + 64)
__global__ __launch_bounds__(256) void ksnp_flank_kernel(const u64* __restrict__ k, u32 n, int K, int T, KeyDir d, u64* __restrict__ kept) {
    const u64 words = ((u64)n + 63) >> 6;
    for (u64 w = (u64)blockIdx.x * 4 + (threadIdx.x >> 6); w < words; w += (u64)gridDim.x * 4) {
        const u64 i = (w << 6) + (threadIdx.x & 63);
        bool f = false;
        if (i < n) {
            const u64 x = k[i];
            if (K == 32 || (x >> (2 * K)) == 0) {          // anything else is no k-mer and has no bucket
#pragma unroll
                for (u64 b = 1; b < 4; b++) {
                    const u64 q = x ^ (b << T);
                    const u32 at = dir_lower(k, d, q);
                    f |= at < n && k[at] == q;
                }
            }
        }
        const u64 m = __ballot(f);
        if ((threadIdx.x & 63) == 0) kept[w] = m;
    }
}

struct KsnpBallot {
    const u64* k; const u64* kept; u64* out;
    __device__ bool flag(u64 i) const { return (kept[i >> 6] >> (i & 63)) & 1ull; }
    __device__ void store(u64 pos, u64 i) const { out[pos] = k[i]; }
};

// the compaction both modes end with: the capacity convention of include/zotk.h
template <class P>
static int ksnp_emit(zk_ctx* c, const P& p, uint64_t n, uint64_t cap, uint64_t* n_out, const char* who) {
    u64* cnt;
    ZK_TRY(compact_count(c, p, n, &cnt, n_out));
    if (*n_out > cap) return no_room(c, who, "k-mers", *n_out, cap);
    ZK_TRY(compact_write(c, p, n, cnt));
    return check_device_error(c);
}

static int ksnp_flank(zk_ctx* c, const u64* k, uint64_t n, int K, u64* out, uint64_t cap, uint64_t* n_out) {
    const int T = 2 * ((K - 1) / 2);
    int bits = 1;
    while (bits < 26 && (8ull << bits) < n) bits++;
    if (bits > 2 * K) bits = 2 * K;
    const u64 nb = 1ull << bits, words = div_up(n, 64);
    const uint64_t need = 4 * (nb + 1) + 8 * words + 16 * div_up(n, CP_TILE) + (1 << 20);
    ZK_TRY(arena_require(c, need, need));
    u32* dir;
    u64* kept;
    ZK_TRY(arena_alloc(c, 4 * (nb + 1), (void**)&dir));
    ZK_TRY(arena_alloc(c, 8 * words, (void**)&kept));
    const KeyDir d{dir, 2 * K - bits};
    ZK_TRY(key_dir_build(c, k, (u32)n, d.shift, nb, dir));
    prof_begin(c, ZK_PROF_KSNP_FLANK, 8 * n + 8 * words);
    hipLaunchKernelGGL(ksnp_flank_kernel, dim3(grid_cap(c, div_up(words, 4), 16)), dim3(256), 0, c->stream, k, (u32)n, K, T, d, kept);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    return ksnp_emit(c, KsnpBallot{k, kept, out}, n, cap, n_out, "zk_ksnp_flank");
}

// ---------------------------------------------------------------------------------------
// the two distances, as "at most d"
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ u32 ks_ham(u64 x, u64 y) {
    const u64 z = x ^ y;
    return (u32)__popcll((z | (z >> 1)) & 0x5555555555555555ull);
}

// the even bits of v, packed: bit i of the result = bit 2 i of v
__device__ __forceinline__ u32 ks_even_bits(u32 v) {
    v &= 0x55555555u;
    v = (v | (v >> 1)) & 0x33333333u;
    v = (v | (v >> 2)) & 0x0f0f0f0fu;
    v = (v | (v >> 4)) & 0x00ff00ffu;
    return (v | (v >> 8)) & 0xffffu;
}

// What a thread keeps of its own member x for a distance: the member (Hamming), or the four match masks of its low m bases
// (bit i of e<c>: base i from the low end is c).
// near(y, first): the pair (x, y), x the member that comes first in the list when `first` is set, else y.
template <bool LEV> struct KsSide;
template <> struct KsSide<false> {
    u64 x;
    __device__ __forceinline__ KsSide(u64 x_, int) : x(x_) {}
    __device__ __forceinline__ bool near(u64 y, bool, int, u32 d) const { return ks_ham(x, y) <= d; }
};
// basics.lev starts its table from a row of zeros: bases at the end of the second k-mer may be left out for nothing.  It is
// the least edit distance between the first k-mer and a leading part of the second -- Myers' search form, the first k-mer the
// pattern and the second the text, both read from the last base on -- and it is not symmetric: the reference passes the
// k-mer that comes first in the list first.
struct KsPattern {
    u32 e0, e1, e2, e3;
    __device__ __forceinline__ KsPattern(u64 x, int m) {
        const u32 full = (1u << m) - 1, lo = ks_even_bits((u32)x), hi = ks_even_bits((u32)x >> 1);
        e0 = ~hi & ~lo & full; e1 = ~hi & lo & full; e2 = hi & ~lo & full; e3 = hi & lo & full;
    }
    // Column t of the table is base t of y; pv / mv = the rows where the column's vertical step is +1 / -1, the score follows
    // row m.  The bits above m never reach the bits below: carries and shifts only go up.
    __device__ __forceinline__ u32 distance(u64 y, int m) const {
        const u32 top = 1u << (m - 1);
        u32 pv = ~0u, mv = 0, score = (u32)m, w = (u32)y;
#pragma unroll 1
        for (int t = 0; t < m; t++, w >>= 2) {
            const u32 c = w & 3u;
            const u32 eq = c == 0 ? e0 : c == 1 ? e1 : c == 2 ? e2 : e3;
            const u32 xv = eq | mv;
            const u32 xh = (((eq & pv) + pv) ^ pv) | eq;
            u32 ph = mv | ~(xh | pv);
            u32 mh = pv & xh;
            score += (ph & top) ? 1u : 0u;
            score -= (mh & top) ? 1u : 0u;
            ph <<= 1;          // row 0 is all zeros: nothing comes in from above
            mh <<= 1;
            pv = mh | ~(xv | ph);
            mv = ph & xv;
        }
        return score;
    }
};
template <> struct KsSide<true> {
    u64 x;
    KsPattern mine;
    __device__ __forceinline__ KsSide(u64 x_, int m) : x(x_), mine(x_, m) {}
    __device__ __forceinline__ bool near(u64 y, bool first, int m, u32 d) const {
        return (first ? mine.distance(y, m) : KsPattern(y, m).distance(x, m)) <= d;
    }
};

// ---------------------------------------------------------------------------------------
// lock-free union-find: parent[i] <= i, a root has parent[i] == i, and a parent is written once, by the swap that hooks a root
// ---------------------------------------------------------------------------------------
template <int SCOPE>
__device__ __forceinline__ u32 ks_find(const u32* parent, u32 i) {
    for (;;) {
        const u32 p = __hip_atomic_load(parent + i, __ATOMIC_RELAXED, SCOPE);
        if (p == i) return i;
        i = p;
    }
}
template <int SCOPE>
__device__ __forceinline__ void ks_union(u32* parent, u32 a, u32 b) {
    for (;;) {
        a = ks_find<SCOPE>(parent, a);
        b = ks_find<SCOPE>(parent, b);
        if (a == b) return;
        if (a < b) { const u32 t = a; a = b; b = t; }
        u32 expect = a;          // a > b: hook a under b, if a is still a root
        if (__hip_atomic_compare_exchange_strong(parent + a, &expect, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE)) return;
        a = expect;              // it was hooked meanwhile, under something smaller: go on from there
    }
}

// ---------------------------------------------------------------------------------------
// the passes of zk_ksnp_components
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ksnp_init_kernel(const u64* __restrict__ k, u32 n, int T, u32* __restrict__ parent, u32* __restrict__ mask) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        parent[i] = (u32)i;
        mask[i] = 1u << ((u32)(k[i] >> T) & 3u);
    }
}

// the first entries of the groups of two or more (compact.hpp)
struct KsnpHeads {
    const u64* k; u64 n; int S; u32* heads;
    __device__ bool flag(u64 i) const {
        const u64 p = k[i] >> S;
        return (i == 0 || (k[i - 1] >> S) != p) && i + 1 < n && (k[i + 1] >> S) == p;
    }
    __device__ void store(u64 pos, u64 i) const { heads[pos] = (u32)i; }
};

struct KsnpLists {
    u32 *size;                         // of every group of KsnpHeads
    u32 *med_start, *med_size;         // the groups above KS_WAVE_MAX, in no order
    u32 *big_start, *big_size;         // ... above KS_LDS_MAX
    u32 *n_med, *n_big;
    u32 cap_med, cap_big;              // more than a sorted list can hold: an append beyond them is dropped, not written
};

// a thread per group: where it ends, and which kernel takes it
__global__ __launch_bounds__(256) void ksnp_classify_kernel(const u64* __restrict__ k, u32 n, int S, const u32* __restrict__ heads, u32 n_groups,
                                                            KsnpLists L) {
    for (u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x; g < n_groups; g += (u64)gridDim.x * blockDim.x) {
        const u64 a = heads[g], p = k[a] >> S;
        // a + 1 belongs to the group; a group that reaches a + KS_WAVE_MAX is searched to the end of the list
        u64 lo = a + 2, hi = a + KS_WAVE_MAX < n ? a + KS_WAVE_MAX : n;
        if (a + KS_WAVE_MAX < n && (k[a + KS_WAVE_MAX] >> S) == p) { lo = a + KS_WAVE_MAX + 1; hi = n; }
        const u64 end = partition_point(lo, hi, [&](u64 i) { return (k[i] >> S) == p; });
        const u32 s = (u32)(end - a);
        L.size[g] = s;
        if (s > (u32)KS_LDS_MAX) {
            const u32 at = atomicAdd(L.n_big, 1u);
            if (at < L.cap_big) { L.big_start[at] = (u32)a; L.big_size[at] = s; }
        } else if (s > (u32)KS_WAVE_MAX) {
            const u32 at = atomicAdd(L.n_med, 1u);
            if (at < L.cap_med) { L.med_start[at] = (u32)a; L.med_size[at] = s; }
        }
    }
}

// One workgroup per group of at most MAXG members (others are skipped: they are another launch's): all pairs, unions in LDS,
// then parent[member] = the group's root of it.
template <int BLOCK, int MAXG, bool LEV>
__global__ __launch_bounds__(BLOCK) void ksnp_group_kernel(const u64* __restrict__ k, int m, u32 d, const u32* __restrict__ starts,
                                                           const u32* __restrict__ sizes, u32 n_groups, u32* __restrict__ parent) {
    __shared__ u64 s_k[MAXG];
    __shared__ u32 s_p[MAXG];
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    const u32 tid = threadIdx.x;
    for (u32 g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const u32 s = sizes[g], a = starts[g];
        if (s < 2 || s > (u32)MAXG) continue;          // the same for the whole workgroup
        for (u32 i = tid; i < s; i += BLOCK) { s_k[i] = k[a + i]; s_p[i] = i; }
        __syncthreads();
        const u32 half = s >> 1;
        for (u32 i = tid; i < s; i += BLOCK) {
            const KsSide<LEV> mine(s_k[i], m);
            const u32 last = ((s & 1u) == 0 && i >= half) ? half - 1 : half;
            u32 j = i;
            for (u32 o = 1; o <= last; o++) {
                j = j + 1 == s ? 0 : j + 1;
                if (mine.near(s_k[j], i < j, m, d)) ks_union<WG>(s_p, i, j);
            }
        }
        __syncthreads();
        for (u32 i = tid; i < s; i += BLOCK) {
            const u32 r = ks_find<WG>(s_p, i);
            if (r != i) parent[a + i] = a + r;
        }
        __syncthreads();          // the next group restages
    }
}

// tiles[q] = the (i-tile <= j-tile) pairs of large group q
__global__ __launch_bounds__(256) void ksnp_tiles_kernel(const u32* __restrict__ big_size, u32 n_big, u64* __restrict__ tiles) {
    for (u32 q = blockIdx.x * blockDim.x + threadIdx.x; q < n_big; q += gridDim.x * blockDim.x) {
        const u64 t = ((u64)big_size[q] + KS_PAIR_TILE - 1) / KS_PAIR_TILE;
        tiles[q] = t * (t + 1) / 2;
    }
}

// Work item w of [0, total): the pair (ti <= tj) number w - incl[g - 1] of large group g, pairs numbered tj (tj + 1) / 2 + ti.
// A thread holds one member of the i-tile and meets the staged j-tile (above its own place only, where the two are one tile).
template <bool LEV>
__global__ __launch_bounds__(KS_PAIR_TILE) void ksnp_pair_kernel(const u64* __restrict__ k, int m, u32 d, const u32* __restrict__ big_start,
                                                                 const u32* __restrict__ big_size, const u64* __restrict__ incl, u32 n_big,
                                                                 u64 total, u32* __restrict__ parent) {
    __shared__ u64 s_j[KS_PAIR_TILE];
    constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
    const u32 tid = threadIdx.x;
    for (u64 w = blockIdx.x; w < total; w += gridDim.x) {
        const u32 g = partition_point(0u, n_big - 1, [&](u32 q) { return incl[q] <= w; });
        const u64 q = w - (g ? incl[g - 1] : 0);
        const u32 a = big_start[g], s = big_size[g];
        u64 tj = (u64)((sqrt(8.0 * (double)q + 1.0) - 1.0) * 0.5);
        while (tj * (tj + 1) / 2 > q) tj--;
        while ((tj + 1) * (tj + 2) / 2 <= q) tj++;
        const u64 ti = q - tj * (tj + 1) / 2;
        const u32 i0 = (u32)ti * KS_PAIR_TILE, j0 = (u32)tj * KS_PAIR_TILE;
        const u32 ci = s - i0 < (u32)KS_PAIR_TILE ? s - i0 : (u32)KS_PAIR_TILE;
        const u32 cj = s - j0 < (u32)KS_PAIR_TILE ? s - j0 : (u32)KS_PAIR_TILE;
        __syncthreads();          // the item before is done with s_j
        if (tid < cj) s_j[tid] = k[a + j0 + tid];
        __syncthreads();
        if (tid < ci) {
            const u32 gi = a + i0 + tid;
            const KsSide<LEV> mine(k[gi], m);
            for (u32 jj = ti == tj ? tid + 1 : 0; jj < cj; jj++)
                if (mine.near(s_j[jj], true, m, d)) ks_union<AG>(parent, gi, a + j0 + jj);
        }
    }
}

// every member points at its root, and the root's mask collects the middle bases of its members
__global__ __launch_bounds__(256) void ksnp_mask_kernel(const u64* __restrict__ k, u32 n, int T, u32* __restrict__ parent, u32* __restrict__ mask) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u32 p = parent[i];
        if (p == (u32)i) continue;
        const u32 r = ks_find<__HIP_MEMORY_SCOPE_AGENT>(parent, p);
        if (r != p) parent[i] = r;
        atomicOr(&mask[r], 1u << ((u32)(k[i] >> T) & 3u));
    }
}

// kept: the members of a component with two middle bases or more
struct KsnpKept {
    const u64* k; const u32* parent; const u32* mask; u64* out;
    __device__ bool flag(u64 i) const { return __popc(mask[parent[i]]) >= 2; }
    __device__ void store(u64 pos, u64 i) const { out[pos] = k[i]; }
};

template <bool LEV>
static int ksnp_pairs(zk_ctx* c, const u64* k, uint64_t n, int m, u32 d, const u32* heads, u32 n_groups, const KsnpLists& L, u64* tiles,
                      u32* parent) {
    // the records of the tag: the first one carries the bytes (16 per k-mer: the key read, the parent and the mask written)
    prof_begin(c, ZK_PROF_KSNP_PAIRS, 16 * n);
    hipLaunchKernelGGL((ksnp_group_kernel<64, KS_WAVE_MAX, LEV>), dim3(grid_cap(c, n_groups, 128)), dim3(64), 0, c->stream, k, m, d, heads,
                       L.size, n_groups, parent);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    u32 n_med = (u32)c->h_scalars->ksnp_lists[0], n_big = (u32)c->h_scalars->ksnp_lists[1];
    if (n_med > L.cap_med) n_med = L.cap_med;
    if (n_big > L.cap_big) n_big = L.cap_big;
    if (n_med) {
        prof_begin(c, ZK_PROF_KSNP_PAIRS, 0);
        hipLaunchKernelGGL((ksnp_group_kernel<256, KS_LDS_MAX, LEV>), dim3(grid_cap(c, n_med, 16)), dim3(256), 0, c->stream, k, m, d,
                           L.med_start, L.med_size, n_med, parent);
        prof_end(c);
        ZK_HIP(c, hipGetLastError());
    }
    if (n_big) {
        hipLaunchKernelGGL(ksnp_tiles_kernel, dim3(grid_cap(c, div_up(n_big, 256), 16)), dim3(256), 0, c->stream, L.big_size, n_big, tiles);
        ZK_HIP(c, hipGetLastError());
        uint64_t total;
        ZK_TRY(scan_total(c, tiles, n_big, &total));
        prof_begin(c, ZK_PROF_KSNP_PAIRS, 0);
        hipLaunchKernelGGL(ksnp_pair_kernel<LEV>, dim3(grid_cap(c, total, 32)), dim3(KS_PAIR_TILE), 0, c->stream, k, m, d, L.big_start,
                           L.big_size, tiles, n_big, total, parent);
        prof_end(c);
        ZK_HIP(c, hipGetLastError());
    }
    return ZK_OK;
}

static int ksnp_components(zk_ctx* c, const u64* k, uint64_t n, int K, int metric, u32 d, u64* out, uint64_t cap, uint64_t* n_out) {
    const int J = (K - 1) / 2, S = 2 * (J + 1), T = 2 * J;
    const uint64_t max_med = n / (KS_WAVE_MAX + 1) + 1, max_big = n / (KS_LDS_MAX + 1) + 1;
    const uint64_t need = 8 * n + 8 * (n / 2 + 1) + 8 * max_med + 16 * max_big + 32 * div_up(n, CP_TILE) + (1 << 20);
    ZK_TRY(arena_require(c, need, need));
    u32 *parent, *mask, *heads;
    ZK_TRY(arena_alloc(c, 4 * n, (void**)&parent));
    ZK_TRY(arena_alloc(c, 4 * n, (void**)&mask));
    hipLaunchKernelGGL(ksnp_init_kernel, dim3(grid_cap(c, div_up(n, 256), 16)), dim3(256), 0, c->stream, k, (u32)n, T, parent, mask);
    ZK_HIP(c, hipGetLastError());

    u64* cnt;
    uint64_t n_groups = 0;
    ZK_TRY(arena_alloc(c, 4 * (n / 2 + 1), (void**)&heads));
    const KsnpHeads hp{k, (u64)n, S, heads};
    ZK_TRY(compact_count(c, hp, n, &cnt, &n_groups));
    if (n_groups) {
        ZK_TRY(compact_write(c, hp, n, cnt));
        KsnpLists L;
        u64* tiles;
        ZK_TRY(arena_alloc(c, 4 * n_groups, (void**)&L.size));
        ZK_TRY(arena_alloc(c, 4 * max_med, (void**)&L.med_start));
        ZK_TRY(arena_alloc(c, 4 * max_med, (void**)&L.med_size));
        ZK_TRY(arena_alloc(c, 4 * max_big, (void**)&L.big_start));
        ZK_TRY(arena_alloc(c, 4 * max_big, (void**)&L.big_size));
        ZK_TRY(arena_alloc(c, 8 * max_big, (void**)&tiles));
        L.n_med = (u32*)&c->d_scalars->ksnp_lists[0];
        L.n_big = (u32*)&c->d_scalars->ksnp_lists[1];
        L.cap_med = (u32)max_med;
        L.cap_big = (u32)max_big;
        ZK_HIP(c, hipMemsetAsync(c->d_scalars->ksnp_lists, 0, sizeof(c->d_scalars->ksnp_lists), c->stream));
        hipLaunchKernelGGL(ksnp_classify_kernel, dim3(grid_cap(c, div_up(n_groups, 256), 16)), dim3(256), 0, c->stream, k, (u32)n, S, heads,
                           (u32)n_groups, L);
        ZK_HIP(c, hipGetLastError());
        ZK_TRY(fetch(c, &c->h_scalars->ksnp_lists));
        ZK_TRY(stream_sync(c));
        if (metric == ZK_KSNP_LEVENSHTEIN) ZK_TRY((ksnp_pairs<true>(c, k, n, J + 1, d, heads, (u32)n_groups, L, tiles, parent)));
        else ZK_TRY((ksnp_pairs<false>(c, k, n, J + 1, d, heads, (u32)n_groups, L, tiles, parent)));
        hipLaunchKernelGGL(ksnp_mask_kernel, dim3(grid_cap(c, div_up(n, 256), 16)), dim3(256), 0, c->stream, k, (u32)n, T, parent, mask);
        ZK_HIP(c, hipGetLastError());
    }
    return ksnp_emit(c, KsnpKept{k, parent, mask, out}, n, cap, n_out, "zk_ksnp_components");
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_ksnp_flank(zk_ctx* c, const uint64_t* d_kmers, uint64_t n, int K, uint64_t* d_out, uint64_t cap, uint64_t* n_out) {
    ZK_ARGS(c, n_out && K >= 1 && K <= 32 && n < 0xFFFFFFFFull && (n == 0 || d_kmers) && (cap == 0 || d_out));
    *n_out = 0;
    if (n == 0) return ZK_OK;
    arena_reset(c);
    return ksnp_flank(c, (const u64*)d_kmers, n, K, (u64*)d_out, cap, n_out);
}

int zk_ksnp_components(zk_ctx* c, const uint64_t* d_kmers, uint64_t n, int K, int metric, uint64_t d, uint64_t* d_out, uint64_t cap,
                       uint64_t* n_out) {
    ZK_ARGS(c, n_out && K >= 1 && K <= 32 && n < 0xFFFFFFFFull && (metric == ZK_KSNP_HAMMING || metric == ZK_KSNP_LEVENSHTEIN) &&
                   (n == 0 || d_kmers) && (cap == 0 || d_out));
    *n_out = 0;
    if (n == 0) return ZK_OK;
    arena_reset(c);
    return ksnp_components(c, (const u64*)d_kmers, n, K, metric, (u32)(d < (uint64_t)K ? d : (uint64_t)K), (u64*)d_out, cap, n_out);
}

}  // extern "C"
