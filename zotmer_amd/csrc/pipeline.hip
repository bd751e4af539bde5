// pipeline.hip -- the device-resident `zot kmerize` batch (zotmer/commands/kmerize.py:450-562)
// and the k-way merge of `zot merge` (zotmer/commands/merge.py:165-253).
//
// kmerize, reference: reads(..., both=True) -> kmersList emits x AND rc(x) for every valid
// window (commands/kmerize.py:490, library/reads.py:113-114); KmerAccumulator2 buffers them,
// radix-sorts and run-length counts (:370-437).  The result is strand-symmetric:
// count(x) == count(rc x), and a palindrome (x == rc x, even K only) is counted twice per window.
//
// Here (default, ZK_KMERIZE_CANONICAL): sort only ONE key per window, c = min(x, rc x) -- half
// the sort volume --, run-length count it, then rebuild both strands exactly: the pairs
// (rc c, n) are sorted by key and union-summed with (c, n); a palindrome meets itself there and
// gets n + n, which is what two emissions per window give.  Any deterministic representative
// would do because it never leaves the device.  ZK_KMERIZE_BOTH sorts both strands directly
// (the literal reference path; kept as a cross-check and for tests).
// -D (murmer subsample, :494-509) is a per-VALUE predicate, so it is applied to the counted set
// instead of to every instance; acgt is taken before any filtering, as in the reference (:492-493).
#include <string.h>

#include <vector>

#include "internal.hpp"

namespace zk {

__global__ void mirror_kernel(const u64* __restrict__ c, const u32* __restrict__ n, u64 m, int K, u64* __restrict__ r,
                              u32* __restrict__ v) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (u64)gridDim.x * blockDim.x) {
        r[i] = revcomp(K, c[i]);
        v[i] = n[i];
    }
}

// ---- the mirror list by groups (see mirror_union) ---------------------------------------------------------
constexpr int MIRROR_GROUP_BITS = 18;      // 9 bases: 2^18 groups, tables of 4 MB
constexpr int MIRROR_GROUP_BASES = MIRROR_GROUP_BITS / 2;

// start[g] = first index whose top gbits bits are >= g (g = 2^gbits: n)
__global__ void mirror_bounds_kernel(const u64* __restrict__ c, u64 n, int K, int gbits, u64* __restrict__ start) {
    const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g > (1u << gbits)) return;
    const u64 want = (u64)g << (2 * K - gbits);
    u64 lo = 0, hi = n;
    if (g == (1u << gbits)) lo = n;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (c[mid] < want) lo = mid + 1; else hi = mid;
    }
    start[g] = lo;
}

// size_v[v] = size of the group whose mirrored keys end in v, i.e. group g = rc(v) (gbits / 2 bases)
__global__ void mirror_sizes_kernel(const u64* __restrict__ start, int gbits, u64* __restrict__ size_v) {
    const u32 v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= (1u << gbits)) return;
    const u32 g = (u32)revcomp(gbits / 2, (u64)v);
    size_v[v] = start[g + 1] - start[g];
}

// place[g] = (where the mirrored words of group g go: the sizes before v = rc(g), inclusive scan minus the group's own) - start[g]:
// the word of entry i of the list goes to place[g] + i.  Indexed by g, the order the copy walks the list in.
__global__ void mirror_place_kernel(const u64* __restrict__ start, const u64* __restrict__ incl_v, int gbits, u64* __restrict__ place) {
    const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (1u << gbits)) return;
    const u32 v = (u32)revcomp(gbits / 2, (u64)g);
    place[g] = incl_v[v] - (start[g + 1] - start[g]) - start[g];
}

// pack > 0: r[pos] = (rc(c) << pack) | n -- one word per pair (v is not written); the caller has checked that every n fits.
// mh: the digit counts of the passes that will sort the words above their group bits, taken on the way (it writes every word anyway).
__global__ __launch_bounds__(256) void mirror_copy_kernel(const u64* __restrict__ c, const u32* __restrict__ n, u64 m, int K, int gbits,
                                                          const u64* __restrict__ place, u64* __restrict__ r, u32* __restrict__ v, int pack, MirrorHist mh) {
    __shared__ u32 bins[4 * 512];
    const bool hist = pack && mh.passes > 0;
    if (hist) {
        for (int q = threadIdx.x; q < 4 * 512; q += blockDim.x) bins[q] = 0;
        __syncthreads();
    }
    const int sh = 2 * K - gbits;
    // four entries of a thread in flight at a time
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i0 = (u64)blockIdx.x * blockDim.x + threadIdx.x; i0 < m; i0 += 4 * stride) {
        u64 x4[4];
        u32 n4[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const u64 i = i0 + q * stride;
            x4[q] = i < m ? c[i] : 0;
            n4[q] = i < m ? n[i] : 0;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const u64 i = i0 + q * stride;
            if (i >= m) break;
            const u64 x = x4[q];
            const u64 pos = place[(u32)(x >> sh)] + i;
            if (pack) {
                const u64 mw = (revcomp(K, x) << pack) | (u64)n4[q];
                r[pos] = mw;
                if (hist) {
#pragma unroll
                    for (int p = 0; p < 4; p++)
                        if (p < mh.passes) atomicAdd(&bins[p * 512 + ((u32)(mw >> mh.shift[p]) & ((1u << mh.bits[p]) - 1u))], 1u);
                }
            } else { r[pos] = revcomp(K, x); v[pos] = n4[q]; }
        }
    }
    if (hist) {
        __syncthreads();
        for (int q = threadIdx.x; q < mh.passes * 512; q += blockDim.x)
            if (bins[q]) atomicAdd(&mh.raw[q], (u64)bins[q]);
    }
}

__global__ void widen_kernel(const u32* __restrict__ in, u64* __restrict__ out, u64 m) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (u64)gridDim.x * blockDim.x) out[i] = in[i];
}

int widen_counts(zk_ctx* c, const u32* in, u64* out, uint64_t n) {
    if (n == 0) return ZK_OK;
    hipLaunchKernelGGL(widen_kernel, dim3(grid_cap(c, div_up(n, 256), 16)), dim3(256), 0, c->stream, in, out, (u64)n);
    ZK_HIP(c, hipGetLastError());
    return ZK_OK;
}

// (key, n) of the side list -> the pair itself and its mirror
__global__ void side_expand_kernel(const u64* __restrict__ k, const u32* __restrict__ n, u64 m, int K, u64* __restrict__ pk,
                                   u32* __restrict__ pv) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (u64)gridDim.x * blockDim.x) {
        const u64 x = k[i];
        const u32 v = n[i];
        pk[2 * i] = x; pv[2 * i] = v;
        pk[2 * i + 1] = revcomp(K, x); pv[2 * i + 1] = v;
    }
}

static int ilog2_ceil(uint64_t x) { int b = 0; while ((1ull << b) < x && b < 63) b++; return b; }

// Spare bits above a 2K-bit k-mer in a 64-bit word: room for the count when pairs travel as one word.  Worth it from 10
// bits up (K <= 27); 0 = keep key and count apart.
static int pack_bits_for(int K) {
    const int spare = 64 - 2 * K;
    return spare >= 10 ? (spare > 31 ? 31 : spare) : 0;
}

__global__ void max_u32_kernel(const u32* __restrict__ v, u64 n, u32* out) {
    u32 m = 0;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) m = v[i] > m ? v[i] : m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u32 t = (u32)__shfl_xor((int)m, o, 64); m = t > m ? t : m; }
    if ((threadIdx.x & 63) == 0 && m > __hip_atomic_load(out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(out, m);
}

static int max_u32(zk_ctx* c, const u32* v, uint64_t n, uint64_t* out) {
    u32* d = (u32*)&c->d_scalars->max_u32;
    ZK_HIP(c, hipMemsetAsync(d, 0, sizeof(u64), c->stream));
    if (n) {
        hipLaunchKernelGGL(max_u32_kernel, dim3(grid_cap(c, div_up(n, 256), 16)), dim3(256), 0, c->stream, v, (u64)n, d);
        ZK_HIP(c, hipGetLastError());
    }
    ZK_TRY(fetch(c, &c->h_scalars->max_u32));
    ZK_TRY(stream_sync(c));
    *out = c->h_scalars->max_u32 & 0xffffffffull;
    return ZK_OK;
}

// how many of the n keys are their own reverse complement (even K only; at odd K none is)
__global__ void palindromes_kernel(const u64* __restrict__ v, u64 n, int K, unsigned long long* out) {
    u32 m = 0;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) m += revcomp(K, v[i]) == v[i] ? 1u : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m += (u32)__shfl_xor((int)m, o, 64);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(out, (unsigned long long)m);
}

static int count_palindromes(zk_ctx* c, const u64* v, uint64_t n, int K, uint64_t* out) {
    ZK_HIP(c, hipMemsetAsync(&c->d_scalars->palindromes, 0, sizeof(u64), c->stream));
    if (n) {
        hipLaunchKernelGGL(palindromes_kernel, dim3(grid_cap(c, div_up(n, 256), 16)), dim3(256), 0, c->stream, v, (u64)n, K, (unsigned long long*)&c->d_scalars->palindromes);
        ZK_HIP(c, hipGetLastError());
    }
    ZK_TRY(fetch(c, &c->h_scalars->palindromes));
    ZK_TRY(stream_sync(c));
    *out = c->h_scalars->palindromes;
    return ZK_OK;
}

// ---- the predicates and layouts the stages of a batch share ---------------------------------------------------------------------
static uint64_t align256(uint64_t x) { return (x + 255) & ~255ull; }

// The k-mers are long enough for the mirror image of a counted list to be grouped by a copy (2^18 groups, then only the bits above
// sorted: mirror_union) ...
static bool mirror_groups(int K) { return 2 * K >= MIRROR_GROUP_BITS + 8; }
// ... and the list is long enough for the group tables to pay
static bool mirror_grouped(int K, uint64_t uc) { return mirror_groups(K) && uc >= (1ull << 16); }
// The mirror travels as words, (rc c << pack) | n, through the key kernel: grouped, and every count fits its field (pack > 0)
static bool mirror_as_words(int pack, int K, uint64_t uc) { return pack && mirror_grouped(K, uc); }

// The width of the count field of such words, or 0 when some count does not fit beside its k-mer (or pairs are not packed at all).
// max_count is the largest count if the route that counted knows it (have_max); only otherwise are the counts read for it.
static int mirror_pack(zk_ctx* c, int K, const u32* cnt, uint64_t uc, bool have_max, uint64_t max_count, int* pack) {
    *pack = 0;
    const int pk = c->packed_pairs ? pack_bits_for(K) : 0;
    if (!pk) return ZK_OK;
    if (!have_max) ZK_TRY(max_u32(c, cnt, uc, &max_count));
    if (max_count < (1ull << pk)) *pack = pk;
    return ZK_OK;
}

// Both strands from the counted canonical list (c, n), c ascending: the pairs (rc c, n) are sorted by key and union-summed
// with (c, n); a palindrome (c == rc c, even K) meets itself there and gets n + n -- two emissions per window, as the
// reference has them (commands/kmerize.py:490, library/reads.py:113-114).  rk / rk2 (8 bytes per entry) and rv / rv2 (4) are
// work buffers; start / dest tables come from the arena.
// pack > 0 (the caller knows every count is below 2^pack, and 2K + pack <= 64): the mirrored pairs travel as single words
// (rc c << pack | n) through the key kernel -- 16 bytes per pair and pass instead of 24 -- and the union reads them so.
static int mirror_union(zk_ctx* c, const u64* sorted, const u32* cnt, uint64_t uc, int K, u64* rk, u64* rk2, u32* rv, u32* rv2,
                        u64* out_k, u32* out_c, uint64_t cap, uint64_t* n_out, int pack = 0) {
    u64* sk; u32* sv;
    if (!mirror_as_words(pack, K, uc)) pack = 0;
    // As pairs (K >= 28, or counts too large for the field) and long enough: the mirrored keys are all different, so the tile sort
    // applies -- three passes over the top bits, reverse-complemented on load, then the rest in LDS -- instead of the grouping copy
    // and five passes.  Should a tile decline (it cannot on distinct keys unless they crowd under one prefix), the passes do it all.
    const int ttop = (!pack && c->tile_sort) ? tile_sort_top_bits(uc, 2 * K, sort_pairs_rbits(c)) : 0;
    if (ttop) {
        bool declined = false;
        ZK_TRY(sort_pairs_mirrored(c, sorted, cnt, rk, rk2, rv, rv2, uc, K, &sk, &sv, 2 * K - ttop));
        ZK_TRY(tile_sort(c, sk, sv, uc, 2 * K, ttop, &declined));
        if (declined) ZK_TRY(sort_pairs_mirrored(c, sorted, cnt, rk, rk2, rv, rv2, uc, K, &sk, &sv));
    } else
    if (mirror_grouped(K, uc)) {
        // The list (c, n) is sorted by c, so the k-mers that share their first 9 bases are contiguous -- and those are
        // exactly the mirrored keys rc(c) that share their LAST 9 bases, i.e. their low 18 bits.  The first two passes of
        // an LSD sort of the mirrored keys would only move these 2^18 groups around whole; one copy does it: group
        // boundaries by binary search, group order = order of the reversed-complemented prefix, then only the bits
        // above 18 are sorted.
        // As single words, and when the list is long enough for the tables to be small beside it: grouped by the first TWELVE bases
        // (2^24 groups; their bounds are 2^24 binary searches) -- one pass less over the words.
        int gbits = MIRROR_GROUP_BITS;
        if (pack && 2 * K - 24 >= 8 && uc >= (1ull << 26) && c->arena_size - c->arena_off > 3 * (8ull << 24) + (64ull << 20) + uc / 16) gbits = 24;
        const u32 groups = 1u << gbits;
        u64 *start, *incl, *place;
        ZK_TRY(arena_alloc(c, sizeof(u64) * ((uint64_t)groups + 1), (void**)&start));
        ZK_TRY(arena_alloc(c, sizeof(u64) * groups, (void**)&incl));
        ZK_TRY(arena_alloc(c, sizeof(u64) * groups, (void**)&place));
        // the digit counts of the passes that will sort the words above their group bits: taken by the copy (sort_keys_upper_counted)
        MirrorHist mh = {};
        if (pack && c->sort_variant == 3) {
            const PassPlan plan = sort_plan_upper(c, 2 * K + pack, gbits + pack);
            if (plan.passes <= 4 && sort_rbits(c) == 9) {
                ZK_TRY(arena_alloc(c, sizeof(u64) * MAX_PASSES * 512, (void**)&mh.raw));
                ZK_HIP(c, hipMemsetAsync(mh.raw, 0, sizeof(u64) * MAX_PASSES * 512, c->stream));
                mh.passes = plan.passes;
                for (int p = 0; p < plan.passes; p++) { mh.shift[p] = plan.shift[p]; mh.bits[p] = plan.bits[p]; }
            }
        }
        prof_begin(c, ZK_PROF_MIRROR, (pack ? 20 : 24) * uc);
        hipLaunchKernelGGL(mirror_bounds_kernel, dim3((groups + 256) / 256), dim3(256), 0, c->stream, sorted, (u64)uc, K, gbits, start);
        hipLaunchKernelGGL(mirror_sizes_kernel, dim3(groups / 256), dim3(256), 0, c->stream, (const u64*)start, gbits, incl);
        ZK_TRY(scan64_inclusive(c, incl, groups));
        hipLaunchKernelGGL(mirror_place_kernel, dim3(groups / 256), dim3(256), 0, c->stream, (const u64*)start, (const u64*)incl, gbits, place);
        hipLaunchKernelGGL(mirror_copy_kernel, dim3(grid_cap(c, div_up(uc, 256), 16)), dim3(256), 0, c->stream, sorted, cnt, (u64)uc, K, gbits, (const u64*)place, rk, rv, pack, mh);
        prof_end(c);
        ZK_HIP(c, hipGetLastError());
        if (pack) {
            if (mh.passes) ZK_TRY(sort_keys_upper_counted(c, rk, rk2, uc, 2 * K + pack, gbits + pack, mh.raw, &sk));
            else ZK_TRY(sort_keys_upper(c, rk, rk2, uc, 2 * K + pack, gbits + pack, &sk));
            return union_sum_packed_b(c, sorted, cnt, uc, sk, uc, pack, out_k, out_c, cap, n_out, (K & 1) != 0);
        }
        ZK_TRY(sort_pairs_upper(c, rk, rk2, rv, rv2, uc, 2 * K, MIRROR_GROUP_BITS, &sk, &sv));
    } else {
        // small inputs / short k-mers: the histogram and the first pass of the sort read (c, n) and reverse-complement on load
        ZK_TRY(sort_pairs_mirrored(c, sorted, cnt, rk, rk2, rv, rv2, uc, K, &sk, &sv));
    }
    // (odd K: no k-mer is its own reverse complement, and a canonical k-mer's mirror image is not canonical: the two lists share no key)
    return union_sum(c, sorted, cnt, uc, sk, sv, uc, out_k, out_c, 32, cap, n_out, nullptr, (K & 1) != 0);
}

// zk_mirror_expand: the strands of an already counted canonical list (multi-GPU: after the exchange)
int mirror_expand(zk_ctx* c, const u64* ck, const u32* cc, uint64_t n, int K, u64* out_k, u32* out_c, uint64_t cap, uint64_t* n_out) {
    *n_out = 0;
    if (K < 1 || K > 32) return fail(c, ZK_EINVAL, "K must be in 1..32 (got %d)", K);
    if (n == 0) return ZK_OK;
    arena_reset(c);
    const uint64_t a8 = align256(8 * n), a4 = align256(4 * n);
    int pack = 0;
    ZK_TRY(mirror_pack(c, K, cc, n, false, 0, &pack));
    // the mirrored pairs as single words (every count fits beside its k-mer): two word buffers, 16 bytes an entry; as pairs: 24
    const bool words = mirror_as_words(pack, K, n);
    const uint64_t wbytes = 2 * a8 + (words ? 0 : 2 * a4);
    const uint64_t need = wbytes + (9 << 20) + n / 8 + (words && n >= (1ull << 26) ? (480ull << 20) : 0);          // work buffers, group tables (2^24 groups of long lists), histograms, merge-path partition
    ZK_TRY(arena_require(c, need, need));
    char* w;
    ZK_TRY(arena_alloc(c, wbytes, (void**)&w));
    ZK_TRY(mirror_union(c, ck, cc, n, K, (u64*)w, (u64*)(w + a8), words ? nullptr : (u32*)(w + 2 * a8), words ? nullptr : (u32*)(w + 2 * a8 + a4), out_k, out_c,
                        cap, n_out, pack));
    return check_device_error(c);
}

// ---- one batch of zk_kmerize, in stages: plan, sort, count, strands ---------------------------------------------------------------
// Canonical mode counts the copies of a k-mer BEFORE the sort is finished -- three ways, tried in this order (zk_tune
// ZK_TUNE_EARLY_COLLAPSE picks one for tests):
//   (1) block dedupe: LSD passes over the TOP bits until the blocks of equal top bits are small, then an LDS hash table per
//       block counts the copies and leaves the block sorted (dedupe_blocks.hip::dedupe_kernel) -- two full-size passes on a
//       50 M-read batch, and the counted list is finished; dedupe_finish also prepares the mirror sort;
//   (2) collapse_kernel: LSD passes over the low bits until the copies are within a tile of each other, the next digit ranked
//       tile by tile with the run lengths counted in LDS, words sorted from that bit up;
//   (3) passes over the low bits until the copies are neighbours, a run-length pass, pairs above (count_runs).
// Reads that do not repeat their k-mers are counted tile by tile in LDS after passes over the top bits, or by a plain run-length
// pass over the sorted keys.  Then the strands are rebuilt (mirror_union, or straight from the blocks).  ZK_KMERIZE_BOTH: every
// bit of both strands sorted, then RLE (the literal path).
enum CountRoute {
    COUNT_TILES,           // top bits by passes, the rest sorted and counted tile by tile in LDS (tile_sort_count)
    COUNT_BLOCKS,          // (1)
    COUNT_FUSED,           // (2)
    COUNT_RUNS,            // (3)
    COUNT_SORTED,          // every bit sorted: a plain run-length pass
    COUNT_REPLAN           // nothing sorted: the caller plans the batch again for the keys of both strands
};

// the look before the sort (sort_stream): the keys whose top `bits` bits are this prefix (AAATCCTA.), declined at 0.6 distinct
constexpr double REPEAT_RATIO = 0.6;          // "the reads repeat their k-mers": at most this share of a sample is distinct
static StreamSample prefix_sample(int K, int bits) { return StreamSample{2 * K - bits, (uint64_t)(0x0D71C8E5u >> (32 - bits)), REPEAT_RATIO}; }

struct KmerizePlan {
    int K;
    bool both, canonical_only;
    int rb;                    // digit width of the key passes
    int pack;                  // count bits beside a k-mer where pairs travel as one word (0: key and count apart)
    int collapse_bit;          // low bits to sort before looking for runs (0: no early collapse)
    int fused_bit;             // > 0: the low passes stop here; the next digit is ranked tile by tile and counted by collapse_kernel
    int dedupe_bit;            // > 0: the passes sort these TOP bits, the blocks of equal top bits are counted in LDS tables
    bool tags;                 // ... and the last pass may write 32-bit tags instead of keys (at most 32 key bits below the blocks)
    int tile_top;              // the top bits to sort before the tile sort (0: switched off, or not worth it)
    int both_top;              // ... for the keys of both strands
    bool replan_pays;          // a declined look may ask for the both-strand tile plan
    bool look;                 // K >= 28: a look before the sort chooses between the tile route and the low-bit plan ...
    int look_bits;             // ... at the keys under a prefix of this many bits
    bool blocks_mirror;        // the block dedupe may write the mirrored words as well (if every count fits the field)
    bool blocks_strands;       // ... and at odd K the strands may be rebuilt block by block (strand_blocks.hip)
    bool blocks_unsorted;      // ... which sorts every block again: the dedupe then leaves them unsorted
    CountRoute low_route() const { return fused_bit ? COUNT_FUSED : collapse_bit ? COUNT_RUNS : COUNT_SORTED; }
};

// Stage 1, the plan: every route decision that the input's size and the knobs settle.  Pure: no HIP call, the context is only read.
static KmerizePlan plan_kmerize(const zk_ctx* c, uint64_t n_bytes, int K, bool both, bool canonical_only) {
    KmerizePlan p = {};
    p.K = K; p.both = both; p.canonical_only = canonical_only;
    const int rb = p.rb = sort_rbits(const_cast<zk_ctx*>(c));          // (reads sort_variant)
    p.pack = c->packed_pairs ? pack_bits_for(K) : 0;
    const int lg = ilog2_ceil(n_bytes);
    // low bits to sort before looking for runs: 2^b >= 8 x keys, a whole number of passes, and at least one pass left over
    if (!both && c->early_collapse) {
        const int b = rb * ((lg + 3 + rb - 1) / rb);
        if (b + rb / 2 < 2 * K) p.collapse_bit = b;
        if (p.collapse_bit >= 2 * rb && (c->early_collapse == 1 || c->early_collapse == 3) && p.pack) p.fused_bit = p.collapse_bit - rb;
    }
    // Better still while the blocks of keys that share b sorted bits are small enough for an LDS hash table (dedupe_kernel: at
    // most 32 K keys per block by the stream's length, at least 2 K so that the copies of a k-mer are spread over many
    // wavefronts): the passes then sort the TOP b bits, the table counts each block and leaves it sorted by the bits below --
    // config 2 is done after TWO passes.
    if (p.fused_bit && c->early_collapse == 1) {
        const int passes = lg > 15 ? (lg - 15 + rb - 1) / rb : 1;
        const int b = rb * passes;
        if (b < p.fused_bit + rb && b + rb / 2 < 2 * K && b <= 24 && (n_bytes >> b) >= 2048) p.dedupe_bit = b;
    }
    // tests (ZK_TUNE_DEDUPE_BITS): the same plan forced on an input of any size -- two passes, tags and blocks of a handful of keys
    // on inputs small enough for the oracle
    if (!both && c->early_collapse == 1 && c->dedupe_bits > 0 && p.pack && c->dedupe_bits % rb == 0 && c->dedupe_bits + rb / 2 < 2 * K &&
        c->dedupe_bits <= 24)
        p.dedupe_bit = c->dedupe_bits;
    p.tags = p.dedupe_bit && c->tag_words && 2 * K - p.dedupe_bit <= 32;
    p.tile_top = c->tile_sort ? tile_sort_top_bits(n_bytes, 2 * K, rb) : 0;
    p.both_top = tile_sort_top_bits(2 * n_bytes, 2 * K, rb);
    p.replan_pays = !canonical_only && c->tile_sort && p.both_top;
    // (K >= 28: no room for a count beside the k-mer, so no block dedupe; about 2^15 keys under the prefix)
    p.look_bits = lg - 15 < 2 ? 2 : (lg - 15 > 30 ? 30 : lg - 15);
    p.look = !p.dedupe_bit && !both && c->early_collapse && !pack_bits_for(K) && p.tile_top && p.look_bits < 2 * K;
    p.blocks_mirror = !canonical_only && p.pack && p.dedupe_bit == MIRROR_GROUP_BITS && mirror_groups(K);
    p.blocks_strands = p.blocks_mirror && (K & 1) && c->strand_blocks;
    p.blocks_unsorted = p.blocks_mirror && (K & 1) && (c->strand_blocks == 1 || c->strand_blocks >= 3);
    return p;
}

// the two sort buffers of a batch, cap_keys words each
struct SortBufs {
    u64 *a, *b;
    uint64_t cap_keys;
    u64* other(const void* p) const { return p == a ? b : a; }          // the buffer the keys at p are not in
};
// the caller's arrays
struct Output { u64* k; u32* c; uint64_t cap; uint64_t* n_out; };

// what the sort stage leaves
struct Sorted {
    u64* keys = nullptr;           // n keys in one sort buffer, sorted as far as `route` needs (32-bit tags when tags.written)
    u64* other = nullptr;          // the other sort buffer: free
    uint64_t n = 0;
    StreamTags tags;
    bool presampled = false;       // the look before the sort was conclusive: the block dedupe takes no sample of its own
    CountRoute route = COUNT_SORTED;
};

// Stage 2, the sort.  Writes both sort buffers; afterwards s->keys holds the keys and s->other is free.
// Block dedupe: sorting the top bits first only pays if the blocks can then be counted; an input that does not repeat its k-mers
// would have to start over.  So the histogram kernel sets aside four whole blocks (prefixes AAATCCTA.: every copy of their
// k-mers) and the sort is declined when they show little duplication -- at the price of one more histogram run.  A declined
// look changes the route: no collapse will pay either, every key goes to the end of the sort -- the top bits by passes, the rest
// tile by tile in LDS (tilesort.hip), or the low-bit plan without the tile sort.  Or, when both strands are wanted and the caller
// has the room (may_replan): COUNT_REPLAN, with nothing sorted yet -- sorting the keys of BOTH strands (twice the keys through
// three passes and the tile sort, which also counts) is then less work than the canonical keys, their mirrored list and the
// union of the two; the caller makes room and calls again with both_tiles.
// K >= 28 (no block dedupe: no room for a count beside the k-mer): reads that repeat their k-mers are collapsed after the low
// passes; reads that do not -- a share of a large genome at low coverage: config 5 -- go the other way: the top bits by passes,
// the rest tile by tile.  Which it is, a look at the keys under one prefix tells (about 2^15 of them: every copy of their k-mers),
// taken by the histogram kernel of the plan that is tried first.
static int sort_by_plan(zk_ctx* c, const KmerizePlan& p, const u8* stream, uint64_t n_bytes, const SortBufs& b, bool may_replan,
                        uint64_t acgt[4], Sorted* s) {
    const int K = p.K;
    StreamSrc src{stream, n_bytes, K, p.both ? ZK_KEYS_BOTH : ZK_KEYS_CANONICAL, 0};
    s->route = p.dedupe_bit ? COUNT_BLOCKS : p.low_route();
    bool sorted = false;
    if (p.dedupe_bit) {
        StreamSample smp = prefix_sample(K, p.dedupe_bit - 2);
        src.lo_bit = 2 * K - p.dedupe_bit; src.sample = &smp;
        if (p.tags) src.tags = &s->tags;          // sort_stream decides (K = 25 after two passes)
        const int rc = sort_stream(c, src, b.a, b.b, b.cap_keys, &s->n, acgt, &s->keys);
        if (rc < 0) return rc;
        src.sample = nullptr; src.tags = nullptr;
        if (rc == 1 && may_replan && p.replan_pays) { s->route = COUNT_REPLAN; return ZK_OK; }
        if (rc == 1) s->route = p.tile_top ? COUNT_TILES : p.low_route();
        else sorted = true;
        s->presampled = smp.seen >= 4096;          // the look was conclusive: no second one after the passes
    } else if (p.look) {
        StreamSample smp = prefix_sample(K, p.look_bits);
        smp.want_distinct = true;
        src.lo_bit = 2 * K - p.tile_top; src.sample = &smp;
        const int rc = sort_stream(c, src, b.a, b.b, b.cap_keys, &s->n, acgt, &s->keys);
        if (rc < 0) return rc;
        src.sample = nullptr;
        if (rc != 1) { s->route = COUNT_TILES; sorted = true; }          // (1: they repeat: the low-bit plan)
    }
    if (!sorted) {
        if (s->route == COUNT_TILES) { src.lo_bit = 2 * K - p.tile_top; src.hi_bit = 0; }
        else { src.lo_bit = 0; src.hi_bit = p.fused_bit ? p.fused_bit : p.collapse_bit; }
        ZK_TRY(sort_stream(c, src, b.a, b.b, b.cap_keys, &s->n, acgt, &s->keys));
    }
    s->other = b.other(s->keys);
    return ZK_OK;
}

// what a counting route leaves: the counted canonical list
enum ListPlace {
    IN_SORT_BUF,          // keys over the sorted keys, counts in the other sort buffer
    IN_AUX,               // in the aux region: both sort buffers are free (they belong to the mirror sort)
    IN_OUTPUT,            // counted straight into the caller's arrays (canonical_only)
    EMITTED               // the route has rebuilt the strands itself: the batch is finished
};
struct Counted {
    u64* keys = nullptr;             // uc distinct canonical k-mers, ascending -- or words, (k-mer << pack) | count, when mwords is set
    u32* cnt = nullptr;
    uint64_t uc = 0;
    ListPlace where = IN_SORT_BUF;
    bool have_max = false;           // max_count is the largest count of the list, or a bound of it: it came for free
    uint64_t max_count = 0;
    u64 *mwords = nullptr, *malt = nullptr;          // the mirrored words, grouped by their low mgroup bits, and their second buffer (dedupe_finish)
    u64* mhist = nullptr;                            // ... and the digit counts of the passes that sort them, when it took those as well
    int mgroup = MIRROR_GROUP_BITS;                  // (6 more than MIRROR_GROUP_BITS when the blocks told how they split)
};

// room for m (key, count) entries in the aux region: the counts start at the next 256-byte boundary behind the keys
static int aux_list(zk_ctx* c, uint64_t m, u64** k, u32** v) {
    char* aux;
    ZK_TRY(aux_require(c, align256(8 * m) + align256(4 * m), &aux));
    *k = (u64*)aux; *v = (u32*)(aux + align256(8 * m));
    return ZK_OK;
}

// Plain run-length count of keys sorted by all their bits.  Reads keys.  canonical_only: writes the caller's arrays, the caller
// wants the counted canonical list itself (multi-GPU: it is exchanged before the strands are rebuilt).  Otherwise in place: the
// distinct k-mers over the keys, the counts into the other sort buffer.
static int count_sorted(zk_ctx* c, const KmerizePlan& p, const SortBufs& b, u64* keys, uint64_t n, const Output& o, Counted* r) {
    if (p.canonical_only) {
        r->where = IN_OUTPUT;
        return rle(c, keys, n, o.k, o.c, o.cap, &r->uc);
    }
    r->keys = keys; r->cnt = (u32*)b.other(keys); r->where = IN_SORT_BUF;
    return rle(c, keys, n, keys, r->cnt, n, &r->uc);
}

// A route has declined: the keys, sorted by their low lo_bit bits (ALL_BITS: not in a way that helps), finish the sort by passes
// into whichever buffer the last pass writes, and are counted there.  Reads keys, overwrites the buffer they are not in.
constexpr int ALL_BITS = -1;
static int count_by_passes(zk_ctx* c, const KmerizePlan& p, const SortBufs& b, u64* keys, uint64_t n, int lo_bit, const Output& o, Counted* r) {
    u64* res = nullptr;
    if (lo_bit == ALL_BITS) ZK_TRY(sort_keys(c, keys, b.other(keys), n, 2 * p.K, &res));
    else ZK_TRY(sort_keys_upper(c, keys, b.other(keys), n, 2 * p.K, lo_bit, &res, ZK_PROF_PASS_KEYS));
    return count_sorted(c, p, b, res, n, o, r);
}

// u1 words, (k-mer << pack) | run length, sorted by their low lo_bit + pack bits: the bits above sorted by the key kernel (alt is
// their second buffer), the split runs summed straight from the words into the aux region; the largest count comes with them.
static int reduce_words(zk_ctx* c, const KmerizePlan& p, u64* words, u64* alt, uint64_t u1, int lo_bit, Counted* r) {
    u64* res = nullptr;
    ZK_TRY(sort_keys_upper(c, words, alt, u1, 2 * p.K + p.pack, lo_bit + p.pack, &res));
    ZK_TRY(aux_list(c, u1, &r->keys, &r->cnt));
    ZK_TRY(reduce_by_key(c, res, nullptr, u1, r->keys, r->cnt, u1, &r->uc, p.pack, &r->max_count));
    r->where = IN_AUX; r->have_max = true;
    return ZK_OK;
}

// COUNT_TILES: the keys are sorted by their top tile_top bits; the tiles sort the rest and count, the distinct k-mers leave them
// with their counts -- straight into the caller's arrays when the canonical list is all that is wanted (the batches of
// library/engine.py), else over the keys, counts in the other buffer.  Declined (a block of equal top bits too long for a tile):
// every bit by passes, from where the keys are now.
static int count_tiles(zk_ctx* c, const KmerizePlan& p, const SortBufs& b, const Sorted& s, const Output& o, Counted* r) {
    bool declined = false;
    if (p.canonical_only) ZK_TRY(tile_sort_count(c, s.keys, s.n, 2 * p.K, p.tile_top, o.k, o.c, o.cap, &r->uc, &declined));
    else ZK_TRY(tile_sort_count(c, s.keys, s.n, 2 * p.K, p.tile_top, s.keys, (u32*)s.other, s.n, &r->uc, &declined));
    if (declined) return count_by_passes(c, p, b, s.keys, s.n, 0, o, r);
    r->keys = s.keys; r->cnt = (u32*)s.other; r->where = p.canonical_only ? IN_OUTPUT : IN_SORT_BUF;
    return ZK_OK;
}

// COUNT_BLOCKS: the keys (or their tags) are sorted by their top dedupe_bit bits.  The dedupe reads them and writes its words into
// the other buffer, so a declined dedupe (little duplication in its sample of the leading blocks, about a million keys, or a table
// filled up) still has the keys: they are sorted the long way, all their bits -- the two passes over the top bits were for nothing
// -- after being made again from their tags, into the buffer the discarded words are in.  Counted: the list lands in the aux
// region, as words when the mirrored words are written too (those go over the keys' buffer), and both sort buffers are free.
// At odd K the strands may be rebuilt block by block instead, from the counted list where the dedupe left it: then the batch is
// finished here (EMITTED; st->n_canonical is set).
static int count_blocks(zk_ctx* c, const KmerizePlan& p, const SortBufs& b, const Sorted& s, const Output& o, zk_kmerize_stats* st, Counted* r) {
    const int K = p.K, pk = p.pack;
    DedupeResult d;
    uint64_t n_in = 0;
    const uint64_t nblocks = 1ull << p.dedupe_bit, per = s.n / nblocks + 1;
    const u32* tg = s.tags.written ? (const u32*)s.keys : nullptr;
    if (!s.presampled) ZK_TRY(dedupe_pass(c, s.keys, s.n, 2 * K, p.dedupe_bit, pk, s.other, b.cap_keys, &d, &n_in, (1u << 20) / per + 4, tg, s.tags.cuts));
    if (s.presampled || (!(d.flags & 1) && (double)d.n_out <= REPEAT_RATIO * (double)n_in)) {
        // the strand route: the dedupe writes the mirror words too, behind the tags it reads (they take the first 4 n bytes of the keys'
        // buffer; whole keys leave no room) -- strand_blocks then finds them there
        DedupeMirror mo;
        const uint64_t tag_words = align256(4 * s.n) / 8;
        if (tg && p.blocks_strands && p.blocks_unsorted && c->strand_blocks != 4 && tag_words < b.cap_keys) {
            mo.out = s.keys + tag_words; mo.cap = b.cap_keys - tag_words; mo.K = K;
            if (c->strand_blocks == 5 && mo.cap > 1024) mo.cap = 1024;
        }
        ZK_TRY(dedupe_pass(c, s.keys, s.n, 2 * K, p.dedupe_bit, pk, s.other, b.cap_keys, &d, nullptr, 0, tg, s.tags.cuts, p.blocks_unsorted, &mo));
        if (!(d.flags & 1)) {
            const uint64_t uc = r->uc = d.n_out;
            // Every count fits the field (the usual case) and both strands are wanted: the copy that closes the gaps also
            // writes the mirrored words grouped by their low 18 bits -- the first stage of the mirror sort (mirror_union's
            // grouping copy) for free; they go over the keys' buffer (the keys are counted, the words are in the other one).
            const bool want_m = !(d.flags & 2) && p.blocks_mirror;
            // ... at odd K (the two strands share no key) without the dense copy and the full mirror sort: block by block, the
            // counted list read where the dedupe left it (strand_blocks.hip)
            if (want_m && p.blocks_strands && 2 * align256(8 * uc) <= 8 * b.cap_keys) {
                st->n_canonical = uc;
                r->where = EMITTED;
                return strand_blocks(c, d, s.keys, b.cap_keys, K, o.k, o.c, o.cap, o.n_out);
            }
            if (d.unsorted) ZK_TRY(dedupe_sort_blocks(c, d));          // the route is not taken after all: the blocks sorted first
            ZK_TRY(aux_list(c, uc, &r->keys, &r->cnt));
            // ... and the counted list itself stays in words, (k-mer << pk) | count: nobody but the final union reads it
            ZK_TRY(dedupe_finish(c, d, r->keys, r->cnt, want_m ? s.keys : nullptr, K, MIRROR_GROUP_BASES, &r->mhist, &r->mgroup, want_m));
            if (want_m) { r->mwords = s.keys; r->malt = s.other; }
            r->where = IN_AUX;
            if (!(d.flags & 2)) { r->max_count = (1ull << pk) - 1; r->have_max = true; }          // every count fits the field
            return ZK_OK;
        }
    }
    u64* keys = s.keys;
    if (tg) {
        ZK_TRY(expand_tags(c, tg, s.tags.cuts, s.tags.blocks, 2 * K - p.dedupe_bit, s.other));
        keys = s.other;
    }
    return count_by_passes(c, p, b, keys, s.n, ALL_BITS, o, r);
}

// COUNT_FUSED: the keys are sorted by their low fused_bit bits.  Runs are counted inside the tile-local ranking of the next digit
// (collapse.hip::collapse_kernel): that pass writes one word per run instead of every key, into the other buffer, and no pass
// of its own reads the keys again to count.  Its output is tile-major, so the passes over the words start at fused_bit.  Whether
// it pays: the same kernel over the first tiles (low bits ascending: a random subset of the k-mers with all their copies).  The
// list lands in the aux region; little duplication: every key to the end.
static int count_fused(zk_ctx* c, const KmerizePlan& p, const SortBufs& b, const Sorted& s, const Output& o, Counted* r) {
    const int pk = p.pack;
    const int cb = sort_first_bits(c, 2 * p.K + pk, p.fused_bit + pk);       // the digit the first pass over the words will use
    const uint64_t sample_tiles = 64, tile_keys = 8192;
    uint64_t us = 0, u1 = 0;
    ZK_TRY(collapse_pass(c, s.keys, s.n, p.fused_bit, cb, pk, s.other, b.cap_keys, &us, sample_tiles));
    const uint64_t m = s.n < sample_tiles * tile_keys ? s.n : sample_tiles * tile_keys;
    if ((double)us > REPEAT_RATIO * (double)m) return count_by_passes(c, p, b, s.keys, s.n, p.fused_bit, o, r);
    ZK_TRY(collapse_pass(c, s.keys, s.n, p.fused_bit, cb, pk, s.other, b.cap_keys, &u1));
    return reduce_words(c, p, s.other, s.keys, u1, p.fused_bit, r);
}

// COUNT_RUNS: the keys are sorted by their low collapse_bit bits.  Sequencing reads repeat every k-mer `coverage` times, and an
// LSD sort drags all those copies through every pass.  But after the passes over the low b bits the copies of a k-mer are
// already NEIGHBOURS as soon as 2^b is well above the number of keys (two distinct k-mers rarely share their low b bits), so the
// run-length count can be taken THEN: the remaining passes move (k-mer, count) pairs -- one per distinct k-mer instead of one per
// copy -- and a final pass adds up the few k-mers whose copies were interleaved with another k-mer's (reduce_by_key).  Exact
// for any input: collapsing adjacent equal keys and summing equal keys later never loses or invents a count; the data
// only decides how much is saved.  Whether it pays is read off a sample of the partially sorted array (its head holds a
// random subset of the k-mers with all their copies); with little duplication the keys finish the sort as before.
// The list lands in the aux region; both sort buffers are scratch on the way.
static int count_runs(zk_ctx* c, const KmerizePlan& p, const SortBufs& b, const Sorted& s, const Output& o, Counted* r) {
    const int K = p.K;
    uint64_t m = 0, heads = 0;
    ZK_TRY(sample_heads(c, s.keys, s.n, &m, &heads));
    if ((double)heads > REPEAT_RATIO * (double)m) return count_by_passes(c, p, b, s.keys, s.n, p.collapse_bit, o, r);      // still every key: the dominant passes
    if (p.pack) {
        // The runs as single words (key << pack | length): written beside the keys (not over them: should a run be longer
        // than 2^pack - 1 the keys are still there and the pair path below takes over), the upper bits sorted by the key
        // kernel, the split runs summed straight from the words.
        uint64_t u1 = 0;
        bool ovf = false;
        const int rc1 = rle(c, s.keys, s.n, s.other, nullptr, b.cap_keys, &u1, p.pack, &ovf);          // `other` holds cap_keys words
        if (rc1 != ZK_OK && rc1 != ZK_ENOSPC) return rc1;
        if (rc1 == ZK_OK && !ovf) return reduce_words(c, p, s.other, s.keys, u1, p.collapse_bit, r);
    }
    u32* cnt = (u32*)s.other;
    uint64_t u1 = 0;
    ZK_TRY(rle(c, s.keys, s.n, s.keys, cnt, s.n, &u1));          // in place: runs of adjacent equal keys
    const uint64_t a8 = align256(8 * u1), a4 = align256(4 * u1);
    // the second key / count buffers of the pair passes sit behind the lists in the two sort buffers; should the
    // sample have been too optimistic for that (it never is on reads), they go to the aux region instead
    const bool fits = a8 + a4 + 512 <= 8 * b.cap_keys;
    char* aux;
    ZK_TRY(aux_require(c, (fits ? 1 : 2) * (a8 + a4), &aux));
    u64* alt = fits ? (u64*)((char*)s.other + a4) : (u64*)(aux + a8 + a4);
    u32* valt = fits ? (u32*)((char*)s.keys + a8) : (u32*)(aux + 2 * a8 + a4);
    u64* sk; u32* sv;
    ZK_TRY(sort_pairs_upper(c, s.keys, alt, cnt, valt, u1, 2 * K, p.collapse_bit, &sk, &sv));
    r->keys = (u64*)aux; r->cnt = (u32*)(aux + a8); r->where = IN_AUX;
    return reduce_by_key(c, sk, sv, u1, r->keys, r->cnt, u1, &r->uc);
}

// Stage 4, the strands, from the counted canonical list r (r.uc > 0).  canonical_only: the list itself goes out -- it is there
// already, or two device copies.  The block dedupe wrote the mirrored words: they are sorted above their group bits (in the two
// sort buffers) and merged with the list's words.  Otherwise mirror_union, whose work buffers are the two sort buffers when the
// list is in the aux region, and the aux region when the list is in the sort buffers.
static int emit_strands(zk_ctx* c, const KmerizePlan& p, const SortBufs& b, const Counted& r, const Output& o) {
    const int K = p.K;
    const uint64_t uc = r.uc;
    if (p.canonical_only) {
        if (uc > o.cap) return fail(c, ZK_ENOSPC, "output holds %llu entries, the batch has %llu distinct canonical k-mers", (unsigned long long)o.cap, (unsigned long long)uc);
        if (r.where != IN_OUTPUT) {
            ZK_HIP(c, hipMemcpyAsync(o.k, r.keys, 8 * uc, hipMemcpyDeviceToDevice, c->stream));
            ZK_HIP(c, hipMemcpyAsync(o.c, r.cnt, 4 * uc, hipMemcpyDeviceToDevice, c->stream));
        }
        *o.n_out = uc;
        return ZK_OK;
    }
    if (r.mwords) {
        u64* sk = nullptr;
        if (r.mhist) ZK_TRY(sort_keys_upper_counted(c, r.mwords, r.malt, uc, 2 * K + p.pack, r.mgroup + p.pack, r.mhist, &sk));
        else ZK_TRY(sort_keys_upper(c, r.mwords, r.malt, uc, 2 * K + p.pack, r.mgroup + p.pack, &sk));
        return union_sum_packed_ab(c, r.keys, uc, sk, uc, p.pack, o.k, o.c, o.cap, o.n_out, (K & 1) != 0);
    }
    const uint64_t a8 = align256(8 * uc), a4 = align256(4 * uc);
    u64 *rk, *rk2; u32 *rv, *rv2;
    if (r.where == IN_AUX) {
        rk = b.a; rv = (u32*)((char*)b.a + a8);
        rk2 = b.b; rv2 = (u32*)((char*)b.b + a8);
    } else {
        char* aux;
        ZK_TRY(aux_require(c, 2 * a8 + 2 * a4, &aux));
        rk = (u64*)aux; rk2 = (u64*)(aux + a8);
        rv = (u32*)(aux + 2 * a8); rv2 = (u32*)(aux + 2 * a8 + a4);
    }
    int pack = 0;
    ZK_TRY(mirror_pack(c, K, r.cnt, uc, r.have_max, r.max_count, &pack));
    return mirror_union(c, r.keys, r.cnt, uc, K, rk, rk2, rv, rv2, o.k, o.c, o.cap, o.n_out, pack);
}

// `both` by the tile-sort plan (top: plan.both_top): the keys of both strands through the passes over their top bits, then sorted
// and counted tile by tile straight into the caller's arrays.  Writes both sort buffers.
static int kmerize_both_tiles(zk_ctx* c, const u8* stream, uint64_t n_bytes, int K, int top, const SortBufs& b, const Output& o, zk_kmerize_stats* st) {
    StreamSrc src{stream, n_bytes, K, ZK_KEYS_BOTH, 2 * K - top};
    uint64_t n = 0;
    u64* sorted = nullptr;
    ZK_TRY(sort_stream(c, src, b.a, b.b, b.cap_keys, &n, st->acgt, &sorted));
    st->n_windows = n / 2;
    st->n_instances = n;
    *o.n_out = 0;
    bool declined = false;
    ZK_TRY(tile_sort_count(c, sorted, n, 2 * K, top, o.k, o.c, o.cap, o.n_out, &declined));
    if (declined) {
        u64* res = nullptr;
        ZK_TRY(sort_keys_upper(c, sorted, b.other(sorted), n, 2 * K, 0, &res, ZK_PROF_PASS_KEYS));
        ZK_TRY(rle(c, res, n, o.k, o.c, o.cap, o.n_out));
    }
    // the table holds x and rc x for every canonical k-mer: two entries each, but one for a palindrome (x == rc x, even K only)
    uint64_t pal = 0;
    if (!(K & 1)) ZK_TRY(count_palindromes(c, o.k, *o.n_out < o.cap ? *o.n_out : o.cap, K, &pal));
    st->n_canonical = (*o.n_out + pal) / 2;
    return ZK_OK;
}

// One batch of zk_kmerize: plan, sort, count by the route the sort stage settled on, strands.
// replan (or null): set to 1, with nothing sorted yet, when the look before the sort asks for the both-strand tile plan (see
// sort_by_plan); the caller makes room and calls again with both_tiles.  both_tiles: `both`, by the tile-sort plan.
static int kmerize_full(zk_ctx* c, const u8* stream, uint64_t n_bytes, int K, bool both, const SortBufs& b, const Output& o,
                        zk_kmerize_stats* st, bool canonical_only = false, int* replan = nullptr, bool both_tiles = false) {
    const KmerizePlan p = plan_kmerize(c, n_bytes, K, both, canonical_only);
    if (both && both_tiles && p.both_top) return kmerize_both_tiles(c, stream, n_bytes, K, p.both_top, b, o, st);
    Sorted s;
    ZK_TRY(sort_by_plan(c, p, stream, n_bytes, b, replan != nullptr, st->acgt, &s));
    if (s.route == COUNT_REPLAN) { *replan = 1; return ZK_OK; }
    st->n_windows = both ? s.n / 2 : s.n;
    st->n_instances = both ? s.n : 2 * s.n;
    *o.n_out = 0;
    if (both) {
        st->n_canonical = 0;
        return rle(c, s.keys, s.n, o.k, o.c, o.cap, o.n_out);
    }
    Counted r;
    switch ((s.n || s.route == COUNT_TILES) ? s.route : COUNT_SORTED) {          // (no keys: nothing to collapse)
    case COUNT_TILES: ZK_TRY(count_tiles(c, p, b, s, o, &r)); break;
    case COUNT_BLOCKS: ZK_TRY(count_blocks(c, p, b, s, o, st, &r)); break;
    case COUNT_FUSED: ZK_TRY(count_fused(c, p, b, s, o, &r)); break;
    case COUNT_RUNS: ZK_TRY(count_runs(c, p, b, s, o, &r)); break;
    default: ZK_TRY(count_sorted(c, p, b, s.keys, s.n, o, &r)); break;
    }
    if (r.where == EMITTED) return ZK_OK;
    st->n_canonical = r.uc;
    if (r.uc == 0) return ZK_OK;
    return emit_strands(c, p, b, r, o);
}

// The short path: sort only the top T bits of the canonical keys (T ~ log2(n) + 3, a whole number
// of digits), so that nearly every group of equal prefix is a single k-mer already in its final
// place; rle_prefix_kernel writes those to the sorted main list and everything else (mixed groups,
// groups cut by a tile edge) to a side list, which simply joins the strand-mirror pairs in the sort
// they need anyway.  Exact for any input; the data only decides how much goes the long way.
// Returns 1 when the side list would not fit (caller falls back to kmerize_full).
static int kmerize_short(zk_ctx* c, const u8* stream, uint64_t n_bytes, int K, int lo_bit, const SortBufs& b, u64* out_k, u32* out_c,
                         uint64_t cap, zk_kmerize_stats* st, uint64_t* n_out) {
    const uint64_t cap_keys = b.cap_keys;
    StreamSrc src{stream, n_bytes, K, ZK_KEYS_CANONICAL, lo_bit};
    uint64_t n = 0;
    u64* sorted = nullptr;
    ZK_TRY(sort_stream(c, src, b.a, b.b, cap_keys, &n, st->acgt, &sorted));
    st->n_windows = n;
    st->n_instances = 2 * n;
    *n_out = 0;
    if (n == 0) return ZK_OK;
    char* other = (char*)b.other(sorted);
    u32* cnt = (u32*)other;
    uint64_t side_cap = n / (uint64_t)(c->side_div > 0 ? c->side_div : 8) + 64;
    const uint64_t off_k = align256(4 * n);
    if (off_k + 12 * side_cap > 8 * cap_keys) side_cap = (8 * cap_keys - off_k) / 12;
    u64* side_k = (u64*)(other + off_k);
    u32* side_c = (u32*)(other + off_k + 8 * side_cap);
    uint64_t um = 0, ns = 0;
    ZK_TRY(rle_prefix(c, sorted, n, lo_bit, sorted, cnt, n, &um, side_k, side_c, side_cap, &ns));
    if (ns > side_cap) return 1;
    const uint64_t m = um + 2 * ns;
    const uint64_t a8 = align256(8 * m), a4 = align256(4 * m);
    char* aux;
    ZK_TRY(aux_require(c, (ns ? 3 : 2) * (a8 + a4), &aux));
    u64* pk = (u64*)aux; u64* pk2 = (u64*)(aux + a8);
    u32* pv = (u32*)(aux + 2 * a8); u32* pv2 = (u32*)(aux + 2 * a8 + a4);
    if (um) {
        prof_begin(c, ZK_PROF_MIRROR, 24 * um);
        hipLaunchKernelGGL(mirror_kernel, dim3(grid_cap(c, div_up(um, 256), 16)), dim3(256), 0, c->stream, sorted, cnt, (u64)um, K, pk, pv);
        prof_end(c);
        ZK_HIP(c, hipGetLastError());
    }
    if (ns) {
        hipLaunchKernelGGL(side_expand_kernel, dim3(grid_cap(c, div_up(ns, 256), 16)), dim3(256), 0, c->stream, side_k, side_c, (u64)ns, K, pk + um, pv + um);
        ZK_HIP(c, hipGetLastError());
    }
    u64* sk; u32* sv;
    ZK_TRY(sort_pairs(c, pk, pk2, pv, pv2, m, 2 * K, &sk, &sv));
    uint64_t mr = m;
    if (ns) {
        u64* rk = (u64*)(aux + 2 * a8 + 2 * a4);
        u32* rv = (u32*)(aux + 3 * a8 + 2 * a4);
        ZK_TRY(reduce_by_key(c, sk, sv, m, rk, rv, m, &mr));
        sk = rk; sv = rv;
    }
    ZK_TRY(union_sum(c, sorted, cnt, um, sk, sv, mr, out_k, out_c, 32, cap, n_out, nullptr));
    // (the side list holds a canonical k-mer once per group it was cut into: its length is no count of them -- the table is)
    uint64_t pal = 0;
    if (!(K & 1)) ZK_TRY(count_palindromes(c, out_k, *n_out, K, &pal));
    st->n_canonical = (*n_out + pal) / 2;
    return ZK_OK;
}

int kmerize(zk_ctx* c, const u8* stream, uint64_t n_bytes, int K, int flags, double p, uint64_t seed, u64* out_k, u32* out_c,
            uint64_t cap, zk_kmerize_stats* st) {
    memset(st, 0, sizeof *st);
    if (K < 1 || K > 32) return fail(c, ZK_EINVAL, "K must be in 1..32 (got %d)", K);
    if (n_bytes == 0) return ZK_OK;
    const bool both = (flags & ZK_KMERIZE_BOTH) != 0;
    const bool canonical_only = (flags & ZK_KMERIZE_CANONICAL_ONLY) != 0;
    if (canonical_only && (both || (flags & ZK_KMERIZE_SUBSAMPLE)))
        return fail(c, ZK_EINVAL, "ZK_KMERIZE_CANONICAL_ONLY cannot be combined with ZK_KMERIZE_BOTH or ZK_KMERIZE_SUBSAMPLE");
    const uint64_t cap_keys = both ? 2 * n_bytes : n_bytes;   // one window per stream byte at most
    arena_reset(c);
    // histograms, merge-path partitions, the mirror group tables (4 MB); from 2^29 stream bytes on (block dedupe with 2^18 blocks) the
    // blocks' tables as well: bounds, sizes, and the 2^24 run places of the mirror grouping (336 MB) -- or, where the blocks were not
    // counted that way, the 2^24 group bounds, ends and places of mirror_union (403 MB)
    const uint64_t slack = (16 << 20) + cap_keys / 16 + ((n_bytes >= (1ull << 29) || c->dedupe_bits >= 18) ? (832ull << 20) : 0);          // (+ the block starts of the tag path: 2 MB; the list of declined blocks: 1 MB)
    ZK_TRY(arena_require(c, 16 * cap_keys + slack, 16 * cap_keys + slack));
    SortBufs b{nullptr, nullptr, cap_keys};
    ZK_TRY(arena_alloc(c, 8 * cap_keys, (void**)&b.a));
    ZK_TRY(arena_alloc(c, 8 * cap_keys, (void**)&b.b));

    uint64_t n_out = 0;
    const Output o{out_k, out_c, cap, &n_out};
    int rc = 1;
    if (!both && c->short_sort && !canonical_only) {
        const int rb = sort_rbits(c);
        const int T = rb * ((ilog2_ceil(n_bytes) + 3 + rb - 1) / rb);
        if (T < 2 * K) {
            rc = kmerize_short(c, stream, n_bytes, K, 2 * K - T, b, out_k, out_c, cap, st, &n_out);
            if (rc < 0) return rc;
            if (rc == 1) st->n_canonical = 0;      // side list overflowed: do it the long way
        }
    }
    if (rc == 1) {
        // Reads that do not repeat their k-mers (the look before the sort says so), both strands wanted: the sort is planned again
        // for the keys of both strands, if the device has the room (twice the sort buffers; the mirror's buffers are not needed then)
        int replan = 0;
        size_t mfree = 0, mtotal = 0;
        const uint64_t need2 = 32 * n_bytes + slack + 2 * n_bytes / 16;
        const bool may = !both && !canonical_only && c->tile_sort && hipMemGetInfo(&mfree, &mtotal) == hipSuccess &&
                         (double)need2 < 0.9 * (double)(mfree + c->arena_size + c->aux_size);
        ZK_TRY(kmerize_full(c, stream, n_bytes, K, both, b, o, st, canonical_only, may ? &replan : nullptr));
        if (replan) {
            arena_reset(c);
            if (need2 > c->arena_size && (double)need2 >= 0.9 * (double)(mfree + c->arena_size) && c->aux) {
                ZK_HIP(c, hipStreamSynchronize(c->stream));
                ZK_HIP(c, hipFree(c->aux));
                c->aux = nullptr; c->aux_size = 0;
            }
            ZK_TRY(arena_require(c, need2, need2));
            b.cap_keys = 2 * n_bytes;
            ZK_TRY(arena_alloc(c, 8 * b.cap_keys, (void**)&b.a));
            ZK_TRY(arena_alloc(c, 8 * b.cap_keys, (void**)&b.b));
            ZK_TRY(kmerize_full(c, stream, n_bytes, K, true, b, o, st, false, nullptr, true));
        }
    }
    if (flags & ZK_KMERIZE_SUBSAMPLE) {
        uint64_t kept = 0;
        ZK_TRY(subsample_pairs(c, out_k, out_c, n_out, seed, p, &kept));
        n_out = kept;
    }
    st->n_unique = n_out;
    return check_device_error(c);
}

// k-way union-sum as a balanced tree of 2-way passes; counts are 32- or 64-bit (count_bits).
// ins: k device arrays (keys, counts, n).  The result lands in (out_k, out_c).
int merge_many(zk_ctx* c, int k, const u64* const* keys, const void* const* cnts, const uint64_t* ns, u64* out_k, void* out_c,
               int count_bits, uint64_t cap, uint64_t* n_out, uint64_t acgt_w[4]) {
    const uint64_t cb = (uint64_t)count_bits / 8;
    *n_out = 0;
    if (acgt_w) acgt_w[0] = acgt_w[1] = acgt_w[2] = acgt_w[3] = 0;
    if (k <= 0) return ZK_OK;
    arena_reset(c);
    uint64_t total = 0;
    for (int i = 0; i < k; i++) total += ns[i];
    if (k == 1) {
        // union with the empty set: a plain copy that also yields the count-weighted acgt
        return union_sum(c, keys[0], cnts[0], ns[0], keys[0], cnts[0], 0, out_k, out_c, count_bits, cap, n_out, acgt_w);
    }
    // two ping-pong regions, each able to hold every intermediate list of one level; behind them the scratch of ONE pass, which is
    // handed back when the pass returns (each pass synchronises first, so nothing of it is in flight).  The largest pass is a k-way
    // pass over at most `total` pairs of up to 16 lists: its sample and the sample's sort buffer (16 B per 64 pairs), the tile bounds
    // (8 B per tile and list, a tile per 16 sample points or more: 0.125 B a pair at 16 lists), the acgt rows, sort_keys' histograms
    // and tile bounds -- below total / 2 + 8 KB a list + 1 MB.  A 2-way pass needs its merge-path partition and acgt rows only.
    const uint64_t slack = 1 << 20;
    const uint64_t rbytes = (8 + cb) * total + 512ull * k;
    const uint64_t need = 2 * rbytes + total / 2 + 8192ull * k + slack;
    ZK_TRY(arena_require(c, need, need));
    struct L { const u64* k; const void* c; uint64_t n; };
    std::vector<L> va(k), vb(k);
    L* cur = va.data();
    L* nxt = vb.data();
    for (int i = 0; i < k; i++) cur[i] = L{keys[i], cnts[i], ns[i]};
    char* region[2];
    ZK_TRY(arena_alloc(c, rbytes, (void**)&region[0]));
    ZK_TRY(arena_alloc(c, rbytes, (void**)&region[1]));
    auto in_regions = [&](const void* q) {
        const char* b = (const char*)q;
        return (b >= region[0] && b < region[0] + rbytes) || (b >= region[1] && b < region[1] + rbytes);
    };
    // Fan-in of a level: up to 16 lists in ONE pass (kway.hip) -- the eight sets of a GPU in BASELINE config 4 are one level, 64 sets
    // two -- or pairs (zk_tune ZK_TUNE_KWAY 0: the tree of 2-way passes)
    // (small inputs keep the tree: the k-way pass sorts a sample with the radix-sort pipeline, eight launches that a few thousand pairs
    // do not pay for; ZK_TUNE_KWAY 2 takes it always -- the tests)
    const int F = (c->kway == 2 || (c->kway == 1 && total >= (1ull << 22))) ? 16 : 2;
    int m = k, level = 0;
    while (m > 1) {
        const bool last = (m <= F);
        char* base = region[level & 1];
        uint64_t off = 0;
        int o = 0;
        for (int i = 0; i < m; i += F) {
            const int g = m - i < F ? m - i : F;          // lists of this group
            if (g == 1) {
                // the odd list sits out this level; if it lives in a ping-pong region the level after next would overwrite it, so
                // move it along with this level's outputs
                L x = cur[i];
                if (in_regions(x.k)) {
                    u64* ok = (u64*)(base + off); off += align256(8 * x.n);
                    void* oc = (void*)(base + off); off += align256(cb * x.n);
                    ZK_HIP(c, hipMemcpyAsync(ok, x.k, 8 * x.n, hipMemcpyDeviceToDevice, c->stream));
                    ZK_HIP(c, hipMemcpyAsync(oc, x.c, cb * x.n, hipMemcpyDeviceToDevice, c->stream));
                    x.k = ok; x.c = oc;
                }
                nxt[o++] = x;
                continue;
            }
            uint64_t capg = 0;
            for (int j = 0; j < g; j++) capg += cur[i + j].n;
            u64* ok; void* oc; uint64_t capo;
            if (last) { ok = out_k; oc = out_c; capo = cap; }
            else {
                ok = (u64*)(base + off); off += align256(8 * capg);
                oc = (void*)(base + off); off += align256(cb * capg);
                capo = capg;
            }
            uint64_t no = 0;
            const uint64_t mark = c->arena_off;          // this pass's scratch starts here and is dead when it returns
            int rc;
            if (g == 2) {
                rc = union_sum(c, cur[i].k, cur[i].c, cur[i].n, cur[i + 1].k, cur[i + 1].c, cur[i + 1].n, ok, oc, count_bits, capo, &no,
                               last ? acgt_w : nullptr);
            } else {
                const u64* gk[16]; const void* gc[16]; uint64_t gn[16];
                for (int j = 0; j < g; j++) { gk[j] = cur[i + j].k; gc[j] = cur[i + j].c; gn[j] = cur[i + j].n; }
                rc = kway_union_sum(c, g, gk, gc, gn, ok, oc, count_bits, capo, &no, last ? acgt_w : nullptr);
            }
            if (rc == ZK_ENOSPC && last) *n_out = no;          // the caller's arrays are too short: the length they need
            if (rc != ZK_OK) return rc;
            c->arena_off = mark;
            nxt[o++] = L{ok, oc, no};
        }
        L* t = cur; cur = nxt; nxt = t;
        m = o;
        level++;
    }
    *n_out = cur[0].n;
    return ZK_OK;
}

}  // namespace zk
