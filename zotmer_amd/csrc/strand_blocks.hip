// strand_blocks.hip -- both strands of a counted canonical list, rebuilt block by block (odd K).
//
// The block dedupe (dedupe2.hip) leaves the counted canonical list C as (k-mer << pack | count) words, cut into 2^18 blocks by the
// k-mer's first nine bases, each block in table order (the dedupe's unsorted mode: nothing here needs more than the block it is in),
// block v at work + cuts[v] (nwords[v] words; its place in the dense list starts at
// incl[v] - nwords[v]).  The table of both strands is C together with its mirror image M = rc(C), sorted.  At odd K no k-mer is its own
// reverse complement, so the two lists share no key and the table is their union without sums: block b of the table holds exactly
// C_b and M_b (the mirrored words whose first nine bases are b), and its place is known before anything is merged:
//
//     place(b) = (entries of C before block b) + (entries of M before block b).
//
// So M needs no more than grouping by its top 18 bits, and the union needs no merge path:
//   1. M written densely, rc(k-mer) << pack | count, in no order at all, with the digit counts of the two passes below: by the dedupe
//      itself beside its words (dedupe2.hip, MIRROR; DedupeResult::m_emitted), this step then only adds the blocks the dedupe declined
//      (strand_mirror_kernel over their list, the words' places from the same cursor) and checks that every word has its mirror image.
//      Else -- whole keys instead of tags, a plan of more than two passes, no room, ZK_TUNE_STRAND_BLOCKS 4 -- strand_mirror_kernel
//      reads the whole list back and writes M at the canonical word's own index (whole lines);
//   2. two passes of the key kernel over M's top 18 key bits (sort_keys_upper_counted): M grouped by block;
//   3. strand_starts_kernel: where every block of M starts (a binary search per block);
//   4. strand_block_union_kernel: one workgroup per block reads C_b (in place, where the dedupe wrote it) and M_b, sorts the two in
//      LDS (tile_group.hpp: the counting sort and the in-group ranks of tilesort.hip; K <= 25: the same on 32-bit tags, see
//      StrandTagSmem) and writes keys and counts at place(b) + rank.  No tile waits for another.
//
// Buffers: C's gapped words stay in the dedupe's work buffer until the union has read them; M and the ping-pong buffer of its passes
// (2 x 8 U bytes for U distinct canonical k-mers) are the first and second half of the keys' buffer, which the dedupe has finished with.
// The dedupe's own M lies behind the tags it read (the first 4 n bytes of that buffer); the second buffer is then the start of the
// buffer, or the room behind M.
//
// A block of more entries than a tile holds (low-complexity sequence, genomes whose 9-base prefixes are far from uniform), or one
// whose entries crowd a few groups, is declined onto a list, and strand_big_block_kernel takes the listed blocks alone: 256 splitters
// sampled from C_b and M_b cut the block's value range, one pass over M_b counts every range, the ranges are packed into sub-tiles
// of at most a tile, and each sub-tile gathers its M entries in one more pass over M_b and is sorted and written like a whole block.
// A block's cost grows with its own size only.  Should a single range still hold more than a tile (or crowd its groups), the union
// is made the other way from the same state, exactly: C's blocks sorted, C copied densely, M sorted on every bit, and the merge-path
// union (setops.hip).
#include "tile_group.hpp"

namespace zk {

constexpr int SB_ITEMS = 16, SB_GROUPS = 2048;          // tiles of 8 K entries (a block at config 2: ~6.1 K) in 2048 groups
constexpr u32 SB_GROUP_MAX = 128;                         // a group of more entries declines its tile (the ranks are quadratic in it)
typedef TileSortSmem<SB_ITEMS, SB_GROUPS, false> StrandSmem;
constexpr int SB_BLOCK_BITS = 18;

// block v's words w -> out_m[incl[v] - nwords[v] + i] = rc(w >> pack) << pack | (w & count mask), with the digit counts of mh.
// list (or null): only the blocks list[0 .. chunks), the ones dedupe2_kernel declined and so wrote no mirror words for; a block takes
// the place of its words behind the dedupe's from the same cursor (m_cap: the words out_m holds; no block is written across it)
__global__ __launch_bounds__(256) void strand_mirror_kernel(const u64* __restrict__ in, const u64* __restrict__ cuts, const u64* __restrict__ incl,
                                                            const u64* __restrict__ nwords, u32 chunks, int pack, int K, u64* __restrict__ out_m,
                                                            MirrorHist mh, const u32* __restrict__ list, u64* cursor, u64 m_cap) {
    __shared__ u32 bins[4 * 512];
    __shared__ u64 placed;
    const bool hist = mh.passes > 0;
    if (hist) {
        for (int q = threadIdx.x; q < 4 * 512; q += blockDim.x) bins[q] = 0;
        __syncthreads();
    }
    const u64 maxc = (1ull << pack) - 1;
    for (u32 t = blockIdx.x; t < chunks; t += gridDim.x) {
        const u32 v = list ? list[t] : t;
        const u64 cnt = nwords[v];
        u64 dst0 = incl[v] - cnt;
        if (list) {
            if (threadIdx.x == 0) placed = atomicAdd(cursor, cnt);
            __syncthreads();
            dst0 = placed;
            __syncthreads();          // (the word is free for the next block)
            if (dst0 + cnt > m_cap) continue;
        }
        const u64* src = in + cuts[v];
        for (u64 i0 = threadIdx.x; i0 < cnt; i0 += 4ull * blockDim.x) {
            u64 w4[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const u64 i = i0 + (u64)q * blockDim.x;
                w4[q] = i < cnt ? src[i] : 0;
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const u64 i = i0 + (u64)q * blockDim.x;
                if (i >= cnt) break;
                const u64 mw = (revcomp(K, w4[q] >> pack) << pack) | (w4[q] & maxc);
                out_m[dst0 + i] = mw;
                if (hist) {
#pragma unroll
                    for (int p = 0; p < 4; p++)
                        if (p < mh.passes) atomicAdd(&bins[p * 512 + ((u32)(mw >> mh.shift[p]) & ((1u << mh.bits[p]) - 1u))], 1u);
                }
            }
        }
    }
    if (hist) {
        __syncthreads();
        for (int q = threadIdx.x; q < mh.passes * 512; q += blockDim.x)
            if (bins[q]) atomicAdd(&mh.raw[q], (u64)bins[q]);
    }
}

// start[g] = first index of m whose bits from `shift` up are >= g (g = 0 .. 2^18; start[2^18] = n)
__global__ void strand_starts_kernel(const u64* __restrict__ m, u64 n, int shift, u64* __restrict__ start) {
    const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g > (1u << SB_BLOCK_BITS)) return;
    u64 lo = 0, hi = n;
    if (g == (1u << SB_BLOCK_BITS)) lo = n;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if ((m[mid] >> shift) < (u64)g) lo = mid + 1; else hi = mid;
    }
    start[g] = lo;
}

struct StrandArgs {
    const u64* cw;          // C's words, block v at cuts[v] (nwords[v] of them)
    const u64* cuts; const u64* nwords; const u64* incl;
    const u64* m;           // M, grouped by block: block b at [mstart[b], mstart[b + 1])
    const u64* mstart;
    u64* ok; u32* oc;       // the table: keys, counts
    int pack;
    int pshift;             // the block bits of a word start here
    u32* n_declined;        // the declined blocks: how many ...
    u32* declined;          // ... and which
    int below;              // the block-local form: the key bits below the block bits (at most 32) ...
    int gshift;             // ... and how far down the top 11 of them are: max(below - 11, 0)
};

// does any group of the tile just grouped hold more than SB_GROUP_MAX entries?  (every thread looks at four groups; a barrier)
template <class S>
__device__ __forceinline__ bool strand_crowded(const S& sm, int tid) {
    static_assert(SB_GROUPS == 4 * TS_BLOCK, "four groups a thread");
    u32 big = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) big |= sm.start[4 * tid + q + 1] - sm.start[4 * tid + q] > SB_GROUP_MAX ? 1u : 0u;
    return __syncthreads_or((int)big) != 0;
}

// the tile's entries, grouped (tile_group), ranked and written: keys to ok[place], counts to oc[place]
__device__ __forceinline__ void strand_write(const StrandSmem& sm, const TileMap& tm, u32 m, u64* ok, u32* oc, int pack, int tid) {
    const u64 maxc = (1ull << pack) - 1;
    constexpr int E = 2;
    for (u32 i0 = (u32)tid; i0 < m; i0 += E * TS_BLOCK) {
        u32 i[E], place[E];
        u64 mine[E];
#pragma unroll
        for (int e = 0; e < E; e++) i[e] = i0 + e * TS_BLOCK;
        tile_rank<E, false>(sm, tm, i, m, mine, place);
#pragma unroll
        for (int e = 0; e < E; e++) {
            if (i[e] >= m) break;
            ok[place[e]] = mine[e] >> pack;
            oc[place[e]] = (u32)(mine[e] & maxc);
        }
    }
}

// ---- a whole block in its own terms: 32-bit tags (2 K - 18 <= 32) -------------------------------------------------------------------
// Inside block b every key is (b << below) | tag, so the tile needs none of tile_group's 64-bit work: an entry is the tag (the key bits
// below the block's) and the count, in two u32 arrays of the same 64 KB; the group is the tag's top 11 bits, a shift; the ranks compare
// tags.  And no LDS access stands under a per-entry branch (each would be waited for on its own, sixteen round trips one after the
// other): a slot beyond the block's entries adds to a spare counter of its lane's and parks at its own index -- the places from m up
// are exactly those slots', and nothing reads them.
struct StrandTagSmem {
    static constexpr int CAP = TS_BLOCK * SB_ITEMS;
    alignas(16) u32 tags[CAP + 16];          // (+ 16: the neighbours read from a group's start on never leave the array)
    u32 cnts[CAP];
    // the groups' counts, then where they start (start[G] = the block's entries); from G + 8 on: what the slots beyond the block's
    // entries count, one word a lane, never read
    alignas(16) u32 start[SB_GROUPS + 8 + 64];
    u32 wsum[TS_BLOCK / 64];
};
// strand_tag_write ranks E entries a thread and round and reads the first F tags of their groups at once.  Measured (profiles/r27):
// E = 2, F = 4: 8.77 ms; E = 4, F = 4: 8.79; E = 2, F = 8: 8.12; E = 4, F = 8: 8.37 -- at ~3 entries a group nearly every wave has a lane
// whose group holds more than four, and with F = 4 the whole wave waits for that lane's second round trip
constexpr int SB_RANK_E = 2, SB_RANK_FIRST = 8;

// The block's m entries (nc of c, then those of mm) into LDS, grouped: sm.tags and sm.cnts group by group, sm.start as tile_group
// leaves it.  Ends with a barrier.
__device__ __forceinline__ void strand_tag_group(StrandTagSmem& sm, const u64* __restrict__ c, const u64* __restrict__ mm, u32 nc, u32 m,
                                                 int pack, int below, int gshift, int tid) {
    constexpr int G = SB_GROUPS, NW = TS_BLOCK / 64;
    static_assert(G == 4 * TS_BLOCK && StrandTagSmem::CAP <= 8192, "four groups a thread in the scan; group | place << 12 in a word");
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const u32 tmask = below >= 32 ? ~0u : (1u << below) - 1u, cmask = (u32)((1ull << pack) - 1ull);
    u32 tag[SB_ITEMS], cnt[SB_ITEMS];
#pragma unroll
    for (int j = 0; j < SB_ITEMS; j++) {
        // (a slot beyond the block loads the last entry again: sixteen loads and no branch)
        const u32 i = (u32)j * TS_BLOCK + tid, ic = i < m ? i : m - 1;
        const u64 w = ic < nc ? c[ic] : mm[ic - nc];
        tag[j] = __builtin_amdgcn_alignbit((u32)(w >> 32), (u32)w, (u32)pack) & tmask;          // (u32)(w >> pack): pack < 32
        cnt[j] = (u32)w & cmask;
    }
    reinterpret_cast<uint4*>(sm.start)[tid] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    u32 gp[SB_ITEMS];          // group | place in the group << 12
#pragma unroll
    for (int j = 0; j < SB_ITEMS; j++) {
        const u32 i = (u32)j * TS_BLOCK + tid;
        gp[j] = i < m ? tag[j] >> gshift : (u32)(G + 8 + lane);
    }
#pragma unroll
    for (int j = 0; j < SB_ITEMS; j++) gp[j] |= atomicAdd(&sm.start[gp[j]], 1u) << 12;
    __syncthreads();
    {
        // counts -> starts: four groups a thread, the waves' sums through LDS
        uint4* z = reinterpret_cast<uint4*>(sm.start);
        const uint4 cq = z[tid];
        const u32 sum = cq.x + cq.y + cq.z + cq.w;
        const u32 inc = wave_incl_scan_u32(sum);
        if (lane == 63) sm.wsum[wave] = inc;
        __syncthreads();
        u32 run = inc - sum;
#pragma unroll
        for (int w = 0; w < NW; w++) run += w < wave ? sm.wsum[w] : 0u;
        uint4 sq;
        sq.x = run; run += cq.x; sq.y = run; run += cq.y; sq.z = run; run += cq.z; sq.w = run;
        z[tid] = sq;
        if (tid == 0) sm.start[G] = m;
    }
    __syncthreads();
    u32 p[SB_ITEMS];
#pragma unroll
    for (int j = 0; j < SB_ITEMS; j++) p[j] = sm.start[gp[j] & 4095u];
#pragma unroll
    for (int j = 0; j < SB_ITEMS; j++) {
        const u32 i = (u32)j * TS_BLOCK + tid;
        p[j] = i < m ? p[j] + (gp[j] >> 12) : i;
    }
#pragma unroll
    for (int j = 0; j < SB_ITEMS; j++) { sm.tags[p[j]] = tag[j]; sm.cnts[p[j]] = cnt[j]; }
    __syncthreads();
}

// the grouped entries ranked in their groups and written: keys ((hi | tag) at place) to ok, counts to oc.  A thread ranks E entries a
// round, their three LDS round trips (entry, group bounds, the group's first SB_RANK_FIRST tags) overlapping.  The group is computed
// again from the tag (one shift) instead of travelling with the entry.
template <int E>
__device__ __forceinline__ void strand_tag_write(const StrandTagSmem& sm, u32 m, u64 hi, int gshift, u64* __restrict__ ok, u32* __restrict__ oc, int tid) {
    constexpr int F = SB_RANK_FIRST;
    static_assert(F + 3 <= 16, "the padding of StrandTagSmem::tags");
    // does the entry at q (tag to) of a group that ends at g1 go before the one at `at` (tag tm)?  No branch: a compare and a carry.
    // (C and M share no key and neither holds one twice; the tie-break by index keeps the places a permutation all the same)
    auto before = [](u32 to, u32 q, u32 g1, u32 tm, u32 at) -> u32 {
        return (u32)(q < g1) & ((u32)(to < tm) | ((u32)(to == tm) & (u32)(q < at)));
    };
    for (u32 i0 = (u32)tid; i0 < m; i0 += E * TS_BLOCK) {
        u32 at[E], mine[E], cnt[E], g0[E], g1[E], o[E][F], place[E];
#pragma unroll
        for (int e = 0; e < E; e++) {          // (an entry beyond the block: the first one again, its place is not used)
            at[e] = i0 + e * TS_BLOCK < m ? i0 + e * TS_BLOCK : 0u;
            mine[e] = sm.tags[at[e]];
            cnt[e] = sm.cnts[at[e]];
        }
#pragma unroll
        for (int e = 0; e < E; e++) {
            const u32 g = mine[e] >> gshift;
            g0[e] = sm.start[g]; g1[e] = sm.start[g + 1];
        }
#pragma unroll
        for (int e = 0; e < E; e++)
#pragma unroll
            for (int r = 0; r < F; r++) o[e][r] = sm.tags[g0[e] + r];
#pragma unroll
        for (int e = 0; e < E; e++) {
            u32 rank = 0;
#pragma unroll
            for (int r = 0; r < F; r++) rank += before(o[e][r], g0[e] + r, g1[e], mine[e], at[e]);
            for (u32 q0 = g0[e] + F; q0 < g1[e]; q0 += 4) {          // (a group of more)
                u32 p4[4];
#pragma unroll
                for (int r = 0; r < 4; r++) p4[r] = sm.tags[q0 + r];
#pragma unroll
                for (int r = 0; r < 4; r++) rank += before(p4[r], q0 + r, g1[e], mine[e], at[e]);
            }
            place[e] = g0[e] + rank;
        }
#pragma unroll
        for (int e = 0; e < E; e++) {
            if (i0 + e * TS_BLOCK >= m) break;
            ok[place[e]] = hi | mine[e];
            oc[place[e]] = cnt[e];
        }
    }
}

// One workgroup per block, two per CU.  Every entry of C_b and M_b is loaded once, grouped in LDS by the next 11 bits of its key, ranked
// in its group, and written to its place: the 64 lanes of a wave hold neighbours of the grouped order, so what a wave writes is a
// permutation of one contiguous run of the table (512 bytes of keys, 256 of counts).  Neither list needs to be sorted: the grouping
// reads only the block's number.  TAGS: the block-local form above (the launch takes it when the key bits below the block's fit 32,
// K <= 25); else tile_group's whole words.
template <bool TAGS>
__global__ __launch_bounds__(TS_BLOCK, 2 * TS_BLOCK / 256) void strand_block_union_kernel(StrandArgs a) {
    using S = std::conditional_t<TAGS, StrandTagSmem, StrandSmem>;
    constexpr u32 CAP = S::CAP;
    static_assert(sizeof(S) <= 80 * 1024, "two workgroups per CU");
    __shared__ S sm;
    const u32 b = blockIdx.x;
    const u64 nc = a.nwords[b], m0 = a.mstart[b], nm = a.mstart[b + 1] - m0;
    const u64 n = nc + nm;
    if (n == 0) return;
    if (n > CAP) {          // too large for a tile: strand_big_block_kernel's
        if (threadIdx.x == 0) a.declined[atomicAdd(a.n_declined, 1u)] = b;
        return;
    }
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const u32 m = (u32)n;
    const u64 out0 = a.incl[b] - nc + m0;
    if constexpr (TAGS) {
        strand_tag_group(sm, a.cw + a.cuts[b], a.m + m0, (u32)nc, m, a.pack, a.below, a.gshift, tid);
        if (strand_crowded(sm, tid)) {
            if (tid == 0) a.declined[atomicAdd(a.n_declined, 1u)] = b;
            return;
        }
        strand_tag_write<SB_RANK_E>(sm, m, (u64)b << a.below, a.gshift, a.ok + out0, a.oc + out0, tid);
    } else {
        const TileMap tm = tile_group<SB_ITEMS, SB_GROUPS, false>(sm, a.cw, nullptr, a.cuts[b], m, a.pshift, tid, a.m, m0, (u32)nc);
        if (strand_crowded(sm, tid)) {          // entries that crowd a few groups: the big blocks' kernel cuts the value range finer
            if (tid == 0) a.declined[atomicAdd(a.n_declined, 1u)] = b;
            return;
        }
        strand_write(sm, tm, m, a.ok + out0, a.oc + out0, a.pack, tid);
    }
}

// ---- the declined blocks, cut by value into sub-tiles ----------------------------------------------------------------------------
constexpr int SB_SPLIT = 256;          // splitters per block: 257 value ranges
struct StrandBigSmem {
    StrandSmem t;
    u64 sp[SB_SPLIT];                  // the splitters, sorted (while they are sorted: the samples)
    u32 cnt[SB_SPLIT + 2];             // entries of C_b and M_b per range, then the entries before each range
    u32 tile[SB_SPLIT + 2];            // the first range of each sub-tile, tile[ntiles] = 257
    u32 ntiles, gcount, fail;
};

// One workgroup per listed block (persistent over the list).  scratch: CAP words per workgroup, where a sub-tile's entries gather.
// Neither C_b nor M_b needs to be sorted: both are read whole to count the ranges and once more for every sub-tile.
__global__ __launch_bounds__(TS_BLOCK) void strand_big_block_kernel(StrandArgs a, u32 n_list, u64* __restrict__ scratch, u32* __restrict__ fail) {
    using S = StrandBigSmem;
    constexpr u32 CAP = StrandSmem::CAP, R = SB_SPLIT + 1;
    __shared__ S sm;
    u64* gat = scratch + (u64)blockIdx.x * CAP;
    const int lane = threadIdx.x & 63;
    for (u32 li = blockIdx.x; li < n_list; li += gridDim.x) {
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const u32 b = a.declined[li];
        const u64 nc = a.nwords[b], m0 = a.mstart[b], nm = a.mstart[b + 1] - m0, n = nc + nm;
        const u64* C = a.cw + a.cuts[b];
        const u64* M = a.m + m0;
        auto entry = [&](u64 i) -> u64 { return i < nc ? C[i] : M[i - nc]; };
        const u64 bmin = (u64)b << a.pshift, bmax = bmin | ((1ull << a.pshift) - 1ull);
        const u64 out0 = a.incl[b] - nc + m0;
        // 1. samples, evenly spaced over C_b and M_b together (all distinct keys: the two lists share none), sorted into splitters
        u64* cand = sm.t.keys;
        if (tid < SB_SPLIT) cand[tid] = entry((u64)tid * n / SB_SPLIT);
        if (tid == 0) { sm.fail = 0; sm.gcount = 0; }
        if (tid < (int)R + 1) sm.cnt[tid] = 0;
        __syncthreads();
        if (tid < SB_SPLIT) {
            const u64 v = cand[tid];
            u32 r = 0;
            for (int q = 0; q < SB_SPLIT; q++) { const u64 o = cand[q]; r += (o < v || (o == v && q < tid)) ? 1u : 0u; }
            sm.sp[r] = v;
        }
        __syncthreads();
        // 2. entries per range (range j: sp[j - 1] <= v < sp[j])
        auto range_of = [&](u64 v) -> u32 {
            u32 lo = 0, hi = SB_SPLIT;          // the number of splitters <= v
            while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (sm.sp[mid] <= v) lo = mid + 1; else hi = mid; }
            return lo;
        };
        for (u64 i = tid; i < n; i += TS_BLOCK) atomicAdd(&sm.cnt[range_of(entry(i))], 1u);
        __syncthreads();
        // 3. ranges packed into sub-tiles of at most CAP entries, in order; cnt becomes the entries before each range
        if (tid == 0) {
            u32 acc = 0, nt = 0, eb = 0;
            sm.tile[nt++] = 0;
            for (u32 j = 0; j < R; j++) {
                const u32 tot = sm.cnt[j];
                if (tot > CAP) { sm.fail = 1; break; }
                if (acc + tot > CAP) { sm.tile[nt++] = j; acc = 0; }
                acc += tot;
                sm.cnt[j] = eb;
                eb += tot;
            }
            sm.cnt[R] = eb;
            sm.tile[nt] = R;
            sm.ntiles = nt;
        }
        __syncthreads();
        if (sm.fail) {
            if (tid == 0) atomicOr(fail, 1u);
            continue;
        }
        const u32 ntiles = sm.ntiles;
        // 4. every sub-tile: its entries gathered (one pass over C_b and M_b), grouped over its own value range, written
        for (u32 t = 0; t < ntiles; t++) {
            const u32 ra = sm.tile[t], rb = sm.tile[t + 1];
            const u64 vlo = ra == 0 ? bmin : sm.sp[ra - 1];
            const u64 vhi = rb == R ? bmax : sm.sp[rb - 1] - 1;          // (sp[rb - 1] > vlo: the ranges between are not empty of values)
            const u32 m = sm.cnt[rb] - sm.cnt[ra];
            if (m == 0) continue;
            for (u64 i0 = 0; i0 < n; i0 += TS_BLOCK) {
                const u64 i = i0 + tid;
                const u64 v = i < n ? entry(i) : 0;
                const bool in = i < n && v >= vlo && v <= vhi;
                const u64 bal = __ballot(in);
                u32 base = 0;
                if (lane == 0 && bal) base = atomicAdd(&sm.gcount, (u32)__popcll(bal));
                base = (u32)__shfl((int)base, 0, 64);
                if (in) gat[base + popc_below(bal)] = v;
            }
            __threadfence_block();
            __syncthreads();
            const TileMap tm = tile_group<SB_ITEMS, SB_GROUPS, false>(sm.t, gat, nullptr, 0, m, a.pshift, tid, nullptr, 0, ~0u, true, vlo, vhi);
            if (strand_crowded(sm.t, tid)) {
                if (tid == 0) atomicOr(fail, 1u);
                break;
            }
            const u64 o = out0 + sm.cnt[ra];
            strand_write(sm.t, tm, m, a.ok + o, a.oc + o, a.pack, tid);
            if (tid == 0) sm.gcount = 0;
            __syncthreads();          // the tile's LDS and the gathered entries are free again
        }
        __syncthreads();
    }
}

// ---- the blocks of an unsorted dedupe, sorted in place (the strand route not taken after all) ------------------------------------
constexpr int DS_ITEMS = 22, DS_GROUPS = 4096;          // a tile of 11 264 words: the most a dedupe2_kernel table holds
typedef TileSortSmem<DS_ITEMS, DS_GROUPS, false> BlockSortSmem;
static_assert(BlockSortSmem::CAP == 11264, "a dedupe2_kernel table");

// One workgroup per CU, strided over the blocks.  A block of more words was counted by dedupe_kernel or the host, and is sorted.
__global__ __launch_bounds__(TS_BLOCK) void dedupe_sort_blocks_kernel(u64* __restrict__ w, const u64* __restrict__ cuts, const u64* __restrict__ nwords,
                                                                     u32 chunks, int pshift) {
    constexpr u32 CAP = BlockSortSmem::CAP;
    __shared__ BlockSortSmem sm;
    for (u32 v = blockIdx.x; v < chunks; v += gridDim.x) {
        const u64 n = nwords[v];
        if (n < 2 || n > CAP) continue;
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const u32 m = (u32)n;
        u64* out = w + cuts[v];
        const TileMap tm = tile_group<DS_ITEMS, DS_GROUPS, false>(sm, w, nullptr, cuts[v], m, pshift, tid);
        constexpr int E = 2;
        for (u32 i0 = (u32)tid; i0 < m; i0 += E * TS_BLOCK) {
            u32 i[E], place[E];
            u64 mine[E];
#pragma unroll
            for (int e = 0; e < E; e++) i[e] = i0 + e * TS_BLOCK;
            tile_rank<E, false>(sm, tm, i, m, mine, place);
#pragma unroll
            for (int e = 0; e < E; e++)
                if (i[e] < m) out[place[e]] = mine[e];
        }
        __syncthreads();          // the tile's LDS is free again
    }
}

int dedupe_sort_blocks(zk_ctx* c, DedupeResult& r) {
    if (!r.unsorted || r.n_out == 0) { r.unsorted = false; return ZK_OK; }
    // booked with the dedupe (whose sort it is): every word read and written once
    prof_begin(c, ZK_PROF_RLE, 16 * r.n_out);
    hipLaunchKernelGGL(dedupe_sort_blocks_kernel, dim3(r.chunks < (u32)c->num_cus ? r.chunks : (u32)c->num_cus), dim3(TS_BLOCK), 0, c->stream, r.work, r.cuts,
                       r.nwords, r.chunks, r.tag_bits + r.pack);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    r.unsorted = false;
    return ZK_OK;
}

// The table of both strands from the block dedupe's result r (odd K, every count in the field): see the top of the file.  keys_buf holds
// buf_words words and is free; r.work must hold C's words until the union is done.
int strand_blocks(zk_ctx* c, const DedupeResult& r, u64* keys_buf, uint64_t buf_words, int K, u64* out_k, u32* out_c, uint64_t cap,
                  uint64_t* n_out) {
    *n_out = 0;
    const uint64_t uc = r.n_out;
    if (uc == 0) return ZK_OK;
    if (!(K & 1) || r.n_big || r.chunks != (1u << SB_BLOCK_BITS)) return fail(c, ZK_EINTERNAL, "strand_blocks: K %d, %u big counts, %u blocks", K, r.n_big, r.chunks);
    const uint64_t a8w = ((8 * uc + 255) & ~255ull) / 8;
    if (2 * a8w > buf_words) return fail(c, ZK_EINTERNAL, "strand_blocks: %llu words do not fit twice in %llu", (unsigned long long)uc, (unsigned long long)buf_words);
    if (2 * uc > cap) return fail(c, ZK_ENOSPC, "output holds %llu entries, the table has %llu", (unsigned long long)cap, (unsigned long long)(2 * uc));
    const int pk = r.pack, key_bits = 2 * K + pk, lo_bit = key_bits - SB_BLOCK_BITS;
    u64* mw = keys_buf;
    u64* malt = keys_buf + a8w;
    // 1. M, densely, with the digit counts of its passes.  The dedupe has written it (all but the blocks it declined), if there is room for
    // the passes' second buffer before or behind it and the digits it counted are the ones the passes will take
    MirrorHist mh = {};
    bool fused = r.m_emitted && r.m_words >= keys_buf && r.m_words + r.m_cap <= keys_buf + buf_words && uc <= r.m_cap && c->sort_variant == 3;
    if (fused) {
        const PassPlan plan = sort_plan_upper(c, key_bits, lo_bit);
        fused = plan.passes == r.mh.passes;
        for (int p = 0; fused && p < plan.passes; p++) fused = plan.shift[p] == r.mh.shift[p] && plan.bits[p] == r.mh.bits[p];
        const uint64_t before = (uint64_t)(r.m_words - keys_buf), behind = buf_words - before;
        if (before < a8w && behind < 2 * a8w) fused = false;
        if (fused) malt = before >= a8w ? keys_buf : r.m_words + a8w;
    }
    if (fused) {
        mw = r.m_words;
        mh = r.mh;
        uint64_t placed = r.m_placed;
        // (the step's record and its algorithmic bytes are the same whoever writes the words: a step's records add up alike on either form)
        prof_begin(c, ZK_PROF_SELECT, 16 * uc);
        if (r.n_retry) {
            // the blocks the dedupe declined (65 536 keys or more, a table that filled up: counted by dedupe_kernel or the host since)
            hipLaunchKernelGGL(strand_mirror_kernel, dim3(grid_cap(c, r.n_retry, 8)), dim3(256), 0, c->stream, r.work, r.cuts, r.incl, r.nwords, r.n_retry, pk, K,
                               mw, mh, r.retry, &c->d_scalars->dedupe_m_cursor, (u64)r.m_cap);
        }
        prof_end(c);
        if (r.n_retry) {
            ZK_HIP(c, hipGetLastError());
            ZK_TRY(fetch(c, &c->h_scalars->dedupe_m_cursor));
            ZK_TRY(stream_sync(c));
            placed = c->h_scalars->dedupe_m_cursor;
        }
        // (the passes scatter by the digit counts: they must be the counts of exactly the uc words that are there)
        if (placed != uc) return fail(c, ZK_EINTERNAL, "strand_blocks: %llu mirror words for %llu entries", (unsigned long long)placed, (unsigned long long)uc);
    } else {
        if (c->sort_variant == 3) {
            const PassPlan plan = sort_plan_upper(c, key_bits, lo_bit);
            if (plan.passes <= 4) {
                ZK_TRY(arena_alloc(c, sizeof(u64) * MAX_PASSES * 512, (void**)&mh.raw));
                ZK_HIP(c, hipMemsetAsync(mh.raw, 0, sizeof(u64) * MAX_PASSES * 512, c->stream));
                mh.passes = plan.passes;
                for (int p = 0; p < plan.passes; p++) { mh.shift[p] = plan.shift[p]; mh.bits[p] = plan.bits[p]; }
            }
        }
        prof_begin(c, ZK_PROF_SELECT, 16 * uc);
        hipLaunchKernelGGL(strand_mirror_kernel, dim3((u32)c->num_cus * 8), dim3(256), 0, c->stream, r.work, r.cuts, r.incl, r.nwords, r.chunks, pk, K, mw, mh,
                           (const u32*)nullptr, (u64*)nullptr, (u64)0);
        prof_end(c);
        ZK_HIP(c, hipGetLastError());
    }
    // 2. grouped by its top 18 key bits
    u64* sk = nullptr;
    if (mh.passes) ZK_TRY(sort_keys_upper_counted(c, mw, malt, uc, key_bits, lo_bit, mh.raw, &sk));
    else ZK_TRY(sort_keys_upper(c, mw, malt, uc, key_bits, lo_bit, &sk));
    // 3. where its blocks start, 4. the union, block by block
    u64* mstart;
    u32* declined;
    ZK_TRY(arena_alloc(c, sizeof(u64) * ((1ull << SB_BLOCK_BITS) + 1), (void**)&mstart));
    ZK_TRY(arena_alloc(c, sizeof(u32) * r.chunks, (void**)&declined));
    StrandArgs a = {};
    a.cw = r.work; a.cuts = r.cuts; a.nwords = r.nwords; a.incl = r.incl; a.m = sk; a.mstart = mstart;
    a.ok = out_k; a.oc = out_c; a.pack = pk; a.pshift = lo_bit;
    a.below = 2 * K - SB_BLOCK_BITS; a.gshift = a.below > 11 ? a.below - 11 : 0;
    a.n_declined = &c->d_scalars->strand.n_declined;
    a.declined = declined;
    u32* fail = &c->d_scalars->strand.fail;
    prof_begin(c, ZK_PROF_UNION, 8 * 2 * uc + 12 * 2 * uc);
    hipLaunchKernelGGL(strand_starts_kernel, dim3(((1u << SB_BLOCK_BITS) + 256) / 256), dim3(256), 0, c->stream, sk, (u64)uc, lo_bit, mstart);
    ZK_HIP(c, hipMemsetAsync(&c->d_scalars->strand, 0, sizeof(zk_strand_counters), c->stream));
    if (a.below <= 32) hipLaunchKernelGGL(strand_block_union_kernel<true>, dim3(r.chunks), dim3(TS_BLOCK), 0, c->stream, a);
    else hipLaunchKernelGGL(strand_block_union_kernel<false>, dim3(r.chunks), dim3(TS_BLOCK), 0, c->stream, a);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(fetch(c, &c->h_scalars->strand));
    ZK_TRY(check_device_error(c));
    const uint32_t n_declined = c->h_scalars->strand.n_declined;
    bool other_way = n_declined && c->strand_blocks == 3;          // (tests: the declined blocks the other way)
    if (n_declined && !other_way) {
        // the declined blocks alone, cut by value into sub-tiles (their bytes: booked as the blocks' share of the union above)
        const uint32_t grid = n_declined < 2u * (uint32_t)c->num_cus ? n_declined : 2u * (uint32_t)c->num_cus;
        u64* scratch;
        ZK_TRY(arena_alloc(c, sizeof(u64) * StrandSmem::CAP * grid, (void**)&scratch));
        prof_begin(c, ZK_PROF_UNION, 0);
        hipLaunchKernelGGL(strand_big_block_kernel, dim3(grid), dim3(TS_BLOCK), 0, c->stream, a, n_declined, scratch, fail);
        prof_end(c);
        ZK_HIP(c, hipGetLastError());
        ZK_TRY(fetch(c, &c->h_scalars->strand));
        ZK_TRY(check_device_error(c));
        other_way = c->h_scalars->strand.fail != 0;
    }
    if (!other_way) {
        *n_out = 2 * uc;
        return ZK_OK;
    }
    // A range of a declined block did not fit a tile: the whole union the other way, from what is still there -- C's words in r.work, M in sk
    // (C's blocks sorted first, if the dedupe left them unsorted: the union merges two sorted lists)
    DedupeResult rs = r;
    ZK_TRY(dedupe_sort_blocks(c, rs));
    char* aux;
    ZK_TRY(aux_require(c, 8 * a8w, &aux));
    ZK_TRY(dedupe_finish(c, rs, (u64*)aux, nullptr, nullptr, K, 0, nullptr, nullptr, true));
    u64* ms = nullptr;
    ZK_TRY(sort_keys_upper(c, sk, sk == mw ? malt : mw, uc, key_bits, pk, &ms));
    return union_sum_packed_ab(c, (const u64*)aux, uc, ms, uc, pk, out_k, out_c, cap, n_out, true);
}

}  // namespace zk
