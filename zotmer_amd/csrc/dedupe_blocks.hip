// dedupe_blocks.hip -- the block dedupe: the keys of a block counted and sorted in an LDS table, one workgroup per CU.
#include "internal.hpp"
#include "dedupe.hpp"

namespace zk {

// ---------------------------------------------------------------------------------------
// Block dedupe (zk_kmerize, canonical keys; see pipeline.hip::kmerize_full): counting AND finishing the sort in LDS.
//
// After LSD passes over the TOP b bits of the keys, the keys that share those bits form a block -- and all copies of a k-mer
// lie in one block (they share every bit).  While a block is small (n / 2^b keys; 23.7 K after two passes on config 2) one
// workgroup counts it in an LDS hash table: a compare-and-swap claims an entry for a key's remaining bits (its tag), an add
// counts the copy.  The block's entries (~3 K distinct tags) are then sorted right there: a counting sort on the tag's top byte
// (LDS counters), and inside each byte's group of a dozen entries the place is the number of smaller tags.  The block's
// distinct k-mers therefore leave the kernel SORTED, and the blocks are in the order of their top bits: the counted list
// needs no further sort pass at all.
// The copies of a k-mer are spread over the whole block (unlike in the tile-local table variant that was measured for
// collapse_kernel, where they sit in the same 64 lanes), so the atomics rarely collide.
// Words (key << pack | count) go to the block's own place in `out` (its input offset: never more words than keys);
// dedupe_unpack_kernel moves them together and splits them into keys and counts.  A count beyond the field leaves the field 0
// and goes to a side list that patches the count afterwards.  A table that fills up (more than ~6 K distinct keys in a block:
// little duplication) raises a flag and the caller sorts the keys the long way -- the result never depends on the table.
// ---------------------------------------------------------------------------------------
// TAG32: a tag fits 32 bits: entries of 4 + 4 bytes.  The blocks are not of one size -- a canonical k-mer more often starts with
// A than with T (it is the smaller strand), so the sizes spread from ~0 to 2 x the mean with the first bases; the table is sized
// for the big ones: one 1024-thread workgroup per CU.
template <bool TAG32>
struct DedupeSmem {
    static constexpr int BLOCK = 1024, ITEMS = 8, TILE = BLOCK * ITEMS, NW = BLOCK / 64, ALL = TAG32 ? 12288 : 6144, SPT = ALL / BLOCK, NB = 256;
    // a wave's side list: what one tile can add at worst (64 * ITEMS) on top of what is left standing after a tile (SIDE_KEEP)
    static constexpr int SIDE_KEEP = 128, SIDE = SIDE_KEEP + 64 * ITEMS;
    typedef typename std::conditional<TAG32, u32, u64>::type E;
    E keys[ALL];             // tags (after the count: the entries again, grouped by their top byte)
    u32 cnt[ALL];
    E side[NW][SIDE];
    u32 bc[NB];              // entries per top byte of the tag
    u32 bbase[NB + 1];       // ... before it
    u32 bfill[NB];
    u32 ticket;
};

// cuts[v] = first index whose key >> tag_bits is >= v, v = 0 .. blocks
__global__ void dedupe_cuts_kernel(const u64* __restrict__ k, u64 n, int tag_bits, u32 blocks, u64* __restrict__ cuts) {
    const u32 v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v > blocks) return;
    u64 lo = 0, hi = n;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if ((k[mid] >> tag_bits) < (u64)v) lo = mid + 1; else hi = mid;
    }
    cuts[v] = lo;
}

// ticket -> block: the blocks in order, or (second chance of the blocks dedupe2_kernel declined) the ones on a list
__device__ __forceinline__ u32 dedupe_block_of(const DedupeArgs& a, u32 ticket) { return a.list ? a.list[ticket] : ticket; }

// what a workgroup carries from one block to the next: the block it is about to count (its ticket), with the first tile of its keys
// already asked for -- the ticket, the bounds and those keys travel while the previous block is being sorted and written
template <int ITEMS>
struct DedupeNext {
    u32 chunk;
    u64 lo, hi;
    u64 key[ITEMS];
};

template <bool TAG32, bool TAGIN>
__device__ __forceinline__ void dedupe_block(const DedupeArgs& a, DedupeSmem<TAG32>& sm, DedupeNext<DedupeSmem<TAG32>::ITEMS>& st, u32 (&ph)[8], u32& tlast) {
    using S = DedupeSmem<TAG32>;
    using E = typename S::E;
    constexpr int BLOCK = S::BLOCK, ITEMS = S::ITEMS, TILE = S::TILE, ALL = S::ALL, SPT = S::SPT, NB = S::NB;
    constexpr E EMPTY = (E)~(E)0;            // no entry.  A 64-bit tag never has all its bits set; a 32-bit one may: see `home`
    constexpr u32 HS = TAG32 ? ALL - 1 : ALL;          // ... then the last entry belongs to the all-ones tag alone
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const u32 chunk = dedupe_block_of(a, st.chunk);
    const u64 lo = st.lo, hi = st.hi;
    const u32 maxc = (1u << a.pack) - 1u;
    // whole tiles: one address, constant offsets; the cut last tile: per-key bounds
    auto load = [&](u64 base, u64 end, u64 (&k)[ITEMS]) {
        if constexpr (TAGIN) {
            // (a tag is a whole key as far as the table goes: the block's bits are added when the words are written)
            if (base + TILE <= end) {
                // four tags per load (16 bytes a lane, a kilobyte a wave instruction; which thread takes which key is the table's
                // business alone); a block starts wherever it starts: the loads are 4-byte aligned, no more
                struct __attribute__((packed, aligned(4))) Tag4 { u32 a, b, c, d; };
                static_assert(ITEMS % 4 == 0, "whole quads");
#pragma unroll
                for (int i = 0; i < ITEMS / 4; i++) {
                    const Tag4 q = *reinterpret_cast<const Tag4*>(a.tin + base + (u64)i * (4 * BLOCK) + 4 * tid);
                    k[4 * i] = q.a; k[4 * i + 1] = q.b; k[4 * i + 2] = q.c; k[4 * i + 3] = q.d;
                }
            } else {
#pragma unroll
                for (int i = 0; i < ITEMS; i++) {
                    const u64 g = base + (u64)i * BLOCK + tid;
                    k[i] = g < end ? (u64)a.tin[g] : ~0ull;
                }
            }
        } else if (base + TILE <= end) {
            const u64* p = a.kin + base + tid;
#pragma unroll
            for (int i = 0; i < ITEMS; i++) k[i] = p[i * BLOCK];
        } else {
#pragma unroll
            for (int i = 0; i < ITEMS; i++) {
                const u64 g = base + (u64)i * BLOCK + tid;
                k[i] = g < end ? a.kin[g] : ~0ull;
            }
        }
    };
    if (tid == 0) sm.ticket = atomicAdd(a.counter, 1u);          // the block after this one: read after the next barrier
    if (hi <= lo) {
        if (tid == 0) a.nwords[chunk] = 0;
        if (a.sub && tid < 64) a.sub[(u64)chunk * 64 + tid] = 0;
        __syncthreads();
        st.chunk = (u32)__builtin_amdgcn_readfirstlane((int)sm.ticket);
        st.lo = st.hi = 0;
        if (st.chunk < a.chunks) { const u32 nb = dedupe_block_of(a, st.chunk); st.lo = a.cuts[nb]; st.hi = a.cuts[nb + 1]; }
        if (st.hi > st.lo) load(st.lo, st.hi, st.key);
        return;
    }
    for (int q = tid; q < ALL * (int)sizeof(E) / 16; q += BLOCK) reinterpret_cast<uint4*>(sm.keys)[q] = make_uint4(~0u, ~0u, ~0u, ~0u);
    for (int q = tid; q < ALL / 4; q += BLOCK) reinterpret_cast<uint4*>(sm.cnt)[q] = make_uint4(0, 0, 0, 0);
    if (tid < NB) { sm.bc[tid] = 0; sm.bfill[tid] = 0; }
    __syncthreads();
    DD_PHASE(0);          // table cleared
    const u32 nchunk = (u32)__builtin_amdgcn_readfirstlane((int)sm.ticket);
    u64 nlo = 0, nhi = 0;
    if (nchunk < a.chunks) { const u32 nb = dedupe_block_of(a, nchunk); nlo = a.cuts[nb]; nhi = a.cuts[nb + 1]; }
    u32 bad = 0;
    // The kernel is bound by its instruction count (188 per key with several keys probing at once, 88 with one tight probing
    // loop per key -- a loop runs as long as the unluckiest of its 64 lanes).  So the common case has NO loop and no branch:
    // one compare-and-swap at the key's home entry, the count added as 1 or 0 (adding 0 to another key's entry harms nobody);
    // a key that finds another key at home goes to the wave's side list (its place from a ballot, no atomic), and the lists --
    // about a tenth of the distinct keys with all their copies -- are inserted by linear probing afterwards, full wavefronts.
    // (An order-preserving "hash" -- the tag scaled to the table -- would leave the table sorted, but the error variants of a
    // k-mer differ from it in a few low bits and all want the same entry: 45 ms instead of 17.)
    const u64 tmask = (1ull << a.tag_bits) - 1;
    u32 nside = 0;          // entries in this wave's side list (the same in every lane)
    auto home = [&](E e) -> u32 {
        // the all-ones 32-bit tag (= the empty marker) has the last entry to itself: there the swap of "empty" for "empty"
        // succeeds and leaves the word as it is; no other key is ever sent there
        u32 x;
        if constexpr (TAG32) x = (u32)e * 0x9E3779B1u; else x = ((u32)((u64)e >> 24) ^ ((u32)e * 0x85EBCA6Bu)) * 0x9E3779B1u;
        if (TAG32 && e == EMPTY) return HS;
        return (u32)(((u64)x * HS) >> 32);
    };
    auto cas = [&](u32 h, E e) -> E {
        if constexpr (TAG32) return atomicCAS(&sm.keys[h], EMPTY, e);
        else return (E)atomicCAS(reinterpret_cast<unsigned long long*>(&sm.keys[h]), (unsigned long long)EMPTY, (unsigned long long)e);
    };
    auto drain = [&]() {          // the wave's side list into the table by linear probing, 64 entries at a time
        for (u32 i = (u32)lane; i < nside; i += 64) {
            const E e = sm.side[wave][i];
            u32 h = home(e) + 1;          // its home entry is taken: that is why it is here
            h = h == HS ? 0u : h;
            int p = 0;
            for (; p < ALL; p++) {
                const E old = cas(h, e);
                if (old == EMPTY || old == e) break;
                h = h + 1 == HS ? 0u : h + 1;
            }
            if (p < ALL) atomicAdd(&sm.cnt[h], 1u); else bad = 1;
        }
        nside = 0;
    };
    // (Measured: the eight compare-and-swaps of a tile issued back to back before any answer is used -- 24.6 ms against 21.3: the
    // insert is bound by the LDS atomic unit's throughput (two atomics per key, ~47 K per block), not by the round trips.)
    auto insert = [&](u64 k, bool valid) {
        const E e = (E)(k & tmask);
        const u32 h = home(e);
        const E old = valid ? cas(h, e) : e;          // (a plain read first, the swap only for the lanes that see "empty": no faster)
        const bool ok = old == EMPTY || old == e;
        atomicAdd(&sm.cnt[h], (ok && valid) ? 1u : 0u);
        const u64 m = __ballot(!ok);
        if (m) {
            if (!ok) sm.side[wave][nside + popc_below(m)] = e;
            nside += (u32)__popcll(m);
        }
    };
    u64 key[ITEMS], nk[ITEMS];
#pragma unroll
    for (int i = 0; i < ITEMS; i++) key[i] = st.key[i];          // the first tile was asked for during the previous block
    for (u64 base = lo; base < hi; base += TILE) {
        if (base + TILE < hi) load(base + TILE, hi, nk);
        if (base + TILE <= hi) {
#pragma unroll
            for (int i = 0; i < ITEMS; i++) insert(key[i], true);
        } else {
#pragma unroll
            for (int i = 0; i < ITEMS; i++) insert(key[i], key[i] != ~0ull);
        }
#pragma unroll
        for (int i = 0; i < ITEMS; i++) key[i] = nk[i];
        if (nside > (u32)S::SIDE_KEEP || base + TILE >= hi) drain();
    }
    DD_PHASE(1);          // keys inserted
    st.chunk = nchunk; st.lo = nlo; st.hi = nhi;
    if (nhi > nlo) load(nlo, nhi, st.key);          // the next block's first tile travels while this one is sorted and written
    const int any_bad = __syncthreads_or((int)bad);
    DD_PHASE(2);          // ... every wave done
    if (any_bad) {
        // the table filled up (a block with more distinct keys than it holds): the block goes on the list of those the host
        // counts by sorting; only when that list is full is the whole run given up
        if (tid == 0) {
            const u32 at = atomicAdd(a.n_bad, 1u);
            if (at < a.bad_cap) a.bad[at] = chunk; else atomicOr(a.flags, 1u);
            a.nwords[chunk] = 0;
        }
        if (a.sub && tid < 64) a.sub[(u64)chunk * 64 + tid] = 0;
        return;
    }
    // ---- the block's entries, sorted: a counting sort on the tag's top byte, then ranks inside each byte's group ---------
    // thread t takes the entries t, t + BLOCK, ... into registers; the table's memory then takes them back grouped
    E et[SPT];
    u32 ec[SPT];
    const int bsh = a.tag_bits > 8 ? a.tag_bits - 8 : 0;
#pragma unroll
    for (int j = 0; j < SPT; j++) {
        et[j] = sm.keys[tid + j * BLOCK];
        ec[j] = sm.cnt[tid + j * BLOCK];
        if (ec[j]) atomicAdd(&sm.bc[(u32)((u64)et[j] >> bsh) & (NB - 1)], 1u);
    }
    __syncthreads();
    DD_PHASE(3);          // entries read, byte groups counted
    if (wave == 0) {
        u32 c4[4], sum = 0;
#pragma unroll
        for (int r = 0; r < 4; r++) { c4[r] = sm.bc[4 * lane + r]; sum += c4[r]; }
        const u32 inc = wave_incl_scan_u32(sum);
        u32 run = inc - sum;
#pragma unroll
        for (int r = 0; r < 4; r++) { sm.bbase[4 * lane + r] = run; run += c4[r]; }
        if (lane == 63) sm.bbase[NB] = inc;
    }
    __syncthreads();
    const u32 total = sm.bbase[NB];
    if (tid == 0) a.nwords[chunk] = total;
    if (a.sub && tid < 64) a.sub[(u64)chunk * 64 + tid] = sm.bbase[4 * tid + 4] - sm.bbase[4 * tid];          // four top bytes = one 6-bit start
#pragma unroll
    for (int j = 0; j < SPT; j++) {
        if (ec[j]) {
            const u32 b = (u32)((u64)et[j] >> bsh) & (NB - 1);
            const u32 p = sm.bbase[b] + atomicAdd(&sm.bfill[b], 1u);
            sm.keys[p] = et[j];
            sm.cnt[p] = ec[j];
        }
    }
    __syncthreads();
    DD_PHASE(4);          // grouped by top byte
    const u64 hi_part = (u64)chunk << a.tag_bits;          // the bits every key of the block has above its tag
    for (u32 i = (u32)tid; i < total; i += BLOCK) {
        const E mine = sm.keys[i];
        const u32 b = (u32)((u64)mine >> bsh) & (NB - 1);
        const u32 g0 = sm.bbase[b], g1 = sm.bbase[b + 1];
        u32 rank = 0;
        for (u32 q = g0; q < g1; q++) rank += sm.keys[q] < mine ? 1u : 0u;
        const u32 c = sm.cnt[i];
        const u64 k = hi_part | (u64)mine;
        if (c > maxc) {
            const u32 at = atomicAdd(a.n_big, 1u);
            if (at < a.big_cap) { a.big[2 * (u64)at] = k; a.big[2 * (u64)at + 1] = c; }
            atomicOr(a.flags, 2u);
        }
        a.out[lo + g0 + rank] = (k << a.pack) | (u64)(c > maxc ? 0u : c);
    }
    DD_PHASE(5);          // ranked and written
}

// Persistent: one workgroup per CU (the table takes most of its LDS) draws the blocks from a counter -- in order, not strided:
// the sizes go with the first bases, a stride of the grid would give one workgroup all the big ones.
template <bool TAG32, bool TAGIN = false>
__global__ __launch_bounds__(1024, 4) void dedupe_kernel(DedupeArgs a) {
    using S = DedupeSmem<TAG32>;
    static_assert(TAG32 || !TAGIN, "32-bit tags in, 32-bit tags in the table");
    __shared__ S sm;
    DedupeNext<S::ITEMS> st;
    if (threadIdx.x == 0) sm.ticket = atomicAdd(a.counter, 1u);
    __syncthreads();
    st.chunk = (u32)__builtin_amdgcn_readfirstlane((int)sm.ticket);
    st.lo = st.hi = 0;
    if (st.chunk < a.chunks) { const u32 nb = dedupe_block_of(a, st.chunk); st.lo = a.cuts[nb]; st.hi = a.cuts[nb + 1]; }
#pragma unroll
    for (int i = 0; i < S::ITEMS; i++) {
        const u64 g = st.lo + (u64)i * S::BLOCK + threadIdx.x;
        if constexpr (TAGIN) st.key[i] = g < st.hi ? (u64)a.tin[g] : ~0ull;
        else st.key[i] = g < st.hi ? a.kin[g] : ~0ull;
    }
    __syncthreads();          // the ticket word is free again
    u32 ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    u32 tlast = a.dbg ? (u32)__builtin_amdgcn_s_memtime() : 0u;
    (void)tlast;
    u32 nblk = 0;
    while (st.chunk < a.chunks) {
        dedupe_block<TAG32, TAGIN>(a, sm, st, ph, tlast);          // leaves the next block in st
        __syncthreads();          // the table and the ticket word are free again
        DD_PHASE(6);
        nblk++;
    }
    if (a.dbg && threadIdx.x == 0) {
        for (int k = 0; k < 8; k++) a.dbg[(u64)blockIdx.x * 16 + k] = ph[k];
        a.dbg[(u64)blockIdx.x * 16 + 8] = nblk;
    }
}

// the words of the blocks, moved together and taken apart: block v's words -> keys / counts [incl[v] - nwords[v], incl[v])
// out_m (or null): beside them the mirrored words (rc(key) << pack | count), already grouped by their low block bits -- block v of
// the list IS group rc(v) of the mirror list (the first bases of a k-mer are the last of its reverse complement), and minc holds
// the groups' inclusive ends: the first stage of the mirror sort comes for free with the copy that is made anyway.

__global__ __launch_bounds__(256) void dedupe_unpack_kernel(const u64* __restrict__ in, const u64* __restrict__ cuts, const u64* __restrict__ incl,
                                                            const u64* __restrict__ nwords, u32 chunks, int pack, u64* __restrict__ out_k,
                                                            u32* __restrict__ out_c, u64* __restrict__ out_m, const u64* __restrict__ minc,
                                                            int K, int gbases, MirrorHist mh, const u64* __restrict__ place24, int packed_out) {
    __shared__ u32 bins[4 * 512];          // the digit histograms of the mirror sort's passes: it reads every word anyway
    const bool hist = out_m && mh.passes > 0;
    if (hist) {
        for (int q = threadIdx.x; q < 4 * 512; q += blockDim.x) bins[q] = 0;
        __syncthreads();
    }
    const u64 maxc = (1ull << pack) - 1;
    for (u32 v = blockIdx.x; v < chunks; v += gridDim.x) {
        const u64 cnt = nwords[v];
        const u64 dst0 = incl[v] - cnt;
        const u64* src = in + cuts[v];
        const u64 mdst = (out_m && !place24) ? minc[(u32)revcomp(gbases, (u64)v)] - cnt : 0;
        const int t6 = 2 * K - 2 * gbases - 6;          // where the 6 bits after the block bits sit in a key
        // four words of a thread in flight at a time (a block is ~3 K words: twelve rounds of one load each otherwise)
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
                const u64 w = w4[q];
                if (packed_out) out_k[dst0 + i] = w;          // (the union reads the words as they are: 12 bytes less moved per entry)
                else { out_k[dst0 + i] = w >> pack; out_c[dst0 + i] = (u32)(w & maxc); }
                if (out_m) {
                    const u64 mw = (revcomp(K, w >> pack) << pack) | (w & maxc);
                    // place24: grouped by 6 more bits -- the block is sorted, so the words that share their next three bases are
                    // a run of it, and place24[v][those 6 bits] + i is the run's place in the group of the mirrored words
                    const u64 at = place24 ? place24[(u64)v * 64 + ((u32)(w >> (pack + t6)) & 63u)] + i : mdst + i;
                    out_m[at] = mw;
                    if (hist) {
#pragma unroll
                        for (int p = 0; p < 4; p++)
                            if (p < mh.passes) atomicAdd(&bins[p * 512 + ((u32)(mw >> mh.shift[p]) & ((1u << mh.bits[p]) - 1u))], 1u);
                    }
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

// msz24[g] = words of the run (block v, 6-bit start j) whose mirror image is group g = rc3(j) << (2 gbases) | rc(v)
__global__ void dedupe_mirror_sizes24_kernel(const u32* __restrict__ sub, u32 chunks, int gbases, u64* __restrict__ msz) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (u64)chunks * 64) return;
    const u32 v = (u32)revcomp(gbases, g & ((u64)chunks - 1)), j = (u32)revcomp(3, g >> (2 * gbases));
    msz[g] = sub[(u64)v * 64 + j];
}
// place24[v][j] = (start of group g(v, j) in the mirror list) - (start of the run inside block v): add the word's index in the block
__global__ void dedupe_mirror_place24_kernel(const u32* __restrict__ sub, const u64* __restrict__ minc24, u32 chunks, int gbases,
                                             u64* __restrict__ place) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;          // one wavefront per block: lane = j
    const u32 v = (u32)(t >> 6), j = (u32)(t & 63);
    if (v >= chunks) return;
    const u32 x = sub[(u64)v * 64 + j];
    const u32 before = wave_incl_scan_u32(x) - x;
    const u64 g = ((u64)revcomp(3, (u64)j) << (2 * gbases)) | revcomp(gbases, (u64)v);
    place[(u64)v * 64 + j] = minc24[g] - x - before;
}

// msz[g] = words of the block whose mirror image is group g
__global__ void dedupe_mirror_sizes_kernel(const u64* __restrict__ nwords, u32 chunks, int gbases, u64* __restrict__ msz) {
    const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < chunks) msz[g] = nwords[(u32)revcomp(gbases, (u64)g)];
}

// the counts that did not fit a word: found again by key in the sorted list
__global__ void dedupe_big_kernel(const u64* __restrict__ big, u32 n_big, const u64* __restrict__ k, u64 n, u32* __restrict__ c, u32* err) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_big) return;
    const u64 key = big[2 * (u64)t], cnt = big[2 * (u64)t + 1];
    u64 lo = 0, hi = n;
    while (lo < hi) { const u64 mid = (lo + hi) >> 1; if (k[mid] < key) lo = mid + 1; else hi = mid; }
    if (lo < n && k[lo] == key) c[lo] = (u32)cnt; else atomicOr(err, ZK_DERR_CAPACITY);
}

__global__ void expand_tags_kernel(const u32* __restrict__ tags, const u64* __restrict__ cuts, u64 first_block, u64 n_blocks, int tag_bits, u64* __restrict__ out) {
    for (u64 v = first_block + blockIdx.x; v < first_block + n_blocks; v += gridDim.x) {
        const u64 lo = cuts[v], hi = cuts[v + 1], top = v << tag_bits;
        for (u64 i = lo + threadIdx.x; i < hi; i += blockDim.x) out[i] = top | (u64)tags[i];
    }
}

int expand_tags(zk_ctx* c, const u32* tags, const u64* cuts, uint32_t blocks, int tag_bits, u64* keys_out, uint64_t first_block, uint64_t n_blocks) {
    if (n_blocks == 0) { first_block = 0; n_blocks = blocks; }
    hipLaunchKernelGGL(expand_tags_kernel, dim3(grid_cap(c, n_blocks, 16)), dim3(256), 0, c->stream, tags, cuts, (u64)first_block, (u64)n_blocks,
                       tag_bits, keys_out);
    ZK_HIP(c, hipGetLastError());
    return ZK_OK;
}

constexpr u32 DEDUPE_BIG_CAP = 1u << 16;          // counts beyond the packed field: entries of the side list
constexpr u32 DEDUPE_BAD_CAP = 64;                // blocks whose table filled up: entries of the list the host counts by sorting

// ---- dedupe_pass, stage 1: the lists (block starts, words per block, the side lists) and the kernels' arguments ----
// The lists go to *r at once; r->unsorted says whether dedupe2_kernel may leave its blocks in table order.
static int dedupe_lists(zk_ctx* c, const u64* keys, uint64_t n, int key_bits, int b, int pack, u64* work, uint64_t max_chunks,
                        const u32* tags, const u64* tag_cuts, bool unsorted, bool two_per_cu, const DedupeMirror* mirror, DedupeArgs& a, DedupeResult* r) {
    uint64_t chunks = 1ull << b;          // one block per value of the top bits
    if (max_chunks && chunks > max_chunks) chunks = max_chunks;
    u64 *cuts, *nwords, *incl, *big;
    if (tags) {
        if (!tag_cuts || key_bits - b > 32) return fail(c, ZK_EINTERNAL, "dedupe_pass: tags of %d bits", key_bits - b);
        cuts = const_cast<u64*>(tag_cuts);
    } else ZK_TRY(arena_alloc(c, sizeof(u64) * (chunks + 1), (void**)&cuts));
    ZK_TRY(arena_alloc(c, sizeof(u64) * chunks, (void**)&nwords));
    ZK_TRY(arena_alloc(c, sizeof(u64) * chunks, (void**)&incl));
    ZK_TRY(arena_alloc(c, sizeof(u64) * 2 * DEDUPE_BIG_CAP, (void**)&big));
    a.tag_bits = key_bits - b;
    if (!tags) hipLaunchKernelGGL(dedupe_cuts_kernel, dim3((u32)div_up(chunks + 1, 256)), dim3(256), 0, c->stream, keys, (u64)n, a.tag_bits, (u32)chunks, cuts);
    a.kin = keys; a.tin = tags; a.n = n; a.cuts = cuts; a.out = work; a.nwords = nwords; a.pack = pack;
    a.chunks = (u32)chunks;
    a.flags = (u32*)&c->d_scalars->dedupe_flags;
    a.counter = (u32*)&c->d_scalars->dedupe_counter;
    a.n_big = (u32*)&c->d_scalars->dedupe_n_big;
    a.big = big; a.big_cap = DEDUPE_BIG_CAP;
    ZK_TRY(arena_alloc(c, sizeof(u32) * DEDUPE_BAD_CAP, (void**)&a.bad));
    a.bad_cap = DEDUPE_BAD_CAP;
    a.n_bad = (u32*)&c->d_scalars->dedupe_n_bad;
    a.dbg = c->dbg ? c->dbg + 8192 : nullptr;
    // the mirror sort can group by 6 more bits if the blocks say how their entries split on them: 64 counts per block, when the
    // workspace has the room (and the finer grouping's tables after it: dedupe_finish)
    // ... leaving what the sorts and the union after it need (their tables are a few bytes per thousand keys)
    unsorted = unsorted && two_per_cu;          // (dedupe_kernel's blocks leave it sorted)
    if (!max_chunks && !unsorted && a.tag_bits >= 14 && c->arena_size - c->arena_off > 64ull * chunks * (4 + 8 + 8) + (32ull << 20) + n / 16)
        ZK_TRY(arena_alloc(c, sizeof(u32) * 64 * chunks, (void**)&a.sub));
    // the strand route: dedupe2_kernel writes the mirror words too, and counts the digits of the passes that will group them by block
    // (sort_keys_upper_counted) -- the plan depends on K and pack alone; more than two passes: strand_mirror_kernel as before
    if (mirror && mirror->out && mirror->cap && unsorted && tags && !max_chunks && c->sort_variant == 3) {
        const PassPlan plan = sort_plan_upper(c, key_bits + pack, key_bits + pack - b);
        if (plan.passes <= 2) {
            ZK_TRY(arena_alloc(c, sizeof(u64) * MAX_PASSES * MIRROR_RADIX, (void**)&a.m_hist));
            ZK_HIP(c, hipMemsetAsync(a.m_hist, 0, sizeof(u64) * MAX_PASSES * MIRROR_RADIX, c->stream));
            a.m_out = mirror->out; a.m_cap = mirror->cap; a.m_K = mirror->K; a.m_passes = plan.passes;
            a.m_cursor = &c->d_scalars->dedupe_m_cursor;
            r->mh.passes = plan.passes; r->mh.raw = a.m_hist;
            for (int p = 0; p < plan.passes; p++) { a.m_shift[p] = r->mh.shift[p] = plan.shift[p]; a.m_bits[p] = r->mh.bits[p] = plan.bits[p]; }
            r->m_words = a.m_out; r->m_cap = a.m_cap;
        }
    }
    ZK_HIP(c, hipMemsetAsync(&c->d_scalars->dedupe_flags, 0, ZK_SPAN(dedupe_flags, dedupe_m_cursor), c->stream));
    r->cuts = cuts; r->nwords = nwords; r->incl = incl; r->big = big; r->chunks = (uint32_t)chunks; r->pack = pack; r->work = work;
    r->tag_bits = a.tag_bits; r->unsorted = unsorted;
    return ZK_OK;
}

static void launch_one_per_cu(zk_ctx* c, const DedupeArgs& d) {
    const u32 grid = d.chunks < (u32)c->num_cus ? d.chunks : (u32)c->num_cus;
    if (d.tin) hipLaunchKernelGGL((dedupe_kernel<true, true>), dim3(grid), dim3(1024), 0, c->stream, d);
    else if (d.tag_bits <= 32) hipLaunchKernelGGL((dedupe_kernel<true, false>), dim3(grid), dim3(1024), 0, c->stream, d);
    else hipLaunchKernelGGL((dedupe_kernel<false, false>), dim3(grid), dim3(1024), 0, c->stream, d);
}

// ---- stage 2: the launch -- dedupe2_kernel with dedupe_kernel as the second chance of what it declines, or dedupe_kernel alone;
// the five counters are in c->h_scalars afterwards
static int dedupe_launch(zk_ctx* c, DedupeArgs& a, bool two_per_cu, bool unsorted, DedupeResult* r) {
    // algorithmic bytes: every key read once (a 32-bit tag, or the whole key), one word written per distinct key (added by
    // dedupe_pass, once the scan has said how many)
    prof_begin(c, ZK_PROF_RLE, (a.tin ? 4 : 8) * a.n);
    if (two_per_cu) {
        ZK_TRY(arena_alloc(c, sizeof(u32) * a.chunks, (void**)&a.retry));
        a.n_retry = (u32*)&c->d_scalars->dedupe_n_retry;
        a.limit = (u32)c->dedupe_limit;
        ZK_TRY(launch_dedupe2(c, a, a.tin != nullptr, c->dedupe_variant, unsorted));
    } else launch_one_per_cu(c, a);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(fetch_span(c, &c->h_scalars->dedupe_flags, ZK_SPAN(dedupe_flags, dedupe_m_cursor)));
    ZK_TRY(fetch(c, &c->h_scalars->dedupe_n_in, a.cuts + a.chunks));
    ZK_TRY(check_device_error(c));
    if (two_per_cu) { r->retry = a.retry; r->n_retry = (uint32_t)c->h_scalars->dedupe_n_retry; }
    if (a.m_out) {
        r->m_placed = c->h_scalars->dedupe_m_cursor;
        r->m_emitted = !((uint32_t)c->h_scalars->dedupe_flags & 4u) && r->m_placed <= a.m_cap;
    }
    if (two_per_cu && (uint32_t)c->h_scalars->dedupe_n_retry) {
        // the blocks dedupe2_kernel declined (65 536 keys or more; a table that filled up): dedupe_kernel's table is larger and its
        // counts are 32 bits wide -- what it declines too goes on the list the host counts by sorting
        DedupeArgs d = a;
        d.list = a.retry; d.chunks = (uint32_t)c->h_scalars->dedupe_n_retry; d.retry = nullptr; d.n_retry = nullptr;
        ZK_HIP(c, hipMemsetAsync(a.counter, 0, sizeof(u32), c->stream));
        launch_one_per_cu(c, d);
        ZK_HIP(c, hipGetLastError());
        ZK_TRY(fetch_span(c, &c->h_scalars->dedupe_flags, ZK_SPAN(dedupe_flags, dedupe_m_cursor)));
        ZK_TRY(check_device_error(c));
    }
    return ZK_OK;
}

// ---- stage 3: the few blocks whose table filled up (a stretch of the key space with more distinct k-mers than a table holds),
// counted the plain way, one by one: their keys sorted by the bits below the block bits (the block's own place in `work` is the
// second buffer), run lengths into words at that place, the block's word count patched in.
static int dedupe_bad_blocks(zk_ctx* c, const DedupeArgs& a, uint32_t n_bad, DedupeResult* r) {
    uint32_t list[DEDUPE_BAD_CAP];
    ZK_HIP(c, hipMemcpy(list, a.bad, sizeof(u32) * n_bad, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n_bad && !(r->flags & 1); i++) {
        u64 lohi[2];
        ZK_HIP(c, hipMemcpy(lohi, a.cuts + list[i], 2 * sizeof(u64), hipMemcpyDeviceToHost));
        const uint64_t m = lohi[1] - lohi[0];
        u64* res = nullptr;
        u64* bk = const_cast<u64*>(a.kin) + lohi[0];          // the block's keys, sorted in place
        if (a.tin) {
            // only tags were written: the block's keys are made again, beside the lists (a block is a few thousand keys)
            ZK_TRY(arena_alloc(c, 8 * m, (void**)&bk));
            ZK_TRY(expand_tags(c, a.tin, a.cuts, a.chunks, a.tag_bits, bk - lohi[0], list[i], 1));
        }
        ZK_TRY(sort_keys(c, bk, a.out + lohi[0], m, a.tag_bits, &res));
        if (res != bk) ZK_HIP(c, hipMemcpyAsync(bk, res, 8 * m, hipMemcpyDeviceToDevice, c->stream));
        uint64_t u = 0;
        bool ovf = false;
        ZK_TRY(rle(c, bk, m, a.out + lohi[0], nullptr, m, &u, a.pack, &ovf));
        if (ovf) { r->flags |= 1; break; }          // (a count beyond the field in such a block: the long way after all)
        ZK_HIP(c, hipMemcpy(a.nwords + list[i], &u, sizeof(u64), hipMemcpyHostToDevice));
    }
    return ZK_OK;
}

// keys[0..n) ordered by their TOP b bits (of key_bits) -> the distinct keys with their counts, SORTED.  Two steps, because the
// caller can only size the result once the first is done:
//   dedupe_pass   counts the blocks (dedupe_kernel): words in `work` (at least as many words as keys), block by block.
//                 *flags: bit 0 = some table filled up (the words are not to be used), bit 1 = some counts went to the side list.
//                 max_chunks > 0: only the leading blocks (the sample; *n_in = the keys they cover).
//   dedupe_finish moves the words together and apart into out_k / out_c (r.n_out entries each).
int dedupe_pass(zk_ctx* c, const u64* keys, uint64_t n, int key_bits, int b, int pack, u64* work, uint64_t cap, DedupeResult* r,
                uint64_t* n_in, uint64_t max_chunks, const u32* tags, const u64* tag_cuts, bool unsorted, const DedupeMirror* mirror) {
    *r = DedupeResult();
    if (n_in) *n_in = n;
    if (n == 0) return ZK_OK;
    if (b < 1 || b > 24 || b >= key_bits || pack < 10 || pack > 31) return fail(c, ZK_EINTERNAL, "dedupe_pass: %d block bits of %d, pack %d", b, key_bits, pack);
    if (cap < n) return fail(c, ZK_ENOSPC, "dedupe_pass: work buffer of %llu words for %llu keys", (unsigned long long)cap, (unsigned long long)n);
    DedupeArgs a = {};
    const bool two_per_cu = key_bits - b <= 32 && c->dedupe_variant >= 0;
    ZK_TRY(dedupe_lists(c, keys, n, key_bits, b, pack, work, max_chunks, tags, tag_cuts, unsorted, two_per_cu, mirror, a, r));
    ZK_TRY(dedupe_launch(c, a, two_per_cu, r->unsorted, r));
    r->flags = (uint32_t)c->h_scalars->dedupe_flags;
    r->n_big = (uint32_t)c->h_scalars->dedupe_n_big;
    if (r->n_big > DEDUPE_BIG_CAP) r->flags |= 1;          // more counts beyond the field than the side list holds: the long way
    const uint32_t n_bad = (uint32_t)c->h_scalars->dedupe_n_bad;
    if (n_bad && n_bad <= DEDUPE_BAD_CAP && !(r->flags & 1) && !max_chunks) {
        ZK_TRY(dedupe_bad_blocks(c, a, n_bad, r));
        a.sub = nullptr;          // the runs of those blocks were not counted: the mirror sort groups by the block bits only
    } else if (n_bad > DEDUPE_BAD_CAP) r->flags |= 1;
    // ---- stage 4: the scan of the blocks' word counts, and the result ----
    ZK_HIP(c, hipMemcpyAsync(r->incl, r->nwords, sizeof(u64) * r->chunks, hipMemcpyDeviceToDevice, c->stream));
    ZK_TRY(scan64_inclusive(c, r->incl, r->chunks));
    ZK_TRY(fetch(c, &c->h_scalars->dedupe_n_out, r->incl + r->chunks - 1));
    ZK_TRY(stream_sync(c));
    r->n_out = c->h_scalars->dedupe_n_out;
    prof_add_bytes(c, ZK_PROF_RLE, 8 * r->n_out);          // one word written per distinct key (its mirror image: booked by strand_blocks)
    r->sub = a.sub;
    if (n_in) *n_in = c->h_scalars->dedupe_n_in;          // keys covered by the blocks that were counted
    return ZK_OK;
}

// out_m (or null; K odd or even, 2 * gbases block bits = all 4^gbases blocks counted): the mirrored words, grouped by their low
// 2 * gbases bits (dedupe_unpack_kernel) -- ready for the passes over the bits above
int dedupe_finish(zk_ctx* c, const DedupeResult& r, u64* out_k, u32* out_c, u64* out_m, int K, int gbases, u64** mirror_hist,
                  int* mirror_group_bits, bool packed_out) {
    if (mirror_hist) *mirror_hist = nullptr;
    int gbits = 2 * gbases;
    if (mirror_group_bits) *mirror_group_bits = gbits;
    if (r.n_out == 0) return ZK_OK;
    u64 *minc = nullptr, *place24 = nullptr;
    if (out_m && (1ull << (2 * gbases)) != r.chunks) return fail(c, ZK_EINTERNAL, "dedupe_finish: %u blocks are not 4^%d", r.chunks, gbases);
    if (out_m && r.sub && mirror_group_bits && 2 * K - gbits - 6 >= 8) {
        // 6 more group bits: one pass less for the mirror sort (26 bits above the groups instead of 32 at K = 25)
        const uint64_t runs = 64ull * r.chunks;
        u64* minc24;
        ZK_TRY(arena_alloc(c, sizeof(u64) * runs, (void**)&minc24));
        ZK_TRY(arena_alloc(c, sizeof(u64) * runs, (void**)&place24));
        hipLaunchKernelGGL(dedupe_mirror_sizes24_kernel, dim3((u32)div_up(runs, 256)), dim3(256), 0, c->stream, r.sub, r.chunks, gbases, minc24);
        ZK_TRY(scan64_inclusive(c, minc24, runs));
        hipLaunchKernelGGL(dedupe_mirror_place24_kernel, dim3((u32)div_up(runs, 256)), dim3(256), 0, c->stream, r.sub, minc24, r.chunks, gbases, place24);
        ZK_HIP(c, hipGetLastError());
        gbits += 6;
        *mirror_group_bits = gbits;
    }
    MirrorHist mh = {};
    if (out_m && mirror_hist && c->sort_variant == 3) {
        // the digit counts of the passes that will sort the mirrored words above their group bits (sort_keys_upper_counted)
        const PassPlan plan = make_plan(2 * K - gbits, MIRROR_RBITS, gbits + r.pack);
        if (plan.passes <= 4) {
            ZK_TRY(arena_alloc(c, sizeof(u64) * MAX_PASSES * MIRROR_RADIX, (void**)&mh.raw));
            ZK_HIP(c, hipMemsetAsync(mh.raw, 0, sizeof(u64) * MAX_PASSES * MIRROR_RADIX, c->stream));
            mh.passes = plan.passes;
            for (int p = 0; p < plan.passes; p++) { mh.shift[p] = plan.shift[p]; mh.bits[p] = plan.bits[p]; }
            *mirror_hist = mh.raw;
        }
    }
    if (out_m && !place24) {
        ZK_TRY(arena_alloc(c, sizeof(u64) * r.chunks, (void**)&minc));
        hipLaunchKernelGGL(dedupe_mirror_sizes_kernel, dim3((r.chunks + 255) / 256), dim3(256), 0, c->stream, r.nwords, r.chunks, gbases, minc);
        ZK_TRY(scan64_inclusive(c, minc, r.chunks));
    }
    if (packed_out && r.n_big) return fail(c, ZK_EINTERNAL, "dedupe_finish: packed words with %u counts beyond the field", r.n_big);
    prof_begin(c, ZK_PROF_SELECT, ((out_m ? 28 : 20) - (packed_out ? 4 : 0)) * r.n_out);
    hipLaunchKernelGGL(dedupe_unpack_kernel, dim3((u32)c->num_cus * 8), dim3(256), 0, c->stream, r.work, r.cuts, r.incl, r.nwords, r.chunks, r.pack, out_k, out_c,
                       out_m, minc, K, gbases, mh, place24, packed_out ? 1 : 0);
    if (r.n_big) hipLaunchKernelGGL(dedupe_big_kernel, dim3((r.n_big + 255) / 256), dim3(256), 0, c->stream, r.big, r.n_big, out_k, (u64)r.n_out, out_c, c->d_err);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    return ZK_OK;
}

}  // namespace zk
