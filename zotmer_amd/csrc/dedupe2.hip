// dedupe2.hip -- K4, the block dedupe with TWO workgroups per CU (32-bit tags only).
//
// Replaces the run-length half of kmerize.merge (zotmer/commands/kmerize.py:41-132) exactly as dedupe_blocks.hip::dedupe_kernel does;
// same inputs, same words out.  What is different is how a CU is used.  dedupe_kernel's table (12 K entries of 4 + 4 bytes, 142 KB
// with its lists) leaves room for one workgroup per CU, and a block's phases -- clear, insert, drain, group, rank, write -- run one
// after the other with a barrier between them: tools/lds_atomic_bench.hip measures the two LDS atomics of an insert at 10.3 ns per
// 64 keys per CU (8 K cycles for a block of 23.7 K keys), the kernel needed 45 K cycles per block.  Nothing in it is short of a unit;
// it is short of something else to run while a phase waits.  So: a table that fits twice --
//   * counts of 16 bits, two to a word (a block of fewer than 65 536 keys cannot carry from one into the other; larger blocks are
//     declined up front and counted by dedupe_kernel afterwards, as are the blocks whose table fills up);
//   * side lists of 128 entries a wave, drained 64 at a time as soon as 64 are there (full wavefronts, no worst-case tile to hold);
// -- 11 K entries in 76 KB, and while one workgroup of the CU sorts and writes its block the other one inserts.
// UNSORTED (the strand route at odd K, strand_blocks.hip, which sorts every block again with its mirror image): the block's distinct
// words are written compacted in table order instead -- no counting sort, no ranks (12.1 -> 9.4 ms at config 2, profiles/r08).  Every
// wave compacts the entries of its own table rows in LDS, in place and without a barrier, and writes them in dense rounds of 64
// (see dedupe2_block; with the mirror words 11.12 -> 10.39 ms, profiles/r29).
// MIRROR (that route, 32-bit tags in): every word's mirror image, rc(k-mer) << pack | count, is written as well, from the registers
// that hold the word -- densely into DedupeArgs::m_out, in no order the route needs: a block takes the place of its words with one add
// on a global cursor, the waves theirs inside it from the LDS add that places the words themselves.  The digits of the two passes
// that will group the list by block are counted in LDS for the life of the workgroup and added to m_hist at its end.  This takes the
// place of strand_mirror_kernel, which read the counted list back to write the same words: 2.95 ms, for 1.76 ms more here (9.37 ->
// 11.12 ms; 0.15 of it the two swaps in flight that make room for the digit counts; profiles/r21).  A list that does not fit m_cap
// words sets flags |= 4 and the host falls back on that kernel; so it does for the blocks this kernel declines.
#include "dedupe.hpp"
#include <type_traits>

namespace zk {

// BATCH: the compare-and-swaps a thread has in flight at a time (their answers are looked at together); a wave's side list must
// take what one batch can add at worst on top of the 63 entries a drain may leave.  ITEMS: tags a thread takes per tile; the next
// tile is asked for before the current one is inserted, so a workgroup has 4 * TILE bytes on their way from memory.
template <int BLOCK_, int BATCH_, int ITEMS_>
struct Dedupe2Smem {
    static constexpr int BLOCK = BLOCK_, BATCH = BATCH_, ITEMS = ITEMS_, TILE = BLOCK * ITEMS, NW = BLOCK / 64, ALL = 11264, SPT = ALL / BLOCK,
                         NB = 1024, SIDE = 64 + 64 * BATCH;
    static_assert(ALL % BLOCK == 0 && ALL % 8 == 0 && ITEMS % BATCH == 0 && ITEMS % 4 == 0, "whole rounds, whole quads, whole batches");
    alignas(16) u32 keys[ALL];            // tags (after the count: the entries again, grouped by their top ten bits)
    alignas(16) u32 cnt[ALL / 2];         // 16-bit counts: entry h in half (h & 1) of word h >> 1
    union {
        u32 side[NW][SIDE];               // while the keys are inserted
        struct { u32 bc[NB]; u32 bbase[NB + 1]; } g;          // afterwards: entries per group (the tag's top ten bits), and before it
    };
    u32 ticket;
    u32 nout;                             // UNSORTED: the block's entries written so far
};
// MIRROR: ... with the digit counts of the mirror words, kept for the life of the workgroup and added to DedupeArgs::m_hist at its end.
// 4 KB more: beside four swaps in flight (77 832 bytes) that is 8 bytes more than two workgroups per CU have -- two swaps (75 788)
template <int BLOCK_, int BATCH_, int ITEMS_>
struct Dedupe2MirrorSmem : Dedupe2Smem<BLOCK_, BATCH_, ITEMS_> {
    u32 bins[2][MIRROR_RADIX];
    u64 mbase;                            // the block's place in DedupeArgs::m_out
};

// what a workgroup carries from one block to the next: the block it is about to count, with the first tile of its tags already
// asked for -- the ticket, the bounds and those tags travel while the previous block is being sorted and written
template <int ITEMS>
struct Dedupe2Next {
    u32 chunk;
    u64 lo;          // where the block's keys start ...
    u32 len;         // ... and how many they are (a block this kernel counts has fewer than 65 536)
    u32 tag[ITEMS];
};

// The tags [pos, pos + TILE) of the block that starts at `lo` (the same in every lane), as far as the block goes (rem = len - pos > 0).
// A whole tile: every thread takes ITEMS tags with 16-byte loads (TAGIN; a block starts wherever it starts: 4-byte aligned, no more) or
// ITEMS keys a stride apart.  The cut last tile: element i * BLOCK + tid each, the ones beyond the block not loaded.  Which thread
// takes which key is the table's business alone.
template <int BLOCK, int ITEMS, bool TAGIN>
__device__ __forceinline__ void dedupe2_load(const DedupeArgs& a, u64 lo, u32 pos, u32 rem, u32 tmask, u32 (&t)[ITEMS]) {
    constexpr u32 TILE = BLOCK * ITEMS;
    u32 tid = threadIdx.x;
    asm volatile("" : "+v"(tid));          // (opaque: or every index derived from it is computed once, as a 64-bit pair, and kept for the whole kernel)
    if constexpr (TAGIN) {
        const u32* tp = a.tin + lo + pos;
        if (rem >= TILE) {
            struct __attribute__((packed, aligned(4))) Tag4 { u32 a, b, c, d; };
            static_assert(ITEMS % 4 == 0, "whole quads");
#pragma unroll
            for (int i = 0; i < ITEMS / 4; i++) {
                const Tag4 q = *reinterpret_cast<const Tag4*>(tp + (u32)i * (4 * BLOCK) + 4 * tid);
                t[4 * i] = q.a; t[4 * i + 1] = q.b; t[4 * i + 2] = q.c; t[4 * i + 3] = q.d;
            }
        } else {
#pragma unroll
            for (int i = 0; i < ITEMS; i++) {
                const u32 g = (u32)i * BLOCK + tid;
                t[i] = g < rem ? tp[g] : 0u;
            }
        }
    } else {
        const u64* kp = a.kin + lo + pos;
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            const u32 g = (u32)i * BLOCK + tid;
            t[i] = g < rem ? (u32)kp[g] & tmask : 0u;
        }
    }
}

template <class S, bool TAGIN, bool UNSORTED, bool MIRROR>
__device__ __forceinline__ void dedupe2_block(const DedupeArgs& a, S& sm, Dedupe2Next<S::ITEMS>& st, u32 (&ph)[8], u32& tlast) {
    constexpr int BLOCK = S::BLOCK, BATCH = S::BATCH, ITEMS = S::ITEMS, TILE = S::TILE, ALL = S::ALL, SPT = S::SPT, NB = S::NB;
    static_assert(!MIRROR || UNSORTED, "the mirror words are written beside the unsorted ones");
    constexpr u32 EMPTY = ~0u;            // no entry; the all-ones tag has the last entry to itself (see `home`)
    constexpr u32 HS = ALL - 1;
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));          // (opaque per block: nothing derived from it is kept from one block to the next)
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const u32 chunk = st.chunk;
    const u64 lo = st.lo;
    const u32 len = st.len;
    const u32 maxc = (1u << a.pack) - 1u;
    const u32 tmask = a.tag_bits >= 32 ? ~0u : (1u << a.tag_bits) - 1u;
    auto next_block = [&](u32 t) {          // t: the ticket drawn at this block's start (read after a barrier)
        st.chunk = t; st.lo = 0; st.len = 0;
        if (t < a.chunks) {
            const u64 nlo = a.cuts[t], nhi = a.cuts[t + 1];
            st.lo = nlo;
            st.len = nhi - nlo < (u64)a.limit ? (u32)(nhi - nlo) : ~0u;          // ~0: too large for this kernel, nothing is loaded
        }
        if (st.len - 1u < ~0u - 1u) dedupe2_load<BLOCK, ITEMS, TAGIN>(a, st.lo, 0, st.len, tmask, st.tag);
    };
    if (tid == 0) sm.ticket = atomicAdd(a.counter, 1u);          // the block after this one: read after the next barrier
    if (len == 0 || len == ~0u) {
        // nothing to count -- or more keys than a 16-bit count is safe for: dedupe_kernel's business
        if (tid == 0) {
            if (len) a.retry[atomicAdd(a.n_retry, 1u)] = chunk;
            a.nwords[chunk] = 0;
        }
        if (a.sub && tid < 64) a.sub[(u64)chunk * 64 + tid] = 0;
        __syncthreads();
        next_block((u32)__builtin_amdgcn_readfirstlane((int)sm.ticket));
        return;
    }
    for (int q = tid; q < ALL / 4; q += BLOCK) reinterpret_cast<uint4*>(sm.keys)[q] = make_uint4(~0u, ~0u, ~0u, ~0u);
    for (int q = tid; q < ALL / 8; q += BLOCK) reinterpret_cast<uint4*>(sm.cnt)[q] = make_uint4(0, 0, 0, 0);
    if (UNSORTED && tid == 0) sm.nout = 0;
    __syncthreads();
    DD_PHASE(0);          // table cleared
    const u32 nchunk = (u32)__builtin_amdgcn_readfirstlane((int)sm.ticket);
    u32 bad = 0;
    u32 nside = 0;          // entries in this wave's side list (the same in every lane)
    auto home = [&](u32 e) -> u32 {
        // the all-ones tag (= the empty marker) has the last entry to itself: there the swap of "empty" for "empty" succeeds and
        // leaves the word as it is; no other key is ever sent there
        u32 hh = __umulhi(e * 0x9E3779B1u, HS);
        asm("" : "+v"(hh));          // (opaque: left to itself the compiler branches around the two multiplies for the one tag that does not need them)
        return e == EMPTY ? HS : hh;          // (24-bit multiplies instead -- fold, multiply, scale: six full-rate operations -- no faster: 12.4 ms)
    };
    auto count = [&](u32 h, u32 inc) { atomicAdd(&sm.cnt[h >> 1], inc << ((h & 1u) << 4)); };
    // up to 64 entries of the wave's side list into the table by linear probing
    auto drain = [&](u32 from, u32 n) {
        if ((u32)lane < n) {
            const u32 e = sm.side[wave][from + lane];
            u32 h = home(e) + 1;          // its home entry is taken: that is why it is here
            h = h >= HS ? 0u : h;
            int p = 0;
            for (; p < ALL; p++) {
                const u32 old = atomicCAS(&sm.keys[h], EMPTY, e);
                if (old == EMPTY || old == e) break;
                h = h + 1 == HS ? 0u : h + 1;
            }
            if (p < ALL) count(h, 1u); else bad = 1;
        }
    };
    // The common case has no loop and no branch: one compare-and-swap at the tag's home entry, the count added as 1 or 0 (adding 0
    // to another key's entry harms nobody); a key that finds another key at home goes to the wave's side list (its place from a
    // ballot, no atomic).  BATCH swaps are issued before the first answer is looked at.  (A plain read first and the swap only for
    // the lanes that see "empty": 13.5 against 13.3 ms.)
    auto insert = [&](auto whole, const u32 (&e)[BATCH], const bool (&valid)[BATCH]) {          // whole: every key of the batch is one (a whole tile)
        constexpr bool WHOLE = decltype(whole)::value;
        u32 h[BATCH], old[BATCH];
#pragma unroll
        for (int j = 0; j < BATCH; j++) h[j] = home(e[j]);
#pragma unroll
        for (int j = 0; j < BATCH; j++) old[j] = (WHOLE || valid[j]) ? atomicCAS(&sm.keys[h[j]], EMPTY, e[j]) : e[j];
#pragma unroll
        for (int j = 0; j < BATCH; j++) {
            const bool ok = old[j] == EMPTY || old[j] == e[j];
            count(h[j], (ok && (WHOLE || valid[j])) ? 1u : 0u);
            const u64 m = __ballot(!ok);
            if (!ok) sm.side[wave][nside + popc_below(m)] = e[j];
            nside += (u32)__popcll(m);
        }
        while (nside >= 64) { nside -= 64; drain(nside, 64); }
    };
    u32 tag[ITEMS], nt[ITEMS];
#pragma unroll
    for (int i = 0; i < ITEMS; i++) tag[i] = st.tag[i];          // the first tile was asked for during the previous block
    for (u32 pos = 0; pos < len; pos += TILE) {
        const u32 rem = len - pos;
        if (rem > (u32)TILE) dedupe2_load<BLOCK, ITEMS, TAGIN>(a, lo, pos + TILE, rem - TILE, tmask, nt);
#pragma unroll
        for (int i0 = 0; i0 < ITEMS; i0 += BATCH) {
            u32 e[BATCH];
            bool valid[BATCH];
#pragma unroll
            for (int j = 0; j < BATCH; j++) { e[j] = tag[i0 + j]; valid[j] = (u32)(i0 + j) * BLOCK + tid < rem; }
            if (rem >= (u32)TILE) insert(std::true_type(), e, valid); else insert(std::false_type(), e, valid);
        }
#pragma unroll
        for (int i = 0; i < ITEMS; i++) tag[i] = nt[i];
    }
    drain(0, nside);
    DD_PHASE(1);          // keys inserted
    const int any_bad = __syncthreads_or((int)bad);
    DD_PHASE(2);          // ... every wave done
    if (any_bad) {
        // the table filled up (a block with more distinct keys than it holds): dedupe_kernel's larger table gets a try
        if (tid == 0) {
            a.retry[atomicAdd(a.n_retry, 1u)] = chunk;
            a.nwords[chunk] = 0;
        }
        if (a.sub && tid < 64) a.sub[(u64)chunk * 64 + tid] = 0;
        next_block(nchunk);
        return;
    }
    if constexpr (UNSORTED) {
        // ---- the block's entries in table order, compacted (the strand route sorts every block again: strand_blocks.hip) ------
        // A wave owns the table rows (j, wave) = the 64 entries j * BLOCK + wave * 64 + lane, j < SPT, from the barrier above to the one
        // at the block's end.  It compacts them in place: the rows are read SPT / 2 at a time (no access under a branch, one wait a
        // batch), and the live entry of rank p in the wave's stream -- rows in order, lanes in order -- goes back to lane p & 63 of the
        // wave's row p >> 6.  p never exceeds the place read and a wave's LDS operations complete in order, so a write lands only in a
        // row the wave has read already: no barrier, no second buffer.  The last rank is what the wave adds to nout.  Then
        // ceil(wn / 64) dense rounds, lane l of round r taking entry 64 r + l: every lane of a round but the last one's builds a word
        // (and its mirror image), and a round's stores are whole runs of 512 bytes.  About 27 % of a table is in use at config 2, so
        // six or seven dense rounds do what took SPT = 22 rounds of mostly idle lanes, each with two dependent LDS reads under its
        // branch (the kernel 11.12 -> 10.39 ms, profiles/r29; reading rows and tags ahead into registers alone, 22 rounds kept: 10.99;
        // with both dense rounds of a pair always run and the slot from shifts and masks: 10.80).
        // MIRROR: the block takes the place of its mirror words in m_out with ONE add on the global cursor, once every wave's share is
        // in nout (a barrier); the answer travels while the next block's bounds are fetched, and a second barrier hands it to the waves,
        // whose words lie in m_out as they lie in the block.  (An add per wave needs neither barrier, but 2 M adds a step on one word
        // that every XCD shares pass through one place: the step took 87-90 ms against 72-73.)
        if constexpr (!MIRROR) next_block(nchunk);          // the next block's first tile travels while this one is written
        const u16* cnt16 = reinterpret_cast<const u16*>(sm.cnt);
        static_assert(SPT % 2 == 0, "two batches of rows; dense rounds are read two at a time");
        constexpr int RB = SPT / 2;
        u32* const wkeys = sm.keys + wave * 64;          // the wave's rows: entry s of row j at [j * BLOCK + s]
        u16* const wcnt = reinterpret_cast<u16*>(sm.cnt) + wave * 64;
        u32 wn = 0;          // the wave's entries so far (the same in every lane)
#pragma unroll
        for (int j0 = 0; j0 < SPT; j0 += RB) {
            u32 rt[RB], rc[RB];
#pragma unroll
            for (int r = 0; r < RB; r++) {
                rt[r] = sm.keys[tid + (j0 + r) * BLOCK];
                rc[r] = cnt16[tid + (j0 + r) * BLOCK];
            }
#pragma unroll
            for (int r = 0; r < RB; r++) asm volatile("" : "+v"(rt[r]));          // (opaque: or a tag's read sinks under its entry's branch)
#pragma unroll
            for (int r = 0; r < RB; r++) {
                const u64 bal = __ballot(rc[r] != 0);
                if (rc[r]) {
                    const u32 p = __builtin_amdgcn_mbcnt_hi((u32)(bal >> 32), __builtin_amdgcn_mbcnt_lo((u32)bal, wn));          // < SPT * 64
                    const u32 s = p + (p >> 6) * (u32)(BLOCK - 64);          // row p >> 6, lane p & 63
                    wkeys[s] = rt[r];
                    wcnt[s] = (u16)rc[r];
                }
                wn += (u32)__popcll(bal);
            }
        }
        u32 wbase = 0;
        if (lane == 0 && wn) wbase = atomicAdd(&sm.nout, wn);
        wbase = (u32)__shfl((int)wbase, 0, 64);
        u64* mp = nullptr;          // the wave's mirror words from here on; null: none are written
        u64* op = nullptr;          // the wave's words from here on (MIRROR: both places from the one count)
        if constexpr (MIRROR) {
            __syncthreads();
            u64 g = 0;
            if (tid == 0) g = atomicAdd(a.m_cursor, (u64)sm.nout);
            next_block(nchunk);
            if (tid == 0) sm.mbase = g;
            __syncthreads();
            const u64 mb = sm.mbase;
            const u64 mbase = ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(mb >> 32)) << 32) | (u64)(u32)__builtin_amdgcn_readfirstlane((int)mb);
            const u32 wb = (u32)__builtin_amdgcn_readfirstlane((int)wbase);
            op = a.out + lo + wb;
            if (mbase + sm.nout <= a.m_cap) mp = a.m_out + mbase + wb;
            else if (tid == 0) atomicOr(a.flags, 4u);          // m_out is too small: the host has strand_mirror_kernel write the list
        }
        DD_PHASE(3);          // entries counted, the wave's words placed
        const u64 hi_part = (u64)chunk << a.tag_bits;
        if constexpr (!MIRROR) op = a.out + lo + wbase;
        // entry i = 64 r + lane of the wave's stream, its tag and count read beforehand; beyond wn the lane holds whatever lies there
        auto dense = [&](u32 i, u32 t, u32 c) {
            const bool live = i < wn;
            const u64 k = hi_part | (u64)t;
            const u64 cw = (u64)(c > maxc ? 0u : c);
            if (live) {
                if (c > maxc) {
                    const u32 at = atomicAdd(a.n_big, 1u);
                    if (at < a.big_cap) { a.big[2 * (u64)at] = k; a.big[2 * (u64)at + 1] = c; }
                    atomicOr(a.flags, 2u);
                }
                op[i] = (k << a.pack) | cw;
            }
            if constexpr (MIRROR) {
                if (mp) {          // (the block's place + wbase + i < the block's place + nout <= m_cap)
                    const u64 mw = (revcomp(a.m_K, k) << a.pack) | cw;
                    if (live) mp[i] = mw;
                    // the digits are the word's top bits: the second one is all there is above the first (one pass: 0, never read);
                    // a lane beyond wn adds 0, wherever: no LDS access under a per-entry branch
                    const u32 top = (u32)(mw >> a.m_shift[0]);
                    atomicAdd(&sm.bins[0][top & ((1u << a.m_bits[0]) - 1u)], live ? 1u : 0u);
                    atomicAdd(&sm.bins[1][(top >> a.m_bits[0]) & (MIRROR_RADIX - 1)], live ? 1u : 0u);
                }
            }
        };
        for (u32 r = 0; r * 64 < wn; r += 2) {          // (wn <= SPT * 64 and SPT is even: row r + 1 exists)
            u32 rt[2], rc[2];
#pragma unroll
            for (int e = 0; e < 2; e++) {
                rt[e] = sm.keys[tid + (r + e) * BLOCK];
                rc[e] = cnt16[tid + (r + e) * BLOCK];
            }
#pragma unroll
            for (int e = 0; e < 2; e++) asm volatile("" : "+v"(rt[e]));          // (opaque: both rounds read together, ahead of any branch)
            dense(r * 64 + (u32)lane, rt[0], rc[0]);
            if ((r + 1) * 64 < wn) dense((r + 1) * 64 + (u32)lane, rt[1], rc[1]);
        }
        __syncthreads();
        if (tid == 0) a.nwords[chunk] = sm.nout;          // (read before the caller's barrier; the next block clears it after)
        DD_PHASE(5);          // written
        return;
    }
    // ---- the block's entries, sorted: a counting sort on the tag's top ten bits, then ranks inside each group of ~3 -----------
    // thread t takes the entries t, t + BLOCK, ... into registers with their places in their groups (a returning add); the table's
    // memory then takes them back grouped.  (256 groups of a dozen entries: the rank loop runs as long as the largest group of a
    // wavefront, one LDS round trip per turn -- 16 K of a block's 58 K cycles.)
    for (int q = tid; q < NB; q += BLOCK) sm.g.bc[q] = 0;          // the side lists are done with: every wave has passed the barrier above
    u32 et[SPT], ec[SPT];          // ec: count | place in the group << 16
    const int gb = a.tag_bits < 10 ? a.tag_bits : 10, bsh = a.tag_bits - gb;
    const u16* cnt16 = reinterpret_cast<const u16*>(sm.cnt);
#pragma unroll
    for (int j = 0; j < SPT; j++) {
        et[j] = sm.keys[tid + j * BLOCK];
        ec[j] = cnt16[tid + j * BLOCK];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SPT; j++) {
        if (ec[j]) ec[j] |= atomicAdd(&sm.g.bc[(et[j] >> bsh) & (NB - 1)], 1u) << 16;
        if (j % 6 == 5) __builtin_amdgcn_sched_barrier(0);          // (all SPT adds scheduled at once: their addresses and answers spill)
    }
    __syncthreads();
    DD_PHASE(3);          // entries read, groups counted
    if (wave == 0) {
        constexpr int PER = NB / 64;
        u32 cs[PER], sum = 0;
#pragma unroll
        for (int r = 0; r < PER; r++) { cs[r] = sm.g.bc[PER * lane + r]; sum += cs[r]; }
        const u32 inc = wave_incl_scan_u32(sum);
        u32 run = inc - sum;
#pragma unroll
        for (int r = 0; r < PER; r++) { sm.g.bbase[PER * lane + r] = run; run += cs[r]; }
        if (lane == 63) sm.g.bbase[NB] = inc;
    }
    __syncthreads();
    const u32 total = sm.g.bbase[NB];
    if (tid == 0) a.nwords[chunk] = total;
    if (a.sub && tid < 64) a.sub[(u64)chunk * 64 + tid] = sm.g.bbase[16 * tid + 16] - sm.g.bbase[16 * tid];          // sixteen groups = one 6-bit start (tag_bits >= 14)
    u16* cw16 = reinterpret_cast<u16*>(sm.cnt);
#pragma unroll
    for (int j = 0; j < SPT; j++) {
        if (ec[j]) {
            const u32 p = sm.g.bbase[(et[j] >> bsh) & (NB - 1)] + (ec[j] >> 16);
            sm.keys[p] = et[j];
            cw16[p] = (u16)ec[j];
        }
    }
    __syncthreads();
    DD_PHASE(4);          // grouped
    next_block(nchunk);          // the next block's first tile travels while this one is ranked and written (asked for any earlier, its
                                 // registers are held beside the entries above: 20 spilled)
    const u64 hi_part = (u64)chunk << a.tag_bits;          // the bits every key of the block has above its tag
    // three entries of a thread at a time: their LDS round trips (entry, group bounds, the group's first four tags) overlap -- one entry
    // after the other this loop was a chain of five round trips per entry, 11 K of a block's 52 K cycles
    constexpr int E = 3;
    for (u32 i0 = (u32)tid; i0 < total; i0 += E * BLOCK) {
        u32 mine[E], cc[E], g0[E], g1[E], rank[E];
#pragma unroll
        for (int e = 0; e < E; e++) {
            const u32 i = i0 + e * BLOCK;
            mine[e] = sm.keys[i < total ? i : 0u];
            cc[e] = cnt16[i < total ? i : 0u];
        }
#pragma unroll
        for (int e = 0; e < E; e++) {
            const u32 b = (mine[e] >> bsh) & (NB - 1);
            g0[e] = sm.g.bbase[b]; g1[e] = sm.g.bbase[b + 1];
        }
        u32 o[E][4];
#pragma unroll
        for (int e = 0; e < E; e++)
#pragma unroll
            for (int r = 0; r < 4; r++) o[e][r] = sm.keys[g0[e] + r < (u32)ALL ? g0[e] + r : (u32)ALL - 1];
#pragma unroll
        for (int e = 0; e < E; e++) {
            rank[e] = 0;
#pragma unroll
            for (int r = 0; r < 4; r++) rank[e] += (g0[e] + r < g1[e] && o[e][r] < mine[e]) ? 1u : 0u;
            for (u32 q = g0[e] + 4; q < g1[e]; q += 4) {          // (a group of more than four: rare with 1024 groups of ~3)
                u32 p4[4];
#pragma unroll
                for (int r = 0; r < 4; r++) p4[r] = sm.keys[q + r < (u32)ALL ? q + r : (u32)ALL - 1];
#pragma unroll
                for (int r = 0; r < 4; r++) rank[e] += (q + r < g1[e] && p4[r] < mine[e]) ? 1u : 0u;
            }
        }
#pragma unroll
        for (int e = 0; e < E; e++) {
            const u32 i = i0 + e * BLOCK;
            if (i >= total) break;
            const u32 c = cc[e];
            const u64 k = hi_part | (u64)mine[e];
            if (c > maxc) {
                const u32 at = atomicAdd(a.n_big, 1u);
                if (at < a.big_cap) { a.big[2 * (u64)at] = k; a.big[2 * (u64)at + 1] = c; }
                atomicOr(a.flags, 2u);
            }
            a.out[lo + g0[e] + rank[e]] = (k << a.pack) | (u64)(c > maxc ? 0u : c);
        }
    }
    DD_PHASE(5);          // ranked and written
}

// Persistent: two workgroups per CU draw the blocks from a counter -- in order, not strided: the sizes go with the first bases, a
// stride of the grid would give one workgroup all the big ones.
template <int BLOCK, int BATCH, int ITEMS, bool TAGIN, bool UNSORTED, bool MIRROR = false>
__global__ __launch_bounds__(BLOCK, 2 * BLOCK / 256) void dedupe2_kernel(DedupeArgs a) {
    using S = typename std::conditional<MIRROR, Dedupe2MirrorSmem<BLOCK, BATCH, ITEMS>, Dedupe2Smem<BLOCK, BATCH, ITEMS>>::type;
    __shared__ S sm;
    static_assert(sizeof(S) <= 80 * 1024, "two workgroups per CU");
    Dedupe2Next<ITEMS> st;
    if constexpr (MIRROR)
        for (int q = threadIdx.x; q < 2 * MIRROR_RADIX; q += BLOCK) (&sm.bins[0][0])[q] = 0;
    if (threadIdx.x == 0) sm.ticket = atomicAdd(a.counter, 1u);
    __syncthreads();
    st.chunk = (u32)__builtin_amdgcn_readfirstlane((int)sm.ticket);
    st.lo = 0; st.len = 0;
    const u32 tmask = a.tag_bits >= 32 ? ~0u : (1u << a.tag_bits) - 1u;
    if (st.chunk < a.chunks) {
        const u64 nlo = a.cuts[st.chunk], nhi = a.cuts[st.chunk + 1];
        st.lo = nlo;
        st.len = nhi - nlo < (u64)a.limit ? (u32)(nhi - nlo) : ~0u;
    }
    if (st.len - 1u < ~0u - 1u) dedupe2_load<BLOCK, ITEMS, TAGIN>(a, st.lo, 0, st.len, tmask, st.tag);
    __syncthreads();          // the ticket word is free again
    u32 ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    u32 tlast = a.dbg ? (u32)__builtin_amdgcn_s_memtime() : 0u;
    (void)tlast;
    u32 nblk = 0;
    while (st.chunk < a.chunks) {
        dedupe2_block<S, TAGIN, UNSORTED, MIRROR>(a, sm, st, ph, tlast);          // leaves the next block in st
        __syncthreads();          // the table and the ticket word are free again
        DD_PHASE(6);
        nblk++;
    }
    if constexpr (MIRROR) {          // (every wave's adds are behind the barrier above, or the one after the ticket)
        for (int q = threadIdx.x; q < a.m_passes * MIRROR_RADIX; q += BLOCK) {
            const u32 x = (&sm.bins[0][0])[q];
            if (x) atomicAdd(&a.m_hist[q], (u64)x);
        }
    }
    if (a.dbg && threadIdx.x == 0 && blockIdx.x < 256) {
        for (int k = 0; k < 8; k++) a.dbg[(u64)blockIdx.x * 16 + k] = ph[k];
        a.dbg[(u64)blockIdx.x * 16 + 8] = nblk;
    }
}

// variant: bits 0-1 = compare-and-swaps in flight per thread (0: 4, 1: 1, 2: 2; with the mirror words 0: 2: 9.37 against 9.51 ms
// without them, profiles/r21).  Tiles of 8 tags a thread; 16 (twice the bytes on
// their way from memory): 14.5 against 12.6 ms.  (1024-thread workgroups, two to a CU, have 64 registers a thread: the entries a
// thread holds while the block is sorted do not fit -- 25 to 40 spilled; not instantiated.)
int launch_dedupe2(zk_ctx* c, const DedupeArgs& a, bool tagin, int variant, bool unsorted) {
    const u32 want = 2u * (u32)c->num_cus;
    const u32 grid = a.chunks < want ? a.chunks : want;
    if (a.m_out) {
        // the mirror words as well: tags in, unsorted, and (the digit counts' 4 KB of LDS) at most two swaps in flight
        if (!tagin || !unsorted || !a.m_cursor || !a.m_hist || a.m_passes < 1 || a.m_passes > 2 || a.m_bits[0] > MIRROR_RBITS || a.m_bits[1] > MIRROR_RBITS)
            return fail(c, ZK_EINTERNAL, "launch_dedupe2: mirror words with %d passes, tags %d, unsorted %d", a.m_passes, (int)tagin, (int)unsorted);
        if ((variant & 3) == 1) hipLaunchKernelGGL((dedupe2_kernel<512, 1, 8, true, true, true>), dim3(grid), dim3(512), 0, c->stream, a);
        else hipLaunchKernelGGL((dedupe2_kernel<512, 2, 8, true, true, true>), dim3(grid), dim3(512), 0, c->stream, a);
        ZK_HIP(c, hipGetLastError());
        return ZK_OK;
    }
#define ZK_DD2(N, T, U) hipLaunchKernelGGL((dedupe2_kernel<512, N, 8, T, U>), dim3(grid), dim3(512), 0, c->stream, a)
#define ZK_DD2B(T, U) switch (variant & 3) { case 1: ZK_DD2(1, T, U); break; case 2: ZK_DD2(2, T, U); break; default: ZK_DD2(4, T, U); break; }
    if (unsorted) {
        if (tagin) ZK_DD2B(true, true) else ZK_DD2B(false, true)
    } else {
        if (tagin) ZK_DD2B(true, false) else ZK_DD2B(false, false)
    }
#undef ZK_DD2B
#undef ZK_DD2
    ZK_HIP(c, hipGetLastError());
    return ZK_OK;
}

}  // namespace zk
