// tile_group.hpp -- a tile of keys sorted in LDS: grouped by a counting sort, then ranked inside the groups (tilesort.hip,
// strand_blocks.hip).
#pragma once
#include "internal.hpp"

namespace zk {

constexpr int TS_BLOCK = 512;
constexpr u32 TS_SLACK = 1024;          // S: no block of equal top bits may be longer

// PAIRS: a 32-bit payload travels with every key, and equal keys keep the order they came in (zk_sort_pairs is stable): the
// place a pair had in the tile is kept beside it and breaks the ties (keys alone need no such thing: equal keys are the same key)
template <int ITEMS, int GROUPS, bool PAIRS>
struct TileSortSmem {
    static constexpr int CAP = TS_BLOCK * ITEMS;
    alignas(16) u64 keys[CAP];
    u32 vals[PAIRS ? CAP : 1];
    u16 idx[PAIRS ? CAP : 1];
    alignas(16) u32 start[GROUPS + 8];          // the groups' counts, then where they start (start[G] = the tile's keys)
    u32 wsum[TS_BLOCK / 64];
};
// the map key -> group of a tile: monotone, g = floor(d * G / ((range >> sh) + 1)) for d = (key - first) >> sh, in 32 bits
struct TileMap {
    u64 kmin; int sh; u32 scale;
    __device__ __forceinline__ u32 group(u64 key) const {
        const u32 d = (u32)((key - kmin) >> sh);
        return scale ? __umulhi(d, scale) : d;
    }
};

// The tile [lo, lo + m) of kin (and vin) into LDS, grouped: sm.keys (vals, idx) hold the tile's entries group by group, sm.start where
// every group starts (start[G] = m).  Ends with a barrier.
// kin2 (keys only): the entries [m1, m) come from kin2 + lo2 instead -- two lists whose keys share their bits from pshift up
// (strand_blocks.hip: a block of the counted list and the same block of its mirror image).  ranged: the groups span the keys
// [vlo, vhi] (every key of the tile lies there) instead of the whole blocks of the first and last key.
template <int ITEMS, int G, bool PAIRS, class S>
__device__ __forceinline__ TileMap tile_group(S& sm, const u64* kin, const u32* vin, u64 lo, u32 m, int pshift, int tid,
                                              const u64* kin2 = nullptr, u64 lo2 = 0, u32 m1 = ~0u, bool ranged = false, u64 vlo = 0,
                                              u64 vhi = 0) {
    constexpr int NW = TS_BLOCK / 64, QPT = G / TS_BLOCK / 4;          // QPT: quads of groups a thread scans
    static_assert(QPT == 1 || QPT == 2, "four or eight groups a thread in the scan");
    static_assert((S::CAP <= 8192 || (!PAIRS && S::CAP <= 16384)) && G <= 4096, "group | place << 12 in a word; u16 places of pairs");
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const u64* kp = kin + lo;
    u64 k[ITEMS];
    u32 v[PAIRS ? ITEMS : 1];
#pragma unroll
    for (int j = 0; j < ITEMS; j++) {
        const u32 i = (u32)j * TS_BLOCK + tid;
        k[j] = i < m ? (i < m1 ? kp[i] : kin2[lo2 + (i - m1)]) : ~0ull;
        if constexpr (PAIRS) v[j] = i < m ? vin[lo + i] : 0u;
    }
    // the tile's value range, from the top bits of its first and last key (whole blocks)
    u64 first, last;
    if (ranged) { first = vlo; last = vhi; pshift = 0; }
    else { first = m1 ? kp[0] : kin2[lo2]; last = m - 1 < m1 ? kp[m - 1] : kin2[lo2 + (m - 1 - m1)]; }
    TileMap tm;
    tm.kmin = (first >> pshift) << pshift;
    const u64 rm1 = (((last >> pshift) - (first >> pshift)) << pshift) | ((1ull << pshift) - 1ull);
    tm.sh = rm1 >> 32 ? 32 - __builtin_clzll(rm1) : 0;
    const u32 rs = (u32)(rm1 >> tm.sh);
    tm.scale = rs < (u32)G ? 0u : (u32)(((u64)G << 32) / ((u64)rs + 1ull));
    {
        uint4* z = reinterpret_cast<uint4*>(sm.start);
#pragma unroll
        for (int q = 0; q < QPT; q++) z[QPT * tid + q] = make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    u32 gp[ITEMS];          // group | place in the group << 12
#pragma unroll
    for (int j = 0; j < ITEMS; j++) {
        const u32 i = (u32)j * TS_BLOCK + tid;
        const u32 g = i < m ? tm.group(k[j]) : 0u;
        gp[j] = g;
        if (i < m) gp[j] |= atomicAdd(&sm.start[g], 1u) << 12;
    }
    __syncthreads();
    {
        // counts -> starts: four or eight groups a thread, the waves' sums through LDS
        uint4* z = reinterpret_cast<uint4*>(sm.start);
        uint4 cq[QPT];
        u32 sum = 0;
#pragma unroll
        for (int q = 0; q < QPT; q++) { cq[q] = z[QPT * tid + q]; sum += cq[q].x + cq[q].y + cq[q].z + cq[q].w; }
        const u32 inc = wave_incl_scan_u32(sum);
        if (lane == 63) sm.wsum[wave] = inc;
        __syncthreads();
        u32 run = inc - sum;
#pragma unroll
        for (int w = 0; w < NW; w++) run += w < wave ? sm.wsum[w] : 0u;
#pragma unroll
        for (int q = 0; q < QPT; q++) {
            uint4 sq;
            sq.x = run; run += cq[q].x; sq.y = run; run += cq[q].y; sq.z = run; run += cq[q].z; sq.w = run; run += cq[q].w;
            z[QPT * tid + q] = sq;
        }
        if (tid == 0) sm.start[G] = m;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < ITEMS; j++) {
        const u32 i = (u32)j * TS_BLOCK + tid;
        if (i < m) {
            const u32 p = sm.start[gp[j] & (G - 1)] + (gp[j] >> 12);
            sm.keys[p] = k[j];
            if constexpr (PAIRS) { sm.vals[p] = v[j]; sm.idx[p] = (u16)i; }
        }
    }
    __syncthreads();
    return tm;
}

// The final places of E grouped entries (i[e] < m or not: entries beyond the tile get a place nobody uses): their group's start plus
// the entries of the group that go before them.  The E entries' LDS round trips (entry, group bounds, the group's first four keys)
// overlap.
template <int E, bool PAIRS, class S>
__device__ __forceinline__ void tile_rank(const S& sm, const TileMap& tm, const u32 (&i)[E], u32 m, u64 (&mine)[E], u32 (&place)[E]) {
    constexpr u32 CAP = S::CAP;
    // does the entry at q (key ko) go before the one at at (key km)?  Equal keys: the one that came first (pairs), any fixed order (keys)
    auto before = [&](u64 ko, u32 q, u64 km, u32 at) -> bool {
        if (ko != km) return ko < km;
        if constexpr (PAIRS) return q != at && sm.idx[q] < sm.idx[at];          // (rare: the two extra reads are taken by the lanes that need them)
        else return q < at;
    };
    u32 g0[E], g1[E];
#pragma unroll
    for (int e = 0; e < E; e++) mine[e] = sm.keys[i[e] < m ? i[e] : 0u];
#pragma unroll
    for (int e = 0; e < E; e++) {
        const u32 g = tm.group(mine[e]);
        g0[e] = sm.start[g]; g1[e] = sm.start[g + 1];
    }
    u64 o[E][4];
#pragma unroll
    for (int e = 0; e < E; e++)
#pragma unroll
        for (int r = 0; r < 4; r++) o[e][r] = sm.keys[g0[e] + r < CAP ? g0[e] + r : CAP - 1];
#pragma unroll
    for (int e = 0; e < E; e++) {
        const u32 at = i[e] < m ? i[e] : 0u;
        u32 rank = 0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const u32 q = g0[e] + r;
            rank += (q < g1[e] && before(o[e][r], q, mine[e], at)) ? 1u : 0u;
        }
        for (u32 q0 = g0[e] + 4; q0 < g1[e]; q0 += 4) {          // (a group of more than four)
            u64 p4[4];
#pragma unroll
            for (int r = 0; r < 4; r++) p4[r] = sm.keys[q0 + r < CAP ? q0 + r : CAP - 1];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const u32 q = q0 + r;
                rank += (q < g1[e] && before(p4[r], q, mine[e], at)) ? 1u : 0u;
            }
        }
        place[e] = g0[e] + rank;
    }
}

}  // namespace zk
