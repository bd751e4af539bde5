// pileup.hip -- `zot alu-finder` (zotmer/commands/alu-finder.py): the reads placed on the reference zones and piled up.
//
// The reference's `hits` (alu-finder.py:116-147) takes one list of (k-mer, position) windows -- one orientation of one mate --
// finds the distinct diagonals (zone, q - p) of its windows' anchors (zone, q), and adds every window of the list, matching or
// not, once per diagonal: acc[zone][r + p][x] += 1.  Two entries of include/zotk.h:
//   * zk_anchor_pileup: one wave per read, 64 windows per step, cut from the raw FASTQ text (read_window.hpp) and looked up in a
//     bait table whose ids are anchors on one u32 axis (bait_table.hpp).  A wave keeps the distinct diagonals of a list in
//     registers, lane q & 63 holding number q in its word q >> 6 (ZK_PILEUP_DIAGS of them at most), and then writes the
//     |D| * windows pairs (d + p, x) behind a cursor it moves with one atomic add per list.  A list with more diagonals is done
//     again by a path that keeps no list: a diagonal belongs to the first window that gives it, which a lane decides by
//     looking the earlier windows of the line up again (slow, exact, and only ever taken by reads on tandem repeats).
//     long_line_kernel runs first: a line longer than pad that hits could name coordinates of another zone (ZK_ERANGE).
//   * zk_pileup_count: the pairs sorted by (coordinate, k-mer) with two stable pair sorts (radix_sort.hip) -- by k-mer carrying
//     the coordinate, then by coordinate carrying the index -- a gather of the k-mers into that order, and the cut into runs:
//     head flags, a scan and a write over tiles that own their output range (compact.hpp), then the run lengths.
// Nothing waits on another workgroup; the only atomics are the cursor's.
#include "internal.hpp"
#include "bait_table.hpp"
#include "compact.hpp"
#include "read_window.hpp"

namespace zk {

constexpr int PU_DIAGS = ZK_PILEUP_DIAGS, PU_WORDS = PU_DIAGS / 64;
static_assert(PU_DIAGS % 64 == 0 && PU_WORDS >= 1, "a lane holds one diagonal per word");
static_assert(ZK_PILEUP_TILE == CP_TILE, "ZK_PILEUP_TILE is the tile of the compaction kernels that cut the sorted pairs into runs");

// ---------------------------------------------------------------------------------------
// zk_anchor_pileup
// ---------------------------------------------------------------------------------------
// (the sequence line of a record is read STRIPPED here: seq_line + strip of read_window.hpp)

// window i of a line of L bytes as the list of orientation o holds it (basics.kmersWithPosLists; hits' p -= 1)
__device__ __forceinline__ void pu_orient(int K, int o, u64 L, u64 i, u64 x, u64& key, u32& p) {
    key = o ? revcomp(K, x) : x;
    p = o ? (u32)(L - i - (u64)K) : (u32)i;
}

__device__ __forceinline__ bool pu_has_anchor(const BaitView& bt, u64 key, u32 a) {
    u32 lo, end;
    if (!bait_find(bt, key, lo, end)) return false;
    lo = lower_bound(bt.ids, lo, end, a);
    return lo < end && bt.ids[lo] == a;
}

// diagonal number q (wave-uniform) of the wave's register list
__device__ __forceinline__ u32 pu_diag(const u32 (&reg)[PU_WORDS], u32 q) {
    u32 v = reg[0];
#pragma unroll
    for (int j = 1; j < PU_WORDS; j++) if ((q >> 6) == (u32)j) v = reg[j];
    return __shfl(v, (int)(q & 63u), 64);
}

// a line longer than pad that has a hit: its diagonals could reach the coordinates of another zone
__global__ __launch_bounds__(256) void long_line_kernel(BaitView bt, const u8* __restrict__ text, const u64* __restrict__ lines, u64 n_reads, int K,
                                                        u64 pad, u64* __restrict__ bad) {
    const WaveIds w = wave_ids();
    for (u64 r = w.wave; r < n_reads; r += w.nw) {
        u64 s, e;
        seq_line(lines, r, s, e);
        strip(text, s, e);
        if (e - s <= pad) continue;
        const bool hit = for_each_chunk(text, s, e, K, w.lane, [&](u64, bool valid, u64 x) {
            u32 lo, hi;
            return __ballot(valid && (bait_find(bt, x, lo, hi) || bait_find(bt, revcomp(K, x), lo, hi))) != 0;
        });
        if (hit && w.lane == 0) *bad = 1;
    }
}

__global__ __launch_bounds__(256) void pileup_kernel(BaitView bt, const u8* __restrict__ text, const u64* __restrict__ lines, u64 n_reads, int K,
                                                     u32* __restrict__ coords, u64* __restrict__ kmers, u64 cap, u64* cursor) {
    const WaveIds w = wave_ids();
    const int lane = w.lane;
    for (u64 r = w.wave; r < n_reads; r += w.nw) {
        u64 s, e;
        seq_line(lines, r, s, e);
        strip(text, s, e);
        const u64 L = e - s;
        if (L < (u64)K) continue;
        for (int o = 0; o < 2; o++) {
            // the distinct diagonals of the list, and its windows
            u32 reg[PU_WORDS];
#pragma unroll
            for (int j = 0; j < PU_WORDS; j++) reg[j] = 0;
            u32 nd = 0, W = 0;
            bool over = false;
            for_each_chunk(text, s, e, K, lane, [&](u64 c0, bool valid, u64 x) {
                u64 key;
                u32 p, t = 0, te = 0;
                W += (u32)__popcll(__ballot(valid));
                if (over) return false;
                pu_orient(K, o, L, c0 - s + lane, x, key, p);
                if (!(valid && bait_find(bt, key, t, te))) t = te = 0;
                // the lowest lane with an anchor left names a diagonal; every lane whose next anchor gives the same one moves on
                while (true) {
                    const u64 pend = __ballot(t < te);
                    if (!pend) break;
                    const u32 my = t < te ? bt.ids[t] - p : 0u;
                    const u32 dd = __shfl(my, __ffsll((long long)pend) - 1, 64);
                    if (t < te && my == dd) t++;
                    bool known = false;
#pragma unroll
                    for (int j = 0; j < PU_WORDS; j++) known |= (u32)(j * 64 + lane) < nd && reg[j] == dd;
                    if (__ballot(known)) continue;
                    if (nd == (u32)PU_DIAGS) { over = true; break; }
#pragma unroll
                    for (int j = 0; j < PU_WORDS; j++) if ((nd >> 6) == (u32)j && (nd & 63u) == (u32)lane) reg[j] = dd;
                    nd++;
                }
                return false;
            });
            if (W == 0) break;                // no window: the other orientation has none either
            if (!over) {
                if (nd == 0) continue;
                u64 base = 0;
                if (lane == 0) base = atomicAdd((unsigned long long*)cursor, (unsigned long long)nd * W);
                base = __shfl(base, 0, 64);
                u32 done = 0;
                for_each_chunk(text, s, e, K, lane, [&](u64 c0, bool valid, u64 x) {
                    u64 key;
                    u32 p;
                    pu_orient(K, o, L, c0 - s + lane, x, key, p);
                    const u64 vm = __ballot(valid);
                    const u32 rank = done + popc_below(vm);
                    for (u32 q = 0; q < nd; q++) {          // diagonal q's pairs are [base + q W, base + (q + 1) W), in window order
                        const u32 dd = pu_diag(reg, q);
                        const u64 pos = base + (u64)q * W + rank;
                        if (valid && pos < cap) { coords[pos] = dd + p; kmers[pos] = key; }
                    }
                    done += (u32)__popcll(vm);
                    return false;
                });
                continue;
            }
            // more diagonals than the registers hold: no list.  An anchor's diagonal is new iff no earlier window of the line
            // gives it too (a window's own anchors are distinct), which its lane finds out by rolling through those windows;
            // the lanes with a new one take W places each and write them one after the other.
            for_each_chunk(text, s, e, K, lane, [&](u64 c0, bool valid, u64 x) {
                u64 key;
                u32 p, t = 0, te = 0;
                const u64 i = c0 - s + lane;
                pu_orient(K, o, L, i, x, key, p);
                if (!(valid && bait_find(bt, key, t, te))) t = te = 0;
                while (__ballot(t < te)) {
                    const bool has = t < te;
                    const u32 d = has ? bt.ids[t] - p : 0u;
                    bool fresh = has;
                    if (has)
                        roll_windows(text, s, i + (u64)K - 1, K, [&](u64 j, u64 xj) {
                            u64 kj; u32 pj;
                            pu_orient(K, o, L, j, xj, kj, pj);
                            if (pu_has_anchor(bt, kj, d + pj)) fresh = false;
                            return !fresh;
                        });
                    const u64 fm = __ballot(fresh);
                    if (fm) {
                        u64 base = 0;
                        if (lane == 0) base = atomicAdd((unsigned long long*)cursor, (unsigned long long)__popcll(fm) * W);
                        base = __shfl(base, 0, 64) + (u64)popc_below(fm) * W;
                        if (fresh)
                            roll_windows(text, s, L, K, [&](u64 j, u64 xj) {
                                u64 kj; u32 pj;
                                pu_orient(K, o, L, j, xj, kj, pj);
                                if (base < cap) { coords[base] = d + pj; kmers[base] = kj; }
                                base++;
                                return false;
                            });
                    }
                    if (has) t++;
                }
                return false;
            });
        }
    }
}

static int anchor_pileup(zk_ctx* c, const zk_bait_table* anchors, const u8* text, const u64* lines, uint64_t n_reads, int K, u32 pad,
                         u32* coords, u64* kmers, uint64_t cap, uint64_t* n_out) {
    *n_out = 0;
    if (n_reads == 0 || anchors->n_keys == 0) return ZK_OK;
    const BaitView bt = view_of(anchors);
    const u32 grid = grid_cap(c, div_up(n_reads, 4), 16);
    u64* d_long = &c->d_scalars->pileup_long;
    u64* d_cur = &c->d_scalars->pileup_cursor;
    ZK_HIP(c, hipMemsetAsync(d_long, 0, sizeof(u64), c->stream));
    ZK_HIP(c, hipMemsetAsync(d_cur, 0, sizeof(u64), c->stream));
    hipLaunchKernelGGL(long_line_kernel, dim3(grid), dim3(256), 0, c->stream, bt, text, lines, (u64)n_reads, K, (u64)pad, d_long);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(fetch(c, &c->h_scalars->pileup_long));
    ZK_TRY(check_device_error(c));
    if (c->h_scalars->pileup_long)
        return fail(c, ZK_ERANGE, "zk_anchor_pileup: a sequence line longer than pad = %u has a hit: its coordinates could name another zone", pad);
    uint64_t text_bytes = 0;
    if (c->profile) ZK_HIP(c, hipMemcpy(&text_bytes, lines + 4 * n_reads - 1, sizeof(u64), hipMemcpyDeviceToHost));
    prof_begin(c, ZK_PROF_PILEUP, text_bytes);
    hipLaunchKernelGGL(pileup_kernel, dim3(grid), dim3(256), 0, c->stream, bt, text, lines, (u64)n_reads, K, coords, kmers, (u64)cap, d_cur);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(fetch(c, &c->h_scalars->pileup_cursor));
    ZK_TRY(check_device_error(c));
    const uint64_t total = c->h_scalars->pileup_cursor;
    *n_out = total;
    prof_add_bytes(c, ZK_PROF_PILEUP, 12 * (total < cap ? total : cap));
    if (total >= (1ull << 32))
        return fail(c, ZK_ERANGE, "zk_anchor_pileup: %llu pairs in one batch (at most 2^32 - 1); use smaller batches", (unsigned long long)total);
    if (total > cap) return no_room(c, "zk_anchor_pileup", "pairs", total, cap);
    return ZK_OK;
}

// ---------------------------------------------------------------------------------------
// zk_pileup_count
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pileup_index_kernel(const u32* __restrict__ v, u64 n, u64* __restrict__ keys, u32* __restrict__ idx) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) { keys[i] = v[i]; idx[i] = (u32)i; }
}

__global__ __launch_bounds__(256) void pileup_gather_kernel(const u64* __restrict__ k, const u32* __restrict__ idx, u64 n, u64* __restrict__ out) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) out[i] = k[idx[i]];
}

struct PileupHeads {     // the first of each run of equal (coordinate, k-mer) in the sorted pairs; heads[pos] = where it starts
    const u64* c; const u64* k; u32* oc; u64* ok; u32* heads;
    __device__ bool flag(u64 i) const { return i == 0 || c[i] != c[i - 1] || k[i] != k[i - 1]; }
    __device__ void store(u64 pos, u64 i) const { oc[pos] = (u32)c[i]; ok[pos] = k[i]; heads[pos] = (u32)i; }
};

__global__ __launch_bounds__(256) void pileup_runs_kernel(const u32* __restrict__ heads, u64 m, u64 n, u32* __restrict__ cnt) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (u64)gridDim.x * blockDim.x)
        cnt[j] = (j + 1 < m ? heads[j + 1] : (u32)n) - heads[j];
}

static int pileup_count(zk_ctx* c, const u32* coords, const u64* kmers, uint64_t n, int K, u32* oc, u64* ok, u32* cnt, uint64_t cap,
                        uint64_t* n_out) {
    *n_out = 0;
    if (n == 0) return ZK_OK;
    const uint64_t need = 52 * n + n / 16 + (8 << 20);
    ZK_TRY(arena_require(c, need, need));
    u64 *ka, *kb, *ca, *cb; u32 *va, *vb, *ia, *ib;
    ZK_TRY(arena_alloc(c, 8 * n, (void**)&ka));
    ZK_TRY(arena_alloc(c, 8 * n, (void**)&kb));
    ZK_TRY(arena_alloc(c, 8 * n, (void**)&ca));
    ZK_TRY(arena_alloc(c, 8 * n, (void**)&cb));
    ZK_TRY(arena_alloc(c, 4 * n, (void**)&va));
    ZK_TRY(arena_alloc(c, 4 * n, (void**)&vb));
    ZK_TRY(arena_alloc(c, 4 * n, (void**)&ia));
    ZK_TRY(arena_alloc(c, 4 * n, (void**)&ib));
    ZK_HIP(c, hipMemcpyAsync(ka, kmers, 8 * n, hipMemcpyDeviceToDevice, c->stream));
    ZK_HIP(c, hipMemcpyAsync(va, coords, 4 * n, hipMemcpyDeviceToDevice, c->stream));
    const u32 g = grid_cap(c, div_up(n, 256), 16);
    u64 *rk, *sc; u32 *rv, *si;
    ZK_TRY(sort_pairs(c, ka, kb, va, vb, n, 2 * K, &rk, &rv));                  // by k-mer, the coordinate carried
    hipLaunchKernelGGL(pileup_index_kernel, dim3(g), dim3(256), 0, c->stream, rv, (u64)n, ca, ia);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(sort_pairs(c, ca, cb, ia, ib, n, 32, &sc, &si));                     // by coordinate, stable: k-mers ascend within one
    u64* sk = rk == ka ? kb : ka;
    prof_begin(c, ZK_PROF_PILEUP_CUT, 20 * n);
    hipLaunchKernelGGL(pileup_gather_kernel, dim3(g), dim3(256), 0, c->stream, rk, si, (u64)n, sk);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    PileupHeads ph{sc, sk, oc, ok, nullptr};
    u64* tiles;
    uint64_t m = 0;
    ZK_TRY(compact_count(c, ph, n, &tiles, &m));
    *n_out = m;
    if (m > cap) return no_room(c, "zk_pileup_count", "distinct pairs", m, cap);
    ph.heads = rv == va ? vb : va;          // m <= n words, free since the first sort
    prof_begin(c, ZK_PROF_PILEUP_CUT, 16 * n + 20 * m);
    ZK_TRY(compact_write(c, ph, n, tiles));
    prof_end(c);
    hipLaunchKernelGGL(pileup_runs_kernel, dim3(grid_cap(c, div_up(m, 256), 16)), dim3(256), 0, c->stream, ph.heads, (u64)m, (u64)n, cnt);
    ZK_HIP(c, hipGetLastError());
    return check_device_error(c);
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_anchor_pileup(zk_ctx* c, const zk_bait_table* anchors, const uint8_t* d_text, const uint64_t* d_lines, uint64_t n_reads, int K,
                     uint32_t pad, uint32_t* d_coords, uint64_t* d_kmers, uint64_t cap, uint64_t* n_out) {
    ZK_ARGS(c, anchors && n_out && n_reads < (1ull << 32) && (n_reads == 0 || (d_text && d_lines)) && (cap == 0 || (d_coords && d_kmers)));
    if (K < 1 || K > 32) return fail(c, ZK_EINVAL, "zk_anchor_pileup: K = %d, 1 <= K <= 32", K);
    if (anchors->K != K) return fail(c, ZK_EINVAL, "zk_anchor_pileup: K = %d, the anchor table was built with K = %d", K, anchors->K);
    arena_reset(c);
    return anchor_pileup(c, anchors, d_text, (const u64*)d_lines, n_reads, K, pad, d_coords, (u64*)d_kmers, cap, n_out);
}

int zk_pileup_count(zk_ctx* c, const uint32_t* d_coords, const uint64_t* d_kmers, uint64_t n, int K, uint32_t* d_oc, uint64_t* d_ok,
                    uint32_t* d_cnt, uint64_t cap, uint64_t* n_out) {
    ZK_ARGS(c, n_out && n < (1ull << 32) && (n == 0 || (d_coords && d_kmers)) && (cap == 0 || (d_oc && d_ok && d_cnt)));
    if (K < 1 || K > 32) return fail(c, ZK_EINVAL, "zk_pileup_count: K = %d, 1 <= K <= 32", K);
    arena_reset(c);
    return pileup_count(c, d_coords, (const u64*)d_kmers, n, K, d_oc, (u64*)d_ok, d_cnt, cap, n_out);
}

}  // extern "C"
