// seq_tally.hip -- `zot hgvs-index -T` (zotmer/commands/hgvs-find.py:884-891): how often does a genome hold each k-mer of a
// bait table?  The reference walks basics.kmers(K, seq) over every chromosome and bumps a dict; zk_sequence_tally takes a piece
// of a FASTA record's body as it comes out of the file -- line breaks and all -- and adds to one u64 per key.
//
// What is new against read_window.hpp: there a window is cut from one line without breaks; here '\n' and '\r' fall inside
// windows and have to vanish (file.readFasta strips and joins the lines), while any other byte that is no base ends a run.
//
//   * A workgroup of 256 takes a tile of ZK_SEQTALLY_TILE text bytes, 16 consecutive bytes a thread (one 16-byte load where the
//     tile is whole).  A thread classifies its bytes -- skipped, base, breaker -- and packs the kept ones, 2 bits a symbol plus a
//     breaker flag; a block scan of the counts gives each thread its dense place, and the packed bits go to LDS with at most
//     four ORs a thread.  Dense position P = ST_PAD + (kept symbols of the tile before it), first symbol highest in a word.
//   * A window belongs to the tile that holds its LAST base, so a tile needs the K - 1 kept symbols before it and nothing after
//     it.  Wave 0 fetches them while the others scatter: it walks back from the tile's start in 64-byte steps until it has
//     K - 1 bases, or meets a breaker, or reaches the text's start, where the caller's state supplies what the pieces before
//     held (tail_bases).  The walk is one step on ordinary text and unbounded only across runs of line breaks.  The halo sits
//     at P in [ST_PAD - h, ST_PAD); everything before it is flagged as a breaker, so no window reaches further back.
//   * Then thread t rolls over the dense symbols [16 t, 16 t + 16): the 32 symbols before them are two LDS words (a ready-made
//     k-mer register) and 32 flags; per symbol one shift-or each, a window is whole when the last K flags are clear, and a
//     whole window is looked up (bait_index: a directory word pair, then ~1 key) and, on a hit, added with a 64-bit atomicAdd.
//     Hits are rare except on repeats, where one key takes many adds: integer adds, so the order does not matter.
//   * The state after the text is tail_bases at n, by a kernel of one wave.
#include "internal.hpp"
#include "bait_table.hpp"
#include "read_window.hpp"

namespace zk {

constexpr int ST_BLOCK = 256, ST_PER = 16, ST_TILE = ST_BLOCK * ST_PER, ST_PAD = 32;
static_assert(ST_TILE == ZK_SEQTALLY_TILE, "the tile include/zotk.h publishes");
constexpr int ST_SYM_WORDS = (ST_PAD + ST_TILE) / 16 + 1, ST_BRK_WORDS = (ST_PAD + ST_TILE) / 32 + 1;   // + 1: the word an OR's empty upper half names

__device__ __forceinline__ bool is_break(u32 ch) { return ch == '\n' || ch == '\r'; }

// The bases that end just before text[pos], at most `need` of them, back to the nearest breaker; where the walk reaches the
// text's start the state (sv: bases, the last one lowest; sr of them) goes on.  -> val (the last base lowest), cnt.  Called by
// a whole wave; every lane returns the same.
__device__ __forceinline__ void tail_bases(const u8* __restrict__ text, u64 pos, u32 need, u64 sv, u32 sr, int lane, u64& val, u32& cnt) {
    val = 0; cnt = 0;
    bool open = true;
    u64 p = pos;
    while (cnt < need && p > 0) {
        const u64 c0 = p >= 64 ? p - 64 : 0;
        u32 ok = 0, code = 0, brk = 0;
        if (c0 + lane < p) {
            const u32 ch = text[c0 + lane];
            code = base_code(ch, ok);
            brk = !ok && !is_break(ch);
        }
        u64 B = __ballot(ok != 0);
        const u64 X = __ballot(brk != 0);
        if (X) {
            const int hb = 63 - __clzll((long long)X);
            B = hb == 63 ? 0 : B & (~0ull << (hb + 1));
        }
        const u32 have = (u32)__popcll(B);
        const u32 take = have < need - cnt ? have : need - cnt;
        u64 mine = 0;
        if ((B >> lane) & 1) {
            const u32 r = (u32)__popcll((B >> lane) >> 1);      // bases of the chunk after mine
            if (r < take) mine = (u64)code << (2 * (cnt + r));
        }
        val |= wave_or_u64(mine);
        cnt += take;
        if (X) { open = false; break; }
        p = c0;
    }
    if (open && p == 0 && cnt < need) {
        const u32 extra = need - cnt < sr ? need - cnt : sr;
        if (extra) val |= (sv & ((1ull << (2 * extra)) - 1)) << (2 * cnt);
        cnt += extra;
    }
}

// out[0] += windows met, out[1] = min(out[1], the first header start)
__global__ __launch_bounds__(ST_BLOCK) void seq_tally_kernel(BaitView t, const u8* __restrict__ text, u64 n, u64 tiles, int K, u64 sv, u32 sr,
                                                             u64* __restrict__ counts, u64* __restrict__ out) {
    __shared__ u32 sym[ST_SYM_WORDS];     // 2 bits a dense symbol, position P at bits 30 - 2 (P % 16) of word P / 16
    __shared__ u32 brk[ST_BRK_WORDS];     // 1 flag a dense symbol (a breaker, or nothing at all), P at bit 31 - P % 32 of word P / 32
    __shared__ u32 wsum[ST_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const u64 kmask = K >= 32 ? ~0ull : (1ull << (2 * K)) - 1, fmask = (1ull << K) - 1;
    u64 nwin = 0, gt = ~0ull;
    for (u64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const u64 base = tile * ST_TILE, b0 = base + (u64)tid * ST_PER;
        for (int i = tid; i < ST_SYM_WORDS; i += ST_BLOCK) if (i >= 2) sym[i] = 0;     // words 0, 1 (and flags word 0) are the halo's: stored below
        for (int i = tid; i < ST_BRK_WORDS; i += ST_BLOCK) if (i >= 1) brk[i] = 0;
        u32 w[4] = {0, 0, 0, 0};
        u32 m = 0;                      // my bytes inside the text
        if (b0 + ST_PER <= n) {
            __builtin_memcpy(w, text + b0, 16);
            m = ST_PER;
        } else if (b0 < n) {
            m = (u32)(n - b0);
#pragma unroll
            for (int i = 0; i < ST_PER; i++)
                if ((u32)i < m) w[i >> 2] |= (u32)text[b0 + i] << (8 * (i & 3));
        }
        u32 s = 0, f = 0, c = 0;        // my kept symbols, the first highest: codes, flags, how many
        bool after_break = false;
#pragma unroll
        for (int i = 0; i < ST_PER; i++) {
            if ((u32)i < m) {
                const u32 ch = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
                if (ch == '>') {
                    const bool starts = i ? after_break : (b0 == 0 || is_break(text[b0 - 1]));
                    if (starts && b0 + i < gt) gt = b0 + i;
                }
                after_break = is_break(ch);
                if (!after_break) {
                    u32 ok;
                    const u32 code = base_code(ch, ok);
                    s |= (ok ? code : 0u) << (30 - 2 * c);
                    f |= (ok ? 0u : 1u) << (31 - c);
                    c++;
                }
            }
        }
        u32 incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const u32 v = __shfl_up(incl, o, 64); if (lane >= o) incl += v; }
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();                // the wave totals; and the zeros before the ORs
        u32 off = incl - c, T = 0;
#pragma unroll
        for (int v = 0; v < ST_BLOCK / 64; v++) { if (v < wv) off += wsum[v]; T += wsum[v]; }
        if (c) {
            const u32 P = ST_PAD + off, sh = 2 * (P & 15), fsh = P & 31;
            atomicOr(&sym[P >> 4], s >> sh);
            if (sh) atomicOr(&sym[(P >> 4) + 1], s << (32 - sh));
            atomicOr(&brk[P >> 5], f >> fsh);
            if (fsh) atomicOr(&brk[(P >> 5) + 1], f << (32 - fsh));
        }
        if (wv == 0) {
            u64 hv; u32 h;
            tail_bases(text, base, (u32)(K - 1), sv, sr, lane, hv, h);
            if (lane == 0) { sym[0] = (u32)(hv >> 32); sym[1] = (u32)hv; brk[0] = 0xffffffffu << h; }      // h <= 31
        }
        __syncthreads();
        if ((u32)tid * ST_PER < T) {
            u64 x = ((u64)sym[tid] << 32) | sym[tid + 1];            // the 32 symbols before mine
            const u32 own = sym[tid + 2];
            u64 q = ((u64)brk[tid >> 1] << 32) | brk[(tid >> 1) + 1];
            if (tid & 1) q <<= 16;
            u64 bm = q >> 32;
            const u32 ownf = (u32)(q >> 16) & 0xffffu;
            const u32 mine = T - (u32)tid * ST_PER < (u32)ST_PER ? T - (u32)tid * ST_PER : (u32)ST_PER;
#pragma unroll
            for (int i = 0; i < ST_PER; i++) {
                if ((u32)i < mine) {
                    x = (x << 2) | ((own >> (30 - 2 * i)) & 3u);
                    bm = (bm << 1) | ((ownf >> (15 - i)) & 1u);
                    if ((bm & fmask) == 0) {
                        nwin++;
                        u32 idx;
                        if (bait_index(t, x & kmask, idx)) atomicAdd(&counts[idx], 1ull);
                    }
                }
            }
        }
        __syncthreads();                // everybody has read the tile before the next one is zeroed
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nwin += __shfl_xor(nwin, o, 64);
    if (lane == 0 && nwin) atomicAdd(&out[0], nwin);
    if (gt != ~0ull) atomicMin(&out[1], gt);
}

// out[2], out[3] = the state after text[0, n)
__global__ __launch_bounds__(64) void seq_state_kernel(const u8* __restrict__ text, u64 n, int K, u64 sv, u32 sr, u64* __restrict__ out) {
    u64 v; u32 h;
    tail_bases(text, n, (u32)(K - 1), sv, sr, (int)threadIdx.x, v, h);
    if (threadIdx.x == 0) { out[2] = v; out[3] = h; }
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_sequence_tally(zk_ctx* c, const zk_bait_table* table, const uint8_t* d_text, uint64_t n, uint64_t state[2], uint64_t* d_counts,
                      uint64_t* n_windows, uint64_t* first_gt) {
    ZK_ARGS(c, table && state && n_windows && first_gt && (n == 0 || d_text) && (table->n_keys == 0 || d_counts));
    const int K = table->K;
    if (K < 1 || K > 32 || state[1] > (uint64_t)(K - 1))
        return fail(c, ZK_EINVAL, "zk_sequence_tally: a state of %llu bases, at most K - 1 = %d", (unsigned long long)state[1], K - 1);
    arena_reset(c);
    const u32 sr = (u32)state[1];
    const u64 sv = sr ? state[0] & ((1ull << (2 * sr)) - 1) : 0;
    u64* d = c->d_scalars->seqtally;
    ZK_HIP(c, hipMemsetAsync(d, 0, sizeof(u64), c->stream));
    ZK_HIP(c, hipMemsetAsync(d + 1, 0xff, sizeof(u64), c->stream));
    if (n) {
        const u64 tiles = div_up(n, ST_TILE);
        prof_begin(c, ZK_PROF_SEQ_TALLY, n);
        hipLaunchKernelGGL(seq_tally_kernel, dim3(grid_cap(c, tiles, 8)), dim3(ST_BLOCK), 0, c->stream, view_of(table), (const u8*)d_text, (u64)n, tiles,
                           K, sv, sr, (u64*)d_counts, d);
        prof_end(c);
        ZK_HIP(c, hipGetLastError());
    }
    hipLaunchKernelGGL(seq_state_kernel, dim3(1), dim3(64), 0, c->stream, (const u8*)d_text, (u64)n, K, sv, sr, d);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(fetch_span(c, c->h_scalars->seqtally, sizeof(c->h_scalars->seqtally)));
    ZK_TRY(check_device_error(c));
    const u64* h = c->h_scalars->seqtally;
    *n_windows = h[0];
    *first_gt = h[1] == ~0ull ? n : h[1];
    state[0] = h[2];
    state[1] = h[3];
    return ZK_OK;
}

}  // extern "C"
