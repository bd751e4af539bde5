// spikein.hip -- `zot spikein` (zotmer/commands/spikein.py): simulated read pairs cut from zones of a genome, as two FASTQ texts.
//
// The reference draws, pair after pair, an allele, a start, a fragment length, a strand and per-base errors from Python's
// random, and formats a record per mate (spikein.py:267-317).  Here every draw is rnd(seed, tag, index) of zotmer_amd/synth.py,
// a pure function of the pair's number p in output order, so the pairs [first, first + count) of any call are the same bytes.
// Two entries of include/zotk.h:
//   * zk_spike_zone_counts: draw n falls into the zone whose cumulative length first exceeds rnd(seed, T_ZONE, n) % T.  A
//     thread per draw, a binary search, an LDS add; a workgroup flushes its LDS counts with one 64-bit add per zone it met.
//   * zk_spike_pairs: spike_size_kernel, a wave per pair, finds the pair's zone, allele, start, length and strand (the same in
//     every lane), checks them against the tables, and counts the errors of both mates, lanes over bases, which is all the
//     record lengths depend on; scan64_inclusive turns the lengths into offsets; spike_write_kernel, a wave per pair again,
//     repeats the draws and writes: lanes take the bytes of the header prefix, then base j of the read and byte j of the
//     quality line, 64 neighbouring bytes a step; the error entries of a step are placed by a wave scan of their lengths.
//     The few bytes of `u fl s` are lane 0's.  No thread's work grows with L beyond its share of L / 64 steps.
// No atomics in zk_spike_pairs, nothing waits on another workgroup but inside scan64_inclusive.
#include "internal.hpp"
#include "search.hpp"

namespace zk {

constexpr u64 SP_T_ZONE = 16, SP_T_ALLELE = 17, SP_T_POS = 18, SP_T_LEN = 19, SP_T_STRAND = 20, SP_T_ERR = 21;     // synth.py
constexpr long long SP_IH_MAX = 6 * 65535;
constexpr long long SP_COORD_MAX = 1ll << 62;

__device__ __host__ __forceinline__ u64 sp_mix64(u64 z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---------------------------------------------------------------------------------------
// zk_spike_zone_counts
// ---------------------------------------------------------------------------------------
constexpr int ZC_BLOCK = 256, ZC_LDS = 4096;      // zones below ZC_LDS are counted in LDS, the ones above straight in memory

__global__ __launch_bounds__(ZC_BLOCK) void spike_zone_kernel(const u64* __restrict__ cum, u64 nz, u64 s_zone, u64 first, u64 count,
                                                              u64* __restrict__ counts, u64* bad) {
    __shared__ u32 bins[ZC_LDS];
    for (int i = threadIdx.x; i < ZC_LDS; i += ZC_BLOCK) bins[i] = 0;
    const u64 T = cum[nz - 1];
    if (T == 0) {                                  // (the same in every thread)
        if (threadIdx.x == 0) *bad = 1;
        return;
    }
    __syncthreads();
    for (u64 n = (u64)blockIdx.x * ZC_BLOCK + threadIdx.x; n < count; n += (u64)gridDim.x * ZC_BLOCK) {
        const u64 r = sp_mix64(s_zone + first + n) % T;
        const u64 lo = upper_bound(cum, 0ull, nz - 1, r);   // the first zone whose cumulative length exceeds r; the last one's does
        if (lo < (u64)ZC_LDS) atomicAdd(&bins[lo], 1u);
        else atomicAdd(&counts[lo], 1ull);
    }
    __syncthreads();
    const u32 m = nz < (u64)ZC_LDS ? (u32)nz : (u32)ZC_LDS;
    for (u32 z = threadIdx.x; z < m; z += ZC_BLOCK)
        if (bins[z]) atomicAdd(&counts[z], (u64)bins[z]);
}

// ---------------------------------------------------------------------------------------
// zk_spike_pairs
// ---------------------------------------------------------------------------------------
struct SpikeArgs {
    const u8* text; u64 n_text;
    const u64* zones;          // 12 words a zone: {text offset, window start, window length, G, s0, e0} of the wild type, then of the mutant
    const u64* first;          // n_zones + 1 pair numbers
    u64 nz;
    const u8* heads; const u64* head_offs; u64 n_heads;
    u64 s_allele, s_pos, s_len, s_strand, s_err;     // mix64(seed + tag)
    u32 L;
    long long I, sd_q;
    u64 thr_v, thr_e;
    u64 p0, count;
};

// what the draws of pair p say, the same in every lane
struct PairGeo {
    u64 text_at;               // where base u of the allele lies in the text
    u64 head_at; u32 plen;     // the header prefix
    long long u, fl;
    u32 minus;
};

// false: the tables do not hold pair p, or its fragment leaves its window
__device__ __forceinline__ bool spike_geo(const SpikeArgs& a, u64 p, PairGeo& g) {
    // The first zone whose pairs end after p.  Hand-written, not search.hpp's partition_point: with that midpoint both kernels
    // that call this ran 1 % slower (3.96 against 3.91 ms a call, three runs each, alternated); lo + hi cannot wrap here, nz
    // counts 96-byte rows of device memory.
    u64 lo = 0, hi = a.nz;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (a.first[mid + 1] <= p) lo = mid + 1; else hi = mid;
    }
    if (lo >= a.nz || a.first[lo] > p) return false;
    const u64 z = lo;
    const u32 mut = (sp_mix64(a.s_allele + p) & 0xffffffffull) < a.thr_v ? 1u : 0u;
    const u64* row = a.zones + 12 * z + 6 * mut;
    const u64 text_off = row[0], wl = row[2];
    const long long w0 = (long long)row[1], G = (long long)row[3], s0 = (long long)row[4], e0 = (long long)row[5];
    if (e0 < s0 || s0 <= -SP_COORD_MAX || e0 >= SP_COORD_MAX || G < 0 || G >= SP_COORD_MAX || w0 < 0 || w0 > G) return false;
    if (wl > a.n_text || text_off > a.n_text - wl || wl > (u64)(G - w0)) return false;
    const u64 span = (u64)(e0 - s0) + 1;
    long long u = s0 + (long long)(sp_mix64(a.s_pos + p) % span);
    long long zsum = -SP_IH_MAX;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const u64 r = sp_mix64(a.s_len + 3 * p + k);
        zsum += (long long)((r & 0xffffu) + ((r >> 16) & 0xffffu) + ((r >> 32) & 0xffffu) + (r >> 48));
    }
    long long fl = a.I + ((a.sd_q * zsum) >> 32);              // arithmetic shift: floors
    const long long fmin = (long long)a.L + (long long)(a.L / 2);
    if (fl < fmin) fl = fmin;
    if (u - fl < 0) u = fl;
    if (u + fl > G) u = G - fl;
    if (u < w0 || u + fl > w0 + (long long)wl) return false;
    const u64 h0 = a.head_offs[z], h1 = a.head_offs[z + 1];
    if (h0 > h1 || h1 > a.n_heads || h1 - h0 >= (1ull << 31)) return false;
    g.text_at = text_off + (u64)(u - w0);
    g.head_at = h0; g.plen = (u32)(h1 - h0);
    g.u = u; g.fl = fl;
    g.minus = (u32)(sp_mix64(a.s_strand + p) & 1);
    return true;
}

// {entry bytes without separators, entries} of the errors of one mate, summed over the wave
__device__ __forceinline__ u64 spike_error_sizes(const SpikeArgs& a, u64 p, u32 m, int lane) {
    u64 acc = 0;
    const u64 base = a.s_err + (2 * p + m) * (u64)a.L;
    for (u32 c0 = 0; c0 < a.L; c0 += 64) {
        const u32 j = c0 + lane;
        if (j < a.L && (sp_mix64(base + j) & 0xffffffffull) < a.thr_e) acc += (u64)(dec_digits(j) + 3) | (1ull << 32);
    }
    return wave_sum_u64(acc);
}

__global__ __launch_bounds__(256) void spike_size_kernel(SpikeArgs a, u64* __restrict__ len1, u64* __restrict__ len2, u64* bad) {
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    const u64 nw = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 i = wave; i < a.count; i += nw) {
        const u64 p = a.p0 + i;
        PairGeo g;
        if (!spike_geo(a, p, g)) {                 // (the same in every lane)
            if (lane == 0) { *bad = 1; len1[i] = 0; len2[i] = 0; }
            continue;
        }
        // '@' prefix u ' ' fl ' ' s ' ' errors '\n' read '\n' '+' '\n' quality '\n'
        const u64 fixed = 1 + (u64)g.plen + dec_digits((u64)g.u) + 1 + dec_digits((u64)g.fl) + 1 + 1 + 1 + 1 + 2 * (u64)a.L + 4;
#pragma unroll
        for (u32 m = 0; m < 2; m++) {
            const u64 e = spike_error_sizes(a, p, m, lane);
            const u64 n = e >> 32, bytes = (e & 0xffffffffull) + (n ? n - 1 : 0);
            if (lane == 0) (m ? len2 : len1)[i] = fixed + bytes;
        }
    }
}

__device__ __forceinline__ void sp_put(u8* __restrict__ out, u64 cap, u64 pos, u32 ch) {
    if (pos < cap) out[pos] = (u8)ch;
}
// x in decimal, its last digit at pos + d - 1
__device__ __forceinline__ void sp_put_number(u8* __restrict__ out, u64 cap, u64 pos, u64 x, u32 d) {
    for (u32 k = d; k-- > 0;) { sp_put(out, cap, pos + k, '0' + (u32)(x % 10)); x /= 10; }
}

__device__ __forceinline__ u32 sp_code(u32 ch) { return ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u; }

__global__ __launch_bounds__(256) void spike_write_kernel(SpikeArgs a, const u64* __restrict__ incl1, const u64* __restrict__ incl2,
                                                          u8* __restrict__ out1, u64 cap1, u8* __restrict__ out2, u64 cap2) {
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    const u64 nw = ((u64)gridDim.x * blockDim.x) >> 6;
    const u32 L = a.L;
    for (u64 i = wave; i < a.count; i += nw) {
        const u64 p = a.p0 + i;
        PairGeo g;
        if (!spike_geo(a, p, g)) continue;         // (the size pass has refused the call: never taken)
        const u32 du = dec_digits((u64)g.u), dfl = dec_digits((u64)g.fl);
        for (u32 m = 0; m < 2; m++) {
            const u64* incl = m ? incl2 : incl1;
            u8* out = m ? out2 : out1;
            const u64 cap = m ? cap2 : cap1;
            const u64 o = i ? incl[i - 1] : 0, end = incl[i];
            const u64 read_at = end - (2 * (u64)L + 4), qual_at = read_at + L + 3;
            u64 err_at = o + 1 + g.plen + du + 1 + dfl + 3;
            for (u32 k = lane; k < g.plen; k += 64) sp_put(out, cap, o + 1 + k, a.heads[g.head_at + k]);
            if (lane == 0) {
                u64 q = o + 1 + g.plen;
                sp_put(out, cap, o, '@');
                sp_put_number(out, cap, q, (u64)g.u, du); q += du;
                sp_put(out, cap, q++, ' ');
                sp_put_number(out, cap, q, (u64)g.fl, dfl); q += dfl;
                sp_put(out, cap, q++, ' ');
                sp_put(out, cap, q++, g.minus ? '-' : '+');
                sp_put(out, cap, q++, ' ');
                sp_put(out, cap, read_at - 1, '\n');
                sp_put(out, cap, read_at + L, '\n');
                sp_put(out, cap, read_at + L + 1, '+');
                sp_put(out, cap, read_at + L + 2, '\n');
                sp_put(out, cap, qual_at + L, '\n');
            }
            const u64 ebase = a.s_err + (2 * p + m) * (u64)L;
            u32 ecnt = 0;                          // entries of the steps before
            for (u32 c0 = 0; c0 < L; c0 += 64) {
                const u32 j = c0 + lane;
                const bool in = j < L;
                u32 ch = 0, d = 0;
                bool hit = false;
                if (in) {
                    // mate 1 is the fragment's first L bases, mate 2 its last L, both on the fragment's strand
                    const u64 at = g.minus ? (m ? (u64)(L - 1 - j) : (u64)g.fl - 1 - j) : (m ? (u64)g.fl - L + j : (u64)j);
                    ch = a.text[g.text_at + at];
                    if (ch >= 'a' && ch <= 'z') ch -= 32;
                    if (g.minus) ch = ch == 'A' ? 'T' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch == 'T' ? 'A' : ch;
                    const u64 r = sp_mix64(ebase + j);
                    hit = (r & 0xffffffffull) < a.thr_e;
                    const u32 k = sp_code(ch), q = (u32)(r >> 32);
                    u32 t;
                    if (k < 4) { t = q % 3; t += t >= k ? 1u : 0u; }
                    else t = q & 3u;
                    d = t == 0 ? 'A' : t == 1 ? 'C' : t == 2 ? 'G' : 'T';
                    sp_put(out, cap, read_at + j, hit ? d : ch);
                    sp_put(out, cap, qual_at + j, 'I');
                }
                const u64 hm = __ballot(hit);
                if (hm == 0) continue;             // (the same in every lane)
                const u32 dj = dec_digits(j);
                const u32 sep = (ecnt == 0 && popc_below(hm) == 0) ? 0u : 1u;
                const u32 mine = hit ? dj + 3 + sep : 0u;
                const u32 upto = wave_incl_scan_u32(mine);
                if (hit) {
                    u64 q = err_at + (upto - mine);
                    if (sep) sp_put(out, cap, q++, ';');
                    sp_put_number(out, cap, q, j, dj); q += dj;
                    sp_put(out, cap, q++, ch);
                    sp_put(out, cap, q++, '>');
                    sp_put(out, cap, q, d);
                }
                err_at += (u32)__shfl((int)upto, 63, 64);
                ecnt += (u32)__popcll(hm);
            }
        }
    }
}

static int spike_pairs(zk_ctx* c, SpikeArgs a, u8* out1, uint64_t cap1, u8* out2, uint64_t cap2, uint64_t n_bytes[2]) {
    const uint64_t n = a.count;
    const uint64_t room = 16 * n + (4 << 20);
    ZK_TRY(arena_require(c, room, room));
    u64 *len1, *len2;
    ZK_TRY(arena_alloc(c, 8 * n, (void**)&len1));
    ZK_TRY(arena_alloc(c, 8 * n, (void**)&len2));
    u64* d_bad = &c->d_scalars->spike_bad;
    ZK_HIP(c, hipMemsetAsync(d_bad, 0, sizeof(u64), c->stream));
    const u32 grid = grid_cap(c, div_up(n, 4), 16);
    prof_begin(c, ZK_PROF_SPIKE_SIZE, 16 * n);
    hipLaunchKernelGGL(spike_size_kernel, dim3(grid), dim3(256), 0, c->stream, a, len1, len2, d_bad);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(scan64_inclusive(c, len1, n));
    ZK_TRY(scan64_inclusive(c, len2, n));
    prof_end(c);
    ZK_TRY(fetch(c, &c->h_scalars->spike_bad));
    ZK_TRY(fetch(c, &c->h_scalars->scan_landing[0], len1 + n - 1));
    ZK_TRY(fetch(c, &c->h_scalars->scan_landing[1], len2 + n - 1));
    ZK_TRY(check_device_error(c));
    if (c->h_scalars->spike_bad)
        return fail(c, ZK_EINVAL, "zk_spike_pairs: a pair of [%llu, %llu) has no zone in the tables, or its fragment leaves its window",
                    (unsigned long long)a.p0, (unsigned long long)(a.p0 + n));
    n_bytes[0] = c->h_scalars->scan_landing[0];
    n_bytes[1] = c->h_scalars->scan_landing[1];
    if (n_bytes[0] > cap1 || n_bytes[1] > cap2)
        return fail(c, ZK_ENOSPC, "zk_spike_pairs: %llu and %llu bytes of records, room for %llu and %llu", (unsigned long long)n_bytes[0],
                    (unsigned long long)n_bytes[1], (unsigned long long)cap1, (unsigned long long)cap2);
    prof_begin(c, ZK_PROF_SPIKE_PAIRS, n_bytes[0] + n_bytes[1]);
    hipLaunchKernelGGL(spike_write_kernel, dim3(grid), dim3(256), 0, c->stream, a, len1, len2, out1, (u64)cap1, out2, (u64)cap2);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    return check_device_error(c);
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_spike_zone_counts(zk_ctx* c, const uint64_t* d_cum, uint64_t n_zones, uint64_t seed, uint64_t first, uint64_t count, uint64_t* d_counts) {
    ZK_ARGS(c, count < (1ull << 40) && (count == 0 || (n_zones && d_cum && d_counts)));
    arena_reset(c);
    if (count == 0) return ZK_OK;
    u64* d_bad = &c->d_scalars->spike_bad;
    ZK_HIP(c, hipMemsetAsync(d_bad, 0, sizeof(u64), c->stream));
    hipLaunchKernelGGL(spike_zone_kernel, dim3(grid_cap(c, div_up(count, ZC_BLOCK * 16), 8)), dim3(ZC_BLOCK), 0, c->stream, (const u64*)d_cum,
                       (u64)n_zones, sp_mix64(seed + SP_T_ZONE), (u64)first, (u64)count, (u64*)d_counts, d_bad);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(fetch(c, &c->h_scalars->spike_bad));
    ZK_TRY(check_device_error(c));
    if (c->h_scalars->spike_bad) return fail(c, ZK_EINVAL, "zk_spike_zone_counts: the zones have no length");
    return ZK_OK;
}

int zk_spike_pairs(zk_ctx* c, const uint8_t* d_text, uint64_t n_text, const uint64_t* d_zones, const uint64_t* d_first, uint64_t n_zones,
                   const uint8_t* d_heads, const uint64_t* d_head_offs, uint64_t n_heads, uint64_t seed, int L, int64_t I, int64_t sd_q,
                   uint64_t thr_v, uint64_t thr_e, uint64_t first, uint64_t count, uint8_t* d_out1, uint64_t cap1, uint8_t* d_out2,
                   uint64_t cap2, uint64_t n_bytes[2]) {
    ZK_ARGS(c, n_bytes && count < (1ull << 40) && first < (1ull << 40) &&
                   (count == 0 || (d_zones && d_first && d_head_offs && n_zones && (n_text == 0 || d_text) && (n_heads == 0 || d_heads))) &&
                   (cap1 == 0 || d_out1) && (cap2 == 0 || d_out2));
    n_bytes[0] = n_bytes[1] = 0;
    if (L < 1 || L > (1 << 20)) return fail(c, ZK_EINVAL, "zk_spike_pairs: L = %d, 1 <= L <= 2^20", L);
    if (I < 1 || I >= (1ll << 40) || sd_q < 0 || sd_q >= (1ll << 43))
        return fail(c, ZK_EINVAL, "zk_spike_pairs: I = %lld (1 .. 2^40 - 1), sd_q = %lld (0 .. 2^43 - 1)", (long long)I, (long long)sd_q);
    if (thr_v > (1ull << 32) || thr_e > (1ull << 32)) return fail(c, ZK_EINVAL, "zk_spike_pairs: a threshold above 2^32");
    arena_reset(c);
    if (count == 0) return ZK_OK;
    SpikeArgs a;
    a.text = d_text; a.n_text = n_text;
    a.zones = (const u64*)d_zones; a.first = (const u64*)d_first; a.nz = n_zones;
    a.heads = d_heads; a.head_offs = (const u64*)d_head_offs; a.n_heads = n_heads;
    a.s_allele = sp_mix64(seed + SP_T_ALLELE); a.s_pos = sp_mix64(seed + SP_T_POS); a.s_len = sp_mix64(seed + SP_T_LEN);
    a.s_strand = sp_mix64(seed + SP_T_STRAND); a.s_err = sp_mix64(seed + SP_T_ERR);
    a.L = (u32)L; a.I = I; a.sd_q = sd_q; a.thr_v = thr_v; a.thr_e = thr_e;
    a.p0 = first; a.count = count;
    return spike_pairs(c, a, d_out1, cap1, d_out2, cap2, n_bytes);
}

}  // extern "C"
