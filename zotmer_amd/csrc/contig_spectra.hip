// contig_spectra.hip -- `zot disass` (zotmer/commands/disass.py): the histogram of k-mer multiplicities of every FASTA record
// and of the whole file.
//
// The reference walks each record's k-mers through a dict (disass.py:91-94) and the dict through a second one for the file
// (disass.py:98-100).  Here a batch of records is one base stream, each record followed by '\n':
//   * zk_contig_spectra: the windows, tagged with their record as capture.hip's BaitWindow tags them, sorted stably by key with
//     the record as payload (stream order makes the records ascend within a key); the heads of the (key, record) runs and of
//     the key runs compacted (compact.hpp: no tile waits for another; a run's length is the distance to the next head); every
//     run turned into a word record << cbits | count and a multiplicity by the rule of include/zotk.h; the words sorted on the
//     bits they use, their multiplicities added up (select.hip's reduce_by_key), the bins of frequency 0 dropped.
//   * zk_count_spectrum: the same rule over a counted key list (the file's union-summed table), then select.hip's count_hist.
#include <cmath>

#include "internal.hpp"
#include "compact.hpp"
#include "read_window.hpp"

namespace zk {

static_assert(ZK_CONTIG_TILE == CP_TILE, "ZK_CONTIG_TILE is the tile of the compaction kernels that cut the runs");

// ---------------------------------------------------------------------------------------
// predicates (compact.hpp: NewlinePos cuts the records, KeyRunHead and PairRunHead the runs)
// ---------------------------------------------------------------------------------------

// item i = the window at position i of the stream: its key (min(x, rc x) with both strands, x with one) and its record
struct ContigWindow {
    const u8* stream; u64 n; int K; int both; const u64* ends; u64 n_ends; u64* keys; u32* ids;
    __device__ bool flag(u64 i) const { u64 x, xb; return point_window(stream, n, K, i, x, xb); }
    __device__ void store(u64 pos, u64 i) const {
        u64 x, xb;
        point_window(stream, n, K, i, x, xb);
        keys[pos] = (both && xb < x) ? xb : x;
        ids[pos] = record_of(ends, n_ends, i);
    }
};

// the head of each run -> its index: RunHeads over (key, record) in a key-sorted, record-stable array, KeyHeads over the keys
template <class H>
struct HeadIndex : H {
    u32* heads;
    __device__ void store(u64 pos, u64 i) const { heads[pos] = (u32)i; }
};
using RunHeads = HeadIndex<PairRunHead>;
using KeyHeads = HeadIndex<KeyRunHead>;

struct LiveBins {        // the reduced (word, frequency) pairs whose frequency is not 0, the word widened to record << 32 | count
    const u64* w; const u32* f; int cbits; u64* ow; u64* of;
    __device__ bool flag(u64 i) const { return f[i] != 0; }
    __device__ void store(u64 pos, u64 i) const {
        const u64 x = w[i];
        ow[pos] = ((x >> cbits) << 32) | (x & ((1ull << cbits) - 1ull));
        of[pos] = f[i];
    }
};

// the dict entries of a counted key list: item i = entry i >> 1, strand i & 1 (the key itself, its reverse complement)
struct SpectrumEntries {
    const u64* keys; const void* cnts; int cbits; int K; int both; u64 seed; double p; u64* out; u32* err;
    __device__ bool flag(u64 i) const {
        const u64 k = keys[i >> 1];
        if ((i & 1) == 0) return sub_keep(k, seed, p);
        if (!both) return false;
        const u64 r = revcomp(K, k);
        return r != k && sub_keep(r, seed, p);
    }
    __device__ void store(u64 pos, u64 i) const {
        const u64 k = keys[i >> 1];
        u64 c = (cbits == 32) ? (u64)((const u32*)cnts)[i >> 1] : ((const u64*)cnts)[i >> 1];
        if (both && revcomp(K, k) == k) {       // a palindrome: x and rc x are one dict key
            if (c >> 63) atomicOr(err, ZK_DERR_COUNT_OVERFLOW);
            c <<= 1;
        }
        out[pos] = c;
    }
};

// ---------------------------------------------------------------------------------------
// runs -> outputs
// ---------------------------------------------------------------------------------------

// key run j = [heads[j], heads[j + 1]) (the last one ends at n): the key and its windows
__global__ void key_runs_kernel(const u64* __restrict__ k, u64 n, const u32* __restrict__ heads, u64 n_heads, u64* __restrict__ ok,
                                u32* __restrict__ oc) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n_heads; j += (u64)gridDim.x * blockDim.x) {
        const u64 s = heads[j], e = (j + 1 < n_heads) ? (u64)heads[j + 1] : n;
        ok[j] = k[s];
        oc[j] = (u32)(e - s);
    }
}

// (key, record) run j of len windows -> the word record << cbits | count and the number of dict entries it stands for
__global__ void run_words_kernel(const u64* __restrict__ k, const u32* __restrict__ v, u64 n, const u32* __restrict__ heads, u64 n_heads,
                                 int K, int both, u64 seed, double p, int cbits, u64* __restrict__ words, u32* __restrict__ mult) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n_heads; j += (u64)gridDim.x * blockDim.x) {
        const u64 s = heads[j], e = (j + 1 < n_heads) ? (u64)heads[j + 1] : n;
        const u64 key = k[s];
        u64 cnt = e - s;
        u32 m = sub_keep(key, seed, p) ? 1u : 0u;
        if (both) {
            const u64 r = revcomp(K, key);
            if (r == key) cnt *= 2;
            else m += sub_keep(r, seed, p) ? 1u : 0u;
        }
        words[j] = ((u64)v[s] << cbits) | cnt;
        mult[j] = m;
    }
}

static int bit_length(uint64_t v) { int b = 0; while (v) { b++; v >>= 1; } return b; }

static int contig_spectra(zk_ctx* c, const u8* stream, uint64_t n, int K, int both, u64 seed, double p, u64* d_words, u64* d_freq,
                          uint64_t cap_bins, u64* d_keys, u32* d_counts, uint64_t cap_keys, zk_contig_stats* st) {
    if (n == 0) return ZK_OK;
    // per window: keys + alt + ids + valt (24 B), the two head lists (8 B), words + alt + mult + malt (24 B), reduced words + sums (12 B);
    // per record 8 B; a record costs the stream a byte and a window one at least
    const uint64_t need = 72 * n + n / 32 + (8 << 20);
    ZK_TRY(arena_require(c, need, need));
    u64* cnt;
    uint64_t n_rec = 0;
    NewlinePos ce{stream, nullptr};
    ZK_TRY(compact_count(c, ce, n, &cnt, &n_rec));
    if (n_rec >= (1ull << 32)) return fail(c, ZK_ERANGE, "contig spectra: %llu records in one batch (fewer than 2^32)", (unsigned long long)n_rec);
    st->n_records = n_rec;
    u64* ends;
    ZK_TRY(arena_alloc(c, 8 * (n_rec + 1), (void**)&ends));
    ce.out = ends;
    ZK_TRY(compact_write(c, ce, n, cnt));

    uint64_t nw = 0;
    ContigWindow cw{stream, (u64)n, K, both, ends, (u64)n_rec, nullptr, nullptr};
    ZK_TRY(compact_count(c, cw, n, &cnt, &nw));
    if (nw >= (1ull << 31)) return fail(c, ZK_ERANGE, "contig spectra: %llu windows in one batch (fewer than 2^31)", (unsigned long long)nw);
    st->n_windows = nw;
    if (nw == 0) return ZK_OK;
    u64 *keys, *alt; u32 *ids, *valt;
    ZK_TRY(arena_alloc(c, 8 * nw + 8, (void**)&keys));
    ZK_TRY(arena_alloc(c, 8 * nw + 8, (void**)&alt));
    ZK_TRY(arena_alloc(c, 4 * nw + 4, (void**)&ids));
    ZK_TRY(arena_alloc(c, 4 * nw + 4, (void**)&valt));
    cw.keys = keys; cw.ids = ids;
    ZK_TRY(compact_write(c, cw, n, cnt));
    u64* rk = keys; u32* rv = ids;
    ZK_TRY(sort_pairs(c, keys, alt, ids, valt, nw, 2 * K, &rk, &rv));

    // the two cuts of the sorted array
    u32 *rheads, *kheads;
    uint64_t n_runs = 0, n_keys = 0;
    RunHeads rh{{rk, rv}, nullptr};
    ZK_TRY(compact_count(c, rh, nw, &cnt, &n_runs));
    ZK_TRY(arena_alloc(c, 4 * n_runs, (void**)&rheads));
    rh.heads = rheads;
    ZK_TRY(compact_write(c, rh, nw, cnt));
    KeyHeads kh{{rk}, nullptr};
    ZK_TRY(compact_count(c, kh, nw, &cnt, &n_keys));
    ZK_TRY(arena_alloc(c, 4 * n_keys, (void**)&kheads));
    kh.heads = kheads;
    ZK_TRY(compact_write(c, kh, nw, cnt));
    st->n_keys = n_keys;
    const bool keys_fit = n_keys <= cap_keys;
    if (keys_fit) {
        hipLaunchKernelGGL(key_runs_kernel, dim3(grid_cap(c, div_up(n_keys, 256), 16)), dim3(256), 0, c->stream, rk, (u64)nw, kheads, (u64)n_keys,
                           d_keys, d_counts);
        ZK_HIP(c, hipGetLastError());
    }

    // runs -> (word, multiplicity), sorted on the bits in use: a count is at most 2 nw, a record at most n_rec - 1
    const int cbits = bit_length(2 * nw), rbits = bit_length(n_rec ? n_rec - 1 : 0);
    u64 *words, *walt; u32 *mult, *malt;
    ZK_TRY(arena_alloc(c, 8 * n_runs + 8, (void**)&words));
    ZK_TRY(arena_alloc(c, 8 * n_runs + 8, (void**)&walt));
    ZK_TRY(arena_alloc(c, 4 * n_runs + 4, (void**)&mult));
    ZK_TRY(arena_alloc(c, 4 * n_runs + 4, (void**)&malt));
    hipLaunchKernelGGL(run_words_kernel, dim3(grid_cap(c, div_up(n_runs, 256), 16)), dim3(256), 0, c->stream, rk, rv, (u64)nw, rheads, (u64)n_runs, K,
                       both, seed, p, cbits, words, mult);
    ZK_HIP(c, hipGetLastError());
    u64* sw = words; u32* sm = mult;
    ZK_TRY(sort_pairs(c, words, walt, mult, malt, n_runs, cbits + (rbits ? rbits : 1), &sw, &sm));
    u64* uniq; u32* sums;
    ZK_TRY(arena_alloc(c, 8 * n_runs + 8, (void**)&uniq));
    ZK_TRY(arena_alloc(c, 4 * n_runs + 4, (void**)&sums));
    uint64_t n_uniq = 0;
    ZK_TRY(reduce_by_key(c, sw, sm, n_runs, uniq, sums, n_runs, &n_uniq));
    uint64_t n_bins = 0;
    LiveBins lb{uniq, sums, cbits, d_words, d_freq};
    ZK_TRY(compact_count(c, lb, n_uniq, &cnt, &n_bins));
    st->n_bins = n_bins;
    const bool bins_fit = n_bins <= cap_bins;
    if (bins_fit) ZK_TRY(compact_write(c, lb, n_uniq, cnt));
    ZK_TRY(check_device_error(c));
    if (!keys_fit || !bins_fit)
        return fail(c, ZK_ENOSPC, "contig spectra: %llu bins and %llu keys, room for %llu and %llu", (unsigned long long)n_bins,
                    (unsigned long long)n_keys, (unsigned long long)cap_bins, (unsigned long long)cap_keys);
    return ZK_OK;
}

static int count_spectrum(zk_ctx* c, const u64* keys, const void* cnts, int count_bits, uint64_t n, int K, int both, u64 seed, double p,
                          uint64_t* vals, uint64_t* freq, uint64_t cap_bins, uint64_t* n_bins) {
    if (n == 0) return ZK_OK;
    // the entries' counts live outside the arena: count_hist starts the arena over
    char* room;
    ZK_TRY(aux_require(c, 16 * n + 256, &room));
    uint64_t m = 0;
    u64* cnt;
    SpectrumEntries se{keys, cnts, count_bits, K, both, seed, p, (u64*)room, c->d_err};
    ZK_TRY(compact_count(c, se, 2 * n, &cnt, &m));
    ZK_TRY(compact_write(c, se, 2 * n, cnt));
    ZK_TRY(check_device_error(c));
    return count_hist(c, room, 64, m, vals, freq, cap_bins, n_bins);
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_contig_spectra(zk_ctx* c, const uint8_t* d_stream, uint64_t n_bytes, int K, int both, uint64_t seed, double p, uint64_t* d_words,
                      uint64_t* d_freq, uint64_t cap_bins, uint64_t* d_keys, uint32_t* d_counts, uint64_t cap_keys, zk_contig_stats* stats) {
    ZK_ARGS(c, stats && K >= 1 && K <= 32 && std::isfinite(p) && (n_bytes == 0 || d_stream) && (cap_bins == 0 || (d_words && d_freq)) &&
                   (cap_keys == 0 || (d_keys && d_counts)));
    *stats = zk_contig_stats{0, 0, 0, 0};
    if (n_bytes) {
        u8 last = 0;
        ZK_HIP(c, hipMemcpyAsync(&last, d_stream + n_bytes - 1, 1, hipMemcpyDeviceToHost, c->stream));
        ZK_HIP(c, hipStreamSynchronize(c->stream));
        if (last != '\n') return fail(c, ZK_EINVAL, "contig spectra: the stream does not end with the '\\n' of its last record");
    }
    arena_reset(c);
    return contig_spectra(c, d_stream, n_bytes, K, both ? 1 : 0, seed, p, (u64*)d_words, (u64*)d_freq, cap_bins, (u64*)d_keys, d_counts, cap_keys,
                          stats);
}

int zk_count_spectrum(zk_ctx* c, const uint64_t* d_keys, const void* d_counts, int count_bits, uint64_t n, int K, int both, uint64_t seed,
                      double p, uint64_t* vals, uint64_t* freq, uint64_t cap_bins, uint64_t* n_bins) {
    ZK_ARGS(c, n_bins && K >= 1 && K <= 32 && std::isfinite(p) && (count_bits == 32 || count_bits == 64) && n < (1ull << 62) &&
                   (n == 0 || (d_keys && d_counts)) && (cap_bins == 0 || (vals && freq)));
    *n_bins = 0;
    arena_reset(c);
    return count_spectrum(c, (const u64*)d_keys, d_counts, count_bits, n, K, both ? 1 : 0, seed, p, vals, freq, cap_bins, n_bins);
}

}  // extern "C"
