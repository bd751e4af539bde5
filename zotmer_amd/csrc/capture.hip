// capture.hip -- `zot capture` (zotmer/commands/capture.py): reads binned by the bait sequences they touch.
//
// Three steps, each an entry of include/zotk.h:
//   * zk_bait_table_build: every K-mer of both strands of each bait record -> the ascending record ids that contain it
//     (capture.py:85-95), as sorted distinct keys + CSR offsets into u32 ids + a bucket directory over the top key bits;
//   * zk_capture_hits: one wave per read slides the read windows over its sequence line(s) in the raw FASTQ text, looks
//     every window up (directory, then a search inside one bucket of ~1 key) and emits the distinct (bait, read) pairs,
//     sorted and deduplicated (capture.py:97-116);
//   * zk_capture_gather: the four stripped lines of every captured record, bait by bait, into one buffer (ReadCache,
//     capture.py:26-69, file.readFastq, file.py:38-52).
// Records are located through the positions of the text's '\n' bytes (zk_line_ends): record r is lines 4r .. 4r+3.
#include "internal.hpp"
#include "bait_table.hpp"
#include "compact.hpp"
#include "read_window.hpp"

namespace zk {


// ---------------------------------------------------------------------------------------
// predicates (compact.hpp: NewlinePos and the run heads)
// ---------------------------------------------------------------------------------------

// item i = window at position i >> 1 of the bait stream, strand i & 1 (basics.kmersList(K, seq, True): x then rc x)
struct BaitWindow {
    const u8* stream; u64 n; int K; const u64* ends; u64 n_ends; u64* keys; u32* ids;
    __device__ bool flag(u64 i) const { u64 x, xb; return point_window(stream, n, K, i >> 1, x, xb); }
    __device__ void store(u64 pos, u64 i) const {
        u64 x, xb;
        point_window(stream, n, K, i >> 1, x, xb);
        keys[pos] = (i & 1) ? xb : x;
        ids[pos] = record_of(ends, n_ends, i >> 1);
    }
};

struct DistinctPairs : PairRunHead {   // (key, id) runs of a key-sorted, id-stable array -> (key, id)
    u64* ok; u32* ov;
    __device__ void store(u64 pos, u64 i) const { ok[pos] = k[i]; ov[pos] = v[i]; }
};
struct DistinctKeys : KeyRunHead {     // key runs -> (key, CSR offset)
    u64* ok; u32* offs;
    __device__ void store(u64 pos, u64 i) const { ok[pos] = k[i]; offs[pos] = (u32)i; }
};
struct DistinctWords : KeyRunHead {    // word runs -> the word
    u64* out;
    __device__ void store(u64 pos, u64 i) const { out[pos] = k[i]; }
};

// ---------------------------------------------------------------------------------------
// the table
// ---------------------------------------------------------------------------------------
// (the table itself, its view and the lookup: bait_table.hpp; the directory: search.hpp)

__global__ void put_u32_kernel(u32* p, u32 v) { *p = v; }

void table_free(zk_bait_table* t) {
    if (!t) return;
    if (t->ctx) { enter(t->ctx); (void)hipStreamSynchronize(t->ctx->stream); }
    if (t->keys) (void)hipFree(t->keys);
    if (t->offs) (void)hipFree(t->offs);
    if (t->ids) (void)hipFree(t->ids);
    if (t->dir) (void)hipFree(t->dir);
    delete t;
}

int tmalloc(zk_ctx* c, void** p, uint64_t bytes) {
    hipError_t e = hipMalloc(p, bytes < 256 ? 256 : bytes);
    if (e != hipSuccess) return fail(c, ZK_ENOMEM, "hipMalloc(%llu) for the bait table failed: %s", (unsigned long long)bytes, hipGetErrorString(e));
    return ZK_OK;
}

int bait_table_directory(zk_ctx* c, zk_bait_table* t) {
    // about one key per bucket
    int bits = 1;
    while (bits < 26 && (1ull << bits) < t->n_keys) bits++;
    if (bits > t->kbits) bits = t->kbits;
    t->bits = bits;
    const u64 nb = 1ull << bits;
    ZK_TRY(tmalloc(c, (void**)&t->dir, 4 * (nb + 1)));
    ZK_TRY(key_dir_build(c, t->keys, (u64)t->n_keys, t->kbits - bits, nb, t->dir));
    return check_device_error(c);
}

static int bait_table_build(zk_ctx* c, const u8* stream, uint64_t n, int K, zk_bait_table* t) {
    t->ctx = c; t->K = K; t->kbits = 2 * K;
    const uint64_t W = 2 * n;             // windows x strands, an upper bound
    ZK_TRY(arena_require(c, 8 * n + 32 * W + W / 32 + (4 << 20), 8 * n + 32 * W + W / 32 + (4 << 20)));
    u64* cnt;
    uint64_t n_rec = 0;
    NewlinePos nl{stream, nullptr};
    ZK_TRY(compact_count(c, nl, n, &cnt, &n_rec));
    u64* ends;
    ZK_TRY(arena_alloc(c, 8 * (n_rec + 1), (void**)&ends));
    nl.out = ends;
    ZK_TRY(compact_write(c, nl, n, cnt));
    t->n_records = n_rec;
    u64 *keys, *alt; u32 *ids, *valt;
    ZK_TRY(arena_alloc(c, 8 * W + 8, (void**)&keys));
    ZK_TRY(arena_alloc(c, 8 * W + 8, (void**)&alt));
    ZK_TRY(arena_alloc(c, 4 * W + 4, (void**)&ids));
    ZK_TRY(arena_alloc(c, 4 * W + 4, (void**)&valt));
    BaitWindow bw{stream, (u64)n, K, ends, (u64)n_rec, keys, ids};
    uint64_t nw = 0;
    ZK_TRY(compact_count(c, bw, W, &cnt, &nw));
    ZK_TRY(compact_write(c, bw, W, cnt));
    if (nw >= 0xffffffffull) return fail(c, ZK_ERANGE, "bait table: %llu k-mers (at most 2^32 - 1)", (unsigned long long)nw);
    u64* rk = keys; u32* rv = ids;
    if (nw) ZK_TRY(sort_pairs(c, keys, alt, ids, valt, nw, 2 * K, &rk, &rv));
    u64* k2 = (rk == keys) ? alt : keys;
    uint64_t n_ids = 0;
    DistinctPairs dp{{rk, rv}, k2, nullptr};
    ZK_TRY(compact_count(c, dp, nw, &cnt, &n_ids));
    ZK_TRY(tmalloc(c, (void**)&t->ids, 4 * n_ids));
    dp.ov = t->ids;
    ZK_TRY(compact_write(c, dp, nw, cnt));
    uint64_t n_keys = 0;
    DistinctKeys dk{{k2}, nullptr, nullptr};
    ZK_TRY(compact_count(c, dk, n_ids, &cnt, &n_keys));
    ZK_TRY(tmalloc(c, (void**)&t->keys, 8 * n_keys));
    ZK_TRY(tmalloc(c, (void**)&t->offs, 4 * (n_keys + 1)));
    dk.ok = t->keys; dk.offs = t->offs;
    ZK_TRY(compact_write(c, dk, n_ids, cnt));
    hipLaunchKernelGGL(put_u32_kernel, dim3(1), dim3(1), 0, c->stream, t->offs + n_keys, (u32)n_ids);
    ZK_HIP(c, hipGetLastError());
    t->n_ids = n_ids; t->n_keys = n_keys;
    return bait_table_directory(c, t);
}

// ---------------------------------------------------------------------------------------
// window lookup: one wave per read
// ---------------------------------------------------------------------------------------

// MARK: lane 0 of a wave whose read is vetoed says so in mark[r] (zk_pulldown_hits counts those reads and keeps them out of its
// histogram); zk_capture_hits runs the instantiation without it
template <bool MARK>
__global__ __launch_bounds__(256) void capture_hits_kernel(BaitView bt, BaitView vt, int RK, Mate m1, Mate m2, u64 n_reads,
                                                           u64* __restrict__ pairs, u64 cap, u64* n_raw, u8* __restrict__ mark) {
    const WaveIds w = wave_ids();
    const int lane = w.lane;
    for (u64 r = w.wave; r < n_reads; r += w.nw) {
        // a read with any window in the veto set is not captured
        const bool veto = vt.n_keys && for_each_mate_chunk(m1, m2, r, RK, lane, [&](u64, bool valid, u64 x) {
            u32 lo, hi;
            return __ballot(valid && bait_find(vt, x, lo, hi)) != 0;
        });
        if (veto) {
            if (MARK && lane == 0) mark[r] = 1;
            continue;
        }
        for_each_mate_chunk(m1, m2, r, RK, lane, [&](u64, bool valid, u64 x) {
            u32 p = 0, pe = 0;
            if (!(valid && bait_find(bt, x, p, pe))) p = pe = 0;
            // the distinct ids of the chunk, smallest first: each lane's list ascends, the wave takes the minimum of the heads
            while (__ballot(p < pe)) {
                const u32 my = p < pe ? bt.ids[p] : 0xffffffffu;
                const u32 mn = wave_min_u32(my);
                if (lane == 0) {
                    const u64 q = atomicAdd(n_raw, 1ull);
                    if (q < cap) pairs[q] = ((u64)mn << 32) | r;
                }
                if (p < pe && my == mn) p++;
            }
            return false;
        });
    }
}

int capture_lookup(zk_ctx* c, const zk_bait_table* baits, const zk_bait_table* veto, int RK, Mate m1, Mate m2, uint64_t n_reads,
                   u64* pairs, uint64_t cap, u8* mark, uint64_t* raw) {
    u64* d_raw = &c->d_scalars->capture_raw;
    ZK_HIP(c, hipMemsetAsync(d_raw, 0, sizeof(u64), c->stream));
    const dim3 grid(grid_cap(c, div_up(n_reads, 4), 16));
    prof_begin(c, ZK_PROF_CAPTURE_HITS, 0);
    if (mark)
        hipLaunchKernelGGL(capture_hits_kernel<true>, grid, dim3(256), 0, c->stream, view_of(baits), view_of(veto), RK, m1, m2, (u64)n_reads, pairs,
                           (u64)cap, d_raw, mark);
    else
        hipLaunchKernelGGL(capture_hits_kernel<false>, grid, dim3(256), 0, c->stream, view_of(baits), view_of(veto), RK, m1, m2, (u64)n_reads, pairs,
                           (u64)cap, d_raw, (u8*)nullptr);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(fetch(c, &c->h_scalars->capture_raw));
    ZK_TRY(check_device_error(c));
    *raw = c->h_scalars->capture_raw;
    return ZK_OK;
}

int capture_sort_dedupe(zk_ctx* c, const zk_bait_table* baits, u64* pairs, uint64_t raw, uint64_t* n_pairs) {
    u64 *alt, *res;
    ZK_TRY(arena_alloc(c, 8 * raw, (void**)&alt));
    int bbits = 1;
    while (bbits < 32 && (1ull << bbits) < baits->n_records) bbits++;
    ZK_TRY(sort_keys(c, pairs, alt, raw, 32 + bbits, &res));
    if (res == pairs) ZK_HIP(c, hipMemcpyAsync(alt, pairs, 8 * raw, hipMemcpyDeviceToDevice, c->stream));
    DistinctWords dw{{alt}, pairs};
    u64* cnt;
    uint64_t n = 0;
    ZK_TRY(compact_count(c, dw, raw, &cnt, &n));
    ZK_TRY(compact_write(c, dw, raw, cnt));
    *n_pairs = n;
    return ZK_OK;
}

static int capture_hits(zk_ctx* c, const zk_bait_table* baits, const zk_bait_table* veto, int RK, Mate m1, Mate m2,
                        uint64_t n_reads, u64* pairs, uint64_t cap, uint64_t* n_pairs) {
    *n_pairs = 0;
    if (n_reads == 0 || baits->n_keys == 0) return ZK_OK;
    uint64_t raw = 0;
    ZK_TRY(capture_lookup(c, baits, veto, RK, m1, m2, n_reads, pairs, cap, nullptr, &raw));
    if (raw > cap) {
        *n_pairs = raw;
        return no_room(c, "capture", "(bait, read) pairs before deduplication", raw, cap);
    }
    if (raw == 0) return ZK_OK;
    ZK_TRY(arena_require(c, capture_sort_bytes(raw), capture_sort_bytes(raw)));
    ZK_TRY(capture_sort_dedupe(c, baits, pairs, raw, n_pairs));
    return check_device_error(c);
}

// ---------------------------------------------------------------------------------------
// record gather
// ---------------------------------------------------------------------------------------
// (a record's lines are gathered stripped: line_at + strip of read_window.hpp)
__global__ void record_len_kernel(const u64* __restrict__ pairs, u64 n, const u8* __restrict__ text, const u64* __restrict__ lines,
                                  u64 n_lines, u64* __restrict__ len, u32* err) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (u64)gridDim.x * blockDim.x) {
        const u64 r = pairs[j] & 0xffffffffull;
        u64 t = 0;
        if (4 * r + 3 < n_lines) {
            for (int i = 0; i < 4; i++) { u64 s, e; line_at(lines, 4 * r + i, s, e); strip(text, s, e); t += e - s + 1; }
        } else {
            atomicOr(err, ZK_DERR_CAPACITY);
        }
        len[j] = t;
    }
}

// one wave per record: its four stripped lines, each followed by '\n', at out + (exclusive prefix of the lengths)
__global__ void record_copy_kernel(const u64* __restrict__ pairs, u64 n, const u8* __restrict__ text, const u64* __restrict__ lines,
                                   u64 n_lines, const u64* __restrict__ incl, u8* __restrict__ out) {
    const WaveIds w = wave_ids();
    const int lane = w.lane;
    for (u64 j = w.wave; j < n; j += w.nw) {
        const u64 r = pairs[j] & 0xffffffffull;
        if (4 * r + 3 >= n_lines) continue;
        u64 o = j ? incl[j - 1] : 0;
        for (int i = 0; i < 4; i++) {
            u64 s, e;
            line_at(lines, 4 * r + i, s, e);
            strip(text, s, e);
            for (u64 k = lane; k < e - s; k += 64) out[o + k] = text[s + k];
            if (lane == 0) out[o + (e - s)] = '\n';
            o += e - s + 1;
        }
    }
}

// spans[b] = first pair of bait b, spans[nb + 1 + b] = its first output byte (b = 0 .. nb)
__global__ void bait_spans_kernel(const u64* __restrict__ pairs, u64 n, const u64* __restrict__ incl, u32 nb, u64* __restrict__ spans) {
    for (u64 b = (u64)blockIdx.x * blockDim.x + threadIdx.x; b <= nb; b += (u64)gridDim.x * blockDim.x) {
        const u64 lo = lower_bound(pairs, 0ull, n, b << 32);
        spans[b] = lo;
        spans[nb + 1 + b] = lo ? incl[lo - 1] : 0;
    }
}

static int capture_gather(zk_ctx* c, const u64* pairs, uint64_t n, uint32_t nb, const u8* text, const u64* lines, uint64_t n_lines,
                          u8* out, uint64_t cap, uint64_t* spans, uint64_t* n_bytes) {
    *n_bytes = 0;
    const uint64_t need = 8 * n + 16ull * (nb + 1) + (1 << 20);
    ZK_TRY(arena_require(c, need, need));
    u64 *len, *d_spans;
    ZK_TRY(arena_alloc(c, 8 * n + 8, (void**)&len));
    ZK_TRY(arena_alloc(c, 16ull * (nb + 1), (void**)&d_spans));
    if (n) {
        hipLaunchKernelGGL(record_len_kernel, dim3(grid_cap(c, div_up(n, 256), 16)), dim3(256), 0, c->stream, pairs, (u64)n, text, lines, (u64)n_lines, len, c->d_err);
        ZK_HIP(c, hipGetLastError());
        ZK_TRY(scan64_inclusive(c, len, n));
    }
    hipLaunchKernelGGL(bait_spans_kernel, dim3(grid_cap(c, div_up((u64)nb + 1, 256), 16)), dim3(256), 0, c->stream, pairs, (u64)n, len, nb, d_spans);
    ZK_HIP(c, hipGetLastError());
    ZK_HIP(c, hipMemcpyAsync(spans, d_spans, 16ull * (nb + 1), hipMemcpyDeviceToHost, c->stream));
    ZK_TRY(check_device_error(c));
    const uint64_t total = spans[2ull * nb + 1];
    *n_bytes = total;
    if (total > cap) return no_room(c, "capture gather", "bytes of records", total, cap);
    if (n) {
        hipLaunchKernelGGL(record_copy_kernel, dim3(grid_cap(c, div_up(n, 4), 16)), dim3(256), 0, c->stream, pairs, (u64)n, text, lines, (u64)n_lines, len, out);
        ZK_HIP(c, hipGetLastError());
    }
    return check_device_error(c);
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_bait_table_build(zk_ctx* c, const uint8_t* d_stream, uint64_t n_bytes, int K, zk_bait_table** table) {
    ZK_ARGS(c, table && K >= 1 && K <= 32 && (n_bytes == 0 || d_stream));
    *table = nullptr;
    arena_reset(c);
    zk_bait_table* t = new zk_bait_table();
    const int rc = bait_table_build(c, d_stream, n_bytes, K, t);
    if (rc != ZK_OK) { table_free(t); return rc; }
    *table = t;
    return ZK_OK;
}

int zk_bait_table_info(const zk_bait_table* t, uint64_t* n_keys, uint64_t* n_ids, uint64_t* n_records) {
    if (!t || !n_keys || !n_ids || !n_records) return ZK_EINVAL;
    *n_keys = t->n_keys; *n_ids = t->n_ids; *n_records = t->n_records;
    return ZK_OK;
}

void zk_bait_table_free(zk_bait_table* t) { table_free(t); }

int zk_line_ends(zk_ctx* c, const uint8_t* d_text, uint64_t n, uint64_t* d_out, uint64_t cap, uint64_t* n_lines) {
    ZK_ARGS(c, n_lines && (n == 0 || d_text));
    *n_lines = 0;
    arena_reset(c);
    NewlinePos nl{d_text, (u64*)d_out};
    u64* cnt;
    uint64_t total = 0;
    ZK_TRY(compact_count(c, nl, n, &cnt, &total));
    *n_lines = total;
    if (total > cap) return no_room(c, "zk_line_ends", "lines", total, cap);
    if (total && !d_out) return fail(c, ZK_EINVAL, "bad argument: d_out");
    ZK_TRY(compact_write(c, nl, n, cnt));
    return check_device_error(c);
}

int zk_capture_hits(zk_ctx* c, const zk_bait_table* baits, const zk_bait_table* veto, int read_K, const uint8_t* d_text1,
                    const uint64_t* d_lines1, const uint8_t* d_text2, const uint64_t* d_lines2, uint64_t n_reads, uint64_t* d_pairs,
                    uint64_t cap, uint64_t* n_pairs) {
    ZK_ARGS(c, baits && n_pairs && read_K >= 1 && read_K <= 32 && n_reads < (1ull << 32) && (!d_text2 == !d_lines2) &&
                   (n_reads == 0 || (d_text1 && d_lines1)) && (cap == 0 || d_pairs));
    arena_reset(c);
    return capture_hits(c, baits, veto, read_K, Mate{d_text1, (const u64*)d_lines1}, Mate{d_text2, (const u64*)d_lines2}, n_reads, (u64*)d_pairs, cap, n_pairs);
}

int zk_capture_gather(zk_ctx* c, const uint64_t* d_pairs, uint64_t n_pairs, uint32_t n_baits, const uint8_t* d_text,
                      const uint64_t* d_lines, uint64_t n_lines, uint8_t* d_out, uint64_t cap, uint64_t* spans, uint64_t* n_bytes) {
    ZK_ARGS(c, spans && n_bytes && n_baits < 0xffffffffu && (n_pairs == 0 || (d_pairs && d_text && d_lines)) && (cap == 0 || d_out));
    arena_reset(c);
    return capture_gather(c, (const u64*)d_pairs, n_pairs, n_baits, d_text, (const u64*)d_lines, n_lines, d_out, cap, spans, n_bytes);
}

}  // extern "C"
