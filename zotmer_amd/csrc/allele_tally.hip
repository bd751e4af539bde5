// allele_tally.hip -- `zot mlst` (zotmer/commands/mlst.py:45-54 over the index of zotmer/library/index.py:67-125): which
// records of a k-mer index have ALL their k-mers in a set?
//
// The index -- S sorted distinct K-mers of both strands of every record, T CSR offsets, U ascending record numbers per k-mer --
// is a bait table (capture.hip builds it from the records' base stream; here zk_bait_table_from_arrays takes it from a file's
// arrays and zk_bait_table_arrays hands them out).  The reference starts every record at lens[j] = its number of distinct
// k-mers and takes one off for every (set k-mer, listed record) pair; zk_bait_tally counts the pairs upwards instead and
// zk_bait_record_sizes gives lens, so a record is complete when the two are equal.
//
//   * One lane per set entry, workgroups of 256 stride over tiles of ZK_TALLY_TILE entries, entry = round * 256 + thread.  The
//     set ascends and the directory is indexed by the top key bits, so neighbouring lanes read neighbouring directory words:
//     the pass streams the set once, 8 bytes an entry.
//   * A hit is a list of records.  A k-mer specific to one allele lists one record, a k-mer of a conserved stretch every allele
//     of its locus.  A lane adds a list of at most TL_SHORT ids itself; longer lists are taken one after the other by the whole
//     wave (a ballot of their lanes, lo / hi broadcast, lane l adds ids[lo + l], ids[lo + l + 64], ...).  Ids within a key are
//     distinct, so one such instruction never adds twice to one address.
//   * The counters are u32 adds without a return value to d_hits in global memory: at most n_ids adds a call (a key is matched
//     at most once: an entry equal to its predecessor is skipped), hits[r] <= sizes[r] < 2^32, and integer sums do not depend on
//     the order -- the same call returns the same bits.
#include "internal.hpp"
#include "bait_table.hpp"

namespace zk {

constexpr int TL_BLOCK = 256, TL_ROUNDS = 8, TL_TILE = TL_BLOCK * TL_ROUNDS;
static_assert(TL_TILE == ZK_TALLY_TILE, "the tile include/zotk.h publishes");
constexpr u32 TL_SHORT = 4;          // a lane adds lists up to this length itself

__global__ __launch_bounds__(TL_BLOCK) void tally_kernel(BaitView t, const u64* __restrict__ k, u64 n, u64 tiles, u32* __restrict__ hits) {
    const int tid = threadIdx.x, lane = tid & 63;
    for (u64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        for (int r = 0; r < TL_ROUNDS; r++) {          // uniform across the wave: every lane reaches the ballot below
            const u64 i = tile * TL_TILE + (u64)r * TL_BLOCK + tid;
            u32 lo = 0, hi = 0;
            if (i < n) {
                const u64 x = k[i];
                if (!(i > 0 && k[i - 1] == x) && !bait_find(t, x, lo, hi)) lo = hi = 0;
            }
            const u32 len = hi - lo;
            if (len <= TL_SHORT)
                for (u32 j = lo; j < hi; j++) atomicAdd(&hits[t.ids[j]], 1u);
            u64 longs = __ballot(len > TL_SHORT);
            while (longs) {
                const int src = __ffsll((unsigned long long)longs) - 1;
                longs &= longs - 1;
                const u32 a = __shfl(lo, src, 64), b = __shfl(hi, src, 64);
                for (u32 j = a + lane; j < b; j += 64) atomicAdd(&hits[t.ids[j]], 1u);
            }
        }
    }
}

__global__ void record_sizes_kernel(const u32* __restrict__ ids, u64 n_ids, u32* __restrict__ sizes) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n_ids; j += (u64)gridDim.x * blockDim.x) atomicAdd(&sizes[ids[j]], 1u);
}

// The rules of zk_bait_table_from_arrays, in the order the header states them; *verdict (0xffffffff before) = the smallest number
// of a broken one.  Nothing is read through a value of the arrays except offs[] at places the search below keeps inside
// [0, n_keys], so arrays that break every rule are still read in bounds.
enum { TV_KEY_ORDER = 1, TV_KEY_RANGE, TV_OFFS_FIRST, TV_OFFS_ORDER, TV_OFFS_LAST, TV_ID_RANGE, TV_ID_ORDER };
static const char* const TV_TEXT[] = {"", "the keys are not strictly ascending", "a key is not below 4^K", "offs[0] is not 0",
                                      "offs is not strictly increasing (a key without records)", "offs[n_keys] is not n_ids",
                                      "a record id is not below n_records", "the ids of a key are not strictly ascending"};

__global__ void table_check_kernel(const u64* __restrict__ keys, u64 n_keys, int kbits, const u32* __restrict__ offs, const u32* __restrict__ ids,
                                   u64 n_ids, u64 n_records, u32* verdict) {
    const u64 m = n_keys > n_ids ? n_keys : n_ids;
    u32 bad = 0xffffffffu;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (u64)gridDim.x * blockDim.x) {
        u32 b = 0xffffffffu;
        if (i < n_ids) {
            // ids[i - 1] < ids[i] unless i is where a list starts: some offs[p] == i.  Rules 3-5 make offs ascend; where they are
            // broken the answer is not used (a smaller rule number wins)
            if (i > 0 && ids[i - 1] >= ids[i]) {
                const u64 lo = lower_bound(offs, 0ull, n_keys + 1, i);
                if (!(lo <= n_keys && offs[lo] == i)) b = TV_ID_ORDER;
            }
            if (ids[i] >= n_records) b = TV_ID_RANGE;
        }
        if (i < n_keys) {
            if (i == 0 && offs[n_keys] != n_ids) b = TV_OFFS_LAST;
            if (offs[i] >= offs[i + 1]) b = TV_OFFS_ORDER;
            if (i == 0 && offs[0] != 0) b = TV_OFFS_FIRST;
            if (kbits < 64 && (keys[i] >> kbits) != 0) b = TV_KEY_RANGE;
            if (i > 0 && keys[i - 1] >= keys[i]) b = TV_KEY_ORDER;
        }
        bad = b < bad ? b : bad;
    }
    if (bad != 0xffffffffu) atomicMin(verdict, bad);
}

static int table_from_arrays(zk_ctx* c, int K, const u64* keys, uint64_t n_keys, const u32* offs, const u32* ids, uint64_t n_ids,
                             uint64_t n_records, zk_bait_table* t) {
    t->ctx = c; t->K = K; t->kbits = 2 * K;
    t->n_keys = n_keys; t->n_ids = n_ids; t->n_records = n_records;
    ZK_TRY(tmalloc(c, (void**)&t->keys, 8 * n_keys));
    ZK_TRY(tmalloc(c, (void**)&t->offs, 4 * (n_keys + 1)));
    ZK_TRY(tmalloc(c, (void**)&t->ids, 4 * n_ids));
    if (n_keys) {
        ZK_HIP(c, hipMemcpyAsync(t->keys, keys, 8 * n_keys, hipMemcpyDeviceToDevice, c->stream));
        ZK_HIP(c, hipMemcpyAsync(t->offs, offs, 4 * (n_keys + 1), hipMemcpyDeviceToDevice, c->stream));
        ZK_HIP(c, hipMemcpyAsync(t->ids, ids, 4 * n_ids, hipMemcpyDeviceToDevice, c->stream));
    } else {
        ZK_HIP(c, hipMemsetAsync(t->offs, 0, 4, c->stream));
    }
    return bait_table_directory(c, t);
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_bait_table_arrays(const zk_bait_table* t, const uint64_t** d_keys, const uint32_t** d_offs, const uint32_t** d_ids) {
    if (!t || !d_keys || !d_offs || !d_ids) return ZK_EINVAL;
    *d_keys = (const uint64_t*)t->keys; *d_offs = t->offs; *d_ids = t->ids;
    return ZK_OK;
}

int zk_bait_table_from_arrays(zk_ctx* c, int K, const uint64_t* d_keys, uint64_t n_keys, const uint32_t* d_offs, const uint32_t* d_ids,
                              uint64_t n_ids, uint64_t n_records, zk_bait_table** table) {
    if (!c) return ZK_EINVAL;
    enter(c);
    if (!table) return fail(c, ZK_EINVAL, "zk_bait_table_from_arrays: a null table pointer");
    if (K < 1 || K > 32) return fail(c, ZK_EINVAL, "zk_bait_table_from_arrays: K = %d, 1 <= K <= 32", K);
    if (n_ids >= 0xffffffffull) return fail(c, ZK_EINVAL, "zk_bait_table_from_arrays: %llu ids (at most 2^32 - 2)", (unsigned long long)n_ids);
    if (n_records > (1ull << 32)) return fail(c, ZK_EINVAL, "zk_bait_table_from_arrays: %llu records (ids are 32 bits wide)", (unsigned long long)n_records);
    if (n_keys > n_ids) return fail(c, ZK_EINVAL, "zk_bait_table_from_arrays: %s (%llu keys, %llu ids)", TV_TEXT[TV_OFFS_ORDER], (unsigned long long)n_keys, (unsigned long long)n_ids);
    if (n_keys == 0 && n_ids != 0) return fail(c, ZK_EINVAL, "zk_bait_table_from_arrays: %s (no keys, %llu ids)", TV_TEXT[TV_OFFS_LAST], (unsigned long long)n_ids);
    if (n_keys && (!d_keys || !d_offs || !d_ids)) return fail(c, ZK_EINVAL, "zk_bait_table_from_arrays: a null array");
    arena_reset(c);
    if (n_keys) {
        u32* verdict = (u32*)&c->d_scalars->table_verdict;
        ZK_HIP(c, hipMemsetAsync(verdict, 0xff, sizeof(u64), c->stream));
        hipLaunchKernelGGL(table_check_kernel, dim3(grid_cap(c, div_up(n_ids, 256), 16)), dim3(256), 0, c->stream, (const u64*)d_keys, (u64)n_keys,
                           2 * K, d_offs, d_ids, (u64)n_ids, (u64)n_records, verdict);
        ZK_HIP(c, hipGetLastError());
        ZK_TRY(fetch(c, &c->h_scalars->table_verdict));
        ZK_TRY(check_device_error(c));
        const u32 v = (u32)c->h_scalars->table_verdict;
        if (v != 0xffffffffu)
            return fail(c, ZK_EINVAL, "zk_bait_table_from_arrays: %s", v < sizeof(TV_TEXT) / sizeof(TV_TEXT[0]) ? TV_TEXT[v] : "the arrays are not a table");
    }
    zk_bait_table* t = new zk_bait_table();
    const int rc = table_from_arrays(c, K, (const u64*)d_keys, n_keys, d_offs, d_ids, n_ids, n_records, t);
    if (rc != ZK_OK) { table_free(t); return rc; }
    *table = t;
    return ZK_OK;
}

int zk_bait_record_sizes(zk_ctx* c, const zk_bait_table* t, uint32_t* d_sizes) {
    if (!c) return ZK_EINVAL;
    enter(c);
    if (!t || (t->n_records && !d_sizes)) return fail(c, ZK_EINVAL, "zk_bait_record_sizes: a null table or array");
    arena_reset(c);
    if (t->n_records) ZK_HIP(c, hipMemsetAsync(d_sizes, 0, 4 * t->n_records, c->stream));
    if (t->n_ids) {
        hipLaunchKernelGGL(record_sizes_kernel, dim3(grid_cap(c, div_up(t->n_ids, 256), 16)), dim3(256), 0, c->stream, t->ids, (u64)t->n_ids, d_sizes);
        ZK_HIP(c, hipGetLastError());
    }
    return check_device_error(c);
}

int zk_bait_tally(zk_ctx* c, const zk_bait_table* t, const uint64_t* d_kmers, uint64_t n, uint32_t* d_hits) {
    if (!c) return ZK_EINVAL;
    enter(c);
    if (!t) return fail(c, ZK_EINVAL, "zk_bait_tally: a null table");
    if ((n && !d_kmers) || (t->n_records && !d_hits)) return fail(c, ZK_EINVAL, "zk_bait_tally: a null array");
    arena_reset(c);
    if (t->n_records) ZK_HIP(c, hipMemsetAsync(d_hits, 0, 4 * t->n_records, c->stream));
    if (n && t->n_keys) {
        const u64 tiles = div_up(n, TL_TILE);
        prof_begin(c, ZK_PROF_BAIT_TALLY, 8 * n);
        hipLaunchKernelGGL(tally_kernel, dim3(grid_cap(c, tiles, 8)), dim3(TL_BLOCK), 0, c->stream, view_of(t), (const u64*)d_kmers, (u64)n, tiles, d_hits);
        prof_end(c);
        ZK_HIP(c, hipGetLastError());
    }
    return check_device_error(c);
}

}  // extern "C"
