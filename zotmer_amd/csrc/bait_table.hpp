// bait_table.hpp -- the table behind the opaque zk_bait_table of the C-ABI, shared by the files that build it (capture.hip,
// allele_tally.hip) and the kernels that look k-mers up in it.
#pragma once
#include "internal.hpp"

// device memory of its own, outlives the calls
struct zk_bait_table {
    zk_ctx* ctx = nullptr;
    u64* keys = nullptr;       // sorted distinct k-mers [n_keys]
    u32* offs = nullptr;       // [n_keys + 1]: ids[offs[i], offs[i+1]) are the records of keys[i], ascending
    u32* ids = nullptr;        // [n_ids]
    u32* dir = nullptr;        // [2^bits + 1]: keys whose top `bits` of `kbits` equal b are keys[dir[b], dir[b+1])
    uint64_t n_keys = 0, n_ids = 0, n_records = 0;
    int K = 0, kbits = 0, bits = 0;
};

namespace zk {

struct BaitView {
    const u64* keys; const u32* offs; const u32* ids; const u32* dir; u64 n_keys; int kbits, shift;
};

static inline BaitView view_of(const zk_bait_table* t) {
    BaitView v{nullptr, nullptr, nullptr, nullptr, 0, 64, 0};
    if (t && t->n_keys) v = BaitView{t->keys, t->offs, t->ids, t->dir, t->n_keys, t->kbits, t->kbits - t->bits};
    return v;
}

// x -> ids[lo, hi) of the key equal to x.  A miss costs the directory's two words (one line) and, in a non-empty
// bucket, a search among its ~1-2 keys.
__device__ __forceinline__ bool bait_find(const BaitView& t, u64 x, u32& lo, u32& hi) {
    if (t.n_keys == 0) return false;
    if (t.kbits < 64 && (x >> t.kbits) != 0) return false;
    const u64 bk = x >> t.shift;
    u32 a = t.dir[bk];
    const u32 end = t.dir[bk + 1];
    u32 e = end;
    while (a < e) { const u32 mid = (a + e) >> 1; if (t.keys[mid] < x) a = mid + 1; else e = mid; }
    if (a < end && t.keys[a] == x) { lo = t.offs[a]; hi = t.offs[a + 1]; return true; }
    return false;
}

// capture.hip
void table_free(zk_bait_table* t);
int tmalloc(zk_ctx* c, void** p, uint64_t bytes);   // memory of a table (at least 256 bytes)
// the directory over t->keys[0, t->n_keys) (t->K, kbits, n_keys set; keys on the device): the end of every way to a table.
// Synchronises and reads the device error word.
int bait_table_directory(zk_ctx* c, zk_bait_table* t);

}  // namespace zk
