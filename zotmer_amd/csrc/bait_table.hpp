// bait_table.hpp -- the table behind the opaque zk_bait_table of the C-ABI: sorted keys, CSR offsets into record ids, and a
// key directory (search.hpp) over the top key bits.
// Built by capture.hip (from bait text) and allele_tally.hip (from arrays); k-mers are looked up in it by capture.hip,
// pulldown.hip (through capture_lookup), allele_tally.hip, pileup.hip and seq_tally.hip.
#pragma once
#include "search.hpp"

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

struct BaitView { const u64* keys; const u32* offs; const u32* ids; KeyDir dir; u64 n_keys; int kbits; };

static inline BaitView view_of(const zk_bait_table* t) {
    BaitView v{nullptr, nullptr, nullptr, KeyDir{nullptr, 0}, 0, 64};
    if (t && t->n_keys) v = BaitView{t->keys, t->offs, t->ids, KeyDir{t->dir, t->kbits - t->bits}, t->n_keys, t->kbits};
    return v;
}

// x -> the position i of the key equal to x (keys[i] == x).  A miss costs the directory's two words (one line) and, in a
// non-empty bucket, a search among its ~1-2 keys.
__device__ __forceinline__ bool bait_index(const BaitView& t, u64 x, u32& i) {
    if (t.n_keys == 0) return false;
    if (t.kbits < 64 && (x >> t.kbits) != 0) return false;
    u32 a, end;
    dir_bucket(t.dir, x, a, end);
    a = lower_bound(t.keys, a, end, x);
    if (a < end && t.keys[a] == x) { i = a; return true; }
    return false;
}

// x -> ids[lo, hi) of the key equal to x
__device__ __forceinline__ bool bait_find(const BaitView& t, u64 x, u32& lo, u32& hi) {
    u32 i;
    if (!bait_index(t, x, i)) return false;
    lo = t.offs[i]; hi = t.offs[i + 1];
    return true;
}

// capture.hip
void table_free(zk_bait_table* t);
int tmalloc(zk_ctx* c, void** p, uint64_t bytes);   // memory of a table (at least 256 bytes)
// the directory over t->keys[0, t->n_keys) (t->K, kbits, n_keys set; keys on the device): the end of every way to a table.
// Synchronises and reads the device error word.
int bait_table_directory(zk_ctx* c, zk_bait_table* t);

// The two halves of zk_capture_hits, shared with zk_pulldown_hits (pulldown.hip).
struct Mate { const u8* text; const u64* lines; };   // a FASTQ text and the positions of its line ends (m2.text null: single reads)
// The window lookup, one wave per read: the (bait, read) pairs as they come, unsorted and with repeats, into pairs[0, cap);
// *raw = how many there were (beyond cap nothing is written: the caller refuses).  mark (null, or u8[n_reads] zeroed on the
// stream): 1 for every read with a window in the veto table.  Uses no arena memory; synchronises.
int capture_lookup(zk_ctx* c, const zk_bait_table* baits, const zk_bait_table* veto, int RK, Mate m1, Mate m2, uint64_t n_reads,
                   u64* pairs, uint64_t cap, u8* mark, uint64_t* raw);
// pairs[0, raw) sorted, the distinct ones back in pairs[0, *n_pairs).  Takes capture_sort_bytes(raw) from the arena (the
// caller has made room: arena_require); asynchronous but for the count.
static inline uint64_t capture_sort_bytes(uint64_t raw) { return 16 * raw + raw / 32 + (4 << 20); }
int capture_sort_dedupe(zk_ctx* c, const zk_bait_table* baits, u64* pairs, uint64_t raw, uint64_t* n_pairs);

}  // namespace zk
