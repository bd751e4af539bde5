// internal.hpp -- host-side context shared by the libzotk translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/zotk.h"
#include "common.hpp"

// Small results (a total, a flag, a few sums) travel from the kernels to the host through one block of device words and its
// pinned mirror.  One field per purpose: a new kernel adds a field here, it never borrows one -- except a pure landing, a word
// that no kernel writes and the host only copies the end of a scan into: those share scan_landing.  Kernels only ever get raw
// pointers into the device block, so the layout is free to change -- except where a comment below says that fields are
// adjacent: those are written through one pointer or copied as one range (ZK_SPAN), and the static_asserts after the struct
// hold them in place.  A u32 counter keeps a whole u64 word (kernels take (u32*)&field, the host reads the low half).
struct zk_strand_counters { u32 n_declined, fail; };   // strand_blocks.hip: the union kernel's declined blocks, the big-block kernel's give-up flag
struct zk_scalars {
    // -- adjacent: rle_prefix reads back [rle_side .. total], the merges [total .. acgt], sort_stream [acgt .. sample_n] --
    u64 rle_side;            // rle_prefix: entries on the side list
    u64 total;               // SHARED BY DESIGN: the look-back total of the launch in flight, written by every SelState / MergeState / KwayState /
                             // tile-sort-count / collapse kernel (select, setops, kway, codec, tilesort, collapse) and read back right after it
    u64 acgt[4];             // base totals: column_sum of encode_list / union_sum / kway_union_sum, the stream histogram
    u64 n_keys;              // hist_scan_kernel: live keys of a sort
    u64 rec_info[3];         // first_newline_kernel + the stream histogram: first newline, newlines, bad bytes (one pointer)
    u64 sample_n;            // (u32) StreamSample: keys set aside; cleared together with rec_info
    // -- adjacent: dedupe_pass clears and reads back [dedupe_flags .. dedupe_m_cursor] as one range --
    u64 dedupe_flags, dedupe_n_retry, dedupe_counter, dedupe_n_big, dedupe_n_bad;   // (u32 each) DedupeArgs
    u64 dedupe_m_cursor;     // DedupeArgs::m_cursor: mirror words placed (dedupe2_kernel, then strand_mirror_kernel over the declined blocks)
    // -- no order below this line --
    u64 scan_landing[2];     // SHARED BY DESIGN: landing of scan_total's last sum (and of zk_spike_pairs' two), always fetched and read inside one
                             // call, never read across calls; the device copy is not used
    u64 dedupe_n_in;         // landing: cuts[chunks]
    u64 dedupe_n_out;        // landing: incl[chunks - 1]
    zk_strand_counters strand;
    u64 hist_big_n;          // count_hist: counts >= HIST_DENSE
    u64 capture_kept;        // capture_filter
    u64 capture_raw;         // capture.hip
    u64 intersect_n;         // intersect_count
    u64 checksum[3];         // zk_checksum
    u64 checksum_any[3];     // checksum_any
    u64 stream_checksum[7];  // zk_stream_checksum
    u64 first_descent;       // zk_first_descent
    u64 ingest_cut;          // ingest.hip
    u64 sample_heads;        // sample_heads
    u64 rle_overflow;        // (u32) rle, packed: a count beyond the field
    u64 reduce_max;          // (u32) reduce_by_key: largest sum
    u64 max_u32;             // (u32) pipeline.hip max_u32
    u64 palindromes;         // pipeline.hip count_palindromes
    u64 tag_nseg;            // (u32) tag_pass.hip: segments planned
    u64 tile_declined;       // (u32) tilesort.hip: a tile declined
    u64 strand_cursor;       // strand_keys: keys written
    u64 strand_sums[2];      // strand_pairs: orphans, palindromes
    u64 project_total;       // project_sum: column_sum of the tiles' sums
    u64 spectrum[8];         // landing: spectrum_sums' partial sums (SP_WORDS)
    u64 table_verdict;       // (u32) allele_tally.hip: the first rule that the arrays of zk_bait_table_from_arrays break
    u64 vars[4];             // vars_scan.hip: sample groups, missing contexts, mixed reference groups, the smallest missing context
    u64 links_bad;           // debruijn.hip: links_check_kernel found a key out of order or of 4^K and above
    u64 render_bad;          // debruijn.hip: contig_len_kernel found an offset out of order or a node that is no index
    u64 pileup_cursor;       // pileup.hip: pairs emitted (or that would have been)
    u64 pileup_long;         // pileup.hip: long_line_kernel found a line longer than pad with a hit
    u64 pulldown_vetoed;     // pulldown.hip: reads with a window in the veto table
    u64 capkmers_bad;        // hgvs_find.hip: capkmers_mark_kernel found a pair whose read is no record of the batch
    u64 place_bad;           // lcp_scan.hip: scan_check_kernel found an array that breaks zk_scan_place's rules
    u64 place_slots;         // landing: the last record offset = the slots of P and Q
    u64 seqtally[4];         // seq_tally.hip: windows met, the first header start (all ones: none), the state's value and its length (one pointer)
    u64 spike_bad;           // spikein.hip: a pair without a zone or a fragment outside its window; zones without length
    u64 ksnp_lists[2];       // (u32 each) ksnp.hip: groups handed to the workgroup kernel, to the tile-pair kernel (one range)
    u64 stop_long;           // stop_frames.hip: stop_long_kernel found a line longer than pad with a hit
    u64 hgvs_bad;            // hgvs_gen.hip: a variant without a zone (1), a sub in a zone without ACGT (2); a row that breaks zk_hgvs_render's rules
    u64 merge_total;         // pileup_merge.hip: pm_scan_kernel's total = the length of the union
    u64 narrow_max;          // pileup_merge.hip: narrow_max_kernel's largest count
};
// bytes of the fields first .. last (declared in that order, adjacent)
#define ZK_SPAN(first, last) (offsetof(zk_scalars, last) + sizeof(zk_scalars::last) - offsetof(zk_scalars, first))
static_assert(sizeof(zk_scalars) == 84 * sizeof(u64), "zk_scalars: u64 words only, no padding");
static_assert(ZK_SPAN(rle_side, total) == 2 * sizeof(u64), "rle_prefix reads rle_side and total back as one range");
static_assert(ZK_SPAN(total, acgt) == 5 * sizeof(u64), "the merges read total and acgt back as one range");
static_assert(ZK_SPAN(acgt, n_keys) == 5 * sizeof(u64) && ZK_SPAN(acgt, sample_n) == 9 * sizeof(u64),
              "sort_stream reads acgt, n_keys, rec_info and sample_n back as one range");
static_assert(ZK_SPAN(rec_info, sample_n) == 4 * sizeof(u64), "sort_stream clears rec_info and sample_n as one range");
static_assert(offsetof(zk_scalars, dedupe_n_retry) == offsetof(zk_scalars, dedupe_flags) + 8 &&
              offsetof(zk_scalars, dedupe_counter) == offsetof(zk_scalars, dedupe_flags) + 16 &&
              offsetof(zk_scalars, dedupe_n_big) == offsetof(zk_scalars, dedupe_flags) + 24 &&
              ZK_SPAN(dedupe_flags, dedupe_m_cursor) == 6 * sizeof(u64), "dedupe_pass clears and reads its six words as one range");

struct zk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cus = 256;
    int sort_variant = 3;      // radix-sort geometry for key arrays (zk_tune); 3 = 512 threads x 16 keys, 9-bit digits
    int short_sort = 0;        // zk_kmerize: 1 = sort only the top ~log2(n)+3 bits and finish in the mirror stage (opt-in:
                               // pays off on uncorrelated reads only)
    int packed_pairs = 1;      // (k-mer, count) pairs travel as ONE word (k-mer << s | count) through the key kernel when the counts fit the
                               // spare bits above 2K (pipeline.hip); zk_tune, tests
    int wide_tiles = 1;        // radix sort, default geometry: smaller array passes on 16 K-key tiles, one workgroup per CU (radix_sort.hip V6)
    int early_collapse = 1;    // zk_kmerize (canonical): count the copies before the sort is finished, finish it on (k-mer, count) words
                               // (pipeline.hip): 1 = as early as possible (dedupe_kernel after the passes that leave blocks of <= 32 K keys,
                               // else collapse_kernel one pass before the copies are neighbours), 3 = collapse_kernel only,
                               // 2 = a run-length pass of its own once the copies are neighbours (the round's first form), 0 = off
    int side_div = 8;          // ... side list capacity = n / side_div (tests shrink it to force the fallback)
    int pairs_variant = 7;     // ... for (key, u32) pairs: 7 = the pipeline with a payload (1024 threads x 8 pairs), 2 = one workgroup per tile, one serial chain per digit
    int stream_pass = 1;       // the first sort pass (from the base stream), over static ranges (stream_pass.hip): 1 = one 1024-thread workgroup
                               // per CU writing whole 128-byte units from LDS, 2 = two 512-thread workgroups per CU writing 64-byte units,
                               // 3 = as 2 with a tile's units leaving in two bursts (measurements); 0 = the look-back pipeline
    int tag_words = 2;         // zk_kmerize, block dedupe after two passes with at most 32 key bits below the blocks: the second pass writes
                               // only those bits, as 32-bit tags (radix_sort.hip's sort_stream); 2 (default) = ... and takes a key's place in its digit's run
                               // from a returning LDS add wherever a tile holds keys of one bucket of the pass before (pass_pipe_kernel VAR 3:
                               // 23.6-24.0 against 24.7 ms); 1 = tags, every tile ranked by ballots; 0 = whole keys
    int dedupe_variant = 0;    // block dedupe at <= 32 tag bits: dedupe2_kernel's variant (dedupe2.hip), -1 = dedupe_kernel alone
    int dedupe_limit = 65536;  // ... blocks of this many keys or more go to dedupe_kernel (16-bit counts in dedupe2_kernel's table)
    int tag_pass = 0;          // ... 1 = the pass that writes them is tag_pass.hip's count / scan / scatter over static segments, reading pass 0's
                               // keys as two arrays (6 bytes a key); 0 (default) = the look-back pipeline over whole keys.  Measured
                               // (profiles/r04/tag_pass_ab.json): the pass 25.0 -> 17.4 + 2.2 ms, but pass 0 21.3 -> 29.8 ms (half-line units)
    int kway = 1;              // zk_merge_n: 1 = up to 16 lists per pass (kway.hip) from 4 Mi pairs on, 2 = always, 0 = the tree of 2-way passes
    int tile_sort = 1;         // sorts of keys that do not repeat: LSD passes over the top bits, then tiles sorted to the end in LDS (tilesort.hip)
    int dedupe_bits = 0;       // tests: > 0 = the block dedupe with this many block bits whatever the input's size (pipeline.hip)
    int strand_blocks = 1;     // zk_kmerize, block dedupe at odd K: both strands rebuilt block by block (strand_blocks.hip); 0 = mirror sort + merge-path union;
                               // 2 = block by block from sorted dedupe blocks (the route before the unsorted dedupe); 3 = tests: as 1, declined blocks go to the merge-path union;
                               // 4 = as 1, the mirror words written by strand_mirror_kernel instead of the dedupe (the route before the fused form);
                               // 5 = tests: as 1, room for 1024 mirror words only (the dedupe runs out of it: strand_mirror_kernel after all)
    int stream_ranges = 0;     // ... ranges the stream is cut into (0 = one per CU for variant 1, two for 2 and 3; tests use a few so that a range has many tiles)

    // workspace arena: a bump allocator reset at the start of every API call
    char* arena = nullptr;
    uint64_t arena_size = 0;
    uint64_t arena_off = 0;

    // second, grow-only region for buffers whose size is known only mid-call (the mirror step of
    // zk_kmerize): keeps the arena from having to be sized for the worst case
    char* aux = nullptr;
    uint64_t aux_size = 0;

    // decoupled look-back state (persistent: cleared once per 31 launches, see common.hpp)
    u64* status = nullptr;
    uint64_t status_words = 0;
    unsigned short* part16 = nullptr;   // radix sort: per-tile digit counts, 16 bits each (radix_sort.hip)
    uint64_t part16_words = 0;
    u32 epoch = 0;
    u32* d_ticket = nullptr;   // monotonically increasing tile ticket
    u32* d_xticket = nullptr;  // radix sort pipeline: one tile counter per XCD, 128 bytes apart (zeroed per launch)
    int num_xcd = 1;           // XCDs seen by a probe launch at zk_create (8 on MI355X in SPX mode)
    int xcd_group = 0;         // consecutive tiles an XCD takes at a time (zk_tune; 0 = one global tile order, the default)
    u32 ticket_base = 0;

    u32* d_err = nullptr;      // device error word
    zk_scalars* d_scalars = nullptr;  // small results of the kernels, on the device (kernels get pointers to its fields)
    zk_scalars* h_scalars = nullptr;  // pinned mirror: fetch() fills a field, stream_sync() makes it readable

    std::string last_error;
    u64* dbg = nullptr;        // diagnostic stamp buffer (zk_debug_buffer), normally null

    // multi-GPU: one RCCL communicator per context (comm.hip); world 1 / rank 0 until zk_comm_init
    void* comm = nullptr;
    int comm_world = 1, comm_rank = 0;
    uint64_t comm_chunk_bytes = 0;      // bytes per message and round of zk_all_to_all_v (0 = 256 MiB; zk_tune, tests)
    int comm_self_loop = 0;             // tests: the piece a rank keeps travels through ncclSend / ncclRecv to itself as well, and one rank
                                        // all-reduces through ncclAllReduce (the RCCL calls of comm.hip on a box with one GPU)

    void* ring = nullptr;               // page-locked staging ring + copy stream of the file <-> device paths (ingest.hip)
    void* row_stage = nullptr;          // page-locked block of zk_spectrum_sums_row: descriptors up, results down (spectrum.hip; made on first use)

    // optional per-launch timing with HIP events on this stream (zk_profile_*)
    struct ProfRec { int tag; uint64_t bytes; hipEvent_t a, b; };
    bool profile = false;
    std::vector<ProfRec> prof;
};

namespace zk {

int fail(zk_ctx* c, int code, const char* fmt, ...);
int no_room(zk_ctx* c, const char* entry, const char* noun, uint64_t needed, uint64_t cap);   // ZK_ENOSPC, "<entry>: <needed> <noun>, room for <cap>"
// HIP's current device is per host thread and other code in the process (torch.cuda.set_device, another ctx) may have
// changed it: every C-ABI entry makes the context's device current before it allocates or launches.
static inline void enter(zk_ctx* c) {
    int d = -1;
    if (c && (hipGetDevice(&d) != hipSuccess || d != c->device)) (void)hipSetDevice(c->device);
}
#define ZK_HIP(c, call)                                                                         \
    do {                                                                                        \
        hipError_t e__ = (call);                                                                \
        if (e__ != hipSuccess)                                                                  \
            return zk::fail((c), ZK_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)
// the argument check every C-ABI entry starts with
#define ZK_ARGS(c, cond) do { if (!(c)) return ZK_EINVAL; zk::enter(c); if (!(cond)) return zk::fail((c), ZK_EINVAL, "bad argument: %s", #cond); } while (0)
#define ZK_TRY(expr)             \
    do {                         \
        int r__ = (expr);        \
        if (r__ != ZK_OK) return r__; \
    } while (0)

// arena
void arena_reset(zk_ctx* c);
int arena_alloc(zk_ctx* c, uint64_t bytes, void** p);   // 256-byte aligned; grows the arena when idle
int arena_require(zk_ctx* c, uint64_t want, uint64_t must);
int aux_require(zk_ctx* c, uint64_t bytes, char** p);   // grows (free + malloc) when too small
// look-back state for one launch that needs `words` status words and `tiles` tickets
int lookback_begin(zk_ctx* c, uint64_t words, uint32_t tiles, u32* epoch, u32* ticket_base);
// zeroed 16-bit words for one sort pass (grow-only buffer, cleared on the stream)
int part16_begin(zk_ctx* c, uint64_t words, unsigned short** out);
// read and clear the device error word (after a stream sync); maps it to a ZK_E* code
int check_device_error(zk_ctx* c);

// per-launch timing: bracket a launch with prof_begin / prof_end (no-ops unless enabled)
void prof_begin(zk_ctx* c, int tag, uint64_t algorithmic_bytes);
void prof_end(zk_ctx* c);
void prof_add_bytes(zk_ctx* c, int tag, uint64_t bytes);   // to the tag's last record: bytes written that only the launch's result tells

// Reading small results back.  fetch_span queues the copy of `bytes` device bytes into the pinned block, starting at the field
// h_first of *c->h_scalars: from that field's own device copy, or from `from` (arena memory) when h_first is a pure landing.
// The host may read the field after stream_sync (or check_device_error, which synchronises too).
int fetch_span(zk_ctx* c, void* h_first, size_t bytes, const void* from = nullptr);
template <class T> static inline int fetch(zk_ctx* c, T* h_field, const void* from = nullptr) { return fetch_span(c, h_field, sizeof(T), from); }
int stream_sync(zk_ctx* c);

static inline uint64_t div_up(uint64_t a, uint64_t b) { return (a + b - 1) / b; }
// a grid of `blocks` workgroups, at most per_cu of them for every CU (the kernels stride over what is left)
static inline u32 grid_cap(const zk_ctx* c, uint64_t blocks, int per_cu) {
    const uint64_t mx = (uint64_t)c->num_cus * per_cu;
    return (u32)(blocks < mx ? blocks : mx);
}

// ---- launchers implemented in the kernel files (all asynchronous on c->stream) -------------
// radix_sort.hip
constexpr int MAX_PASSES = 8;
struct PassPlan {          // the digits of an LSD sort: pass p takes bits [shift[p], shift[p] + bits[p])
    int passes;
    int shift[MAX_PASSES];
    int bits[MAX_PASSES];
};
// the bits [lo, lo + key_bits) in digits of at most rbits, as even as they come
static inline PassPlan make_plan(int key_bits, int rbits, int lo = 0) {
    PassPlan p;
    if (key_bits < 1) key_bits = 1;
    if (key_bits > 64) key_bits = 64;
    p.passes = (key_bits + rbits - 1) / rbits;
    int base = key_bits / p.passes, rem = key_bits % p.passes, s = lo;
    for (int i = 0; i < MAX_PASSES; i++) { p.shift[i] = 0; p.bits[i] = 0; }
    for (int i = 0; i < p.passes; i++) {
        p.bits[i] = base + (i < rem ? 1 : 0);
        p.shift[i] = s;
        s += p.bits[i];
    }
    return p;
}
int sort_keys(zk_ctx* c, u64* keys, u64* alt, uint64_t n, int key_bits, u64** result);
int sort_pairs(zk_ctx* c, u64* keys, u64* alt, u32* vals, u32* valt, uint64_t n, int key_bits, u64** rk, u32** rv);
int sort_keys_upper(zk_ctx* c, u64* keys, u64* alt, uint64_t n, int key_bits, int lo_bit, u64** result, int prof_tag = ZK_PROF_PASS_PACKED);
int sort_pairs_upper(zk_ctx* c, u64* keys, u64* alt, u32* vals, u32* valt, uint64_t n, int key_bits, int lo_bit, u64** rk, u32** rv);
int sort_pairs_mirrored(zk_ctx* c, const u64* src_k, const u32* src_v, u64* keys, u64* alt, u32* vals, u32* valt, uint64_t n, int K,
                        u64** rk, u32** rv, int lo_bit = 0);
int sort_pairs_rbits(zk_ctx* c);
// sort whose first pass generates the keys from a base stream (encode_tile.hpp + radix_sort.hip)
// Ask sort_stream to look before it sorts: the histogram kernel sets aside the keys whose bits from `shift` up equal `value` (a
// few whole blocks of the block dedupe: every copy of their k-mers), and if more than max_ratio of them are distinct the sort is
// declined (return 1, nothing sorted) -- the caller then plans for an input that does not repeat its k-mers.
// want_distinct: the other way round -- the sort goes ahead if the set-aside keys are (nearly) all distinct and is declined if they repeat.
struct StreamSample { int shift; uint64_t value; double max_ratio; uint64_t seen = 0, distinct = 0; bool want_distinct = false; };
// Ask sort_stream to let the last of its two passes write the keys' low 32 bits only (the bits [32, 2K) are the ones sorted:
// lo_bit == 32): *result is then a u32 array, and `cuts` says where each block of equal sorted bits starts (see tag_cuts_kernel).
struct StreamTags { bool written = false; u64* cuts = nullptr; uint32_t blocks = 0; };
struct StreamSrc { const u8* stream; uint64_t n_bytes; int K; int mode; int lo_bit; int hi_bit = 0; StreamSample* sample = nullptr;
                   StreamTags* tags = nullptr; };   // mode: ZK_KEYS_*; sort bits [lo_bit, hi_bit) (hi_bit 0 = 2K)
int sort_stream(zk_ctx* c, const StreamSrc& src, u64* buf_a, u64* buf_b, uint64_t cap, uint64_t* n_keys,
                uint64_t acgt[4], u64** result);
int sort_rbits(zk_ctx* c);
PassPlan sort_plan_upper(zk_ctx* c, int key_bits, int lo_bit);   // the digits sort_keys_upper(_counted) takes for the bits [lo_bit, key_bits)
int sort_first_bits(zk_ctx* c, int key_bits, int lo_bit);
// digit counts of the passes to come, taken by the kernel that writes the words they will sort (no histogram pass of its own then)
constexpr int MIRROR_RBITS = 9, MIRROR_RADIX = 1 << MIRROR_RBITS;          // the default geometry's digits (radix_sort.hip asserts it)
struct MirrorHist { int passes; int shift[4]; int bits[4]; u64* raw; };          // raw: [MAX_PASSES][MIRROR_RADIX], += by the producer
// ... and the sort that takes them (dedupe_finish; default geometry only)
int sort_keys_upper_counted(zk_ctx* c, u64* keys, u64* alt, uint64_t n, int key_bits, int lo_bit, u64* counted, u64** result);
// dedupe_blocks.hip
// where dedupe2_kernel may write the mirror image of its words (the strand route, strand_blocks.hip): cap words at out, K bases a key
struct DedupeMirror { u64* out = nullptr; uint64_t cap = 0; int K = 0; };
struct DedupeResult {
    uint64_t n_out = 0;          // distinct keys
    uint32_t flags = 0;          // bit 0: a table filled up (unusable), bit 1: counts beyond the packed field exist (patched by dedupe_finish),
                                 // bit 2: the mirror words did not fit their room (m_emitted is false)
    uint32_t n_big = 0;
    u64 *cuts = nullptr, *nwords = nullptr, *incl = nullptr, *big = nullptr, *work = nullptr;
    u32* sub = nullptr;          // [chunks][64] or null: how a block's entries split on the 6 bits after the block bits
    uint32_t chunks = 0;
    int pack = 0;
    int tag_bits = 0;            // key bits below the block bits
    bool unsorted = false;       // the blocks dedupe2_kernel counted are in table order (dedupe_sort_blocks sorts them)
    // the mirror words rc(key) << pack | count of the blocks dedupe2_kernel counted: m_placed of them at m_words, densely, in no order,
    // their digit counts added to mh.raw.  The blocks it declined (retry[0 .. n_retry)) are still missing: strand_mirror_kernel's
    bool m_emitted = false;
    u64* m_words = nullptr;
    uint64_t m_cap = 0, m_placed = 0;
    MirrorHist mh = {};
    u32* retry = nullptr;
    uint32_t n_retry = 0;
};
// unsorted: dedupe2_kernel leaves its blocks in table order (the strand route sorts every block again; nobody else may read them so)
// mirror (unsorted, tags, no sample): ... and writes their mirror words there, if the passes over them are at most two
int dedupe_pass(zk_ctx* c, const u64* keys, uint64_t n, int key_bits, int b, int pack, u64* work, uint64_t cap, DedupeResult* r,
                uint64_t* n_in = nullptr, uint64_t max_chunks = 0, const u32* tags = nullptr, const u64* tag_cuts = nullptr,
                bool unsorted = false, const DedupeMirror* mirror = nullptr);
// the keys back from their tags: key = (block number << tag_bits) | tag
int expand_tags(zk_ctx* c, const u32* tags, const u64* cuts, uint32_t blocks, int tag_bits, u64* keys_out, uint64_t first_block = 0, uint64_t n_blocks = 0);
// packed_out: out_k takes the words themselves, (key << pack) | count, and out_c is not written (the caller merges them as they are)
int dedupe_finish(zk_ctx* c, const DedupeResult& r, u64* out_k, u32* out_c, u64* out_m = nullptr, int K = 0, int gbases = 0,
                  u64** mirror_hist = nullptr, int* mirror_group_bits = nullptr, bool packed_out = false);
// strand_blocks.hip
// r.unsorted: every block of at most a dedupe2_kernel table's entries sorted in place; r.unsorted is false after
int dedupe_sort_blocks(zk_ctx* c, DedupeResult& r);
// both strands of the block dedupe's counted list at odd K, block by block (keys_buf: buf_words free words)
int strand_blocks(zk_ctx* c, const DedupeResult& r, u64* keys_buf, uint64_t buf_words, int K, u64* out_k, u32* out_c, uint64_t cap,
                  uint64_t* n_out);
// collapse.hip
int collapse_pass(zk_ctx* c, const u64* keys, uint64_t n, int shift, int bits, int pack, u64* out, uint64_t cap, uint64_t* n_out,
                  uint64_t max_tiles = 0);
// stream_pass.hip: histogram + first pass over static stream ranges
struct StreamRows { u32* rows = nullptr; u64* offs = nullptr; u32 ranges = 0, radix = 0; u32* gcodes = nullptr; u16* gvalid = nullptr;
                    u32 strands = 1;             // 2 (ZK_KEYS_BOTH): rows [ranges + w] are the reverse strand of range w
                    bool wide = false; };        // the ranges are cut for the wide pass (1024 threads, 8 K-window tiles)
int stream_hist(zk_ctx* c, const u8* stream, uint64_t n_bytes, int K, int mode, const PassPlan& plan, u64* ghist, u32 gstride,
                u64* d_acgt, u64* d_n, u64* rec_info, u64* sample, u32 sample_cap, int sample_shift, u64 sample_value, u32* sample_n,
                void* image_room, uint64_t image_room_bytes, StreamRows* out);
// planes (or null): the pass writes the keys' low 32 bits (u32[n] at kout) and the next pass's digit, (key >> shift) & (2^bits - 1),
// as u16[n] at dig -- 6 bytes a key instead of 8; stream_pass1 takes them from there
struct StreamPlanes { u16* dig; int shift, bits; };
int stream_pass0(zk_ctx* c, uint64_t n_bytes, int K, int mode, int shift, int bits, const u64* ghist0, const StreamRows& rows,
                 uint64_t first_nl, bool uniform, u64* kout, uint64_t n, int variant, const StreamPlanes* planes = nullptr);
// tag_pass.hip: the second pass of the two-pass plan over pass 0's two arrays; writes the tags ordered by (d1, d0) and the blocks' starts
int stream_pass1(zk_ctx* c, const u32* tags, const u16* dig, uint64_t n, const u64* ghist0, uint32_t radix0, int bits1, u32* tout, u64* cuts);
// tilesort.hip: the lower bits of a sort, tile by tile in LDS
int tile_sort_top_bits(uint64_t n, int key_bits, int rbits);   // the top bits the LSD passes must have sorted first (0 = not worth it)
int tile_sort(zk_ctx* c, u64* keys, u32* vals, uint64_t n, int key_bits, int top, bool* declined);   // in place
// ... and run-length counted in the same kernel: the distinct keys and their counts (uniq may be keys)
int tile_sort_count(zk_ctx* c, const u64* keys, uint64_t n, int key_bits, int top, u64* uniq, u32* counts, uint64_t cap, uint64_t* n_unique,
                    bool* declined);
// select.hip
int trim(zk_ctx* c, const u64* keys, const void* cnts, int cbits, uint64_t n, u64 lo, u64 hi, u64* ok, void* oc,
         uint64_t cap, uint64_t* n_out);
int project_dedupe(zk_ctx* c, const u64* keys, uint64_t n, int shift, u64* out, uint64_t cap, uint64_t* n_out);
int subsample(zk_ctx* c, const u64* keys, uint64_t n, u64 seed, double p, u64* out, uint64_t cap, uint64_t* n_out);
int sample_pairs(zk_ctx* c, const u64* keys, const u64* cnts, uint64_t n, u64 seed, double p, u64* ok, u64* oc, uint64_t cap,
                 uint64_t* n_out);
int subsample_pairs(zk_ctx* c, u64* keys, u32* cnts, uint64_t n, u64 seed, double p, uint64_t* n_out);   // in place
int encode_list(zk_ctx* c, const u8* stream, uint64_t n_bytes, int K, int both, u64* out, uint64_t cap, uint64_t* n_out,
                uint64_t acgt[4]);
int capture_filter(zk_ctx* c, const u8* stream, uint64_t n_bytes, int K, const u64* baits, uint64_t n_baits, u8* out,
                   uint64_t* n_reads, uint64_t* n_kept);
int rle_prefix(zk_ctx* c, const u64* sorted, uint64_t n, int pshift, u64* uniq, u32* counts, uint64_t cap, uint64_t* n_main,
               u64* side_k, u32* side_c, uint64_t side_cap, uint64_t* n_side);
int sample_heads(zk_ctx* c, const u64* keys, uint64_t n, uint64_t* sampled, uint64_t* heads);   // adjacent-distinct count of a prefix
int reduce_by_key(zk_ctx* c, const u64* sorted, const u32* w, uint64_t n, u64* uniq, u32* sums, uint64_t cap, uint64_t* n_out, int pack = 0,
                  uint64_t* max_sum = nullptr);
int rle(zk_ctx* c, const u64* sorted, uint64_t n, u64* uniq, u32* counts, uint64_t cap, uint64_t* n_unique, int pack = 0,
        bool* overflow = nullptr);
int count_hist(zk_ctx* c, const void* counts, int count_bits, uint64_t n, uint64_t* vals, uint64_t* freq,
               uint64_t cap_bins, uint64_t* n_bins);
// codec.hip
int codec_decode(zk_ctx* c, const u64* d_words, uint64_t nw, int delta, u64* d_out, uint64_t cap, uint64_t* n_out);
int fastq_mask(zk_ctx* c, const u8* d_text, uint64_t n, uint32_t line_phase, u8* d_out, uint64_t* n_newlines);
int codec_encode(zk_ctx* c, const u64* d_vals, uint64_t n, int delta, u64* d_words, uint64_t cap, uint64_t* n_words);
int codec_encode_u32(zk_ctx* c, const u32* d_vals, uint64_t n, u64* d_words, uint64_t cap, uint64_t* n_words);
int scan64_inclusive(zk_ctx* c, u64* d_v, uint64_t n);   // in place, asynchronous
// v[0 .. n) -> its inclusive sums, in place; *total = the last one (0 when n == 0).  Synchronises the stream and reports a device error.
int scan_total(zk_ctx* c, u64* v, uint64_t n, uint64_t* total);
int add_u64(zk_ctx* c, u64* d_v, uint64_t n, u64 x);     // v[i] += x, asynchronous
// ingest.hip
void ring_destroy(zk_ctx* c);
// partition.hip
int hash_partition(zk_ctx* c, const u64* keys, const void* cnts, int count_bits, uint64_t n, int world, u64 seed, u64* ok, void* oc,
                   uint64_t* offsets);
int checksum_any(zk_ctx* c, const u64* keys, const void* cnts, int count_bits, uint64_t n, uint64_t sums[3]);
// kway.hip: the union-sum of 2 .. 16 sorted lists in one pass
int kway_union_sum(zk_ctx* c, int k, const u64* const* keys, const void* const* cnts, const uint64_t* ns, u64* out_k, void* out_c, int count_bits,
                   uint64_t cap, uint64_t* n_out, uint64_t acgt_w[4]);
// setops.hip
// disjoint: the caller knows that no key occurs in both lists (a canonical list and its mirror image at odd K): no tile waits for
// another; a shared key is reported (ZK_EINTERNAL), never merged wrongly in silence
int union_sum(zk_ctx* c, const u64* A, const void* cA, u64 nA, const u64* B, const void* cB, u64 nB, u64* ok, void* oc,
              int count_bits, uint64_t cap, uint64_t* n_out, uint64_t acgt_w[4], bool disjoint = false);
// 32-bit counts; the B side is ONE array of (key << pack) | count words
int union_sum_packed_b(zk_ctx* c, const u64* A, const u32* cA, u64 nA, const u64* Bp, u64 nB, int pack, u64* ok, u32* oc, uint64_t cap,
                       uint64_t* n_out, bool disjoint = false);
int union_sum_packed_ab(zk_ctx* c, const u64* Ap, u64 nA, const u64* Bp, u64 nB, int pack, u64* ok, u32* oc, uint64_t cap, uint64_t* n_out,
                        bool disjoint = false);
int column_sum(zk_ctx* c, const u64* rows, uint64_t n_rows, int cols, u64* out);   // out[c] = sum of rows[r][c]
int project(zk_ctx* c, const u64* ref, u64 n_ref, const u64* B, const u64* cB, u64 nB, u64* ok, u64* oc, uint64_t cap, uint64_t* n_out);
int intersect_count(zk_ctx* c, const u64* A, u64 nA, const u64* B, u64 nB, uint64_t abc[3]);
// the merge-path cut of two sorted lists into tiles of MERGE_TILE merged elements (ties: A first): part[t] (arena) = the A elements
// among the first t * MERGE_TILE; packb / packa > 0: that side holds (key << pack) | count words
constexpr int MERGE_TILE = 4096;
int make_partition(zk_ctx* c, const u64* A, u64 nA, const u64* B, u64 nB, u64** part, u32* tiles, int packb = 0, int packa = 0);
// spectrum.hip
int project_sum(zk_ctx* c, const u64* keys, const void* cnts, int count_bits, uint64_t n, int shift, u64* out_k, u64* out_s, uint64_t cap,
                uint64_t* n_out, uint64_t* total);
int spectrum_sums(zk_ctx* c, const u64* A, const u64* sA, u64 nA, const u64* B, const u64* sB, u64 nB, double cx, double cy, zk_spectrum* out);
int spectrum_sums_row(zk_ctx* c, const u64* A, const u64* sA, u64 nA, double cx, u32 m, const u64* const* yk, const u64* const* ys,
                      const uint64_t* ny, const double* cy, zk_spectrum* out);
// lcp_scan.hip: zk_lcp_resolve and zk_scan_place; nothing of it is called from another unit
// pileup_merge.hip: zk_pileup_merge and zk_narrow_counts; nothing of it is called from another unit
}  // namespace zk
