/*
 * zotk.h -- C-ABI of libzotk.so, the MI355X (gfx950) k-mer counting and set-algebra core that
 * sits under `zot kmerize | merge | dist | trim`.
 *
 * The reference (drtconway/zotmer, file:line relative to its root) has no FFI: its commands call
 * pure-Python functions.  Each entry point below names the reference function it stands in for;
 * INTEGRATION.md shows the ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - plain C: pointers and sizes only; no C++ or torch types cross this boundary;
 *   - every function returns ZK_OK (0) or a negative ZK_E* code; zk_last_error(ctx) has the text;
 *   - a zk_ctx is bound to one HIP device and one stream; calls on one ctx are serialised by the
 *     caller; use one ctx per GPU (and per thread);
 *   - pointers named d_* are DEVICE pointers (from zk_alloc, hipMalloc or a torch tensor's
 *     data_ptr()); pointers without the prefix are host memory;
 *   - work is queued on the ctx's stream; a function that returns a host scalar (n_out, acgt...)
 *     has synchronised the stream before returning;
 *   - k-mers are uint64, 2 bits per base, first base in the highest used bits (A0 C1 G2 T/U3),
 *     exactly basics.kmer (zotmer/library/basics.py:48-59).  1 <= K <= 32.
 *   - a "base stream" is the concatenation of the sequences of a batch, each followed by one
 *     byte that is not a base (the host parser keeps the line's '\n'); any byte outside
 *     AaCcGgTtUu ends the windows that touch it, as in basics.kmersList (basics.py:329-339).
 *     Which entries need a stream on a 16-byte boundary is said below.
 *   - ARRAYS AND THEIR ALIGNMENT.  A d_* array needs only the alignment of its element type: 8 bytes for uint64_t, 4 for
 *     uint32_t (and for `void*` counts of 32 bits), 1 for bytes.  A sub-range of a larger array -- a view at any element offset
 *     of a slab, data_ptr() + 8 * off of a torch tensor -- is a valid argument, for inputs and outputs alike, and the arrays of
 *     one call need not share a phase.  The one exception: the entries marked "16" below want their base stream or text (most
 *     read it in 16-byte units; zk_fastq_mask writes its output so too) on a 16-byte boundary; given another pointer they
 *     return ZK_EINVAL before any launch, write nothing, and the context stays usable.
 *         entry                   stream / text argument            needs     (where the code says so)
 *         zk_encode               d_stream                          16        select.hip:771
 *         zk_capture_filter       d_stream                          16        select.hip:849        (d_out: any address)
 *         zk_kmerize              d_stream                          16        radix_sort.hip:1820   (the first work of every plan)
 *         zk_stream_checksum      d_stream                          16        capi.hip:379
 *         zk_fastq_mask           d_text and d_stream               16 both   codec.hip:405
 *         zk_pack_reads           d_bases, d_stream (output)        any address
 *         zk_synth_reads          d_stream (output)                 any address
 *         zk_bait_table_build     d_stream                          any address
 *         zk_contig_spectra       d_stream                          any address
 *         zk_line_ends            d_text                            any address
 *         zk_last_newline         d_text                            any address
 *         zk_capture_hits         d_text1, d_text2                  any address
 *         zk_capture_gather       d_text, d_out                     any address
 *         zk_pulldown_hits        d_text1, d_text2                  any address
 *         zk_strand_keys          d_text                            any address
 *         zk_anchor_pileup        d_text                            any address
 *         zk_capture_kmers        d_text1, d_text2                  any address
 *         zk_format_pairs         d_out                             any address
 *         zk_contig_render        d_out                             any address
 *         zk_spike_pairs          d_text, d_heads, d_out1, d_out2   any address
 *         zk_fizzle_votes         d_text1, d_text2                  any address
 *         zk_hgvs_draw            d_text, d_pool                    any address
 *         zk_hgvs_render          d_text, d_pool, d_accs, d_names, d_out   any address
 *         zk_copy                 d_dst, d_src                      any address, any byte count
 *     An entry writes only the elements [0, result length) of its outputs and never more than [0, cap) -- nothing in front of the
 *     pointer, nothing behind the result but what the capacity convention below allows (the work space of zk_capture_hits and of
 *     zk_kmerize with ZK_KMERIZE_SUBSAMPLE is [0, cap)).  An entry does not change an input that is not also an output; the
 *     exceptions are the ones the entries state: zk_sort_count destroys d_keys, and the in-place forms (zk_sort_keys,
 *     zk_sort_pairs, zk_undelta, zk_add_u64, zk_rle with d_uniq == d_sorted, zk_can with d_out == d_kmers).
 *     tests/test_gpu_views.py pins all of this, on views at the last place before a 128-byte line among others.
 *   - THE CAPACITY CONVENTION.  An entry that produces a list takes `cap`, the number of entries each of its output arrays
 *     holds (bytes for text).  ZK_ENOSPC when the result exceeds `cap`: nothing is written at or beyond index `cap` of any
 *     output array, the count output (*n_out, *n_unique, *n_words ...) = the length needed, and the call may be repeated with
 *     room on the same context.  What lies below index `cap` is unspecified after a refusal.  A capacity equal to the length
 *     needed is enough; cap = 0 sizes the output.  The entries say where they differ (no count: zk_kmerize; a capacity that
 *     is not the result's length: zk_kmerize with ZK_KMERIZE_SUBSAMPLE, zk_capture_hits).  tests/test_gpu_capacity.py pins it.
 *
 * There is no CPU fallback: without a visible MI355X zk_create returns NULL.
 */
#ifndef ZOTK_H
#define ZOTK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZK_OK 0
#define ZK_EINVAL (-1)    /* bad argument */
#define ZK_ENOMEM (-2)    /* device memory / workspace exhausted */
#define ZK_EHIP (-3)      /* HIP runtime error */
#define ZK_ENOSPC (-4)    /* an output array is too small (capacity argument) */
#define ZK_EOVERFLOW (-5) /* a count does not fit its type (reference: array('I'), kmerize.py:373-374) */
#define ZK_EINTERNAL (-6) /* device-side failure */
#define ZK_ERANGE (-7)    /* codec64: value >= 2^60 has no code (reference: IndexError, codec64.py:33-40) */

typedef struct zk_ctx zk_ctx;

/* ---- context and buffers ------------------------------------------------------------------ */
zk_ctx* zk_create(int device, uint64_t workspace_bytes);   /* NULL when no such GPU */
void zk_destroy(zk_ctx* ctx);
const char* zk_last_error(zk_ctx* ctx);
int zk_set_stream(zk_ctx* ctx, void* hip_stream);          /* borrow a hipStream_t (NULL: own stream) */
void* zk_get_stream(zk_ctx* ctx);
int zk_sync(zk_ctx* ctx);
int zk_reserve(zk_ctx* ctx, uint64_t workspace_bytes);     /* grow the internal workspace now */
int zk_release_workspace(zk_ctx* ctx);                      /* give the internal workspace back (it regrows on demand) */
int zk_mem_info(zk_ctx* ctx, uint64_t* free_bytes, uint64_t* total_bytes);
int zk_alloc(zk_ctx* ctx, uint64_t bytes, void** d_ptr);
int zk_free(zk_ctx* ctx, void* d_ptr);
int zk_upload(zk_ctx* ctx, void* d_dst, const void* src, uint64_t bytes);
int zk_download(zk_ctx* ctx, void* dst, const void* d_src, uint64_t bytes);
int zk_copy(zk_ctx* ctx, void* d_dst, const void* d_src, uint64_t bytes);   /* device to device, async */
/* page-locked host memory: transfers from / to it run at PCIe rate and asynchronously (the ingest path reads files
 * straight into it); zk_upload_async queues the copy on the ctx's stream and returns */
int zk_host_alloc(zk_ctx* ctx, uint64_t bytes, void** ptr);
int zk_host_free(zk_ctx* ctx, void* ptr);
int zk_upload_async(zk_ctx* ctx, void* d_dst, const void* src, uint64_t bytes);

/* Tuning knobs (performance only; results never depend on them: tests/test_gpu_knobs.py holds the library to it -- zk_kmerize under a
 * covering array of every two knobs' values and under every sort geometry, every core entry under the knobs its own tests leave
 * alone -- and tests/_knob_cases.py is the table of the knobs, their defaults and the values crossed). */
#define ZK_TUNE_SORT_VARIANT 1   /* radix-sort geometry index for key arrays, see radix_sort.hip */
#define ZK_TUNE_PAIRS_VARIANT 2  /* ... for (key, payload) pairs */
#define ZK_TUNE_SHORT_SORT 3     /* zk_kmerize: 1 = sort only the top ~log2(n)+3 bits, finish in the mirror stage (default 0) */
#define ZK_TUNE_XCD_GROUP 5    /* radix-sort pipeline: runs of this many consecutive tiles go to one XCD (0 = off, the default; <= 32) */
#define ZK_TUNE_SIDE_DIV 4       /* ... side-list capacity = n / value (default 8); overflow falls back to the full sort */
#define ZK_TUNE_EARLY_COLLAPSE 7 /* zk_kmerize: count the copies of a k-mer before the sort is finished and finish it on (k-mer, count) words:
                                    1 (default) = as early as possible (block hash tables, else tile-local ranking), 3 = tile-local ranking only,
                                    2 = a run-length pass of its own once the copies are neighbours, 0 = off */
#define ZK_TUNE_PACKED_PAIRS 8   /* zk_kmerize / zk_mirror_expand: 1 (default) = (k-mer, count) pairs travel as one 64-bit word when the counts fit the bits above 2K */
#define ZK_TUNE_WIDE_TILES 9     /* radix sort: 1 (default) = array passes use 16 K-key tiles, one 1024-thread workgroup per CU; 0 = 8 K-key tiles, two of 512 */
#define ZK_TUNE_STREAM_PASS 10   /* the first sort pass of zk_kmerize / zk_sort_stream: 1 (default) = static stream ranges, one 1024-thread workgroup
                                  * per CU, whole 128-byte units written out of LDS (stream_pass.hip); 2 = the same with two 512-thread workgroups
                                  * per CU and 64-byte units; 3 = as 2, a tile's units leaving in two bursts (measurements); 0 = the look-back
                                  * pipeline.  Other values are refused */
#define ZK_TUNE_STREAM_RANGES 11 /* ... the number of ranges the stream is cut into, one workgroup each (0 = the default: one per CU for
                                  * variant 1, two for 2 and 3; <= 4096) */
#define ZK_TUNE_TAG_WORDS 12     /* zk_kmerize: 1 = the pass before the block dedupe writes 32-bit tags instead of whole keys when the key bits
                                  * below the blocks fit (K <= 25 after two passes); 2 (default) = ... and ranks the keys of a tile by LDS adds
                                  * where the tile lies inside one bucket of the pass before (nobody needs the order inside a block);
                                  * 0 = whole keys */
#define ZK_TUNE_DEDUPE_VARIANT 13 /* the block dedupe of zk_kmerize at <= 32 key bits below the blocks: 0 (default) = dedupe2_kernel, two 512-thread
                                  * workgroups per CU; 1 / 2 = one / two compare-and-swaps in flight per thread instead of four;
                                  * -1 = dedupe_kernel alone (one workgroup per CU, the table of rounds 2 and 3) */
#define ZK_TUNE_DEDUPE_LIMIT 14  /* ... dedupe2_kernel declines blocks of this many keys or more (they are counted by dedupe_kernel afterwards);
                                  * 65536 (default, the most its 16-bit counts allow); tests lower it to reach the second kernel */
#define ZK_TUNE_DEDUPE_BITS 15   /* tests: zk_kmerize takes the block dedupe with this many block bits (a whole number of 9-bit passes, e.g. 18)
                                  * whatever the size of the input, so that small oracle-checked inputs run two passes, tags and tiny blocks; 0 = by size (default) */
#define ZK_TUNE_COMM_CHUNK 6     /* zk_all_to_all_v: bytes per message and round (0 = 256 MiB, the default) */
#define ZK_TUNE_TAG_PASS 17      /* zk_kmerize, the two-pass plan with tags: 1 = pass 0 writes the keys as two arrays (low words, next digits: 6 bytes a key)
                                  * and the second pass is a count / scan / scatter over static segments that writes whole 64-byte units of tags
                                  * (tag_pass.hip); 0 (default) = whole keys and the look-back pipeline.  Same result either way; measured slower
                                  * in all (profiles/r04/tag_pass_ab.json: the second pass gains 5 ms, pass 0 loses 8.5) */
#define ZK_TUNE_KWAY 18          /* zk_merge_n: 1 (default) = inputs of 4 Mi pairs or more are union-summed up to 16 lists at a time, in one pass over the data
                                  * (kway.hip); 2 = every input (tests); 0 = always the tree of 2-way passes */
#define ZK_TUNE_TILE_SORT 19     /* sorts of keys that do not repeat (zk_sort_keys, zk_kmerize on such reads): 1 (default) = LSD passes over the top bits
                                  * only, until blocks of equal top bits are a few dozen keys, then every tile of ~6 K keys sorted to the end in LDS
                                  * (tilesort.hip); 0 = LSD passes over every bit */
#define ZK_TUNE_STRAND_BLOCKS 20  /* zk_kmerize, block dedupe with 18 block bits at odd K, both strands wanted: 1 (default) = the table is rebuilt block
                                  * by block -- the mirror words grouped by their top 18 bits in two passes, each block's two lists sorted in LDS and
                                  * written to a place known in advance (strand_blocks.hip), the dedupe leaving its blocks in table order; 0 = the
                                  * mirror words sorted on 26 bits in three passes and merged with the counted list by the merge-path union; 2 = block
                                  * by block, the dedupe sorting its blocks (the route before the unsorted dedupe, for the A / B); 3 = tests: as 1,
                                  * but blocks declined by the union go straight to the last resort (the counted list sorted and copied densely,
                                  * the merge-path union); 4 = as 1, but the mirror words are written by a kernel of their own that reads the counted
                                  * list back, not by the dedupe beside its words (the route before that, for the A / B); 5 = tests: as 1, with room
                                  * for 1024 mirror words only, so that the dedupe runs out of it and the kernel of 4 takes over */
#define ZK_TUNE_COMM_SELF_LOOP 16 /* tests: 1 = the piece a rank keeps goes through grouped ncclSend / ncclRecv to itself, in the same rounds as
                                  * the other pieces (instead of a device copy), and zk_allreduce_u64 calls ncclAllReduce with one rank too:
                                  * the RCCL data path of zk_comm_* executed on a box with one GPU; 0 (default) */
int zk_tune(zk_ctx* ctx, int what, int value);

/* Per-launch timing with HIP events recorded on the ctx's own stream (what bench.py's roofline
 * figure is computed from).  Tags name the kernels. */
#define ZK_PROF_HIST_STREAM 1   /* digit histogram straight from the base stream */
#define ZK_PROF_HIST_ARRAY 2
#define ZK_PROF_PASS_STREAM 3   /* radix pass 0: encode in LDS + scatter            (8 B written per key) */
#define ZK_PROF_PASS_KEYS 4     /* radix pass over a key array                      (16 B per key)        */
#define ZK_PROF_PASS_PAIRS 5    /* radix pass over (key, u32) pairs                 (24 B per key)        */
#define ZK_PROF_RLE 6
#define ZK_PROF_UNION 7
#define ZK_PROF_SELECT 8
#define ZK_PROF_MIRROR 9
#define ZK_PROF_INTERSECT 10
#define ZK_PROF_COUNT_HIST 11
#define ZK_PROF_PASS_PACKED 12  /* radix pass of the key kernel over a collapsed list of (k-mer << s | count) words (16 B per word) */
#define ZK_PROF_SAMPLE 13       /* the look before the sort: the few set-aside blocks, sorted and counted (tiny launches) */
#define ZK_PROF_TILE_SORT 14    /* the lower bits of a sort finished tile by tile in LDS (tilesort.hip: 16 B per key, 24 per pair, once) */
#define ZK_PROF_CAPTURE_HITS 15 /* zk_capture_hits: the window lookup, one wave per read (capture.hip) */
#define ZK_PROF_PROJECT_SUM 16  /* zk_project_sum: the count pass (8 B read per entry) and the write pass (8 + count bytes read per entry,
                                   16 B written per distinct prefix), one record each (spectrum.hip) */
#define ZK_PROF_SPECTRUM 17     /* zk_spectrum_sums: the one pass over both lists (16 B read per entry) */
#define ZK_PROF_STRAND_KEYS 18  /* zk_strand_keys: the window pass, one wave per read (strand_bias.hip; bytes = the keys written) */
#define ZK_PROF_STRAND_PAIRS 19 /* zk_strand_pairs: the count pass (8 B read per entry) and the write pass (8 + count bytes read per
                                   entry, 16 B written per line), one record each */
#define ZK_PROF_FORMAT_PAIRS 20 /* zk_format_pairs: the length pass (16 B read, 8 written per pair) and the write pass (24 B read per
                                   pair + the text), one record each */
#define ZK_PROF_PROBE_SCAN 21   /* zk_probe_scan: the one pass over the set (8 B read per entry, whatever the number of windows) */
#define ZK_PROF_BAIT_TALLY 22   /* zk_bait_tally: the one pass over the set (8 B read per entry; the adds depend on the hits) */
#define ZK_PROF_VARS_SCAN 23    /* zk_vars_scan: the one pass over both lists (8 + count bytes read per entry) */
#define ZK_PROF_LINKS 24        /* zk_debruijn_links: the successor kernel (8 B read, 4 written per k-mer; the check and the directory are not in it) */
#define ZK_PROF_LINKS_RC 25     /* zk_debruijn_links: the reverse-complement ranks, a launch of their own (8 B read, 4 written per k-mer) */
#define ZK_PROF_CONTIG_RENDER 26 /* zk_contig_render: the length pass (4 B per node, 16 per contig) and the write pass (12 B read per node + the text) */
#define ZK_PROF_PILEUP 27       /* zk_anchor_pileup: the lookup-and-emit kernel, one wave per read (pileup.hip; bytes = the text read + 12 B per pair
                                   written; the check of the long lines is not in it) */
#define ZK_PROF_PILEUP_CUT 28   /* zk_pileup_count: the gather (12 B read, 8 written per pair) and the cut (12 B read per pair, 16 B written per
                                   distinct pair), one record each; the two sorts are ZK_PROF_PASS_PAIRS / ZK_PROF_TILE_SORT records */
#define ZK_PROF_PULLDOWN_TALLY 29 /* zk_pulldown_hits: the tally (8 B read per distinct pair, one add each) and the histogram (5 B read per
                                   read), one record each; the lookup before them is a ZK_PROF_CAPTURE_HITS record */
#define ZK_PROF_CAPTURE_KMERS 30 /* zk_capture_kmers: the emit kernel, one wave per (bait, read) pair (hgvs_find.hip; bytes = 12 B written per entry);
                                   the count passes before it are not in it */
#define ZK_PROF_PATH_SCAN 31    /* zk_path_scan: the count pass and the emit pass over the entries (16 B read per entry each, 8 B written per
                                   match), one record each */
#define ZK_PROF_LCP_RESOLVE 32  /* zk_lcp_resolve: every launch of the call as one record (lcp_scan.hip; bytes = 48 per index k-mer + 12 per
                                   k-mer and doubling round; the searches in the sample are not in the figure) */
#define ZK_PROF_SCAN_PLACE 33   /* zk_scan_place: the offer pass and the gather (8 B per entry, 17 B per slot); the check before them is not in it */
#define ZK_PROF_SEQ_TALLY 34    /* zk_sequence_tally: the tile kernel (seq_tally.hip; bytes = the text read); the one-wave state kernel is not in it */
#define ZK_PROF_SPIKE_PAIRS 35  /* zk_spike_pairs: the write pass, one wave per pair (spikein.hip; bytes = the two texts written) */
#define ZK_PROF_SPIKE_SIZE 36   /* zk_spike_pairs: the size pass and the two scans behind it as one record (bytes = 16 per pair) */
#define ZK_PROF_KSNP_FLANK 37   /* zk_ksnp_flank: the search pass (ksnp.hip; 8 B read per k-mer + one ballot word per 64 written; the
                                   directory and the compaction are not in it) */
#define ZK_PROF_KSNP_PAIRS 38   /* zk_ksnp_components: the pair kernels, one record per size class that occurs (the first carries the
                                   bytes: 16 per k-mer, the key read and the parent and mask words written; the time grows with the
                                   pair tests, not with the bytes) */
#define ZK_PROF_STOP_FRAMES 39  /* zk_stop_frames: the lookup, draw and count kernel, one wave per read (stop_frames.hip; bytes = the
                                   text read + 16 B written per read; the long-line pass and the scan are not in it) */
#define ZK_PROF_STOP_EMIT 40    /* zk_stop_frames: the emit kernel (16 B read per read, 12 B written per stop + the text of the reads
                                   that have one) */
#define ZK_PROF_STOP_NEAREST 41 /* zk_stop_nearest: the one kernel (25 B per entry; the time grows with the pair tests) */
#define ZK_PROF_FIZZLE_COUNT 42 /* zk_fizzle_votes: the lookup-and-count kernel, one wave per pair (fizzle.hip; bytes = the two texts read
                                   + 16 B written per record; the scan is not in it) */
#define ZK_PROF_FIZZLE_EMIT 43  /* zk_fizzle_votes: the pass after the decision as one record, the adds of the one-class records and the
                                   emit kernel (16 B read per record, 12 B written per entry + the text of the pairs that have one) */
#define ZK_PROF_HGVS_DRAW 44    /* zk_hgvs_draw: the draw kernel and the scan behind it as one record (hgvs_gen.hip; bytes = 64 per variant) */
#define ZK_PROF_HGVS_FILL 45    /* zk_hgvs_draw: the fill kernel (104 B per variant read and written + the pool bytes) */
#define ZK_PROF_HGVS_SIZE 46    /* zk_hgvs_render: the size pass and the scan behind it as one record (bytes = 64 per row) */
#define ZK_PROF_HGVS_RENDER 47  /* zk_hgvs_render: the write pass (56 B read per row + the text written) */
#define ZK_PROF_DUP_COVER 48    /* zk_dup_join: the cover pass, one search per occurrence (dup_join.hip; bytes = 16 per occurrence + 4 written) */
#define ZK_PROF_DUP_JOIN 49     /* zk_dup_join: the count pass (16 B read per entry, 8 written) and the emit pass (... + 12 B written per row), one
                                   record each; the time grows with the searches and the pairs, not with these bytes */
#define ZK_PROF_PILEUP_MERGE 50 /* zk_pileup_merge: the partition, the count pass, the scan and the emit pass as one record per call (pileup_merge.hip;
                                   bytes = 12 per input element for the count pass, 20 per A element, 16 or 24 per B element, 20 per output element) */
int zk_debug_buffer(zk_ctx* ctx, void* d_buf);   /* diagnostic builds (-DZK_STAMPS) only; NULL turns it off */
int zk_profile(zk_ctx* ctx, int enable);   /* clears the records; enable != 0 starts recording */
int zk_profile_read(zk_ctx* ctx, int tag, uint64_t* launches, double* total_ms, uint64_t* algorithmic_bytes);

/* ---- K1/K2: encode ------------------------------------------------------------------------- */

/* reads given as bases[offs[r] .. offs[r+1]) -> base stream (d_stream holds offs[n_reads] + n_reads
 * bytes; read r starts at offs[r] + r and is followed by '\n').  For callers that hold the
 * classic (bases, offsets) layout instead of text lines. */
int zk_pack_reads(zk_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_offs, uint64_t n_reads, uint8_t* d_stream);

/* basics.kmersList(K, seq, both) over every sequence of the stream (library/basics.py:303-347,
 * called from reads.next, library/reads.py:108-117): k-mers in stream order, x then rc(x) per
 * window when both != 0.  acgt (may be NULL) = histogram of the low base of every emitted k-mer
 * (commands/kmerize.py:492-493).  d_out holds cap values; *n_out = values produced.
 * ZK_ENOSPC when they exceed cap: nothing is written at or beyond index cap (with both != 0 a window's pair is written whole or
 * not at all), *n_out = the length needed, and the call may be repeated with room; acgt is complete either way. */
int zk_encode(zk_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, int K, int both,
              uint64_t* d_out, uint64_t cap, uint64_t* n_out, uint64_t acgt[4]);

/* basics.sub(seed, p, x) as a filter (library/basics.py:252-259; commands/kmerize.py:494-509):
 * keeps x iff float(murmer(x, seed)) / float(2**61 - 1) < p, compared in doubles.
 * ZK_ENOSPC when the kept k-mers exceed cap: nothing is written at or beyond index cap of d_out, *n_out = the length needed,
 * and the call may be repeated with room. */
int zk_subsample(zk_ctx* ctx, const uint64_t* d_kmers, uint64_t n, uint64_t seed, double p,
                 uint64_t* d_out, uint64_t cap, uint64_t* n_out);

/* capture mode, `zot kmerize -C BAITS` (commands/kmerize.py:480-485,510-520): a read is kept iff one
 * of its k-mers is in the sorted bait array (both strands of the bait sequences); reads without a hit
 * are blanked ('N') in d_out, which then feeds zk_kmerize.  A read is a '\n'-terminated piece of the
 * stream.  d_out holds n_bytes. */
int zk_capture_filter(zk_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, int K, const uint64_t* d_baits, uint64_t n_baits,
                      uint8_t* d_out, uint64_t* n_reads, uint64_t* n_kept);

/* ---- read capture against a bait panel, `zot capture` (commands/capture.py) ---------------------------------------
 * A bait table: every K-mer of both strands of every bait sequence -> the ascending indices of the sequences that hold it
 * (capture.py:85-95 with basics.kmersList(K, seq, True), basics.py:303-347).  Built on the device from a base stream of the
 * bait sequences, each followed by one '\n' (record i = the piece before the (i+1)-th '\n'); 1 <= K <= 32.  Held as sorted
 * distinct keys, CSR offsets into u32 record ids, and a directory over the top key bits (about one key per bucket), so that a
 * lookup that misses costs one directory line.  The memory is the table's own until zk_bait_table_free. */
typedef struct zk_bait_table zk_bait_table;
int zk_bait_table_build(zk_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, int K, zk_bait_table** table);
int zk_bait_table_info(const zk_bait_table* table, uint64_t* n_keys, uint64_t* n_ids, uint64_t* n_records);
void zk_bait_table_free(zk_bait_table* table);

/* the positions of the '\n' bytes of d_text[0, n), ascending, into d_out (cap entries; ZK_ENOSPC with *n_lines = the count if
 * they do not fit: nothing at all is written then, and the call may be repeated with room).  The line structure file.readFastq walks (file.py:38-52): record r of a text cut at a record boundary is
 * lines 4r .. 4r+3, line i = [d_out[i-1] + 1, d_out[i]). */
int zk_line_ends(zk_ctx* ctx, const uint8_t* d_text, uint64_t n, uint64_t* d_out, uint64_t cap, uint64_t* n_lines);

/* The reads of capture.py:97-116: read r of FASTQ text (d_lines from zk_line_ends, at least 4 * n_reads of them) hits every
 * bait record whose table holds one of the forward read_K-mers of its sequence line (reads.reads(..., fwdOnly=True), whose K is
 * 25 whatever `-k` says: reads.py:38, capture.py:103; windows restart after any byte outside AaCcGgTtUu).  A k-mer matches a
 * key of equal value, whatever the two K are.  Paired reads (capture.py -p): d_text2 / d_lines2 are mate 2, the hits are the
 * union over both mates.  veto (may be NULL): a read with any window in it is not captured (the -U of pulldown.py).
 * Output: the distinct (bait, read) pairs as words bait << 32 | read, ascending (each bait's reads contiguous and in input
 * order), in d_pairs.  cap must hold the pairs BEFORE deduplication (one per bait and chunk of 64 window starts of a sequence
 * line that holds one of its k-mers), which d_pairs[0, cap) is the work space of; ZK_ENOSPC with *n_pairs = that count if it does
 * not: nothing is written at or beyond index cap, and the call may be repeated with room (that count is then enough, though
 * *n_pairs, the distinct pairs, comes back smaller). */
int zk_capture_hits(zk_ctx* ctx, const zk_bait_table* baits, const zk_bait_table* veto, int read_K, const uint8_t* d_text1,
                    const uint64_t* d_lines1, const uint8_t* d_text2, const uint64_t* d_lines2, uint64_t n_reads, uint64_t* d_pairs,
                    uint64_t cap, uint64_t* n_pairs);

/* ReadCache.add / flush (capture.py:26-69) for one batch: the records of d_pairs (from zk_capture_hits) as their four lines,
 * each stripped as str.strip() does (file.py:38-52) and followed by '\n', bait by bait, into d_out (cap bytes; ZK_ENOSPC with
 * *n_bytes = the size needed if they do not fit: no byte of d_out is written then, spans is complete, and the call may be
 * repeated with room).  spans (host, 2 * (n_baits + 1) words): spans[b] = the first pair of bait b,
 * spans[n_baits + 1 + b] = its first byte in d_out (b = n_baits: the ends).  Paired input: once per mate, with that mate's text. */
int zk_capture_gather(zk_ctx* ctx, const uint64_t* d_pairs, uint64_t n_pairs, uint32_t n_baits, const uint8_t* d_text,
                      const uint64_t* d_lines, uint64_t n_lines, uint8_t* d_out, uint64_t cap, uint64_t* spans, uint64_t* n_bytes);

/* ---- read pairs per bait with a histogram, `zot pulldown` (commands/pulldown.py) ---------------------------------------------
 * zk_capture_hits with the bookkeeping of pulldown.py:77-99 behind it.  Arguments up to n_pairs: as zk_capture_hits, with the
 * same contract for d_pairs, cap and *n_pairs (ZK_ENOSPC included).  veto (may be NULL) is the table of the -U sequences: a
 * read with a window in it is "pushed up" -- it gives no pair and counts in no row -- and it is looked at even when baits
 * has no keys.  d_hist (device, hist_cap words; hist_cap < n_records + 1 is ZK_EINVAL): d_hist[n], n = 0 .. n_records, = the reads
 * of this batch that are not vetoed and hit exactly n distinct baits; the words from n_records + 1 on are not touched.
 * *n_vetoed = the vetoed reads: sum(d_hist) + *n_vetoed == n_reads.  n_reads == 0 gives zeros.  After ZK_ENOSPC d_hist and
 * *n_vetoed are unspecified. */
int zk_pulldown_hits(zk_ctx* ctx, const zk_bait_table* baits, const zk_bait_table* veto, int read_K, const uint8_t* d_text1,
                     const uint64_t* d_lines1, const uint8_t* d_text2, const uint64_t* d_lines2, uint64_t n_reads, uint64_t* d_pairs,
                     uint64_t cap, uint64_t* n_pairs, uint64_t* d_hist, uint64_t hist_cap, uint64_t* n_vetoed);

/* ---- complete alleles of a k-mer index, `zot mlst` (commands/mlst.py, library/index.py) -----------------------------------
 * The index of library/index.py:67-125 -- S, the sorted distinct K-mers of both strands of every FASTA record; T, CSR offsets;
 * U, the ascending record numbers per k-mer -- is a bait table: zk_bait_table_build makes it from the records' base stream.
 *
 * zk_bait_table_arrays: borrowed device pointers to a table's arrays (keys[n_keys], offs[n_keys + 1], ids[n_ids]; the S, T and
 * U that index.py:117-123 writes), valid until zk_bait_table_free. */
int zk_bait_table_arrays(const zk_bait_table* table, const uint64_t** d_keys, const uint32_t** d_offs, const uint32_t** d_ids);

/* A table from arrays (copied device to device), for an index read from a file (KmerIndex.__init__, index.py:37-47).  Checked
 * ON THE DEVICE before the directory is built, so that a damaged file can never become an out-of-range add in zk_bait_tally:
 * 1 <= K <= 32, keys strictly ascending and < 4^K, offs[0] == 0, offs strictly increasing, offs[n_keys] == n_ids,
 * n_ids < 2^32 - 1, every id < n_records, ids strictly ascending within a key.  Anything else: ZK_EINVAL, a message that names
 * the first rule broken, *table untouched, nothing leaked.  n_keys == 0 (then n_ids == 0) is the empty table. */
int zk_bait_table_from_arrays(zk_ctx* ctx, int K, const uint64_t* d_keys, uint64_t n_keys, const uint32_t* d_offs,
                              const uint32_t* d_ids, uint64_t n_ids, uint64_t n_records, zk_bait_table** table);

/* index.py:91 (lens[i] = len(xs), the distinct K-mers of both strands of record i): d_sizes[r] = the number of keys that list
 * record r (n_records words, overwritten). */
int zk_bait_record_sizes(zk_ctx* ctx, const zk_bait_table* table, uint32_t* d_sizes);

/* mlst.py:45-49 (for x in xs: for j in idx[x]: cs[j] -= 1) counted upwards: d_hits[r] = the number of entries of d_kmers
 * (ascending K-mers; an entry equal to its predecessor counts once) that are keys listing record r.  n_records words,
 * overwritten.  n == 0, or a table without keys, writes zeros.  Record r is complete (mlst.py:51-54) when d_hits[r] equals its
 * zk_bait_record_sizes.  The hits are sums of integers: the same call returns the same bits.  ZK_TALLY_TILE = the entries a
 * workgroup takes per step (tests place their sizes around it). */
#define ZK_TALLY_TILE 2048
int zk_bait_tally(zk_ctx* ctx, const zk_bait_table* table, const uint64_t* d_kmers, uint64_t n, uint32_t* d_hits);

/* basics.can (library/basics.py:231-250; used by `zot vars`): per k-mer, whichever of x and rc(x) has the smaller
 * murmer(., 17) -- x on a tie.  Element-wise, asynchronous; d_out may equal d_kmers. */
int zk_can(zk_ctx* ctx, int K, const uint64_t* d_kmers, uint64_t n, uint64_t* d_out);

/* ---- strand bias of read pairs, `zot strand` (commands/strand.py, the mode without -r) ------------------------------
 * A window is one TAGGED KEY (c << 1) | (oriented != c), c = min(x, rc x), 2K + 1 bits wide: 1 <= K <= 31 (K = 32 is refused;
 * basics.rc disclaims K > 30 itself, basics.py:115-121).  Sorted, the two orientations of a k-mer are neighbours.
 *
 * zk_strand_keys: the tagged keys of every window of the sequence line of each of the first n_reads records of a FASTQ text
 * (d_lines from zk_line_ends, at least 4 * n_reads of them; windows restart after any byte outside AaCcGgTtUu, basics.kmersList,
 * basics.py:303-347).  oriented = x when reverse == 0 (mate 1: kmersList(K, fq1[1], False)), rc x otherwise (mate 2:
 * [rc(K, x) for x in kmersList(K, fq2[1], False)], strand.py:59).  Only windows with (murmer(c, seed) & (4^K - 1)) <= T are
 * kept (strand.py:136-139 with seed 17; T = int(M * p), computed by the host as Python does, strand.py:72-73).  The order of
 * the keys in d_keys is unspecified, the multiset is not.  ZK_ENOSPC with *n_keys = the count if they exceed cap. */
int zk_strand_keys(zk_ctx* ctx, const uint8_t* d_text, const uint64_t* d_lines, uint64_t n_reads, int K, int reverse, uint64_t seed,
                   uint64_t T, uint64_t* d_keys, uint64_t cap, uint64_t* n_keys);

/* The output loop of strand.py:142-155 over the ascending distinct tagged keys and their counts (count_bits 32 or 64): for each
 * k-mer x seen with x <= rc x, xc = its count, yc = the count of rc x (entry i + 1 iff it holds the same c with tag 1; 0 if
 * absent; xc itself for a palindrome, where rc x is x); d_a[j], d_b[j] = (xc, yc) if murmer(x, seed) >= murmer(rc x, seed), else
 * (yc, xc) -- one line per such k-mer, in ascending x.  A k-mer seen only as the greater of {x, rc x} (an "orphan": a tag-1
 * entry whose predecessor is not its partner) prints nothing in the reference; with ZK_STRAND_ORPHANS it is a line with xc = 0.
 * stats: n_pairs = lines written, n_orphans = orphans (printed or not), n_palindromes.  ZK_ENOSPC with the stats filled in if
 * n_pairs exceeds cap. */
#define ZK_STRAND_ORPHANS 1
typedef struct { uint64_t n_pairs, n_orphans, n_palindromes; } zk_strand_stats;
int zk_strand_pairs(zk_ctx* ctx, const uint64_t* d_keys, const void* d_counts, int count_bits, uint64_t n, int K, uint64_t seed, int flags,
                    uint64_t* d_a, uint64_t* d_b, uint64_t cap, zk_strand_stats* stats);

/* print '%d\t%d' % (ac, bc) (strand.py:155) for n pairs of unsigned 64-bit values: the lines, each ended by '\n', one after the
 * other in d_out.  ZK_ENOSPC with *n_bytes = the size needed if they exceed cap. */
int zk_format_pairs(zk_ctx* ctx, const uint64_t* d_a, const uint64_t* d_b, uint64_t n, uint8_t* d_out, uint64_t cap, uint64_t* n_bytes);

/* ---- probe presence within Hamming distance 2, `zot spoligo` (commands/spoligo.py:50-84) ----------------------------
 * findApprox(J, v, K, xs, D) asks whether the sorted set holds an entry in [y << s, (y + 1) << s), s = 2 (K - J), for y = v or for
 * one of v's substitution neighbours -- neigh(J, v, d) (spoligo.py:26-45) is the values at Hamming distance exactly d, d = 1, 2 --
 * one range search per neighbour (spoligo.py:50-67); findProbe (spoligo.py:69-84) cuts a probe longer than K into its windows of
 * K bases.  Here one pass over the set answers every window of a panel: for window w, tallies[3 * w + d] (d = 0, 1, 2) = the
 * number of entries x of d_kmers with ham(x >> 2 * (K - J_w), value_w) == d, ham as basics.ham (basics.py:123-133):
 * popcount((z | z >> 1) & 0x5555...) of the xor z, so a base that differs in both bits is one mismatch.  Distances of 3 and more
 * are not counted; findApprox(J, v, K, xs, D) is tallies[3 * w + 0] + ... + tallies[3 * w + D] > 0.
 * d_kmers: ascending distinct K-mers (the order is not used); 1 <= K <= 32, 1 <= J <= K, value < 4^J, n_windows <=
 * ZK_PROBE_MAX_WINDOWS -- anything else is ZK_EINVAL before any launch.  windows and tallies are HOST arrays (tallies:
 * 3 * n_windows words); `reserved` is ignored.  n == 0 writes zeros.  The tallies are sums of integers: the same call returns the
 * same bits.  ZK_PROBE_TILE = the entries a workgroup takes per step (tests place their sizes around it). */
#define ZK_PROBE_TILE 4096
#define ZK_PROBE_MAX_WINDOWS 1024
typedef struct { uint64_t value; int32_t J; int32_t reserved; } zk_probe_window;
int zk_probe_scan(zk_ctx* ctx, const uint64_t* d_kmers, uint64_t n, int K, const zk_probe_window* windows, uint32_t n_windows,
                  uint64_t* tallies);

/* ---- k-mer spectra per contig and per file, `zot disass` (commands/disass.py) --------------------------------------------
 * The reference counts, per FASTA record, the k-mers of basics.kmersList(K, seq, both) that pass basics.sub(seed, p, .) in a dict
 * (disass.py:91-94) and summarises the dict's values; a second dict sums the records' dicts per file (disass.py:98-100).
 * Key form: with both strands a window's key is c = min(x, rc x).  Every window emits x and rc x, so a run of n windows of c in
 * a record stands for the dict entries
 *     c a palindrome (c == rc c):   one entry of count 2n            if sub(c)
 *     otherwise:                    [sub(c)] + [sub(rc c)] entries of count n
 * With one strand (both == 0) the key is x and the run is [sub(x)] entries of count n.  sub is zk_subsample's comparison.
 *
 * zk_contig_spectra: d_stream holds the records' bases, each record followed by one '\n' (as zk_bait_table_build takes them; a
 * non-empty stream ends with '\n'); windows restart after any byte outside AaCcGgTtUu.  Output:
 *   d_words / d_freq   every record's histogram in one array: the distinct words record << 32 | count, ascending, each with the
 *                      number of dict entries of that record and count (bins of frequency 0 are dropped; a record without
 *                      entries has no word);
 *   d_keys / d_counts  the batch's counted key list: ascending distinct keys with the number of windows of each, BEFORE the
 *                      rule above (lists of several batches are union-summed, then zk_count_spectrum applies the rule once);
 *   stats              n_records = '\n' bytes, n_windows, n_keys, n_bins.
 * ZK_ENOSPC with the stats filled in (the sizes needed) if n_bins exceeds cap_bins or n_keys exceeds cap_keys; the array that
 * fits is still written.  1 <= K <= 32 and p finite, else ZK_EINVAL before any launch; a batch of 2^31 windows or more, or of
 * 2^32 records or more, is ZK_ERANGE.  All integer work: the same call returns the same bits.  ZK_CONTIG_TILE = the entries a
 * workgroup takes per step in the kernels that cut the sorted (key, record) array into runs (tests place their sizes around
 * it). */
#define ZK_CONTIG_TILE 4096
typedef struct { uint64_t n_records, n_windows, n_keys, n_bins; } zk_contig_stats;
int zk_contig_spectra(zk_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, int K, int both, uint64_t seed, double p,
                      uint64_t* d_words, uint64_t* d_freq, uint64_t cap_bins, uint64_t* d_keys, uint32_t* d_counts, uint64_t cap_keys,
                      zk_contig_stats* stats);

/* The histogram of a counted key list under the same rule: d_keys ascending distinct keys (canonical when both != 0), d_counts
 * their window counts (count_bits 32 or 64) -> the ascending (count value, number of dict entries) bins in HOST arrays of
 * cap_bins entries, with zk_hist's convention: ZK_ENOSPC with *n_bins = the number of bins (the first cap_bins are written).
 * A palindrome's doubled count must fit 64 bits (ZK_EOVERFLOW).  K and p as above. */
int zk_count_spectrum(zk_ctx* ctx, const uint64_t* d_keys, const void* d_counts, int count_bits, uint64_t n, int K, int both,
                      uint64_t seed, double p, uint64_t* vals, uint64_t* freq, uint64_t cap_bins, uint64_t* n_bins);

/* ---- bases enriched over a reference k-mer set, `zot vars -r` (commands/vars.py:85-119) -----------------------------------
 * A group is the run of entries of a list that share x >> 2 (the context: the first K - 1 bases), at most 4, one per next base
 * x & 3.  For every sample group whose context the reference has, the reference takes, per base j, p = gx[j] / gt (gx = the
 * reference group's counts, gt their sum) and v = logBinGe(p, st, sx[j]) (sx = the sample group's counts, st their sum; v = 0
 * unless 0 < p < 1), and prints the group when some v < -10.  logBinGe's first term is
 *     F(p, n, k) = logChoose(n, k) + log(p) k + log1p(-p) (n - k)        (library/stats.py:214-222)
 * and v >= F; for k <= n p the tail is at least 1/2.
 *
 * zk_vars_scan reads both lists once and returns, in ascending context order, one ROW for every sample group whose context is
 * in the reference, whose reference group has at least 2 entries and which has a CANDIDATE base j:
 *     0 < gx[j] < gt   and   sx[j] gt > st gx[j]  (exact, 128-bit products)   and   0 < p < 1 as a double   and
 *     F_dev < threshold + G
 * F_dev is F in double precision with the reference's logFac (the 25-entry table, n log n - n + log(n (1 + 4n (1 + 2n))) / 6 +
 * log(pi) / 2 from 25 up) in the reference's order of operations, and G = 2^-47 * S bounds |F_dev - F| of any conforming libm,
 * where S = k |log p| + (n - k) |log1p(-p)|, plus A(n) + A(n - k) + A(k) when 0 < k < n, A(m) = 64 below 25 and
 * m log m + m + 64 from 25 up.  Every group the reference would print at `threshold` is a row; the host
 * evaluates logBinGe on the rows only.
 *   d_ctx          the rows' contexts (x >> 2), ascending;
 *   d_row_counts   8 words per row: sx[0..3], gx[0..3] (0 where a base is absent);
 *   stats          n_groups = sample groups; n_missing = those whose context is not in the reference, first_missing = the
 *                  smallest such context (0 when there is none); n_mixed = joined groups whose reference group has >= 2
 *                  entries; n_rows.
 * Both lists: strictly ascending keys below 4^K (a precondition, not checked), counts of 32 or 64 bits (per list).  Either list
 * may be empty.  ZK_ENOSPC when n_rows exceeds cap_rows: nothing is written, the stats are complete and zk_last_error names the
 * size.  ZK_EOVERFLOW when the counts of a sample group, or of a reference group that a sample group joins, do not add up in 64
 * bits.  ZK_EINVAL before any launch for K outside 1..32, count bits other than 32 / 64 or a threshold that is not finite.
 *
 * How the lists are cut (tests place groups on the borders): the merged sequence of both lists, the reference entry first where
 * the keys are equal, is cut every ZK_VARS_TILE elements; tile t takes the reference entries [a_t, a_t+1) and the sample entries
 * [b_t, b_t+1) with a_t + b_t = t * ZK_VARS_TILE, a_t = the reference entries among the first t * ZK_VARS_TILE merged elements.
 * A tile sees 4 reference entries before and 3 after its slice, 1 sample entry before and 3 after; a sample group belongs to the
 * tile that holds its first entry. */
#define ZK_VARS_TILE 4096
typedef struct { uint64_t n_groups, n_missing, first_missing, n_mixed, n_rows; } zk_vars_stats;
int zk_vars_scan(zk_ctx* ctx, const uint64_t* d_ref_keys, const void* d_ref_counts, int ref_count_bits, uint64_t n_ref,
                 const uint64_t* d_sam_keys, const void* d_sam_counts, int sam_count_bits, uint64_t n_sam, int K, double threshold,
                 uint64_t* d_ctx, uint64_t* d_row_counts, uint64_t cap_rows, zk_vars_stats* stats);

/* ---- zot contigs (commands/contigs.py): the non-branching paths of a k-mer set's de Bruijn graph ----------------------------
 *
 * The reference walks the ascending k-mer array S (n entries, m = 4^K - 1) from every index not yet seen: from x it goes to the
 * only entry of S in [y0, y0 + 3], y0 = (x << 2) & m, while there is exactly one and it is not seen, and marks, for every node
 * after the first, the index rank(rc(K, x)) = the number of entries below the reverse complement as seen too.  The two searches
 * per k-mer are zk_debruijn_links (device), the ordered walk is zk_contig_walk (host: it depends on its order, DESIGN.md section
 * 6i), the text is zk_contig_render (device).
 *
 * zk_debruijn_links:
 *   d_next[i] = the index of the only entry in [y0, y0 | 3] when there is exactly one, else ZK_NO_LINK (none, or 2 to 4);
 *   d_rc[i]   = the number of entries < rc(K, d_kmers[i]): 0 .. n (n only when the set is not closed under rc).
 * d_kmers strictly ascending and below 4^K, 1 <= K <= 32, n < 2^32 - 1: anything else is ZK_EINVAL (checked on the device before
 * anything is written: the outputs stay as they were).  n = 0 writes nothing.  The same call returns the same bits.
 * How the set is cut (tests place sizes around it): workgroup t takes the entries [t * ZK_LINKS_TILE, (t + 1) * ZK_LINKS_TILE).
 * Within one first base y0 ascends with x, so the successors of a tile lie in at most 4 ascending windows of S, which are staged
 * in LDS; a tile whose windows hold more than 5 * ZK_LINKS_TILE entries searches them in place instead. */
#define ZK_NO_LINK 0xFFFFFFFFu
#define ZK_LINKS_TILE 1024
int zk_debruijn_links(zk_ctx* ctx, const uint64_t* d_kmers, uint64_t n, int K, uint32_t* d_next, uint32_t* d_rc);
/* The walk, on HOST arrays (no zk_ctx, no device call).  For i = 0 .. n - 1 ascending, unless seen[i]: path = [i], seen[i] = 1;
 * while j = next[cur] is a link and j is not seen: append j, seen[j] = 1, seen[rc[j]] = 1 (dropped when rc[j] == n: the set is not
 * closed under rc), cur = j.  A path is kept iff len + K - 1 >= min_len; the marks of a path that is not kept stay.  Kept paths
 * are appended to nodes in start order: contig c is nodes[offs[c], offs[c + 1]), its start index nodes[offs[c]]; offs takes
 * cap_contigs + 1 entries.  ZK_ENOSPC with both counts filled in (the sizes needed) when cap_nodes or cap_contigs is too small;
 * what the arrays hold is not specified then.  ZK_EINVAL for a next[i] that is neither below
 * n nor ZK_NO_LINK, an rc[i] above n (found as the walk reads them: nothing is indexed out of range), K outside 1..32,
 * n >= 2^32 - 1 or a null array. */
int zk_contig_walk(const uint32_t* next, const uint32_t* rc, uint64_t n, int K, uint64_t min_len, uint32_t* nodes, uint64_t cap_nodes,
                   uint64_t* offs, uint64_t cap_contigs, uint64_t* n_nodes, uint64_t* n_contigs);
/* ">contig_<start>\n<the K bases of the first node><the last base of every later node>\n" for every contig, in order, letters
 * ACGT, into d_out.  d_nodes (u32[n_nodes], every entry < n) and d_offs (u64[n_contigs + 1], ascending from 0 to n_nodes, no empty
 * contig) are device copies of what zk_contig_walk left; both are checked on the device (ZK_EINVAL, nothing written).
 * ZK_ENOSPC with *n_bytes = the size needed if it exceeds cap.  n_contigs = 0 writes nothing.  The body is written one byte per
 * thread: the work of a thread does not grow with a contig's length. */
int zk_contig_render(zk_ctx* ctx, const uint64_t* d_kmers, uint64_t n, int K, const uint32_t* d_nodes, uint64_t n_nodes,
                     const uint64_t* d_offs, uint64_t n_contigs, uint8_t* d_out, uint64_t cap, uint64_t* n_bytes);

/* ---- reads placed on reference zones, `zot alu-finder` (commands/alu-finder.py:309-322, hits: 116-147) -----------------------
 * The reference keeps refIdx[x] = [(zone, position), ...] for every K-mer of its zones, and per read pair runs `hits` on four
 * lists of (k-mer, position): both orientations (basics.kmersWithPosLists, basics.py:490-533) of both mates.  `hits` collects the
 * distinct diagonals (zone, q - p) over all windows (x, p) of the list and all (zone, q) in refIdx[x], then adds EVERY window of
 * the list, matching or not, once per diagonal: acc[zone][r + p][x] += 1.
 *
 * Here the index is a bait table whose ids are ANCHORS (zk_bait_table_from_arrays: ascending and distinct per key).  The host
 * lays the zones out on one u32 axis, one after another with at least 2 * pad free coordinates between them and pad before the
 * first, so that anchor + (p' - p) names one (zone, position) for any two window positions p, p' of a line of at most pad
 * bytes.
 *
 * zk_anchor_pileup: for each of the first n_reads records of a FASTQ text (d_lines from zk_line_ends, at least 4 * n_reads of
 * them) the sequence line is stripped as str.strip() does (file.py:46; L bytes are left) and cut into its windows (x_j, j),
 * j = the 0-based start; windows restart after any byte outside AaCcGgTtUu.  Orientation 0 is the list (x_j, p_j = j),
 * orientation 1 the list (rc x_j, p_j = L - j - K).  Per orientation, D = {a - p_i : a in anchors(x_i)} (distinct), and the
 * output is the multiset {(d + p_j, x_j) : d in D, j a window} over both orientations of every read: coordinates in d_coords,
 * k-mers in d_kmers, |D| * windows pairs per read and orientation, in no specified order (zk_pileup_count sorts them).  One
 * call takes one mate.
 *   - 1 <= K <= 32 and K equal to the table's, else ZK_EINVAL before any launch.
 *   - A line longer than pad with a hit (in either orientation) is ZK_ERANGE, found by a pass of its own before anything is
 *     written: its coordinates could name another zone.  A batch of 2^32 pairs or more is ZK_ERANGE.
 *   - The capacity convention: ZK_ENOSPC with *n_out = the pairs needed when they exceed cap, nothing written at or beyond
 *     cap, repeatable with room.
 *   - Exact for any number of diagonals: a wave keeps up to ZK_PILEUP_DIAGS diagonals of a read's orientation in registers;
 *     a list with more is done again by a path without that bound (a diagonal belongs to the first window that gives it,
 *     decided by looking its earlier windows up again), tests straddle the bound.
 *   - An empty table, n_reads = 0, lines shorter than K: nothing is emitted.  All integer work. */
#define ZK_PILEUP_DIAGS 256
int zk_anchor_pileup(zk_ctx* ctx, const zk_bait_table* anchors, const uint8_t* d_text, const uint64_t* d_lines, uint64_t n_reads, int K,
                     uint32_t pad, uint32_t* d_coords, uint64_t* d_kmers, uint64_t cap, uint64_t* n_out);

/* The counted pile-up: the distinct (coordinate, k-mer) pairs of d_coords / d_kmers[0, n) (inputs, left as they are; n < 2^32;
 * k-mers below 4^K), ascending by coordinate and then by k-mer, in d_oc / d_ok with the number of copies of each in d_cnt.
 * Two stable pair sorts (by k-mer carrying the coordinate, by coordinate carrying the index), a gather, and a cut of the
 * sorted pairs into runs -- head flags, a scan, run lengths -- over tiles of ZK_PILEUP_TILE pairs (tests place runs across
 * them).  The capacity convention: ZK_ENOSPC with *n_out = the distinct pairs when they exceed cap, nothing written at all.
 * All integer work: the same call returns the same bits. */
#define ZK_PILEUP_TILE 4096
int zk_pileup_count(zk_ctx* ctx, const uint32_t* d_coords, const uint64_t* d_kmers, uint64_t n, int K, uint32_t* d_oc, uint64_t* d_ok,
                    uint32_t* d_cnt, uint64_t cap, uint64_t* n_out);

/* The union of two counted lists: A = d_ac / d_ak / d_an[0, na) and B = d_bc / d_bk / d_bn[0, nb), each strictly ascending by
 * (coordinate, k-mer) as zk_pileup_count writes them or as an earlier call of this entry left them, into d_oc / d_ok / d_on:
 * ascending, every pair once, the counts of a pair that both lists hold added modulo 2^64.  A's counts are u64; B's are u32 or
 * u64 (b_count_bits), so a fresh zk_pileup_count list goes in as it is.  Inputs are left as they are; outputs may not overlap
 * inputs.  The order of the inputs is not checked: on other input the output is unspecified, but no access leaves the arrays.
 *   - b_count_bits outside {32, 64} is ZK_EINVAL before any launch.  na == 0 and nb == 0 are plain cases.
 *   - The capacity convention: ZK_ENOSPC with *n_out = the length needed when it exceeds cap, nothing written at all,
 *     repeatable with room.  Indices are 64 bits wide throughout.
 *   - A merge-path cut of the merged order (coordinate, then k-mer, both unsigned; A before B on ties) into tiles of
 *     ZK_PILEUP_MERGE_TILE merged inputs; a count pass over the keys, a scan of the tiles' counts by one workgroup, an emit
 *     pass that writes each tile's survivors as one run.  A pair of equal keys belongs to the tile that holds its A element
 *     (tests place pairs across every tile boundary).  No workgroup waits for another, no atomics: the same call returns
 *     the same bits.  Work space: 16 bytes per tile. */
#define ZK_PILEUP_MERGE_TILE 2048
int zk_pileup_merge(zk_ctx* ctx, const uint32_t* d_ac, const uint64_t* d_ak, const uint64_t* d_an, uint64_t na,
                    const uint32_t* d_bc, const uint64_t* d_bk, const void* d_bn, int b_count_bits, uint64_t nb,
                    uint32_t* d_oc, uint64_t* d_ok, uint64_t* d_on, uint64_t cap, uint64_t* n_out);

/* The counterpart of zk_widen_counts: d_out[i] = min(d_in[i], 2^32 - 1) for i < n, and *max_in = the largest d_in[i] (0 for
 * n == 0) -- a caller whose next entry takes 32-bit counts refuses the list when *max_in says that one was clipped. */
int zk_narrow_counts(zk_ctx* ctx, const uint64_t* d_in, uint32_t* d_out, uint64_t n, uint64_t* max_in);

/* ---- variants called from captured read pairs, `zot hgvs-find` (commands/hgvs-find.py:917-1131) ---------------------------------
 * The reference hands every read pair to capture.addReadPairAndKmers (library/capture.py:99-135): ns = the baits that hold a
 * k-mer of either mate, and for each n in ns every element of kmersList(K, mate, True) of both mates -- every window x and its
 * reverse complement, a palindrome therefore twice -- is added to capKmers[n].  The alleles are then recovered from capKmers[n]
 * through Hamming neighbours of an expected k-mer path (library/debruijn.py:334-409, hgvs-find.py:517-583).
 *
 * zk_capture_kmers: d_pairs[0, n_pairs) is what zk_capture_hits returns (bait << 32 | read, ascending; any 8-byte aligned
 * address).  For every pair word, every window x of the sequence line of that read in each text (d_lines* from zk_line_ends;
 * d_text2 and d_lines2 both NULL: single reads) gives the entries (bait, x) and (bait, rc x): baits in d_baits, k-mers in d_kmers.
 * Windows restart after any byte outside AaCcGgTtUu (white space around the line gives no window, so the line needs no
 * stripping).  The order of the entries is unspecified, their multiset is fixed: zk_pileup_count sorts and counts them.
 *   - 1 <= K <= 32, else ZK_EINVAL before any launch.  A pair whose read is >= n_reads is ZK_EINVAL, nothing written.
 *   - 2^32 entries or more is ZK_ERANGE (use shorter slices of the pair list), *n_out = the entries.
 *   - The capacity convention: ZK_ENOSPC with *n_out = the entries needed when they exceed cap, nothing written at all,
 *     repeatable with room.
 *   - Three passes: the reads the pairs name are marked and their valid windows counted, once per read however many baits hit
 *     it; the pairs' exclusive offsets (a scan); then one wave per pair, 64 window starts per step, the lanes of a step writing
 *     neighbouring entries (the windows of the step, then their reverse complements).  No atomics; all integer work. */
int zk_capture_kmers(zk_ctx* ctx, const uint64_t* d_pairs, uint64_t n_pairs, const uint8_t* d_text1, const uint64_t* d_lines1,
                     const uint8_t* d_text2, const uint64_t* d_lines2, uint64_t n_reads, int K, uint32_t* d_baits, uint64_t* d_kmers,
                     uint64_t cap, uint64_t* n_out);

/* fixed_path_kmers' candidate search (library/debruijn.py:364-383) and findAnchors' (hgvs-find.py:534-553), for many windows and
 * many baits in one call.  The entries d_baits / d_kmers / d_counts[0, n) are a counted list as zk_pileup_count writes it:
 * ascending by bait and then by k-mer, n < 2^32, k-mers below 4^K.  windows is a HOST array ascending by bait (a bait may have
 * many).  Entry e matches window w iff
 *     d_baits[e] == w.bait  &&  (d_kmers[e] & w.mask) == (w.value & w.mask)  &&  ham(d_kmers[e], w.value) <= w.max_ham
 *     &&  d_counts[e] >= w.min_count,
 * ham being basics.ham (basics.py:123-133, as for zk_probe_scan: a base that differs in one bit or in both is one mismatch).
 * Every match is written as (window index, entry index) into d_win / d_entry, ascending by window and then by entry.
 *   - ZK_EINVAL before any launch: K outside 1 .. 32, windows not ascending by bait, a value or a mask >= 4^K.
 *   - n == 0 or n_windows == 0: *n_out = 0.  The capacity convention: ZK_ENOSPC with *n_out = the matches when they exceed cap,
 *     nothing written at all, repeatable with room.
 *   - A workgroup takes one tile of ZK_PATH_TILE entries, a wave a quarter of it; the windows of the baits that occur in the
 *     tile are staged in LDS, ZK_PATH_CHUNK at a time.  A count pass writes the matches per (window, tile), window-major; a scan
 *     turns them into offsets; the emit pass repeats the comparison and ranks a match by ballots within its wave and by the
 *     waves' counts within its tile.  No atomics: the same call returns the same bits.  `reserved` is ignored. */
#define ZK_PATH_TILE 4096
#define ZK_PATH_CHUNK 256
typedef struct { uint64_t value, mask; uint32_t bait, max_ham, min_count, reserved; } zk_path_window;
int zk_path_scan(zk_ctx* ctx, const uint32_t* d_baits, const uint64_t* d_kmers, const uint32_t* d_counts, uint64_t n, int K,
                 const zk_path_window* windows, uint32_t n_windows, uint32_t* d_win, uint32_t* d_entry, uint64_t cap, uint64_t* n_out);

/* ---- gene alleles from a k-mer set, `zot scan` (commands/scan.py) -----------------------------------------------------------------
 * zk_lcp_resolve: d_S[0, nS) are the index's k-mers and d_X[0, nX) the sample's, both strictly ascending and below 4^K (not
 * checked).  With lcp = basics.lcp (basics.py:160-170), d_L / d_Y receive exactly what resolveAll (scan.py:95-120) leaves in
 * its L and Y, which is the result of two SEQUENTIAL loops:
 *     pass 1   x = the first element of X that is >= S[i], or the last element of X where there is none;
 *              l = lcp(K, x, S[i]);  (L[i], Y[i]) = (l, x) if l > 0, else (0, 0)
 *     pass 2   for i = 1 .. nS - 1 in this order:  x = Y[i - 1] as it stands NOW;  l = lcp(K, x, S[i]);
 *              if l > L[i]: (L[i], Y[i]) = (l, x)
 * This is NOT the better of the two neighbours of S[i] in X: a value travels on through pass 2 for as long as it beats every
 * pass-1 value it meets, a 0 left by pass 1 travels too (it matches leading A's), and a predecessor in X that no entry
 * carried is never looked at.
 *   - 1 <= K <= 32, else ZK_EINVAL (K = 32 uses all 64 bits of the xor).  nS == 0: nothing is written, ZK_OK.  nX == 0 with
 *     nS > 0: ZK_EINVAL (the reference dies there with NameError).  nS >= 2^32: ZK_ERANGE (the index's T is 32 bits wide).
 *   - How it is computed (csrc/lcp_scan.hip): pass 1 is a search per entry.  For pass 2 every j finds
 *     nb(j), the first i > j where Y1[j] no longer beats L1[i]; the entries that keep their pass-1 value are the orbit of 0
 *     under nb, marked by pointer doubling in ceil(log2 nS) rounds; every other entry takes the value of the last marked entry
 *     before it.  A workgroup takes ZK_LCP_TILE entries in every kernel of the call.
 *   - How far one thread can walk: the search for nb(j) looks at entries one by one only inside a tile, steps over a whole
 *     tile (and over 256 tiles at once) whose largest L1 is below the value's lcp with the tile's last entry, and can walk a
 *     tile to its end without stopping only where that lcp falls inside it, at most K times.  That bounds every walk by
 *     512 (K + 2) + nS / 65536 steps.  The input that drives it there is a sample of two elements around an index whose
 *     k-mers all begin with A, with pass-1 values that rise just under a falling lcp; on clustered trial lists of up to 400
 *     k-mers the longest walk was 142 steps.  Without the stepping the same input costs nS steps per entry.
 *   - No atomics, no floating point: the same call returns the same bits.  Workspace: 9 bytes per index k-mer.
 *
 * zk_scan_place: scan.py:281-304 for all records in one call.  The index lists, for S[i], the entries j in [T[i], T[i + 1]):
 * record U[j] and signed 1-based position V[j] (negative: the reverse strand).  Record n owns the slots
 * [d_rec_off[n], d_rec_off[n + 1]) of d_P / d_Q (d_rec_off: n_rec + 1 words, the exclusive prefix sum of lens[n] - K + 1), and
 * entry j names slot q = V[j] - 1 of its record, on the reverse strand -(V[j] + 1), where it offers y = Y[i], on the reverse
 * strand rc(K, Y[i]).  Per slot the winner is the entry with the largest L[i]; among equals the smallest j, which is the first
 * in the reference's (i, j) order; Q = its L, P = its y.  A slot whose best L is 0, or that no entry names, is (0, 0).
 * d_cnt[n * (K + 1) + l] = the entries of record n whose L is l.  All three outputs are written in full.
 *   - ZK_EINVAL with nothing written: K outside 1 .. 32; T not ascending from 0 to n_entries; d_rec_off not ascending from 0;
 *     an L above K; an entry whose record is >= n_rec, whose V is 0 or whose slot lies outside its record.
 *     nS, n_entries or n_rec >= 2^32: ZK_ERANGE.
 *   - A check pass; then per entry a search of its i in T, one 32-bit add and (where L > 0) one 64-bit max of
 *     (L << 32 | 2^32 - 1 - j) on a workspace word per slot; then a gather per slot.  Integer atomics only: the result does
 *     not depend on their order.  Workspace: 8 bytes per slot. */
#define ZK_LCP_TILE 256
int zk_lcp_resolve(zk_ctx* ctx, const uint64_t* d_S, uint64_t nS, const uint64_t* d_X, uint64_t nX, int K, uint8_t* d_L, uint64_t* d_Y);
int zk_scan_place(zk_ctx* ctx, const uint8_t* d_L, const uint64_t* d_Y, uint64_t nS, const uint32_t* d_T, const uint32_t* d_U,
                  const int32_t* d_V, uint64_t n_entries, const uint64_t* d_rec_off, uint64_t n_rec, int K, uint64_t* d_P, uint8_t* d_Q,
                  uint32_t* d_cnt);

/* ---- `zot hgvs-index -T`: how often the genome holds the k-mers of a bait table (seq_tally.hip) --------------------------------
 * zotmer/commands/hgvs-find.py:884-891 for one piece of one sequence: `for x in kmers(K, seq): if x in counts: counts[x] += 1`
 * with seq the stripped, joined lines of a FASTA record (file.readFasta, file.py:19-36) and kmers the forward windows
 * (basics.py:261-301).  d_text[0, n) is a piece of the record's body, cut anywhere; K is the table's.
 *   - '\n' and '\r' are skipped; any other byte outside AaCcGgTtUu ends the current run of bases.  Every window of K
 *     consecutive bases that equals key i of the table (the i-th of its ascending keys, zk_bait_table_arrays) adds 1 to
 *     d_counts[i]: d_counts is ADDED TO, so that a caller sums over pieces and files.
 *   - state (host, in / out; zeros before a record) = {the last min(run, K - 1) bases of the text so far, as a 2-bit value with
 *     the last base lowest; that length}.  A text fed in pieces gives the counts and the final state of the text fed whole.
 *   - *n_windows = the windows of K bases met (whether or not they are keys).  *first_gt = the least i with d_text[i] == '>'
 *     and (i == 0 or d_text[i - 1] is '\n' or '\r'), else n: where a next record's header would start.  Counting does not stop
 *     there; the caller decides what to feed.
 *   - n == 0 or a table without keys: d_counts untouched, the state still advanced, ZK_OK.
 *   - ZK_EINVAL: a null ctx, table, state, n_windows or first_gt; a null d_text with n > 0; a null d_counts with keys in the
 *     table; state[1] > K - 1 (bits of state[0] above 2 * state[1] are ignored).
 *   - A workgroup takes ZK_SEQTALLY_TILE text bytes; a window belongs to the tile that holds its last base.  Integer adds only:
 *     the same call returns the same bits. */
#define ZK_SEQTALLY_TILE 4096
int zk_sequence_tally(zk_ctx* ctx, const zk_bait_table* table, const uint8_t* d_text, uint64_t n, uint64_t state[2], uint64_t* d_counts,
                      uint64_t* n_windows, uint64_t* first_gt);

/* ---- `zot spikein`: simulated read pairs with variants (spikein.hip) ------------------------------------------------------------
 * zotmer/commands/spikein.py:380-394 and :267-317 with the draws of zotmer_amd/synth.py: rnd(seed, tag, index), integers only.
 *
 * zk_spike_zone_counts: draw n of [first, first + count) falls into the first zone z with d_cum[z] > rnd(seed, 16, n) % T, where
 * d_cum[0 .. n_zones) are the inclusive cumulative zone lengths (ascending) and T = d_cum[n_zones - 1]; d_counts[z] (u64) is
 * ADDED TO, so a caller may cut the draws into calls.  count == 0: nothing is touched.  ZK_EINVAL: n_zones == 0 or a null array
 * with count > 0, T == 0, count >= 2^40.  Integer adds only: the same call returns the same bits.
 *
 * zk_spike_pairs: the FASTQ records of the pairs [first, first + count), mate 1 to d_out1 and mate 2 to d_out2, in pair order.
 *   - Pair p belongs to the zone z with d_first[z] <= p < d_first[z + 1] (d_first: n_zones + 1 ascending pair numbers; a zone
 *     may be empty).  d_zones holds 12 words a zone, 6 for the wild type and then 6 for the mutant: {offset of the allele's
 *     window in d_text, first allele coordinate of the window, its length, G = the allele's length, s0, e0} (the coordinates
 *     signed).  The windows are raw bytes, any case, any character.  The header prefix `ch:st-en nm ` of zone z is
 *     d_heads[d_head_offs[z], d_head_offs[z + 1]).
 *   - The pair is a mutant when the low 32 bits of rnd(seed, 17, p) are below thr_v (thresholds are fractions of 2^32, at most
 *     2^32 = always); u = s0 + rnd(seed, 18, p) % (e0 - s0 + 1); fl = max(I + ((sd_q * z) >> 32), L + L / 2) with z the sum of
 *     the twelve 16-bit fields of rnd(seed, 19, 3 p + k), k = 0, 1, 2, less 6 * 65535, and the shift arithmetic; u - fl < 0
 *     gives u = fl, then u + fl > G gives u = G - fl; bit 0 of rnd(seed, 20, p) set is strand '-', the reverse complement of
 *     allele[u, u + fl), bases upper-cased first and only ACGT complemented.  Mate 1 is the fragment's first L bases, mate 2
 *     its last L.  Base j of mate m is replaced when the low 32 bits of r = rnd(seed, 21, (2 p + m) L + j) are below thr_e: by
 *     element (r >> 32) % 3 of the other three of ACGT, or by 'ACGT'[(r >> 32) % 4] where it is none of them.
 *   - The record: '@' prefix u ' ' fl ' ' strand ' ' errors '\n' read '\n' '+' '\n' 'I' * L '\n', the errors `j c > d` (j
 *     decimal, c the upper-cased base before) joined by ';'.
 *   - n_bytes[0], n_bytes[1] = the bytes of the two texts.  ZK_ENOSPC when either exceeds its capacity: both needed sizes are
 *     in n_bytes, nothing is written beyond [0, cap) of either output, the call may be repeated with room; cap 0 sizes.
 *   - ZK_EINVAL, with nothing written to the outputs: a pair that no zone holds, a fragment that leaves its window, a window
 *     outside d_text or outside [0, G], e0 < s0, header offsets out of order (all found by the size pass); L outside
 *     1 .. 2^20, I outside 1 .. 2^40 - 1, sd_q outside 0 .. 2^43 - 1, a threshold above 2^32, first or count >= 2^40.
 *   - count == 0 writes nothing.  No atomics: the same call returns the same bytes, and a run cut at any pair numbers into
 *     several calls returns the bytes of one call.  Workspace: 16 bytes per pair. */
int zk_spike_zone_counts(zk_ctx* ctx, const uint64_t* d_cum, uint64_t n_zones, uint64_t seed, uint64_t first, uint64_t count,
                         uint64_t* d_counts);
int zk_spike_pairs(zk_ctx* ctx, const uint8_t* d_text, uint64_t n_text, const uint64_t* d_zones, const uint64_t* d_first, uint64_t n_zones,
                   const uint8_t* d_heads, const uint64_t* d_head_offs, uint64_t n_heads, uint64_t seed, int L, int64_t I, int64_t sd_q,
                   uint64_t thr_v, uint64_t thr_e, uint64_t first, uint64_t count, uint8_t* d_out1, uint64_t cap1, uint8_t* d_out2,
                   uint64_t cap2, uint64_t n_bytes[2]);

/* ---- `zot ksnp`: the candidate-SNP k-mers of a set (ksnp.hip) -------------------------------------------------------------------
 * zotmer/commands/ksnp.py: ksnp, hamming, levenshtein.  With J = (K - 1) / 2 a k-mer x has the prefix x >> 2 (J + 1) (its top
 * K - J - 1 bases), the middle base (x >> 2 J) & 3 and a tail of J bases; a group is the k-mers of one prefix, one contiguous range
 * of the ascending list d_kmers.
 *
 * zk_ksnp_flank: x is kept iff another k-mer of the set differs from it in the middle base only.  Three searches per k-mer, no
 * atomics.
 * zk_ksnp_components: inside every group the pairs with ham(x, y) <= d (ZK_KSNP_HAMMING, basics.ham) or lev(K, x, y) <= d
 * (ZK_KSNP_LEVENSHTEIN, basics.lev, unit costs) are joined, and a connected component is kept iff its members carry at least two
 * different middle bases.  d = 0 keeps nothing; d >= K is d = K (everything of a group is joined).  Every unordered pair of a
 * group is tested once: the work is quadratic in the group size, as the reference's is, and nothing is refused for it.
 *
 * Both: d_out[0 .. *n_out) = the kept k-mers, ascending (the kept entries in input order).  d_kmers is taken to be strictly
 * ascending and below 4^K (unchecked: another input gives an unspecified list, and no access outside the arrays); it is not
 * changed.  1 <= K <= 32 and n < 2^32 - 1 (32-bit parents and directory), else ZK_EINVAL before any launch.  n = 0: ZK_OK,
 * *n_out = 0, nothing launched.  The capacity convention above: ZK_ENOSPC with *n_out = the length needed, nothing written at or
 * beyond cap.  The partition does not depend on the schedule (a component's root is its smallest member): the same call returns
 * the same list.  Workspace: a bit per k-mer and a directory of at most 256 MiB (flank), 12 bytes per k-mer (components).
 *
 * How zk_ksnp_components cuts its work (tests place group sizes around each): groups of 1 are skipped; groups of up to
 * ZK_KSNP_WAVE_GROUP members take one wave each and up to ZK_KSNP_LDS_GROUP one workgroup each, members and parents in LDS;
 * larger groups are cut into tiles of ZK_KSNP_PAIR_TILE members, one workgroup per (i-tile <= j-tile) pair, parents in global
 * memory.  The flat passes over the list work on tiles of 4096 entries. */
#define ZK_KSNP_HAMMING 0
#define ZK_KSNP_LEVENSHTEIN 1
#define ZK_KSNP_WAVE_GROUP 64
#define ZK_KSNP_LDS_GROUP 1024
#define ZK_KSNP_PAIR_TILE 256
int zk_ksnp_flank(zk_ctx* ctx, const uint64_t* d_kmers, uint64_t n, int K, uint64_t* d_out, uint64_t cap, uint64_t* n_out);
int zk_ksnp_components(zk_ctx* ctx, const uint64_t* d_kmers, uint64_t n, int K, int metric, uint64_t d, uint64_t* d_out, uint64_t cap,
                       uint64_t* n_out);

/* ---- `zot stop`: in-frame stop codons of reads placed on transcripts (stop_frames.hip; commands/stop.py:112-158) ---------------
 * The reference keeps frameAnchors[x] = {(name, q)} for every K-mer of its transcripts.  Per read (single reads) the windows
 * (x_j, p = j) are orientation 0 and (rc x_j, p = L - j - K) orientation 1, as zk_anchor_pileup cuts them (the stripped
 * sequence line, restarts after a byte outside AaCcGgTtUu).  Every pair (window (x, p) of orientation i, anchor (name, q) of x)
 * is one vote for the frame (name, o = q - p, i), with multiplicity; n = the votes.  One frame is drawn with probability
 * votes / n; every window (x, p) of the drawn orientation with (p + o + K - 3) mod 3 == 0 and x & 63 in {TAA, TAG, TGA} is
 * one stop (name, x).
 *
 * The draw: the frames ascend by (name, o, i), names as bytes; read g (its 0-based ordinal over the whole run) draws the
 * frame that holds the vote of rank r = mulhi64(rnd(seed, 24, g) & ~2047, n) = ((R >> 11) * n) >> 53 in that order, with rnd
 * the counter-based generator of zotmer_amd/synth.py -- floor(u n) for the 53-bit fraction u = (R >> 11) / 2^53, which is the
 * frame the reference's walk picks when its random.random() returns u.  Integers only.
 *
 * zk_stop_frames: `anchors` is a bait table whose ids are anchors on one u32 axis (zk_bait_table_from_arrays), the transcripts
 * laid out in ascending byte order of their names, pad free coordinates before the first and at least 2 * pad between two;
 * d_starts[0, n_tx) = the coordinate of position 0 of every transcript, ascending.  The transcript of a diagonal d = a - p is
 * then the last t with d_starts[t] <= d + pad, o = d - d_starts[t] (negative where the read overhangs the start), and a frame's
 * sort key is (d << 1) | i.  `first` = the ordinal g of the batch's first read: a run cut at any read numbers into several
 * calls gives the multiset of one call.  Output: the stops as (transcript index, k-mer) in d_tx / d_kmers, in no specified
 * order (zk_pileup_count sorts and counts them as they are).
 *   - 3 <= K <= 32 and K equal to the table's, else ZK_EINVAL before any launch.
 *   - A line longer than pad with a hit (in either orientation) is ZK_ERANGE, found by a pass of its own before anything is
 *     written.  2^32 stops or more in one batch is ZK_ERANGE.
 *   - The capacity convention: ZK_ENOSPC with *n_out = the stops when they exceed cap, nothing written at all, repeatable
 *     with room.
 *   - Exact for any number of votes.  A read whose votes share one key (the common one) needs no selection; otherwise the
 *     drawn key is the smallest k with #(votes <= k) > r, found by bisection: over the keys of the read kept in LDS when there
 *     are at most ZK_STOP_VOTES of them, and by walking the read's windows again for every probe when there are more (tests
 *     straddle the bound).
 *   - An empty table, n_tx = 0, n_reads = 0, lines shorter than K: nothing is emitted.  A count pass, a scan and an emit
 *     pass: no atomics, no float, the same call returns the same pairs in the same places.  Workspace: 16 bytes per read.
 *
 * zk_stop_nearest: d_tx / d_kmers[0, m) = the counted stops ascending by (transcript, k-mer), as zk_pileup_count leaves them;
 * d_tk[d_tk_offs[t], d_tk_offs[t + 1]) = the distinct k-mers of transcript t, ascending (n_tx + 1 offsets); d_known[0, n_known)
 * = the known stops, ascending.  Per entry i: d_dist[i] = min over y of the transcript of ham(x >> 3, y >> 3) (basics.ham; the
 * shift by three BITS is the reference's nearest3), d_near[i] = the y that gives it, the smallest among ties, d_flags[i] = 1
 * iff x is in d_known.  A transcript without k-mers (or an index >= n_tx) gives d_dist = K + 1, d_near = x, nearest3's
 * initial values.  m = 0: nothing launched.  3 <= K <= 32 else ZK_EINVAL.  m * |transcript| pair tests: a workgroup takes
 * ZK_STOP_NEAR_ENTRIES entries, one per lane, and streams the k-mers of each of their transcripts through LDS in tiles of
 * ZK_STOP_NEAR_TILE.  No atomics; the same call returns the same bits. */
#define ZK_STOP_VOTES 512
#define ZK_STOP_NEAR_ENTRIES 64
#define ZK_STOP_NEAR_TILE 1024
int zk_stop_frames(zk_ctx* ctx, const zk_bait_table* anchors, const uint32_t* d_starts, uint64_t n_tx, const uint8_t* d_text,
                   const uint64_t* d_lines, uint64_t n_reads, int K, uint32_t pad, uint64_t seed, uint64_t first, uint32_t* d_tx,
                   uint64_t* d_kmers, uint64_t cap, uint64_t* n_out);
int zk_stop_nearest(zk_ctx* ctx, const uint32_t* d_tx, const uint64_t* d_kmers, uint64_t m, int K, const uint64_t* d_tk,
                    const uint64_t* d_tk_offs, uint64_t n_tx, const uint64_t* d_known, uint64_t n_known, uint32_t* d_dist,
                    uint64_t* d_near, uint8_t* d_flags);

/* ---- `zot fizzle`: the exon-tuple classes that read pairs hit (fizzle.hip; commands/fizzle.py:354-371, 555-583) -----------------
 * The reference keeps idx[x] = the ascending tuple of the exons that hold K-mer x (forward strand only).  Per read pair it makes
 * two records -- orientation 0: the forward windows of mate 1 and the reverse-complement windows of mate 2, orientation 1: the
 * reverse complements of mate 1 and the forward windows of mate 2 -- and recHits starts from sdx = {tuple: the windows of the
 * record that have it, with multiplicity}.  The host numbers the distinct tuples as classes; this entry computes sdx.
 *
 * zk_fizzle_votes: `classes` is a bait table (zk_bait_table_from_arrays) in which every key lists exactly one id, its class;
 * n_classes = its record count.  Texts and lines as zk_capture_hits takes them (FASTQ text, zk_line_ends, at least 4 * n_reads
 * lines each); both mates are required.  Record 2 p + o is orientation o of pair p of the batch; its windows are cut as
 * zk_anchor_pileup cuts them (the stripped sequence line, restarts after a byte outside AaCcGgTtUu).
 *   - A record with hits in exactly one class c adds 1 to d_single[2 c], its hits to d_single[2 c + 1] and 1 to
 *     d_hist[min(hits, n_hist - 1)], and writes nothing else.  A record with hits in two or more classes writes one entry
 *     (record, class, hits) per class into d_rec / d_cls / d_cnt and adds nothing.  A record without hits does nothing.
 *   - The entries ascend by record and, within a record, by class: a count pass, a scan, then the writes, every record at its own
 *     offset, so the same call leaves the same bytes.  d_single (2 words a class) and d_hist (n_hist words) are ADDED TO with
 *     64-bit integer atomics: totals do not depend on the schedule, and a batch cut anywhere into several calls gives the totals
 *     of one call.  No float.
 *   - The capacity convention, and more: ZK_ENOSPC with *n_out = the entries needed when they exceed cap; then nothing is written
 *     to the three lists and nothing is added to d_single or d_hist -- the adds belong to the pass after the decision -- so the
 *     repeat with room counts once.
 *   - ZK_EINVAL before any launch: K outside 1..32, K other than the table's, n_classes other than the table's record count, a
 *     null array that would be used, n_hist == 0 with n_reads > 0.  2 * n_reads >= 2^32 is ZK_ERANGE (record numbers are u32).
 *   - An empty table, n_reads == 0, lines shorter than K: nothing is added or written, *n_out = 0.
 *   - Exact for any number of distinct classes in a record: up to ZK_FIZZLE_CLASSES they are held in LDS; a record with more is
 *     walked again once per class, the classes taken in ascending order (tests straddle the bound).
 *   - Workspace: 32 bytes per read pair (16 per record: its entries, its class, its hits). */
#define ZK_FIZZLE_CLASSES 512
int zk_fizzle_votes(zk_ctx* ctx, const zk_bait_table* classes, int K, const uint8_t* d_text1, const uint64_t* d_lines1,
                    const uint8_t* d_text2, const uint64_t* d_lines2, uint64_t n_reads, uint64_t n_classes, uint64_t* d_single,
                    uint64_t* d_hist, uint64_t n_hist, uint32_t* d_rec, uint32_t* d_cls, uint32_t* d_cnt, uint64_t cap,
                    uint64_t* n_out);

/* ---- `zot vardyger`: candidate tandem duplications, joined (dup_join.hip; commands/vardyger.py:82-133, 403-431) -------------------
 * With J = K / 2 (K even) a K-mer x is a first half x >> 2J and a second half x & (4^J - 1).  The reference's findDup + positions
 * name, per sequence, the tuples (a, b, c, d) with ab and cd K-mers of the sequence at pa and pc > pa + J, a != c, b != d, and cb and
 * cd among the K-mers counted for the sequence at least ten times.
 *
 * zk_dup_join: d_baits / d_kmers / d_counts[0, n) = the counted list as zk_pileup_count writes it, ascending by (bait, k-mer), a bait
 * being a sequence.  d_rseq / d_rkmer / d_rpos[0, m) = the occurrence table of all sequences, one entry per window, ascending by
 * (sequence, k-mer, position); d_by_second[0, m) = the indices of the same entries ascending by (sequence, second half, first half,
 * position).
 *   - d_cover[i] = the count of the entry (d_rseq[i], d_rkmer[i]), 0 if the list has none.  Written whenever m > 0, also by a call
 *     that returns ZK_ENOSPC.
 *   - A row is (e, i, j): the entry e is cb, the occurrence i is ab, the occurrence j is cd.  It exists iff d_counts[e] >= min_count,
 *     d_rseq[i] == d_rseq[j] == d_baits[e], the second half of d_rkmer[i] and the first half of d_rkmer[j] are those of d_kmers[e],
 *     the first half of d_rkmer[i] and the second half of d_rkmer[j] are not, d_cover[j] >= min_count and d_rpos[j] > d_rpos[i] + J.
 *     The rows go to d_entry / d_left / d_right ascending by e, then by the place of i in d_by_second, then by j.
 *   - The capacity convention: ZK_ENOSPC with *n_out = the rows needed when they exceed cap, nothing written to the three row
 *     arrays, repeatable with room; cap 0 sizes.
 *   - ZK_EINVAL before any launch: K odd or outside 2..32, n or m >= 2^32, a null array that would be used.  n == 0 or m == 0:
 *     *n_out = 0 (with n == 0 < m the cover is all zeros).  Lists that are not in the orders above give unspecified rows and no
 *     access outside the arrays (a value of d_by_second that is no index is read as m - 1).
 *   - An entry costs two searches when either of its runs is empty, which is nearly always.  An entry whose runs have more than
 *     ZK_DUP_WAVE_PAIRS pairs between them (low-complexity sequence) is done by a wave, 64 pairs a step, the others by a lane
 *     each (tests straddle the bound).  A cover pass, a count pass, a scan and an emit pass; no atomics, integers only: the same
 *     call returns the same bits.  Workspace: 8 bytes per entry. */
#define ZK_DUP_WAVE_PAIRS 64
int zk_dup_join(zk_ctx* ctx, const uint32_t* d_baits, const uint64_t* d_kmers, const uint32_t* d_counts, uint64_t n, const uint32_t* d_rseq,
                const uint64_t* d_rkmer, const uint32_t* d_rpos, const uint32_t* d_by_second, uint64_t m, int K, uint32_t min_count,
                uint32_t* d_cover, uint32_t* d_entry, uint32_t* d_left, uint32_t* d_right, uint64_t cap, uint64_t* n_out);

/* ---- `zot hgvs-gen`: random variants over zones, as HGVS lines (hgvs_gen.hip) ---------------------------------------------------
 * zotmer/commands/hgvs-gen.py:120-171 and :257-271, zotmer/library/hgvs.py, with the draws of zotmer_amd/synth.py: rnd(seed, tag,
 * index), integers only.  Variants are numbered v in output order; zk_spike_zone_counts spreads them over the zones.
 *
 * Shared tables.  d_zones holds 3 words a zone, {offset of its window in d_text, s, e}: the window is seq[s .. e] of the zone's
 * chromosome, both ends inclusive, raw bytes of any case.  d_first: n_zones + 1 ascending variant numbers, variant v belongs to
 * the zone z with d_first[z] <= v < d_first[z + 1].  A row is ZK_HGVS_ROW_WORDS words: {kind, zone, p, q, m, pool offset}, kind
 * one of ZK_HGVS_SUB .. ZK_HGVS_AND, p and q 0-based positions on the chromosome (q = p for sub, ins and ani), m the inserted
 * length (1 for a sub, 0 for del and dup); the pool holds the alternative base of a sub and the m bases of an ins or a delins.
 *
 * zk_hgvs_draw: the rows of the variants [first, first + count) to d_rows, their bases to d_pool (offsets from 0 in every call).
 *   - kind: the first k with the low 32 bits of rnd(seed, 25, v) below type_thr[k] (7 ascending thresholds, the last 2^32).
 *   - p = s + rnd(seed, 26, 64 v + t) % (e - s + 1) with t = 0; a sub takes the first of t = 0 .. 63 whose upper-cased base is one
 *     of ACGT and, if none is, the first such base after try 63, going round the zone once; its alternative base is element
 *     rnd(seed, 31, v) % 3 of the other three of ACGT.
 *   - geom(k, r) = 1 + the entries above the low 32 bits of r of table k; the three descending tables (of -D, -I and -U, geom_n
 *     entries each, at most ZK_HGVS_TABLE_MAX) stand one after the other in d_geom.  del: q = min(p + geom(0, rnd(seed, 27, v)),
 *     e); dup: the same with table 2; ins and ani: m = geom(1, rnd(seed, 28, v)); delins and `and`: the low 32 bits of
 *     rnd(seed, 29, v) below mix_thr give l = 1, m = 1 + geom(1, .), otherwise l = 1 + geom(0, .), m = geom(1, .), and q =
 *     min(p + l, e).  Tables that do not descend give an unspecified law and no access outside the arrays.
 *   - Base j of an insertion is bits 2 (j & 31) of rnd(seed, 30, v W + (j >> 5)) as ACGT, W = (geom_n[1] + 2 + 31) / 32.
 *   - n_out[0] = count, n_out[1] = the pool bytes.  ZK_ENOSPC when either exceeds its capacity (cap_rows in rows): both are in
 *     n_out, nothing is written beyond [0, cap) of either output, the call may be repeated with room; capacity 0 sizes.
 *   - ZK_EINVAL, with nothing written to the outputs: a variant that no zone holds, e < s, a window outside d_text, a sub that
 *     falls into a zone without a base of ACGT (all found by the first pass); a threshold above 2^32 or out of order, a last type
 *     threshold other than 2^32, a table beyond ZK_HGVS_TABLE_MAX, first or count >= 2^40.
 *   - count == 0 writes nothing.  A count pass, a scan and a fill pass, no atomics: the same call returns the same bits, and a run
 *     cut at any variant numbers returns the rows of one call (the pool offsets restart).  Workspace: 56 bytes per variant.
 *
 * zk_hgvs_render: the lines of the rows [0, n_rows), in row order, each ended by '\n'.
 *   - The spellings of str(v): `A:g.<p+1>R>B` (R the upper-cased base at p), `A:g.<p+1>_<q+1>del` / `dup` / `delinsBASES` /
 *     `delins<m>`, with `<p+1>` alone when p = q, and `A:g.<p>_<p+1>insBASES` / `ins<m>`; A = d_accs[d_acc_offs[z], d_acc_offs[z +
 *     1]).  ZK_HGVS_TABULAR puts `A \t r0 \t r1 \t size \t wt \t mut \t` in front: range() = (p, p) for the two insertions and (p, q
 *     + 1) otherwise, size() = m, 0 for del and 2 (q - p + 1) for dup, wt = seq[r0:r1] upper-cased, mut = the bases, nothing for
 *     del, wt twice for dup and m times 'N' for ani and `and`.
 *   - ZK_HGVS_HEADERS: row i is variant `first` + i of the run; where that is d_first[z], the first of its zone, and the zone's
 *     name d_names[d_name_offs[z], d_name_offs[z + 1]) is not empty, the line `# A : name` goes in front.  (The caller leaves a
 *     name empty where it repeats the name before it.)  Without the flag d_names, d_name_offs and d_first are not read.
 *   - *n_bytes = the bytes of the text.  The capacity convention: ZK_ENOSPC with *n_bytes = the bytes needed, nothing written
 *     at or beyond cap; cap 0 sizes.
 *   - ZK_EINVAL, with nothing written: a row of unknown kind or zone, not s <= p <= q <= e, q != p for a sub or an insertion, an
 *     m that its kind does not allow (or >= 2^40), a pool range outside [0, n_pool), a zone with e < s or a window outside
 *     d_text, prefix offsets out of order (all found by the size pass); flags other than the three; n_rows or first >= 2^40.
 *   - A size pass, a scan and a write pass, no atomics.  A workgroup takes 256 rows.  A line longer than ZK_HGVS_LONG_LINE bytes
 *     is written by a wave, lanes over its bases, a shorter one by a thread; a tile whose text is at most ZK_HGVS_TILE_BYTES is
 *     put together in LDS and leaves in aligned 16-byte stores, a larger one is written in place (tests straddle both bounds).
 *     ZK_HGVS_DIRECT writes every tile in place: the same bytes, kept for measurements.  Workspace: 8 bytes per row. */
#define ZK_HGVS_SUB 0
#define ZK_HGVS_DEL 1
#define ZK_HGVS_INS 2
#define ZK_HGVS_DELINS 3
#define ZK_HGVS_DUP 4
#define ZK_HGVS_ANI 5
#define ZK_HGVS_AND 6
#define ZK_HGVS_ROW_WORDS 6
#define ZK_HGVS_TABLE_MAX 65536
#define ZK_HGVS_TABULAR 1
#define ZK_HGVS_HEADERS 2
#define ZK_HGVS_DIRECT 4
#define ZK_HGVS_LONG_LINE 256
#define ZK_HGVS_TILE_BYTES 32768
int zk_hgvs_draw(zk_ctx* ctx, const uint8_t* d_text, uint64_t n_text, const uint64_t* d_zones, const uint64_t* d_first, uint64_t n_zones,
                 const uint64_t type_thr[7], const uint64_t* d_geom, const uint64_t geom_n[3], uint64_t mix_thr, uint64_t seed, uint64_t first,
                 uint64_t count, uint64_t* d_rows, uint64_t cap_rows, uint8_t* d_pool, uint64_t cap_pool, uint64_t n_out[2]);
int zk_hgvs_render(zk_ctx* ctx, const uint64_t* d_rows, uint64_t n_rows, const uint8_t* d_pool, uint64_t n_pool, const uint8_t* d_text,
                   uint64_t n_text, const uint64_t* d_zones, uint64_t n_zones, const uint8_t* d_accs, const uint64_t* d_acc_offs, uint64_t n_accs,
                   const uint8_t* d_names, const uint64_t* d_name_offs, uint64_t n_names, const uint64_t* d_first, uint64_t first, int flags,
                   uint8_t* d_out, uint64_t cap, uint64_t* n_bytes);

/* ---- K3/K4: sort and count ------------------------------------------------------------------ */

/* misc.radix_sort(key_bits, xs) (library/misc.py:400-424): ascending, in place. */
int zk_sort_keys(zk_ctx* ctx, uint64_t* d_keys, uint64_t n, int key_bits);
/* the same carrying a 32-bit payload (stable) */
int zk_sort_pairs(zk_ctx* ctx, uint64_t* d_keys, uint32_t* d_vals, uint64_t n, int key_bits);
/* the run-length half of kmerize.merge (commands/kmerize.py:41-132): distinct values of a sorted
 * array and their multiplicities.  d_uniq may equal d_sorted.
 * ZK_ENOSPC when the distinct values exceed cap: nothing is written at or beyond index cap of d_uniq or d_counts (with d_uniq ==
 * d_sorted the array still holds its input from cap on), *n_unique = the length needed, and the call may be repeated with room
 * (in place: on the input again, the entries below cap have been overwritten). */
int zk_rle(zk_ctx* ctx, const uint64_t* d_sorted, uint64_t n, uint64_t* d_uniq, uint32_t* d_counts,
           uint64_t cap, uint64_t* n_unique);
/* KmerAccumulator2.flush on an empty table (commands/kmerize.py:412-424): sort (destroys d_keys)
 * then count.  ZK_ENOSPC as zk_rle: nothing is written at or beyond index cap of d_uniq or d_counts, *n_unique = the length
 * needed, and the call may be repeated with room (on the keys again: the sort has destroyed d_keys). */
int zk_sort_count(zk_ctx* ctx, uint64_t* d_keys, uint64_t n, int key_bits,
                  uint64_t* d_uniq, uint32_t* d_counts, uint64_t cap, uint64_t* n_unique);

/* ---- the fused kmerize batch ------------------------------------------------------------------ */
#define ZK_KMERIZE_CANONICAL 0   /* default: sort one strand, mirror after counting (same result) */
#define ZK_KMERIZE_BOTH 1        /* sort both strands literally, as the reference does */
#define ZK_KMERIZE_SUBSAMPLE 2   /* -D FRAC -S SEED (commands/kmerize.py:469-478,494-509) */
#define ZK_KMERIZE_CANONICAL_ONLY 4   /* stop before the strands are rebuilt: d_kmers / d_counts get the counted CANONICAL list
                                         (c = min(x, rc x) per window, count = windows), n_unique = its length.  The multi-GPU
                                         path exchanges this half-size list and calls zk_mirror_expand on what a rank owns. */

typedef struct {
    uint64_t n_windows;     /* valid windows seen */
    uint64_t n_instances;   /* k-mers the reference would have emitted = 2 * n_windows (kmerize.py:523-525) */
    uint64_t n_unique;      /* entries written to d_kmers / d_counts */
    uint64_t n_canonical;   /* distinct canonical k-mers (0 in ZK_KMERIZE_BOTH mode), the same on every plan; with
                               ZK_KMERIZE_SUBSAMPLE counted BEFORE the subsample (n_unique is after it) */
    uint64_t acgt[4];       /* acgt[x & 3] over every instance, before any filtering (kmerize.py:492-493) */
} zk_kmerize_stats;

/* One in-memory `zot kmerize` (commands/kmerize.py:490-546 with KmerAccumulator2, :370-437) over
 * the base stream: sorted distinct k-mers of BOTH strands and their counts.
 * ZK_ENOSPC when the table exceeds cap: nothing is written at or beyond index cap of d_kmers or d_counts, and the call may be
 * repeated with room; a capacity equal to the table's length is enough on every plan.  The length needed is NOT returned:
 * stats->n_unique is 0 and the other fields are unspecified after a refusal (some plans refuse before they have merged the
 * strands); 2 * n_bytes entries always hold the table, n_bytes the canonical list.  With ZK_KMERIZE_SUBSAMPLE the subsample is
 * applied to the counted table in the caller's arrays: cap must hold the table BEFORE the subsample, n_unique is its length
 * after.  With ZK_KMERIZE_CANONICAL_ONLY cap counts the entries of the canonical list. */
int zk_kmerize(zk_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, int K, int flags, double p, uint64_t seed,
               uint64_t* d_kmers, uint32_t* d_counts, uint64_t cap, zk_kmerize_stats* stats);

/* The second half of zk_kmerize for a counted canonical list (ascending c, counts): sorted distinct k-mers of BOTH strands
 * -- (c, n) and (rc c, n) for every entry, a palindrome (c == rc c) counted n + n, as two emissions per window give
 * (commands/kmerize.py:490; library/reads.py:113-114).  zk_kmerize(flags) == zk_mirror_expand(zk_kmerize(flags |
 * ZK_KMERIZE_CANONICAL_ONLY)).
 * ZK_ENOSPC when the table (2 n entries less the palindromes) exceeds cap: nothing is written at or beyond index cap of d_kmers
 * or d_counts, *n_out = the length needed, and the call may be repeated with room.
 * ZK_EOVERFLOW when the n + n of a palindrome does not fit 32 bits (n >= 2^31; the reference's array('I') raises OverflowError
 * there): no wrapped count is handed out as a result, the contents of d_kmers / d_counts are unspecified, and the ctx stays usable. */
int zk_mirror_expand(zk_ctx* ctx, const uint64_t* d_canon_kmers, const uint32_t* d_canon_counts, uint64_t n, int K,
                     uint64_t* d_kmers, uint32_t* d_counts, uint64_t cap, uint64_t* n_out);

/* hist[c] += 1 per distinct k-mer (commands/kmerize.py:543-545; merge.py:88-92), as ascending
 * (value, frequency) pairs in HOST arrays of cap_bins entries.  count_bits is 32 or 64.  ZK_ENOSPC: more than
 * cap_bins bins; *n_bins is then the number of bins (the first cap_bins are written, nothing at or beyond index cap_bins of
 * vals or freq), so one more call sizes it; the call may be repeated with room. */
int zk_hist(zk_ctx* ctx, const void* d_counts, int count_bits, uint64_t n,
            uint64_t* vals, uint64_t* freq, uint64_t cap_bins, uint64_t* n_bins);

/* uint32 counts -> uint64 counts (kmerize keeps array('I'), merge works on Python ints) */
int zk_widen_counts(zk_ctx* ctx, const uint32_t* d_in, uint64_t* d_out, uint64_t n);

/* ---- K5/K6: union with summed counts ---------------------------------------------------------- */

/* merge.merge (commands/merge.py:26-86) and the merge half of kmerize.merge: two sorted-unique
 * (k-mer, count) lists -> one; equal k-mers add.  count_bits (32 or 64) is the element type of all
 * three count arrays.  acgt_w (may be NULL): acgt_w[x & 3] += count (merge.py:159).
 * ZK_ENOSPC when the union exceeds cap: nothing is written at or beyond index cap of d_ok or d_oc, *n_out = the length needed
 * (acgt_w is complete as well), and the call may be repeated with room. */
int zk_union_sum(zk_ctx* ctx, const uint64_t* d_xk, const void* d_xc, uint64_t nx,
                 const uint64_t* d_yk, const void* d_yc, uint64_t ny,
                 uint64_t* d_ok, void* d_oc, int count_bits, uint64_t cap, uint64_t* n_out, uint64_t acgt_w[4]);

/* mergeNinto (commands/merge.py:127-163; twin commands/kmerize.py:269-304): k sorted-unique lists
 * -> one.  d_keys / d_counts / ns are HOST arrays of k device pointers / sizes; count_bits (32 or 64)
 * is the element type of every count array.
 * ZK_ENOSPC when the union exceeds cap: nothing is written at or beyond index cap of d_ok or d_oc, *n_out = the length needed,
 * and the call may be repeated with room.  Only the last pass writes the caller's arrays; the passes before it work in the
 * context's workspace at the sizes they need. */
int zk_merge_n(zk_ctx* ctx, int k, const uint64_t* const* d_keys, const void* const* d_counts, const uint64_t* ns,
               uint64_t* d_ok, void* d_oc, int count_bits, uint64_t cap, uint64_t* n_out, uint64_t acgt_w[4]);

/* ---- K8/K9: dist ------------------------------------------------------------------------------- */

/* Measure.prep, set mode (commands/dist.py:43-49): y = x >> shift, adjacent duplicates dropped.
 * ZK_ENOSPC when the result exceeds cap: nothing is written at or beyond index cap of d_out, *n_out = the length needed, and the
 * call may be repeated with room. */
int zk_project_dedupe(zk_ctx* ctx, const uint64_t* d_kmers, uint64_t n, int shift,
                      uint64_t* d_out, uint64_t cap, uint64_t* n_out);
/* dist.split (library/dist.py:241-265): abc = (|X & Y|, |X \ Y|, |Y \ X|) of two sorted unique arrays. */
int zk_split(zk_ctx* ctx, const uint64_t* d_x, uint64_t nx, const uint64_t* d_y, uint64_t ny, uint64_t abc[3]);

/* Measure.prep, vector mode (commands/dist.py:35-41: v[x >> S] += c), without the vector: the distinct values of kmer >> shift of
 * ascending distinct k-mers, ascending, in d_keys, and the sum of the counts under each in d_sums; *total = the sum of all counts.
 * count_bits (32 or 64) is the element type of d_counts.  shift == 0 copies the k-mers and widens the counts.  The sums are
 * 64-bit: where the reference's array('I') raises OverflowError above 2^32 - 1 this goes on counting -- the one deliberate
 * difference.  The counts of a set must add up to less than 2^64.  ZK_ENOSPC with *n_out = the number of prefixes if they
 * exceed cap: nothing at all is written to d_keys or d_sums then, *total is unspecified, and the call may be repeated with room. */
int zk_project_sum(zk_ctx* ctx, const uint64_t* d_kmers, const void* d_counts, int count_bits, uint64_t n, int shift,
                   uint64_t* d_keys, uint64_t* d_sums, uint64_t cap, uint64_t* n_out, uint64_t* total);

/* What the spectrum measures of library/dist.py (the vec=True branches) need of two spectra held as zk_project_sum leaves them,
 * in one merge pass.  A key is shared when it is in both lists with non-zero sums x and y (a zero counter is an absent k-mer).
 * The sum of |x - y| over the union is cx + cy - 2 * s_min and has no field of its own. */
typedef struct {
    uint64_t n_shared;   /* shared keys */
    uint64_t s_min;      /* sum of min(x, y)                          (dist.py:37, :165) */
    uint64_t x_shared;   /* sum of x over the shared keys: decompose's yxy   (dist.py:276) */
    uint64_t y_shared;   /* sum of y over the shared keys: decompose's yyx   (dist.py:277) */
    uint64_t s_xy_lo;    /* sum of x * y, exact, as 128 bits                 (dist.py:64) */
    uint64_t s_xy_hi;
    double s_sqrt;       /* sum of sqrt(x * y)                               (dist.py:90) */
    double s_js;         /* sum of x/cx * log(2*cy*x / (cy*x + cx*y)) + y/cy * log(2*cx*y / (cx*y + cy*x)), each term computed in
                            the reference's operation order (dist.py:138-139) */
} zk_spectrum;
/* cx, cy: the two totals as doubles (they enter s_js only).  The integers are exact.  The doubles are sums of per-workgroup
 * partial sums taken in a fixed order: the same call on the same device returns the same bits.  Either list may be empty. */
int zk_spectrum_sums(zk_ctx* ctx, const uint64_t* d_xk, const uint64_t* d_xs, uint64_t nx, const uint64_t* d_yk, const uint64_t* d_ys,
                     uint64_t ny, double cx, double cy, zk_spectrum* out);

/* One row of a distance matrix: the spectrum x against m others in three launches, one read-back and one synchronise, whatever
 * m is.  d_yk, d_ys, ny and cy are HOST arrays of m entries (d_yk[j], d_ys[j]: device pointers, as zk_merge_n takes its
 * lists); out is a HOST array of m entries, and out[j] is what zk_spectrum_sums(x, y_j, cx, cy[j]) defines.  The six integers
 * are exact and equal that entry's.  The two doubles have the same terms, each computed operation by operation in the same
 * way, added in an order that is a function of (nx, ny[j]) alone: the same pair returns the same bits wherever it stands in
 * a row, whatever else the row holds and whatever the device's number of compute units -- but not necessarily the bits of
 * zk_spectrum_sums, whose order depends on its grid.  An empty x or an empty y_j gives a zero struct (its pointers are not
 * read); m = 0 does nothing.  m > ZK_SPECTRUM_ROW_MAX is ZK_EINVAL: callers cut longer rows. */
#define ZK_SPECTRUM_ROW_MAX 4096
int zk_spectrum_sums_row(zk_ctx* ctx, const uint64_t* d_xk, const uint64_t* d_xs, uint64_t nx, double cx, uint32_t m,
                         const uint64_t* const* d_yk, const uint64_t* const* d_ys, const uint64_t* ny, const double* cy,
                         zk_spectrum* out /* HOST, m entries */);

/* positions[q] = how many elements of the sorted device array are < queries[q] (HOST arrays of m
 * entries): the cut points of a value-range partition for the multi-GPU exchange. */
int zk_lower_bound(zk_ctx* ctx, const uint64_t* d_sorted, uint64_t n, const uint64_t* queries, uint32_t m, uint64_t* positions);

/* ---- next-row commands on the same kernels ---------------------------------------- */

/* project.project2 (commands/project.py:29-40): the (k-mer, count) entries of a set whose k-mer is in the
 * sorted reference set; 64-bit counts.
 * ZK_ENOSPC when the entries kept exceed cap: nothing is written at or beyond index cap of d_ok or d_oc, *n_out = the length
 * needed, and the call may be repeated with room. */
int zk_project(zk_ctx* ctx, const uint64_t* d_ref, uint64_t n_ref, const uint64_t* d_kmers, const uint64_t* d_counts, uint64_t n,
               uint64_t* d_ok, uint64_t* d_oc, uint64_t cap, uint64_t* n_out);
/* sample.sampleD (commands/sample.py:27-34): keep iff float(murmer(x, seed) & (2^40 - 1)) / float(2^40 - 1) < p.
 * ZK_ENOSPC when the entries kept exceed cap: nothing is written at or beyond index cap of d_ok or d_oc, *n_out = the length
 * needed, and the call may be repeated with room. */
int zk_sample(zk_ctx* ctx, const uint64_t* d_kmers, const uint64_t* d_counts, uint64_t n, uint64_t seed, double p,
              uint64_t* d_ok, uint64_t* d_oc, uint64_t cap, uint64_t* n_out);

/* ---- multi-GPU: partitioning and the RCCL seam ------------------------------------- */

/* Hash-range owner: owner(x) = floor(murmer(x, seed) * world / 2^64) (basics.murmer, library/basics.py:191-229).
 * Splits a sorted (k-mer, count) table into `world` pieces, each still sorted (a stable partition); piece o is
 * d_ok[offsets[o] .. offsets[o+1]).  d_counts / d_oc may be NULL (keys only); offsets is a HOST array of world + 1
 * entries; world <= 32.  The value-range owner needs no kernel: a sorted table is already partitioned, the cut
 * points come from zk_lower_bound. */
int zk_hash_partition(zk_ctx* ctx, const uint64_t* d_kmers, const void* d_counts, int count_bits, uint64_t n, int world, uint64_t seed,
                      uint64_t* d_ok, void* d_oc, uint64_t* offsets);

/* One RCCL communicator per context, one process per GPU.  The reference is single-process (no counterpart);
 * these are the entry points a host that is not PyTorch binds to drive the 8-GPU path.  Rank 0 makes the id and
 * the host carries its 128 bytes to the other ranks (file, MPI, torch.distributed store ...). */
#define ZK_COMM_ID_BYTES 128
#define ZK_REDUCE_SUM 0          /* modulo 2^64 */
#define ZK_REDUCE_MAX 1
int zk_comm_unique_id(uint8_t id[ZK_COMM_ID_BYTES]);
int zk_comm_init(zk_ctx* ctx, int world, int rank, const uint8_t id[ZK_COMM_ID_BYTES]);
int zk_comm_destroy(zk_ctx* ctx);
int zk_comm_info(zk_ctx* ctx, int* world, int* rank);          /* 1, 0 without a communicator */
/* The exchange step: elements [send_off[r], send_off[r] + send_cnt[r]) of d_send go to rank r, which receives them
 * at recv_off[me] of its d_recv (recv_cnt[r] on this rank must equal send_cnt[me] on rank r); offsets and counts are
 * HOST arrays of `world` entries in units of elem_bytes.  Grouped ncclSend / ncclRecv, one hop per peer on the xGMI
 * mesh, straight between the callers' arrays, <= 256 MiB per message and round; asynchronous on the ctx's stream. */
int zk_all_to_all_v(zk_ctx* ctx, const void* d_send, const uint64_t* send_off, const uint64_t* send_cnt, void* d_recv,
                    const uint64_t* recv_off, const uint64_t* recv_cnt, int elem_bytes);
/* The messages zk_all_to_all_v issues, as data (host only; no GPU, no RCCL needed): rank `rank` of `world`, same arguments; chunk_bytes 0 =
 * 256 MiB; self_loop as ZK_TUNE_COMM_SELF_LOOP.  ops[0 .. min(*n_ops, cap)) in issue order: recv 0 = a send of bytes [offset, offset + bytes)
 * of d_send to `peer`, 1 = a receive into those bytes of d_recv from `peer`; all the ops of one `round` form one ncclGroup.  For tests: what
 * a box with one GPU cannot execute -- the pairing of the ranks and the offsets of their pieces -- is checked on the CPU. */
typedef struct { int32_t recv; int32_t peer; uint64_t round; uint64_t offset; uint64_t bytes; } zk_comm_op;
int zk_comm_plan(int world, int rank, const uint64_t* send_off, const uint64_t* send_cnt, const uint64_t* recv_off, const uint64_t* recv_cnt,
                 int elem_bytes, uint64_t chunk_bytes, int self_loop, zk_comm_op* ops, uint64_t cap, uint64_t* n_ops);
/* in-place all-reduce of n HOST values (dist's (a, b, c), checksums, the splitter histogram); synchronises */
int zk_allreduce_u64(zk_ctx* ctx, uint64_t* vals, uint64_t n, int op);

/* ---- K10: trim ---------------------------------------------------------------------------------- */

/* trim.trim (commands/trim.py:54-62): keep (x, f) iff f >= lo and (hi == 0 or f <= hi).
 * ZK_ENOSPC when the entries kept exceed cap: nothing is written at or beyond index cap of d_ok or d_oc, *n_out = the length
 * needed, and the call may be repeated with room. */
int zk_trim(zk_ctx* ctx, const uint64_t* d_kmers, const void* d_counts, int count_bits, uint64_t n,
            uint64_t lo, uint64_t hi, uint64_t* d_ok, void* d_oc, uint64_t cap, uint64_t* n_out);

/* ---- host-side format code (CPU; no ctx, no GPU): next-row f1/f2 of SURVEY.md section 8 ------------ */

/* codec64.encode (library/codec64.py:42-120) over HOST arrays; delta != 0 first replaces ascending
 * k-mers by their differences (files.delta, library/files.py:85-98).  ZK_ERANGE when a value or delta
 * is >= 2^60 (the reference raises there).  words needs at most n entries. */
int zk_codec64_encode(const uint64_t* vals, uint64_t n, int delta, uint64_t* words, uint64_t cap, uint64_t* n_words);
/* sum of the tags = number of values in a word stream */
int zk_codec64_count(const uint64_t* words, uint64_t nw, uint64_t* n_values);
/* codec64.decode (library/codec64.py:122-151); delta != 0 also undoes the delta transform
 * (files.undelta, library/files.py:100-110) */
int zk_codec64_decode(const uint64_t* words, uint64_t nw, int delta, uint64_t* out, uint64_t cap, uint64_t* n_out);

/* The same codec on the device (K11 / K12): values and words are DEVICE arrays; streams are byte-exact
 * with the host functions above and with the reference.  encode: d_words needs at most n entries;
 * ZK_ENOSPC when the words exceed cap: nothing is written at or beyond index cap of d_words, *n_words = the length needed, and
 * the call may be repeated with room.
 * decode: the exact value count comes back in *n_out, also with ZK_ENOSPC when it exceeds cap (so a first
 * call with cap = 0 sizes the output): nothing is written at or beyond index cap of d_out -- with delta != 0 the values are
 * summed in place only once they are known to fit -- and the call may be repeated with room. */
int zk_codec64_encode_dev(zk_ctx* ctx, const uint64_t* d_vals, uint64_t n, int delta, uint64_t* d_words, uint64_t cap, uint64_t* n_words);
int zk_codec64_decode_dev(zk_ctx* ctx, const uint64_t* d_words, uint64_t nw, int delta, uint64_t* d_out, uint64_t cap, uint64_t* n_out);
/* zk_codec64_encode_dev (delta = 0) of 32-bit values: the counts of `zot kmerize` (array('I'), commands/kmerize.py:370-437) go into
 * the 'counts' member (files.writeKmersAndCounts2, library/files.py:209-217) without being widened to 64 bits first; same words,
 * same ZK_ENOSPC: nothing at or beyond index cap of d_words, *n_words = the length needed, the call may be repeated with room. */
int zk_codec64_encode_u32_dev(zk_ctx* ctx, const uint32_t* d_vals, uint64_t n, uint64_t* d_words, uint64_t cap, uint64_t* n_words);

/* files.undelta (library/files.py:100-110) of a PIECE of a delta stream: in-place inclusive prefix sum of the decoded
 * deltas, continued from `base` (the last k-mer before the piece; 0 for the first piece).  With zk_add_u64 (v[i] += x,
 * asynchronous) this lets every rank of a multi-GPU `zot dist` decode its own contiguous range of the words of a
 * 'kmers' member: scan from 0, exchange the pieces' totals, add the base. */
int zk_undelta(zk_ctx* ctx, uint64_t* d_vals, uint64_t n, uint64_t base);
int zk_add_u64(zk_ctx* ctx, uint64_t* d_vals, uint64_t n, uint64_t x);

/* file.readFastq / file.readFasta (library/file.py:19-52) as chunked text -> base stream converters.
 * state: 4 words, zero before the first chunk, state[1] = records seen.  Feed text; *consumed says how
 * much was used (present the rest again in front of the next chunk); final != 0 on the last chunk.
 * *out_len is read (append position) and updated. */
int zk_parse_fastq(const char* buf, uint64_t len, int final, uint64_t state[4], uint8_t* out, uint64_t out_cap,
                   uint64_t* out_len, uint64_t* consumed);
int zk_parse_fasta(const char* buf, uint64_t len, int final, uint64_t state[4], uint8_t* out, uint64_t out_cap,
                   uint64_t* out_len, uint64_t* consumed);

/* FASTQ text on the device -> base stream of the same length (file.readFastq, library/file.py:38-52):
 * every byte that is not on the second line of a group of four becomes '\n'.  line_phase = number of
 * complete lines before this text, mod 4 (feed whole lines); *n_newlines = '\n' bytes in the text.
 * d_stream may not alias d_text; both 16-byte aligned. */
int zk_fastq_mask(zk_ctx* ctx, const uint8_t* d_text, uint64_t n, uint32_t line_phase, uint8_t* d_stream, uint64_t* n_newlines);

/* ---- ingest: file bytes <-> device memory (next-row f2 of SURVEY.md section 8) --------------------------------------
 * Replaces file.readFastq / openFile + `gunzip -c` (library/file.py:38-52,79-123) feeding reads.next (library/reads.py:86-98):
 * the text is parsed on the device (zk_fastq_mask), the host only moves bytes.  A zk_source reads a file -- plain, or gzip
 * (detected by its magic; multi-member files included) -- AHEAD of the device: a background thread fills page-locked
 * buffers (parallel pread, or zlib inflate) and queues them as asynchronous H2D copies on a copy stream of its own, so
 * reading / inflating, PCIe and the kernels working on the previous batch overlap.  zk_source_start names the device
 * buffer of the next batch and returns at once; zk_source_finish waits and says how many bytes arrived (fewer than
 * asked only at the end of the input).  Batches are cut at line ends with zk_last_newline (position just after the last
 * newline of d_text[0, n), 0 if none) and the tail is carried to the front of the next buffer by the caller (zk_copy). */
typedef struct zk_source zk_source;
zk_source* zk_source_open(zk_ctx* ctx, const char* path, int threads);      /* NULL on failure: zk_last_error(ctx) */
int zk_source_is_gzip(zk_source* src);
int zk_source_start(zk_source* src, uint8_t* d_dst, uint64_t cap);
int zk_source_finish(zk_source* src, uint64_t* n_bytes, int* eof);
void zk_source_close(zk_source* src);
int zk_last_newline(zk_ctx* ctx, const uint8_t* d_text, uint64_t n, uint64_t* cut);
/* a member of a k-mer set between device memory and a region of an open file (files.writeWords / readWords,
 * library/files.py:54-83): D2H / H2D through the page-locked ring, pwrite / pread in `threads` parallel slices */
int zk_device_to_file(zk_ctx* ctx, const void* d_src, uint64_t bytes, int fd, uint64_t file_offset, int threads);
int zk_file_to_device(zk_ctx* ctx, int fd, uint64_t file_offset, uint64_t bytes, void* d_dst, int threads);

/* ---- synthetic input (bench / tests) ------------------------------------- */

/* Reads first .. first+count-1 of the counter-based generator (zotmer_amd/synth.py) as a base
 * stream of count*(L+1) bytes.  genome == 0: uniform bases.  Thresholds are fractions of 2^32. */
int zk_synth_reads(zk_ctx* ctx, uint64_t seed, uint64_t first, uint64_t count, int L, uint64_t genome,
                   uint32_t sub_thr, uint32_t n_thr, uint8_t* d_stream);

/* sum of x and of murmer(x, 0) * count over a counted set, mod 2^64: order-free checksums used by
 * the full-size parity tests.  d_counts may be NULL (every count 1). */
int zk_checksum(zk_ctx* ctx, const uint64_t* d_kmers, const uint32_t* d_counts, uint64_t n, uint64_t sums[3]);

/* The sorted-set format stores strictly ascending k-mers (library/files.py:54-110 delta-codes them; every consumer merges on
 * that order, commands/merge.py:26-86).  *first_bad = the first index i >= 1 with d_kmers[i] <= d_kmers[i - 1], or n if the
 * array is strictly ascending: the order check of the full-size parity tests (the checksums are order-free). */
int zk_first_descent(zk_ctx* ctx, const uint64_t* d_kmers, uint64_t n, uint64_t* first_bad);

/* zk_checksum over 32- or 64-bit counts (`zot merge` works on 64-bit counts) */
int zk_checksum_counts(zk_ctx* ctx, const uint64_t* d_kmers, const void* d_counts, int count_bits, uint64_t n, uint64_t sums[3]);

/* Synthetic k-mer sets (BASELINE configs 3 and 4; zotmer_amd/synth.py set_keys / set_counts is the specification).
 * d_out[i] = rnd(seed, 7, (mul * (first + i) + add) % mod) & (2^key_bits - 1): element first + i of an affine walk through
 * a pool of `mod` random keys (unsorted; sort and dedupe with zk_sort_count).  zk_synth_counts: geometric counts
 * (mean 8) as a function of (seed, key). */
int zk_synth_keys(zk_ctx* ctx, uint64_t seed, uint64_t first, uint64_t count, int key_bits, uint64_t mul, uint64_t add, uint64_t mod,
                  uint64_t* d_out);
int zk_synth_counts(zk_ctx* ctx, uint64_t seed, const uint64_t* d_keys, uint64_t n, uint64_t* d_counts);

/* the same three sums over every k-mer instance (x and rc(x) of each valid window) of a base
 * stream, computed straight from the stream without sorting anything; sums[3..6] = acgt[x & 3]
 * over the same instances (commands/kmerize.py:492-493) */
int zk_stream_checksum(zk_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, int K, uint64_t sums[7]);

/* internal key-source selectors (shared with the kernels) */
#define ZK_KEYS_FORWARD 0
#define ZK_KEYS_BOTH 1
#define ZK_KEYS_CANONICAL 2

#ifdef __cplusplus
}
#endif
#endif /* ZOTK_H */
