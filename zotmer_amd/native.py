"""
ctypes binding of libzotk.so (include/zotk.h) -- the only way Python reaches the HIP kernels.

There is no CPU fallback: if the shared library is missing, or no MI355X is visible, the calls
below raise.  The library is built in-tree by `__graft_entry__.build()` (or
`make -C zotmer_amd/csrc`) so that it travels with the source tree.

Device memory is handled through small `DeviceArray` objects (pointer + dtype + length) that
free themselves; numpy arrays go up with `Context.upload` and come back with
`DeviceArray.to_host`.  torch tensors can be used instead: pass `tensor.data_ptr()` wrapped in
`DeviceArray.borrow(...)`.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# ZOTK_LIB: load a differently built libzotk.so (diagnostic builds, tools/stamps.py); same ABI required
LIB_PATH = os.environ.get("ZOTK_LIB") or os.path.join(_HERE, "libzotk.so")

ZK_OK, ZK_EINVAL, ZK_ENOMEM, ZK_EHIP, ZK_ENOSPC, ZK_EOVERFLOW, ZK_EINTERNAL, ZK_ERANGE = 0, -1, -2, -3, -4, -5, -6, -7
KMERIZE_CANONICAL, KMERIZE_BOTH, KMERIZE_SUBSAMPLE, KMERIZE_CANONICAL_ONLY = 0, 1, 2, 4
STRAND_ORPHANS = 1
PROBE_TILE, PROBE_MAX_WINDOWS = 4096, 1024      # ZK_PROBE_TILE, ZK_PROBE_MAX_WINDOWS
TALLY_TILE = 2048                               # ZK_TALLY_TILE
CONTIG_TILE = 4096                              # ZK_CONTIG_TILE
VARS_TILE = 4096                                # ZK_VARS_TILE
LINKS_TILE = 1024                               # ZK_LINKS_TILE
NO_LINK = 0xFFFFFFFF                            # ZK_NO_LINK
PILEUP_DIAGS, PILEUP_TILE = 256, 4096           # ZK_PILEUP_DIAGS, ZK_PILEUP_TILE
PILEUP_MERGE_TILE = 2048                        # ZK_PILEUP_MERGE_TILE
PATH_TILE, PATH_CHUNK = 4096, 256               # ZK_PATH_TILE, ZK_PATH_CHUNK
LCP_TILE = 256                                  # ZK_LCP_TILE
SEQTALLY_TILE = 4096                            # ZK_SEQTALLY_TILE
KSNP_HAMMING, KSNP_LEVENSHTEIN = 0, 1           # ZK_KSNP_HAMMING, ZK_KSNP_LEVENSHTEIN
KSNP_WAVE_GROUP, KSNP_LDS_GROUP, KSNP_PAIR_TILE = 64, 1024, 256   # ZK_KSNP_WAVE_GROUP, ZK_KSNP_LDS_GROUP, ZK_KSNP_PAIR_TILE
STOP_VOTES, STOP_NEAR_ENTRIES, STOP_NEAR_TILE = 512, 64, 1024    # ZK_STOP_VOTES, ZK_STOP_NEAR_ENTRIES, ZK_STOP_NEAR_TILE
FIZZLE_CLASSES = 512                            # ZK_FIZZLE_CLASSES
DUP_WAVE_PAIRS = 64                             # ZK_DUP_WAVE_PAIRS
DEFAULT_TAG_WORDS = 2         # zk_tune(ZK_TUNE_TAG_WORDS) as the library starts (csrc/internal.hpp)

_ERRNAMES = {-1: "ZK_EINVAL", -2: "ZK_ENOMEM", -3: "ZK_EHIP", -4: "ZK_ENOSPC", -5: "ZK_EOVERFLOW",
             -6: "ZK_EINTERNAL", -7: "ZK_ERANGE"}


class ZotkError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (_ERRNAMES.get(code, code), msg))
        self.code = code


class Spectrum(C.Structure):
    """zk_spectrum: the sums of one zk_spectrum_sums pass over two spectra (include/zotk.h)"""
    _fields_ = [("n_shared", C.c_uint64), ("s_min", C.c_uint64), ("x_shared", C.c_uint64), ("y_shared", C.c_uint64),
                ("s_xy_lo", C.c_uint64), ("s_xy_hi", C.c_uint64), ("s_sqrt", C.c_double), ("s_js", C.c_double)]


class StrandStats(C.Structure):
    """zk_strand_stats: what zk_strand_pairs found (include/zotk.h)"""
    _fields_ = [("n_pairs", C.c_uint64), ("n_orphans", C.c_uint64), ("n_palindromes", C.c_uint64)]


class ContigStats(C.Structure):
    """zk_contig_stats: what zk_contig_spectra saw, and the sizes its outputs need (include/zotk.h)"""
    _fields_ = [("n_records", C.c_uint64), ("n_windows", C.c_uint64), ("n_keys", C.c_uint64), ("n_bins", C.c_uint64)]


class VarsStats(C.Structure):
    """zk_vars_stats: what zk_vars_scan saw, and the number of rows its outputs need (include/zotk.h)"""
    _fields_ = [("n_groups", C.c_uint64), ("n_missing", C.c_uint64), ("first_missing", C.c_uint64), ("n_mixed", C.c_uint64),
                ("n_rows", C.c_uint64)]


class ProbeWindow(C.Structure):
    """zk_probe_window: the J bases `value` of a probe, compared with the top J bases of every k-mer (include/zotk.h)"""
    _fields_ = [("value", C.c_uint64), ("J", C.c_int32), ("reserved", C.c_int32)]


class PathWindow(C.Structure):
    """zk_path_window: a k-mer `value` that the entries of `bait` are compared with, under `mask`, up to `max_ham` substituted
    bases, from `min_count` copies on (include/zotk.h)"""
    _fields_ = [("value", C.c_uint64), ("mask", C.c_uint64), ("bait", C.c_uint32), ("max_ham", C.c_uint32),
                ("min_count", C.c_uint32), ("reserved", C.c_uint32)]


class KmerizeStats(C.Structure):
    _fields_ = [("n_windows", C.c_uint64), ("n_instances", C.c_uint64), ("n_unique", C.c_uint64),
                ("n_canonical", C.c_uint64), ("acgt", C.c_uint64 * 4)]


# name -> (restype, argtypes): every symbol include/zotk.h declares
_vp, _u64, _u32, _i, _d = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_double
_pu64 = C.POINTER(C.c_uint64)
SIGNATURES = {
    "zk_create": (_vp, [_i, _u64]),
    "zk_destroy": (None, [_vp]),
    "zk_last_error": (C.c_char_p, [_vp]),
    "zk_set_stream": (_i, [_vp, _vp]),
    "zk_get_stream": (_vp, [_vp]),
    "zk_sync": (_i, [_vp]),
    "zk_reserve": (_i, [_vp, _u64]),
    "zk_release_workspace": (_i, [_vp]),
    "zk_mem_info": (_i, [_vp, _pu64, _pu64]),
    "zk_alloc": (_i, [_vp, _u64, C.POINTER(_vp)]),
    "zk_free": (_i, [_vp, _vp]),
    "zk_upload": (_i, [_vp, _vp, _vp, _u64]),
    "zk_download": (_i, [_vp, _vp, _vp, _u64]),
    "zk_copy": (_i, [_vp, _vp, _vp, _u64]),
    "zk_host_alloc": (_i, [_vp, _u64, C.POINTER(_vp)]),
    "zk_host_free": (_i, [_vp, _vp]),
    "zk_upload_async": (_i, [_vp, _vp, _vp, _u64]),
    "zk_tune": (_i, [_vp, _i, _i]),
    "zk_debug_buffer": (_i, [_vp, _vp]),
    "zk_profile": (_i, [_vp, _i]),
    "zk_profile_read": (_i, [_vp, _i, _pu64, C.POINTER(C.c_double), _pu64]),
    "zk_pack_reads": (_i, [_vp, _vp, _vp, _u64, _vp]),
    "zk_encode": (_i, [_vp, _vp, _u64, _i, _i, _vp, _u64, _pu64, _pu64]),
    "zk_capture_filter": (_i, [_vp, _vp, _u64, _i, _vp, _u64, _vp, _pu64, _pu64]),
    "zk_subsample": (_i, [_vp, _vp, _u64, _u64, _d, _vp, _u64, _pu64]),
    "zk_can": (_i, [_vp, _i, _vp, _u64, _vp]),
    "zk_sort_keys": (_i, [_vp, _vp, _u64, _i]),
    "zk_sort_pairs": (_i, [_vp, _vp, _vp, _u64, _i]),
    "zk_rle": (_i, [_vp, _vp, _u64, _vp, _vp, _u64, _pu64]),
    "zk_sort_count": (_i, [_vp, _vp, _u64, _i, _vp, _vp, _u64, _pu64]),
    "zk_kmerize": (_i, [_vp, _vp, _u64, _i, _i, _d, _u64, _vp, _vp, _u64, C.POINTER(KmerizeStats)]),
    "zk_mirror_expand": (_i, [_vp, _vp, _vp, _u64, _i, _vp, _vp, _u64, _pu64]),
    "zk_hist": (_i, [_vp, _vp, _i, _u64, _pu64, _pu64, _u64, _pu64]),
    "zk_widen_counts": (_i, [_vp, _vp, _vp, _u64]),
    "zk_union_sum": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _i, _u64, _pu64, _pu64]),
    "zk_merge_n": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_vp), _pu64, _vp, _vp, _i, _u64, _pu64, _pu64]),
    "zk_project_dedupe": (_i, [_vp, _vp, _u64, _i, _vp, _u64, _pu64]),
    "zk_project": (_i, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _u64, _pu64]),
    "zk_sample": (_i, [_vp, _vp, _vp, _u64, _u64, _d, _vp, _vp, _u64, _pu64]),
    "zk_split": (_i, [_vp, _vp, _u64, _vp, _u64, _pu64]),
    "zk_project_sum": (_i, [_vp, _vp, _vp, _i, _u64, _i, _vp, _vp, _u64, _pu64, _pu64]),
    "zk_spectrum_sums": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _d, _d, C.POINTER(Spectrum)]),
    "zk_spectrum_sums_row": (_i, [_vp, _vp, _vp, _u64, _d, _u32, C.POINTER(_vp), C.POINTER(_vp), _pu64, C.POINTER(_d), C.POINTER(Spectrum)]),
    "zk_lower_bound": (_i, [_vp, _vp, _u64, _pu64, _u32, _pu64]),
    "zk_trim": (_i, [_vp, _vp, _vp, _i, _u64, _u64, _u64, _vp, _vp, _u64, _pu64]),
    "zk_codec64_encode": (_i, [_vp, _u64, _i, _vp, _u64, _pu64]),
    "zk_codec64_count": (_i, [_vp, _u64, _pu64]),
    "zk_codec64_decode": (_i, [_vp, _u64, _i, _vp, _u64, _pu64]),
    "zk_codec64_encode_dev": (_i, [_vp, _vp, _u64, _i, _vp, _u64, _pu64]),
    "zk_codec64_encode_u32_dev": (_i, [_vp, _vp, _u64, _vp, _u64, _pu64]),
    "zk_codec64_decode_dev": (_i, [_vp, _vp, _u64, _i, _vp, _u64, _pu64]),
    "zk_fastq_mask": (_i, [_vp, _vp, _u64, _u32, _vp, _pu64]),
    "zk_source_open": (_vp, [_vp, C.c_char_p, _i]),
    "zk_source_is_gzip": (_i, [_vp]),
    "zk_source_start": (_i, [_vp, _vp, _u64]),
    "zk_source_finish": (_i, [_vp, _pu64, C.POINTER(_i)]),
    "zk_source_close": (None, [_vp]),
    "zk_last_newline": (_i, [_vp, _vp, _u64, _pu64]),
    "zk_device_to_file": (_i, [_vp, _vp, _u64, _i, _u64, _i]),
    "zk_file_to_device": (_i, [_vp, _i, _u64, _u64, _vp, _i]),
    "zk_undelta": (_i, [_vp, _vp, _u64, _u64]),
    "zk_add_u64": (_i, [_vp, _vp, _u64, _u64]),
    "zk_parse_fastq": (_i, [_vp, _u64, _i, _pu64, _vp, _u64, _pu64, _pu64]),
    "zk_parse_fasta": (_i, [_vp, _u64, _i, _pu64, _vp, _u64, _pu64, _pu64]),
    "zk_synth_reads": (_i, [_vp, _u64, _u64, _u64, _i, _u64, _u32, _u32, _vp]),
    "zk_checksum": (_i, [_vp, _vp, _vp, _u64, _pu64]),
    "zk_checksum_counts": (_i, [_vp, _vp, _vp, _i, _u64, _pu64]),
    "zk_first_descent": (_i, [_vp, _vp, _u64, _pu64]),
    "zk_synth_keys": (_i, [_vp, _u64, _u64, _u64, _i, _u64, _u64, _u64, _vp]),
    "zk_synth_counts": (_i, [_vp, _u64, _vp, _u64, _vp]),
    "zk_hash_partition": (_i, [_vp, _vp, _vp, _i, _u64, _i, _u64, _vp, _vp, _pu64]),
    "zk_comm_unique_id": (_i, [_vp]),
    "zk_comm_init": (_i, [_vp, _i, _i, _vp]),
    "zk_comm_destroy": (_i, [_vp]),
    "zk_comm_info": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "zk_all_to_all_v": (_i, [_vp, _vp, _pu64, _pu64, _vp, _pu64, _pu64, _i]),
    "zk_allreduce_u64": (_i, [_vp, _pu64, _u64, _i]),
    "zk_comm_plan": (_i, [_i, _i, _pu64, _pu64, _pu64, _pu64, _i, _u64, _i, _vp, _u64, _pu64]),
    "zk_stream_checksum": (_i, [_vp, _vp, _u64, _i, _pu64]),
    "zk_bait_table_build": (_i, [_vp, _vp, _u64, _i, C.POINTER(_vp)]),
    "zk_bait_table_info": (_i, [_vp, _pu64, _pu64, _pu64]),
    "zk_bait_table_free": (None, [_vp]),
    "zk_bait_table_arrays": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "zk_bait_table_from_arrays": (_i, [_vp, _i, _vp, _u64, _vp, _vp, _u64, _u64, C.POINTER(_vp)]),
    "zk_bait_record_sizes": (_i, [_vp, _vp, _vp]),
    "zk_bait_tally": (_i, [_vp, _vp, _vp, _u64, _vp]),
    "zk_line_ends": (_i, [_vp, _vp, _u64, _vp, _u64, _pu64]),
    "zk_capture_hits": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _u64, _vp, _u64, _pu64]),
    "zk_capture_gather": (_i, [_vp, _vp, _u64, _u32, _vp, _vp, _u64, _vp, _u64, _pu64, _pu64]),
    "zk_pulldown_hits": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _u64, _vp, _u64, _pu64, _vp, _u64, _pu64]),
    "zk_strand_keys": (_i, [_vp, _vp, _vp, _u64, _i, _i, _u64, _u64, _vp, _u64, _pu64]),
    "zk_strand_pairs": (_i, [_vp, _vp, _vp, _i, _u64, _i, _u64, _i, _vp, _vp, _u64, C.POINTER(StrandStats)]),
    "zk_format_pairs": (_i, [_vp, _vp, _vp, _u64, _vp, _u64, _pu64]),
    "zk_probe_scan": (_i, [_vp, _vp, _u64, _i, C.POINTER(ProbeWindow), _u32, _pu64]),
    "zk_vars_scan": (_i, [_vp, _vp, _vp, _i, _u64, _vp, _vp, _i, _u64, _i, _d, _vp, _vp, _u64, C.POINTER(VarsStats)]),
    "zk_debruijn_links": (_i, [_vp, _vp, _u64, _i, _vp, _vp]),
    "zk_contig_walk": (_i, [_vp, _vp, _u64, _i, _u64, _vp, _u64, _vp, _u64, _pu64, _pu64]),
    "zk_contig_render": (_i, [_vp, _vp, _u64, _i, _vp, _u64, _vp, _u64, _vp, _u64, _pu64]),
    "zk_anchor_pileup": (_i, [_vp, _vp, _vp, _vp, _u64, _i, _u32, _vp, _vp, _u64, _pu64]),
    "zk_pileup_count": (_i, [_vp, _vp, _vp, _u64, _i, _vp, _vp, _vp, _u64, _pu64]),
    "zk_pileup_merge": (_i, [_vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _i, _u64, _vp, _vp, _vp, _u64, _pu64]),
    "zk_narrow_counts": (_i, [_vp, _vp, _vp, _u64, _pu64]),
    "zk_capture_kmers": (_i, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _i, _vp, _vp, _u64, _pu64]),
    "zk_path_scan": (_i, [_vp, _vp, _vp, _vp, _u64, _i, C.POINTER(PathWindow), _u32, _vp, _vp, _u64, _pu64]),
    "zk_lcp_resolve": (_i, [_vp, _vp, _u64, _vp, _u64, _i, _vp, _vp]),
    "zk_scan_place": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _u64, _vp, _u64, _i, _vp, _vp, _vp]),
    "zk_sequence_tally": (_i, [_vp, _vp, _vp, _u64, _pu64, _vp, _pu64, _pu64]),
    "zk_spike_zone_counts": (_i, [_vp, _vp, _u64, _u64, _u64, _u64, _vp]),
    "zk_spike_pairs": (_i, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _u64, _u64, _i, C.c_int64, C.c_int64, _u64, _u64, _u64, _u64,
                            _vp, _u64, _vp, _u64, _pu64]),
    "zk_ksnp_flank": (_i, [_vp, _vp, _u64, _i, _vp, _u64, _pu64]),
    "zk_ksnp_components": (_i, [_vp, _vp, _u64, _i, _i, _u64, _vp, _u64, _pu64]),
    "zk_stop_frames": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _i, _u32, _u64, _u64, _vp, _vp, _u64, _pu64]),
    "zk_stop_nearest": (_i, [_vp, _vp, _vp, _u64, _i, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp]),
    "zk_fizzle_votes": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _u64, _pu64]),
    "zk_dup_join": (_i, [_vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _i, _u32, _vp, _vp, _vp, _vp, _u64, _pu64]),
    "zk_hgvs_draw": (_i, [_vp, _vp, _u64, _vp, _vp, _u64, _pu64, _vp, _pu64, _u64, _u64, _u64, _u64, _vp, _u64, _vp, _u64, _pu64]),
    "zk_hgvs_render": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _u64, _i, _vp, _u64, _pu64]),
    "zk_contig_spectra": (_i, [_vp, _vp, _u64, _i, _i, _u64, _d, _vp, _vp, _u64, _vp, _vp, _u64, C.POINTER(ContigStats)]),
    "zk_count_spectrum": (_i, [_vp, _vp, _vp, _i, _u64, _i, _i, _u64, _d, _pu64, _pu64, _u64, _pu64]),
}

_lib = None


def load():
    """dlopen libzotk.so and bind every declared symbol.  Raises if the library is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ZotkError(ZK_EINTERNAL, "%s is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                          "or `make -C zotmer_amd/csrc` (needs hipcc; there is no CPU fallback)" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)      # AttributeError here = header and library disagree
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def contig_walk(next_, rc, K, min_len):
    """zk_contig_walk on host arrays (u32 next / rc of zk_debruijn_links) -> (nodes u32, offs u64[n_contigs + 1]): the paths
    `zot contigs` keeps, in start order.  Host only: no context, no device.  Capacities that prove too small are grown once."""
    lib = load()
    next_ = np.ascontiguousarray(next_, dtype=np.uint32)
    rc = np.ascontiguousarray(rc, dtype=np.uint32)
    n = len(next_)
    assert len(rc) == n
    cap_nodes, cap_contigs = n, min(n, 1 << 16)
    nn, nc = C.c_uint64(0), C.c_uint64(0)
    for _ in range(2):
        nodes, offs = np.empty(max(cap_nodes, 1), dtype=np.uint32), np.empty(cap_contigs + 1, dtype=np.uint64)
        r = lib.zk_contig_walk(next_.ctypes.data, rc.ctypes.data, n, int(K), int(min_len), nodes.ctypes.data, cap_nodes, offs.ctypes.data,
                               cap_contigs, C.byref(nn), C.byref(nc))
        if r != ZK_ENOSPC:
            break
        cap_nodes, cap_contigs = max(cap_nodes, nn.value), max(cap_contigs, nc.value)
    if r != ZK_OK:
        raise ZotkError(r, "zk_contig_walk: the links are damaged (a next that is no index or ZK_NO_LINK, an rc above n) or an argument is bad")
    return nodes[:nn.value], offs[:nc.value + 1]


class DeviceArray:
    """A typed view of device memory: .ptr, .dtype, .n (elements).  Owns the allocation unless borrowed."""

    def __init__(self, ctx, ptr, dtype, n, owned=True, keep=None):
        self.ctx, self.ptr, self.dtype, self.n, self.owned, self._keep = ctx, ptr, np.dtype(dtype), int(n), owned, keep

    @classmethod
    def borrow(cls, ctx, ptr, dtype, n, keep=None):
        return cls(ctx, ptr, dtype, n, owned=False, keep=keep)

    @property
    def nbytes(self):
        return self.n * self.dtype.itemsize

    def view(self, n, offset=0):
        """First n elements (from element `offset`) as a borrowed array that keeps this one alive."""
        return DeviceArray(self.ctx, self.ptr + offset * self.dtype.itemsize, self.dtype, n, owned=False, keep=self)

    def to_host(self, n=None):
        n = self.n if n is None else int(n)
        out = np.empty(n, dtype=self.dtype)
        if n:
            self.ctx._check(load().zk_download(self.ctx.h, out.ctypes.data, self.ptr, n * self.dtype.itemsize))
        return out

    def free(self):
        if self.owned and self.ptr and self.ctx.h:
            load().zk_free(self.ctx.h, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Source:
    """zk_source: a file (plain or gzip) read ahead of the device through page-locked buffers and a copy stream."""

    def __init__(self, ctx, path, threads):
        self.ctx = ctx
        self.h = ctx.lib.zk_source_open(ctx.h, os.fsencode(path), int(threads))
        if not self.h:
            raise IOError(ctx.lib.zk_last_error(ctx.h).decode(errors="replace"))
        self.gzip = bool(ctx.lib.zk_source_is_gzip(self.h))

    def start(self, dst, offset, cap):
        """begin reading up to cap bytes into dst[offset:] (a uint8 DeviceArray); returns at once"""
        self.ctx._check(self.ctx.lib.zk_source_start(self.h, dst.ptr + int(offset), int(cap)))

    def finish(self):
        """wait for the request -> (bytes that arrived, end of input reached)"""
        n, eof = C.c_uint64(0), C.c_int(0)
        self.ctx._check(self.ctx.lib.zk_source_finish(self.h, C.byref(n), C.byref(eof)))
        return n.value, bool(eof.value)

    def close(self):
        if self.h:
            self.ctx.lib.zk_source_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class BaitTable:
    """zk_bait_table: sorted distinct K-mers of both strands of a set of sequences -> the ascending indices of the sequences
    that hold each one (device memory of its own, freed with the object)."""

    def __init__(self, ctx, h, K=None):
        self.ctx, self.h, self.K = ctx, h, K
        nk, ni, nr = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        ctx._check(ctx.lib.zk_bait_table_info(h, C.byref(nk), C.byref(ni), C.byref(nr)))
        self.n_keys, self.n_ids, self.n_records = nk.value, ni.value, nr.value

    def arrays(self):
        """(keys u64[n_keys], offs u32[n_keys + 1], ids u32[n_ids]) as borrowed DeviceArrays that keep the table alive"""
        k, o, i = _vp(), _vp(), _vp()
        self.ctx._check(self.ctx.lib.zk_bait_table_arrays(self.h, C.byref(k), C.byref(o), C.byref(i)))
        return (DeviceArray.borrow(self.ctx, k.value, np.uint64, self.n_keys, keep=self),
                DeviceArray.borrow(self.ctx, o.value, np.uint32, self.n_keys + 1, keep=self),
                DeviceArray.borrow(self.ctx, i.value, np.uint32, self.n_ids, keep=self))

    def free(self):
        if self.h and self.ctx.h:
            self.ctx.lib.zk_bait_table_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """One zk_ctx: one GPU, one stream."""

    def __init__(self, device=0, workspace_bytes=0):
        self.lib = load()
        self.h = self.lib.zk_create(device, workspace_bytes)
        if not self.h:
            why = self.lib.zk_last_error(None).decode(errors="replace")
            raise ZotkError(ZK_EHIP, "zk_create(%d) failed: %s -- no usable MI355X (there is no CPU fallback)" % (device, why))
        self.device = device

    def close(self):
        if self.h:
            self.lib.zk_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != ZK_OK:
            raise ZotkError(rc, self.lib.zk_last_error(self.h).decode(errors="replace"))

    def _sized(self, rc, n, unfit=(ZK_ENOSPC,)):
        """the end of a sized entry -> (n, whether the result fit): a code of `unfit` is no error, n then says what is needed"""
        if rc not in unfit:
            self._check(rc)
        return n, rc == ZK_OK

    def _fit(self, into, bufs, grow):
        """into(*bufs) -> (n, fit); when the result did not fit, once more into grow(n).  -> (n, bufs)"""
        n, fit = into(*bufs)
        if not fit:
            bufs = grow(n)
            n, fit = into(*bufs)
            assert fit
        return n, bufs

    # ---- memory ---------------------------------------------------------------------------
    def mem_info(self):
        f, t = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.zk_mem_info(self.h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def release_workspace(self):
        self._check(self.lib.zk_release_workspace(self.h))

    def reserve(self, nbytes):
        self._check(self.lib.zk_reserve(self.h, int(nbytes)))

    def sync(self):
        self._check(self.lib.zk_sync(self.h))

    def set_stream(self, handle):
        """queue this context's work on a borrowed hipStream_t (an integer handle: torch.cuda.Stream().cuda_stream), which the
        context never destroys; None: a new stream of its own.  Work already queued is waited for first.  The null stream --
        handle 0, which is what torch's default stream reports -- cannot be borrowed (zk_set_stream reads NULL as "a stream of
        your own"): ValueError, so that nobody gets an unordered stream without noticing; create a torch.cuda.Stream()."""
        if handle is not None and int(handle) == 0:
            raise ValueError("set_stream(0): the null stream cannot be borrowed; pass the handle of a stream that was created, or None")
        self._check(self.lib.zk_set_stream(self.h, C.c_void_p(int(handle)) if handle is not None else None))

    def get_stream(self):
        """the hipStream_t the context queues its work on, as an integer handle"""
        return self.lib.zk_get_stream(self.h) or 0

    def empty(self, n, dtype):
        dt = np.dtype(dtype)
        p = C.c_void_p(0)
        self._check(self.lib.zk_alloc(self.h, max(int(n), 1) * dt.itemsize, C.byref(p)))
        return DeviceArray(self, p.value, dt, n)

    def upload(self, arr, dtype=None):
        a = np.ascontiguousarray(arr, dtype=dtype)
        d = self.empty(a.size, a.dtype)
        if a.size:
            self._check(self.lib.zk_upload(self.h, d.ptr, a.ctypes.data, a.nbytes))
        return d

    def pinned(self, nbytes):
        """A page-locked uint8 host buffer as a numpy array (freed with the returned object)."""
        p = C.c_void_p(0)
        self._check(self.lib.zk_host_alloc(self.h, int(nbytes), C.byref(p)))
        ctx = self

        class _Pinned:
            def __init__(s):
                s.ptr, s.n = p.value, int(nbytes)
                s.array = np.ctypeslib.as_array((C.c_uint8 * max(s.n, 1)).from_address(s.ptr))[:s.n]

            def free(s):
                if s.ptr and ctx.h:
                    s.array = None
                    ctx.lib.zk_host_free(ctx.h, s.ptr)
                s.ptr = None

            def __del__(s):
                try:
                    s.free()
                except Exception:
                    pass
        return _Pinned()

    def upload_async(self, dst, src_ptr, nbytes):
        self._check(self.lib.zk_upload_async(self.h, dst.ptr, src_ptr, int(nbytes)))

    # ---- ingest: files <-> device memory (csrc/ingest.hip) -------------------------------------------------
    IO_THREADS = int(os.environ.get("ZOT_IO_THREADS", 0)) or max(1, min(8, (os.cpu_count() or 2) - 1))

    def source_open(self, path, threads=None):
        return Source(self, path, threads or self.IO_THREADS)

    def last_newline(self, text, n):
        """position just after the last newline of the first n bytes of a device text buffer (0: none)"""
        cut = C.c_uint64(0)
        self._check(self.lib.zk_last_newline(self.h, text.ptr, int(n), C.byref(cut)))
        return cut.value

    def device_to_file(self, arr, fileno, offset, threads=None):
        self._check(self.lib.zk_device_to_file(self.h, arr.ptr, arr.nbytes, int(fileno), int(offset), threads or self.IO_THREADS))

    def file_to_device(self, fileno, offset, nbytes, dtype=np.uint8, threads=None):
        dt = np.dtype(dtype)
        out = self.empty(nbytes // dt.itemsize, dt)
        self._check(self.lib.zk_file_to_device(self.h, int(fileno), int(offset), int(nbytes), out.ptr, threads or self.IO_THREADS))
        return out

    def upload_stream(self, data):
        """bytes / uint8 array -> device base stream (zk_alloc memory is 256-byte aligned)."""
        a = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.asarray(data, np.uint8)
        return self.upload(a)

    # ---- per-launch timing (HIP events on the ctx stream) -----------------------------------
    PROF_TAGS = {"hist_stream": 1, "hist_array": 2, "pass_stream": 3, "pass_keys": 4, "pass_pairs": 5, "rle": 6,
                 "union_sum": 7, "select": 8, "mirror": 9, "intersect": 10, "count_hist": 11, "pass_packed": 12, "sample": 13, "tile_sort": 14,
                 "capture_hits": 15, "project_sum": 16, "spectrum": 17, "strand_keys": 18, "strand_pairs": 19, "format_pairs": 20,
                 "probe_scan": 21, "bait_tally": 22, "vars_scan": 23, "links": 24, "links_rc": 25, "contig_render": 26,
                 "pileup": 27, "pileup_cut": 28, "pulldown_tally": 29, "capture_kmers": 30, "path_scan": 31, "lcp_resolve": 32, "scan_place": 33,
                 "seq_tally": 34, "spike_pairs": 35, "spike_size": 36, "ksnp_flank": 37, "ksnp_pairs": 38,
                 "stop_frames": 39, "stop_emit": 40, "stop_nearest": 41, "fizzle_count": 42, "fizzle_emit": 43,
                 "hgvs_draw": 44, "hgvs_fill": 45, "hgvs_size": 46, "hgvs_render": 47, "dup_cover": 48, "dup_join": 49,
                 "pileup_merge": 50}

    # zk_tune's knob ids (independent assignments in the library: the order they are applied in does not matter)
    TUNE_IDS = dict(sort_variant=1, pairs_variant=2, short_sort=3, side_div=4, xcd_group=5, comm_chunk=6, early_collapse=7,
                    packed_pairs=8, wide_tiles=9, stream_pass=10, stream_ranges=11, tag_words=12, dedupe_variant=13, dedupe_limit=14,
                    dedupe_bits=15, comm_self_loop=16, tag_pass=17, kway=18, tile_sort=19, strand_blocks=20)

    def tune(self, **knobs):
        for name in knobs:
            if name not in self.TUNE_IDS:
                raise TypeError("tune() got an unexpected keyword argument %r" % name)
        for name, value in knobs.items():
            if value is not None:
                self._check(self.lib.zk_tune(self.h, self.TUNE_IDS[name], int(value)))

    def profile(self, enable=True):
        self._check(self.lib.zk_profile(self.h, int(enable)))

    def profile_read(self):
        """{kernel: dict(launches, ms, bytes)} for everything recorded since profile(True)."""
        out = {}
        for name, tag in self.PROF_TAGS.items():
            n, b, ms = C.c_uint64(0), C.c_uint64(0), C.c_double(0)
            self._check(self.lib.zk_profile_read(self.h, tag, C.byref(n), C.byref(ms), C.byref(b)))
            if n.value:
                out[name] = dict(launches=n.value, ms=ms.value, bytes=b.value)
        return out

    # ---- kernels ------------------------------------------------------------------------------
    def pack_reads(self, bases, offs):
        n_reads = offs.n - 1
        total = int(offs.to_host()[-1]) if offs.n else 0
        out = self.empty(total + n_reads, np.uint8)
        self._check(self.lib.zk_pack_reads(self.h, bases.ptr, offs.ptr, n_reads, out.ptr))
        return out

    def encode(self, stream, K, both=True):
        cap = stream.n * (2 if both else 1)
        out = self.empty(cap, np.uint64)
        n = C.c_uint64(0)
        acgt = (C.c_uint64 * 4)()
        self._check(self.lib.zk_encode(self.h, stream.ptr, stream.n, K, int(both), out.ptr, cap, C.byref(n), acgt))
        return out.view(n.value), [int(v) for v in acgt]

    def subsample(self, kmers, seed, p):
        out = self.empty(kmers.n, np.uint64)
        n = C.c_uint64(0)
        self._check(self.lib.zk_subsample(self.h, kmers.ptr, kmers.n, int(seed), float(p), out.ptr, kmers.n, C.byref(n)))
        return out.view(n.value)

    def can(self, K, kmers):
        """basics.can per element: the strand with the smaller murmer(., 17)"""
        out = self.empty(kmers.n, np.uint64)
        self._check(self.lib.zk_can(self.h, int(K), kmers.ptr, kmers.n, out.ptr))
        self.sync()
        return out

    def sort_keys(self, keys, key_bits):
        self._check(self.lib.zk_sort_keys(self.h, keys.ptr, keys.n, key_bits))
        return keys

    def sort_pairs(self, keys, vals, key_bits):
        self._check(self.lib.zk_sort_pairs(self.h, keys.ptr, vals.ptr, keys.n, key_bits))
        return keys, vals

    def rle(self, sorted_keys, in_place=False):
        uniq = sorted_keys if in_place else self.empty(sorted_keys.n, np.uint64)
        cnt = self.empty(sorted_keys.n, np.uint32)
        n = C.c_uint64(0)
        self._check(self.lib.zk_rle(self.h, sorted_keys.ptr, sorted_keys.n, uniq.ptr, cnt.ptr, sorted_keys.n, C.byref(n)))
        return uniq.view(n.value), cnt.view(n.value)

    def sort_count(self, keys, key_bits):
        uniq = self.empty(keys.n, np.uint64)
        cnt = self.empty(keys.n, np.uint32)
        n = C.c_uint64(0)
        self._check(self.lib.zk_sort_count(self.h, keys.ptr, keys.n, key_bits, uniq.ptr, cnt.ptr, keys.n, C.byref(n)))
        return uniq.view(n.value), cnt.view(n.value)

    def kmerize(self, stream, K, flags=KMERIZE_CANONICAL, p=0.0, seed=0, cap=None, out=None):
        """-> (kmers DeviceArray u64, counts DeviceArray u32, KmerizeStats).  `out` = (kmers, counts)
        preallocated arrays to write into (their length is the capacity)."""
        if out is None:
            cap = int(cap) if cap is not None else 2 * stream.n
            ok, oc = self.empty(cap, np.uint64), self.empty(cap, np.uint32)
        else:
            ok, oc = out
            cap = min(ok.n, oc.n)
        st = KmerizeStats()
        self._check(self.lib.zk_kmerize(self.h, stream.ptr, stream.n, K, flags, float(p), int(seed), ok.ptr, oc.ptr, cap, C.byref(st)))
        return ok.view(st.n_unique), oc.view(st.n_unique), st

    def mirror_expand(self, ck, cc, K, out=None):
        """counted canonical list (zk_kmerize with KMERIZE_CANONICAL_ONLY) -> (kmers, counts) of both strands"""
        if out is None:
            ok, oc = self.empty(2 * ck.n, np.uint64), self.empty(2 * ck.n, np.uint32)
        else:
            ok, oc = out
        n = C.c_uint64(0)
        self._check(self.lib.zk_mirror_expand(self.h, ck.ptr, cc.ptr, ck.n, int(K), ok.ptr, oc.ptr, min(ok.n, oc.n), C.byref(n)))
        return ok.view(n.value), oc.view(n.value)

    def hist(self, counts):
        bits = counts.dtype.itemsize * 8
        cap = 1 << 16
        for _ in range(2):            # ZK_ENOSPC = more bins than cap; n then holds how many there are
            vals = np.empty(cap, dtype=np.uint64)
            freq = np.empty(cap, dtype=np.uint64)
            n = C.c_uint64(0)
            rc = self.lib.zk_hist(self.h, counts.ptr, bits, counts.n, vals.ctypes.data_as(_pu64), freq.ctypes.data_as(_pu64), cap, C.byref(n))
            if rc != ZK_ENOSPC or n.value <= cap:
                break
            cap = n.value
        self._check(rc)
        return {int(v): int(f) for v, f in zip(vals[:n.value], freq[:n.value])}

    def widen(self, counts32):
        out = self.empty(counts32.n, np.uint64)
        self._check(self.lib.zk_widen_counts(self.h, counts32.ptr, out.ptr, counts32.n))
        return out

    def union_sum(self, xk, xc, yk, yc, want_acgt=False, out=None):
        bits = xc.dtype.itemsize * 8
        assert yc.dtype == xc.dtype
        if out is None:
            cap = xk.n + yk.n
            ok, oc = self.empty(cap, np.uint64), self.empty(cap, xc.dtype)
        else:
            ok, oc = out
            cap = min(ok.n, oc.n)
        n = C.c_uint64(0)
        acgt = (C.c_uint64 * 4)()
        self._check(self.lib.zk_union_sum(self.h, xk.ptr, xc.ptr, xk.n, yk.ptr, yc.ptr, yk.n, ok.ptr, oc.ptr, bits, cap,
                                          C.byref(n), acgt if want_acgt else None))
        r = (ok.view(n.value), oc.view(n.value))
        return r + ([int(v) for v in acgt],) if want_acgt else r

    def merge_n(self, sets, out=None):
        """sets = [(kmers u64 DeviceArray, counts u32|u64 DeviceArray), ...] -> (kmers, counts, acgt_weighted).
        out = (kmers, counts) preallocated arrays to write into (their length is the capacity)."""
        k = len(sets)
        cdt = sets[0][1].dtype if k else np.dtype(np.uint64)
        assert all(s[1].dtype == cdt for s in sets)
        pk = (_vp * k)(*[s[0].ptr for s in sets])
        pc = (_vp * k)(*[s[1].ptr for s in sets])
        ns = (C.c_uint64 * k)(*[s[0].n for s in sets])
        if out is None:
            cap = sum(s[0].n for s in sets)
            ok, oc = self.empty(cap, np.uint64), self.empty(cap, cdt)
        else:
            ok, oc = out
            cap = min(ok.n, oc.n)
        n = C.c_uint64(0)
        acgt = (C.c_uint64 * 4)()
        self._check(self.lib.zk_merge_n(self.h, k, pk, pc, ns, ok.ptr, oc.ptr, cdt.itemsize * 8, cap, C.byref(n), acgt))
        return ok.view(n.value), oc.view(n.value), [int(v) for v in acgt]

    def project_dedupe(self, kmers, shift):
        out = self.empty(kmers.n, np.uint64)
        n = C.c_uint64(0)
        self._check(self.lib.zk_project_dedupe(self.h, kmers.ptr, kmers.n, shift, out.ptr, kmers.n, C.byref(n)))
        return out.view(n.value)

    def split(self, x, y):
        abc = (C.c_uint64 * 3)()
        self._check(self.lib.zk_split(self.h, x.ptr, x.n, y.ptr, y.n, abc))
        return tuple(int(v) for v in abc)

    def project_sum(self, kmers, counts, shift):
        """ascending distinct k-mers and their (u32 | u64) counts -> (distinct kmer >> shift ascending, the u64 sum of the counts
        under each, the sum of all counts)"""
        assert counts.n == kmers.n
        ok, os_ = self.empty(kmers.n, np.uint64), self.empty(kmers.n, np.uint64)
        n, total = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.zk_project_sum(self.h, kmers.ptr, counts.ptr, counts.dtype.itemsize * 8, kmers.n, int(shift), ok.ptr, os_.ptr,
                                            kmers.n, C.byref(n), C.byref(total)))
        return ok.view(n.value), os_.view(n.value), int(total.value)

    def spectrum_sums(self, xk, xs, cx, yk, ys, cy):
        """two spectra as project_sum leaves them (keys, u64 sums, total) -> dict of the sums every spectrum measure is a
        function of (library/measures.py: SPECTRUM); the integers exact, S_xy as one Python int"""
        assert xs.n == xk.n and ys.n == yk.n and xs.dtype.itemsize == 8 and ys.dtype.itemsize == 8
        r = Spectrum()
        self._check(self.lib.zk_spectrum_sums(self.h, xk.ptr, xs.ptr, xk.n, yk.ptr, ys.ptr, yk.n, float(cx), float(cy), C.byref(r)))
        return dict(cx=int(cx), cy=int(cy), n_shared=int(r.n_shared), S_min=int(r.s_min), X_shared=int(r.x_shared),
                    Y_shared=int(r.y_shared), S_xy=int(r.s_xy_lo) | (int(r.s_xy_hi) << 64), S_sqrt=float(r.s_sqrt), S_js=float(r.s_js))

    SPECTRUM_ROW_MAX = 4096             # ZK_SPECTRUM_ROW_MAX: the pairs of one zk_spectrum_sums_row call; longer rows are cut here

    def spectrum_sums_row(self, x, ys):
        """x = (keys, u64 sums, total) against every (keys, u64 sums, total) of ys in one device call per SPECTRUM_ROW_MAX pairs
        (zk_spectrum_sums_row) -> the list of dicts spectrum_sums returns pair by pair.  The integers are that entry's; the two
        doubles have its terms in an order of their own (the same pair gives the same bits in whatever row it stands)."""
        xk, xs, cx = x
        assert xs.n == xk.n and xs.dtype.itemsize == 8
        out = []
        for lo in range(0, len(ys), self.SPECTRUM_ROW_MAX):
            part = ys[lo:lo + self.SPECTRUM_ROW_MAX]
            m = len(part)
            assert all(s.n == k.n and s.dtype.itemsize == 8 for k, s, _ in part)
            pk = (_vp * m)(*[k.ptr if k.n else None for k, _, _ in part])
            ps = (_vp * m)(*[s.ptr if s.n else None for _, s, _ in part])
            ns = (C.c_uint64 * m)(*[k.n for k, _, _ in part])
            cys = (C.c_double * m)(*[float(cy) for _, _, cy in part])
            res = (Spectrum * m)()
            self._check(self.lib.zk_spectrum_sums_row(self.h, xk.ptr if xk.n else None, xs.ptr if xs.n else None, xk.n, float(cx), m,
                                                      pk, ps, ns, cys, res))
            for r, (_, _, cy) in zip(res, part):
                out.append(dict(cx=int(cx), cy=int(cy), n_shared=int(r.n_shared), S_min=int(r.s_min), X_shared=int(r.x_shared),
                                Y_shared=int(r.y_shared), S_xy=int(r.s_xy_lo) | (int(r.s_xy_hi) << 64), S_sqrt=float(r.s_sqrt),
                                S_js=float(r.s_js)))
        return out

    def codec_encode(self, values, delta):
        """uint64 (or, delta=False, uint32) device values -> device codec64 words (delta=True: ascending k-mers, stored as
        differences).  The word buffer starts at half a word per value (device memory costs ~25 ms per GB to allocate: sorted
        k-mers pack three to a word, counts six) and is grown to the worst case, one word per value, only if that is too small."""
        n = C.c_uint64(0)
        for cap in ((values.n + 1) // 2 + 1024, values.n):
            cap = min(cap, values.n)
            words = self.empty(cap, np.uint64)
            if values.dtype.itemsize == 4:
                if delta:
                    raise ValueError("delta coding is for 64-bit k-mers")
                rc = self.lib.zk_codec64_encode_u32_dev(self.h, values.ptr, values.n, words.ptr, words.n, C.byref(n))
            else:
                rc = self.lib.zk_codec64_encode_dev(self.h, values.ptr, values.n, int(delta), words.ptr, words.n, C.byref(n))
            if rc == ZK_ENOSPC and cap < values.n:
                del words
                continue
            self._check(rc)
            return words.view(n.value)

    def codec_decode(self, words, delta, n_values=None):
        """device codec64 words -> uint64 device values (delta=True also undoes the k-mer differences)."""
        n = C.c_uint64(0)
        if n_values is None:                 # a first pass with no output only counts
            rc = self.lib.zk_codec64_decode_dev(self.h, words.ptr, words.n, 0, None, 0, C.byref(n))
            if rc not in (ZK_OK, ZK_ENOSPC):
                self._check(rc)
            n_values = n.value
        out = self.empty(n_values, np.uint64)
        self._check(self.lib.zk_codec64_decode_dev(self.h, words.ptr, words.n, int(delta), out.ptr, int(n_values), C.byref(n)))
        return out.view(n.value)

    def undelta(self, vals, base=0):
        """in-place prefix sum of decoded k-mer deltas, continued from `base` (files.undelta)"""
        self._check(self.lib.zk_undelta(self.h, vals.ptr, vals.n, int(base) & 0xFFFFFFFFFFFFFFFF))
        return vals

    def add_u64(self, vals, x):
        self._check(self.lib.zk_add_u64(self.h, vals.ptr, vals.n, int(x) & 0xFFFFFFFFFFFFFFFF))
        return vals

    def fastq_mask(self, text, line_phase=0, out=None):
        """FASTQ text on the device -> (base stream of the same length, number of newlines)."""
        out = out if out is not None else self.empty(text.n, np.uint8)
        n = C.c_uint64(0)
        self._check(self.lib.zk_fastq_mask(self.h, text.ptr, text.n, int(line_phase) & 3, out.ptr, C.byref(n)))
        return out, n.value

    def lower_bound(self, sorted_keys, queries):
        q = np.ascontiguousarray(queries, dtype=np.uint64)
        pos = np.zeros(len(q), dtype=np.uint64)
        self._check(self.lib.zk_lower_bound(self.h, sorted_keys.ptr, sorted_keys.n, q.ctypes.data_as(_pu64), len(q),
                                            pos.ctypes.data_as(_pu64)))
        return pos if isinstance(queries, np.ndarray) else [int(p) for p in pos]

    def project(self, ref, kmers, counts):
        ok, oc = self.empty(kmers.n, np.uint64), self.empty(kmers.n, np.uint64)
        n = C.c_uint64(0)
        self._check(self.lib.zk_project(self.h, ref.ptr, ref.n, kmers.ptr, counts.ptr, kmers.n, ok.ptr, oc.ptr, kmers.n, C.byref(n)))
        return ok.view(n.value), oc.view(n.value)

    def sample(self, kmers, counts, seed, p):
        ok, oc = self.empty(kmers.n, np.uint64), self.empty(kmers.n, np.uint64)
        n = C.c_uint64(0)
        self._check(self.lib.zk_sample(self.h, kmers.ptr, counts.ptr, kmers.n, int(seed), float(p), ok.ptr, oc.ptr, kmers.n, C.byref(n)))
        return ok.view(n.value), oc.view(n.value)

    def trim(self, kmers, counts, lo, hi=0):
        bits = counts.dtype.itemsize * 8
        ok, oc = self.empty(kmers.n, np.uint64), self.empty(kmers.n, counts.dtype)
        n = C.c_uint64(0)
        self._check(self.lib.zk_trim(self.h, kmers.ptr, counts.ptr, bits, kmers.n, int(lo), int(hi), ok.ptr, oc.ptr, kmers.n, C.byref(n)))
        return ok.view(n.value), oc.view(n.value)

    def synth_reads(self, seed, first, count, L, genome=0, sub_thr=0, n_thr=0, out=None):
        out = out if out is not None else self.empty(count * (L + 1), np.uint8)
        self._check(self.lib.zk_synth_reads(self.h, int(seed), int(first), int(count), int(L), int(genome), int(sub_thr), int(n_thr), out.ptr))
        return out

    def checksum(self, kmers, counts=None):
        s = (C.c_uint64 * 3)()
        self._check(self.lib.zk_checksum(self.h, kmers.ptr, counts.ptr if counts is not None else None, kmers.n, s))
        return tuple(int(v) for v in s)

    def first_descent(self, kmers):
        """first index whose k-mer is not above its predecessor; kmers.n if strictly ascending"""
        r = C.c_uint64(0)
        self._check(self.lib.zk_first_descent(self.h, kmers.ptr, kmers.n, C.byref(r)))
        return int(r.value)

    def checksum_counts(self, kmers, counts):
        """zk_checksum over 32- or 64-bit counts"""
        s = (C.c_uint64 * 3)()
        self._check(self.lib.zk_checksum_counts(self.h, kmers.ptr, counts.ptr if counts is not None else None,
                                                counts.dtype.itemsize * 8 if counts is not None else 64, kmers.n, s))
        return tuple(int(v) for v in s)

    def synth_set(self, seed, first, count, key_bits, mul=1, add=0, mod=1 << 62, counts=True):
        """A synthetic sorted k-mer set (zotmer_amd/synth.py set_keys / set_counts): sorted distinct keys of the
        affine pool walk, and geometric 64-bit counts.  -> (keys u64, counts u64 | None)"""
        raw = self.empty(count, np.uint64)
        self._check(self.lib.zk_synth_keys(self.h, int(seed), int(first), int(count), int(key_bits), int(mul), int(add), int(mod), raw.ptr))
        k, _ = self.sort_count(raw, key_bits)
        del raw
        k = self.copy_of(k)
        if not counts:
            return k, None
        c = self.empty(k.n, np.uint64)
        self._check(self.lib.zk_synth_counts(self.h, int(seed), k.ptr, k.n, c.ptr))
        return k, c

    def copy_of(self, a):
        """A right-sized copy of a (possibly oversized or borrowed) device array."""
        out = self.empty(a.n, a.dtype)
        if a.n:
            self._check(self.lib.zk_copy(self.h, out.ptr, a.ptr, a.nbytes))
            self.sync()
        return out

    def hash_partition(self, kmers, counts, world, seed=0, out=None):
        """Stable split of a sorted table by the hash-range owner -> (kmers, counts | None, offsets[world + 1])."""
        if out is None:
            ok = self.empty(kmers.n, np.uint64)
            oc = self.empty(kmers.n, counts.dtype) if counts is not None else None
        else:
            ok, oc = out
        offs = (C.c_uint64 * (world + 1))()
        self._check(self.lib.zk_hash_partition(self.h, kmers.ptr, counts.ptr if counts is not None else None,
                                               counts.dtype.itemsize * 8 if counts is not None else 64, kmers.n, int(world), int(seed),
                                               ok.ptr, oc.ptr if oc is not None else None, offs))
        return ok, oc, [int(v) for v in offs]

    # ---- multi-GPU seam (zk_comm_*: RCCL bound by the library itself) -----------------------------------
    @staticmethod
    def comm_unique_id():
        buf = (C.c_uint8 * 128)()
        rc = load().zk_comm_unique_id(buf)
        if rc != ZK_OK:
            raise ZotkError(rc, "zk_comm_unique_id failed (RCCL not loadable?)")
        return bytes(buf)

    def comm_init(self, world, rank, uid):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._check(self.lib.zk_comm_init(self.h, int(world), int(rank), buf))

    def comm_destroy(self):
        self._check(self.lib.zk_comm_destroy(self.h))

    def comm_info(self):
        w, r = C.c_int(1), C.c_int(0)
        self._check(self.lib.zk_comm_info(self.h, C.byref(w), C.byref(r)))
        return w.value, r.value

    def all_to_all_v(self, send_ptr, send_off, send_cnt, recv_ptr, recv_off, recv_cnt, elem_bytes):
        W = len(send_cnt)
        arr = lambda v: (C.c_uint64 * W)(*[int(x) for x in v])
        self._check(self.lib.zk_all_to_all_v(self.h, send_ptr, arr(send_off), arr(send_cnt), recv_ptr, arr(recv_off), arr(recv_cnt),
                                             int(elem_bytes)))

    @staticmethod
    def comm_plan(world, rank, send_off, send_cnt, recv_off, recv_cnt, elem_bytes, chunk_bytes=0, self_loop=False):
        """The messages zk_all_to_all_v issues for this rank, as a list of dicts (host only: no GPU, no RCCL) -- zk_comm_plan."""
        class Op(C.Structure):
            _fields_ = [("recv", C.c_int32), ("peer", C.c_int32), ("round", C.c_uint64), ("offset", C.c_uint64), ("bytes", C.c_uint64)]
        arr = lambda v: (C.c_uint64 * world)(*[int(x) for x in v])
        a = (arr(send_off), arr(send_cnt), arr(recv_off), arr(recv_cnt))
        n = C.c_uint64(0)
        lib = load()
        rc = lib.zk_comm_plan(world, rank, a[0], a[1], a[2], a[3], int(elem_bytes), int(chunk_bytes), int(bool(self_loop)), None, 0, C.byref(n))
        if rc != ZK_OK:
            raise ZotkError(rc, "zk_comm_plan: bad argument")
        ops = (Op * max(n.value, 1))()
        lib.zk_comm_plan(world, rank, a[0], a[1], a[2], a[3], int(elem_bytes), int(chunk_bytes), int(bool(self_loop)), ops, n.value, C.byref(n))
        return [dict(recv=o.recv, peer=o.peer, round=o.round, offset=o.offset, bytes=o.bytes) for o in ops[:n.value]]

    def allreduce_u64(self, vals, op=0):
        a = np.ascontiguousarray(vals, dtype=np.uint64).copy()
        if a.size:
            self._check(self.lib.zk_allreduce_u64(self.h, a.ctypes.data_as(_pu64), a.size, int(op)))
        return a

    def stream_checksum(self, stream, K):
        s = (C.c_uint64 * 7)()
        self._check(self.lib.zk_stream_checksum(self.h, stream.ptr, stream.n, K, s))
        return tuple(int(v) for v in s[:3])

    def stream_acgt(self, stream, K):
        """acgt[x & 3] over every k-mer instance of the stream (commands/kmerize.py:492-493)"""
        s = (C.c_uint64 * 7)()
        self._check(self.lib.zk_stream_checksum(self.h, stream.ptr, stream.n, K, s))
        return [int(v) for v in s[3:7]]

    # ---- read capture (csrc/capture.hip) ------------------------------------------------------------------
    def bait_table(self, stream, K):
        """BaitTable of a base stream of sequences, each followed by one '\\n' (a uint8 DeviceArray)."""
        h = _vp()
        self._check(self.lib.zk_bait_table_build(self.h, stream.ptr, stream.n, int(K), C.byref(h)))
        return BaitTable(self, h.value, int(K))

    # ---- complete alleles of a k-mer index (csrc/allele_tally.hip) ---------------------------------------------
    def bait_table_from_arrays(self, K, keys, offs, ids, n_records):
        """BaitTable from device arrays (u64 keys, u32 offs[len(keys) + 1], u32 ids), checked on the device and copied"""
        assert keys.dtype.itemsize == 8 and offs.dtype.itemsize == 4 and ids.dtype.itemsize == 4 and offs.n == keys.n + 1
        h = _vp()
        self._check(self.lib.zk_bait_table_from_arrays(self.h, int(K), keys.ptr, keys.n, offs.ptr, ids.ptr, ids.n, int(n_records), C.byref(h)))
        return BaitTable(self, h.value, int(K))

    def bait_record_sizes(self, table):
        """the number of keys that list each record -> u32 DeviceArray [n_records]"""
        out = self.empty(table.n_records, np.uint32)
        self._check(self.lib.zk_bait_record_sizes(self.h, table.h, out.ptr))
        return out

    def bait_tally(self, table, kmers, out=None):
        """per record, the number of the ascending k-mers that are keys listing it -> u32 DeviceArray [n_records]"""
        out = out if out is not None else self.empty(table.n_records, np.uint32)
        assert out.n >= table.n_records and out.dtype.itemsize == 4
        self._check(self.lib.zk_bait_tally(self.h, table.h, kmers.ptr, kmers.n, out.ptr))
        return out

    def line_ends(self, text, out=None):
        """positions of the '\\n' bytes of a device text -> u64 DeviceArray view (out: a buffer to reuse; grown when too small)"""
        n = C.c_uint64(0)
        into = lambda o: self._sized(self.lib.zk_line_ends(self.h, text.ptr, text.n, o.ptr, o.n, C.byref(n)), n.value)
        first = out if out is not None else self.empty(text.n // 8 + 64, np.uint64)
        m, (out,) = self._fit(into, (first,), lambda m: (self.empty(m, np.uint64),))
        return out.view(m)

    def capture_hits(self, table, read_K, text1, lines1, n_reads, text2=None, lines2=None, veto=None, out=None):
        """distinct (bait, read) pairs as bait << 32 | read, ascending -> u64 DeviceArray view (out: a buffer to reuse)"""
        assert 4 * n_reads <= lines1.n and (lines2 is None or 4 * n_reads <= lines2.n)
        n = C.c_uint64(0)
        into = lambda o: self._sized(self.lib.zk_capture_hits(
            self.h, table.h, veto.h if veto is not None else None, int(read_K), text1.ptr, lines1.ptr, text2.ptr if text2 is not None else None,
            lines2.ptr if lines2 is not None else None, int(n_reads), o.ptr, o.n, C.byref(n)), n.value)
        first = out if out is not None else self.empty(2 * n_reads + 1024, np.uint64)
        m, (out,) = self._fit(into, (first,), lambda m: (self.empty(m, np.uint64),))
        return out.view(m)

    def capture_gather(self, pairs, n_baits, text, lines, out=None):
        """the captured records, bait by bait -> (uint8 DeviceArray view, pair offsets u64[n_baits + 1], byte offsets u64[n_baits + 1])"""
        spans = np.zeros(2 * (n_baits + 1), dtype=np.uint64)
        n = C.c_uint64(0)
        into = lambda o: self._sized(self.lib.zk_capture_gather(self.h, pairs.ptr, pairs.n, int(n_baits), text.ptr, lines.ptr, lines.n, o.ptr, o.n,
                                                                spans.ctypes.data_as(_pu64), C.byref(n)), n.value)
        first = out if out is not None else self.empty(text.n + 1024, np.uint8)
        m, (out,) = self._fit(into, (first,), lambda m: (self.empty(m, np.uint8),))
        return out.view(m), spans[:n_baits + 1], spans[n_baits + 1:]

    # ---- read pairs per bait (csrc/pulldown.hip) --------------------------------------------------------------
    def pulldown_hits(self, table, read_K, text1, lines1, n_reads, text2=None, lines2=None, veto=None, out=None):
        """capture_hits with pulldown.py's bookkeeping -> (pairs: u64 DeviceArray view as capture_hits gives it, hist:
        numpy u64[n_records + 1] with hist[n] = the reads that are not vetoed and hit n distinct baits, the vetoed reads)"""
        assert 4 * n_reads <= lines1.n and (lines2 is None or 4 * n_reads <= lines2.n)
        n, nv = C.c_uint64(0), C.c_uint64(0)
        hist = self.empty(table.n_records + 1, np.uint64)
        into = lambda o: self._sized(self.lib.zk_pulldown_hits(
            self.h, table.h, veto.h if veto is not None else None, int(read_K), text1.ptr, lines1.ptr, text2.ptr if text2 is not None else None,
            lines2.ptr if lines2 is not None else None, int(n_reads), o.ptr, o.n, C.byref(n), hist.ptr, hist.n, C.byref(nv)), n.value)
        first = out if out is not None else self.empty(2 * n_reads + 1024, np.uint64)
        m, (out,) = self._fit(into, (first,), lambda m: (self.empty(m, np.uint64),))
        return out.view(m), hist.to_host(), nv.value

    # ---- strand bias (csrc/strand_bias.hip) ------------------------------------------------------------------
    def strand_keys(self, text, lines, n_reads, K, reverse, T, out, offset=0, seed=17):
        """the kept tagged keys of the first n_reads records of a device FASTQ text, written to out[offset:] (a u64 DeviceArray)
        -> (keys written or, if they did not fit, needed; whether they fit)"""
        assert 4 * n_reads <= lines.n and 0 <= offset <= out.n
        n = C.c_uint64(0)
        rc = self.lib.zk_strand_keys(self.h, text.ptr, lines.ptr, int(n_reads), int(K), int(bool(reverse)), int(seed), int(T),
                                     out.ptr + 8 * offset, out.n - offset, C.byref(n))
        return self._sized(rc, n.value)

    def strand_pairs(self, keys, counts, K, orphans=False, seed=17):
        """ascending distinct tagged keys + counts (u32 | u64) -> (a u64 view, b u64 view, StrandStats): the lines of `zot strand`"""
        assert counts.n == keys.n
        a, b = self.empty(keys.n, np.uint64), self.empty(keys.n, np.uint64)
        st = StrandStats()
        self._check(self.lib.zk_strand_pairs(self.h, keys.ptr, counts.ptr, counts.dtype.itemsize * 8, keys.n, int(K), int(seed),
                                             STRAND_ORPHANS if orphans else 0, a.ptr, b.ptr, keys.n, C.byref(st)))
        return a.view(st.n_pairs), b.view(st.n_pairs), st

    def format_pairs(self, a, b, out=None):
        """'%d\\t%d\\n' per pair -> uint8 DeviceArray view (out: a buffer to reuse; grown when too small)"""
        assert a.n == b.n
        n = C.c_uint64(0)
        into = lambda o: self._sized(self.lib.zk_format_pairs(self.h, a.ptr, b.ptr, a.n, o.ptr, o.n, C.byref(n)), n.value)
        first = out if out is not None else self.empty(8 * a.n + 1024, np.uint8)
        m, (out,) = self._fit(into, (first,), lambda m: (self.empty(m, np.uint8),))
        return out.view(m)

    # ---- probe presence (csrc/probe_scan.hip) -----------------------------------------------------------------
    def probe_scan(self, kmers, K, windows):
        """windows = [(J, value), ...]: per window the number of k-mers whose top J bases are at Hamming distance 0, 1 and 2 of
        value -> an (n_windows, 3) uint64 array.  Lists longer than PROBE_MAX_WINDOWS take several calls."""
        out = np.zeros((len(windows), 3), dtype=np.uint64)
        for lo in range(0, len(windows), PROBE_MAX_WINDOWS):
            part = windows[lo:lo + PROBE_MAX_WINDOWS]
            arr = (ProbeWindow * len(part))(*[ProbeWindow(int(v), int(J), 0) for J, v in part])
            t = np.zeros(3 * len(part), dtype=np.uint64)
            self._check(self.lib.zk_probe_scan(self.h, kmers.ptr, kmers.n, int(K), arr, len(part), t.ctypes.data_as(_pu64)))
            out[lo:lo + len(part)] = t.reshape(-1, 3)
        return out

    # ---- k-mer spectra per contig (csrc/contig_spectra.hip) ---------------------------------------------------
    def contig_spectra(self, stream, K, both=True, seed=17, p=1.0, cap_bins=None, cap_keys=None, out=None):
        """a base stream of records, each followed by '\\n' -> (words u64 view: record << 32 | count, ascending; freq u64 view;
        keys u64 view: the counted key list; counts u32 view; ContigStats).  Capacities that prove too small are grown once.
        out: (words, freq, keys, counts) arrays to write into first (their lengths are the capacities)."""
        cap_bins = stream.n // 4 + 1024 if cap_bins is None else int(cap_bins)      # a guess; a record has at least one window per bin
        cap_keys = stream.n if cap_keys is None else int(cap_keys)                   # a key has at least one window, a window one byte
        st = ContigStats()
        if out is not None:
            cap_bins, cap_keys = min(out[0].n, out[1].n), min(out[2].n, out[3].n)
        for _ in range(2):
            if out is not None:
                words, freq, keys, counts = out
                out = None
            else:
                words, freq = self.empty(cap_bins, np.uint64), self.empty(cap_bins, np.uint64)
                keys, counts = self.empty(cap_keys, np.uint64), self.empty(cap_keys, np.uint32)
            rc = self.lib.zk_contig_spectra(self.h, stream.ptr, stream.n, int(K), int(bool(both)), int(seed), float(p), words.ptr, freq.ptr,
                                            cap_bins, keys.ptr, counts.ptr, cap_keys, C.byref(st))
            if rc != ZK_ENOSPC:
                break
            cap_bins, cap_keys = max(cap_bins, st.n_bins), max(cap_keys, st.n_keys)
        self._check(rc)
        return words.view(st.n_bins), freq.view(st.n_bins), keys.view(st.n_keys), counts.view(st.n_keys), st

    def count_spectrum(self, keys, counts, K, both=True, seed=17, p=1.0):
        """a counted key list (ascending distinct keys, u32 | u64 window counts) -> [(count, frequency), ...] ascending: the
        histogram of the dict the reference would hold (zk_count_spectrum)"""
        assert counts.n == keys.n
        bits = counts.dtype.itemsize * 8
        cap = 1 << 16
        for _ in range(2):            # ZK_ENOSPC = more bins than cap; n then holds how many there are
            vals = np.empty(cap, dtype=np.uint64)
            freq = np.empty(cap, dtype=np.uint64)
            n = C.c_uint64(0)
            rc = self.lib.zk_count_spectrum(self.h, keys.ptr, counts.ptr, bits, keys.n, int(K), int(bool(both)), int(seed), float(p),
                                            vals.ctypes.data_as(_pu64), freq.ctypes.data_as(_pu64), cap, C.byref(n))
            if rc != ZK_ENOSPC or n.value <= cap:
                break
            cap = n.value
        self._check(rc)
        return [(int(v), int(f)) for v, f in zip(vals[:n.value], freq[:n.value])]

    # ---- bases enriched over a reference set (csrc/vars_scan.hip) ---------------------------------------------
    def vars_scan(self, ref_keys, ref_counts, sam_keys, sam_counts, K, threshold=-10.0, cap_rows=None):
        """two counted key lists (ascending distinct keys, u32 | u64 counts) -> (contexts u64 view, ascending; row counts u64
        view, 8 per row: sx[0..3], gx[0..3]; VarsStats): the sample groups that can have a base with logBinGe below threshold
        (zk_vars_scan).  A capacity that proves too small is grown once."""
        assert ref_counts.n == ref_keys.n and sam_counts.n == sam_keys.n
        cap = 1024 if cap_rows is None else int(cap_rows)
        st = VarsStats()
        for _ in range(2):
            ctxs, rows = self.empty(cap, np.uint64), self.empty(8 * cap, np.uint64)
            rc = self.lib.zk_vars_scan(self.h, ref_keys.ptr, ref_counts.ptr, ref_counts.dtype.itemsize * 8, ref_keys.n, sam_keys.ptr,
                                       sam_counts.ptr, sam_counts.dtype.itemsize * 8, sam_keys.n, int(K), float(threshold), ctxs.ptr,
                                       rows.ptr, cap, C.byref(st))
            if rc != ZK_ENOSPC or st.n_rows <= cap:
                break
            cap = st.n_rows
        self._check(rc)
        return ctxs.view(st.n_rows), rows.view(8 * st.n_rows), st

    # ---- de Bruijn paths of a k-mer set (csrc/debruijn.hip) ----------------------------------------------------
    def debruijn_links(self, kmers, K, out=None):
        """ascending k-mers -> (next u32 DeviceArray: the index of the only successor or NO_LINK; rc u32 DeviceArray: the
        number of k-mers below the reverse complement).  out: (next, rc) arrays to write into."""
        nx, rc = out if out is not None else (self.empty(kmers.n, np.uint32), self.empty(kmers.n, np.uint32))
        assert nx.n >= kmers.n and rc.n >= kmers.n and nx.dtype.itemsize == 4 and rc.dtype.itemsize == 4
        self._check(self.lib.zk_debruijn_links(self.h, kmers.ptr, kmers.n, int(K), nx.ptr, rc.ptr))
        return nx, rc

    def contig_render(self, kmers, K, nodes, offs, out=None):
        """device copies of contig_walk's nodes (u32) and offs (u64) -> the FASTA text as a uint8 DeviceArray view (out: a buffer
        to reuse; grown when too small)"""
        assert nodes.dtype.itemsize == 4 and offs.dtype.itemsize == 8 and offs.n >= 1
        n_contigs = offs.n - 1
        n = C.c_uint64(0)
        into = lambda o: self._sized(self.lib.zk_contig_render(self.h, kmers.ptr, kmers.n, int(K), nodes.ptr, nodes.n, offs.ptr, n_contigs, o.ptr, o.n,
                                                               C.byref(n)), n.value)
        first = out if out is not None else self.empty(nodes.n + n_contigs * (int(K) + 19), np.uint8)
        m, (out,) = self._fit(into, (first,), lambda m: (self.empty(m, np.uint8),))
        return out.view(m)

    # ---- reads piled up on reference zones (csrc/pileup.hip) ----------------------------------------------------
    def anchor_pileup(self, table, text, lines, n_reads, K, pad, out=None):
        """one mate of a FASTQ batch against a table whose ids are anchors -> (coordinates u32 view, k-mers u64 view): the pairs
        (d + p, x) of every window of every read, once per diagonal d of its orientation's list, in no order (zk_anchor_pileup).
        out: (coords, kmers) arrays to write into first; grown when too small."""
        assert 4 * n_reads <= lines.n
        n = C.c_uint64(0)
        oc, ok = out if out is not None else (self.empty(text.n + 1024, np.uint32), self.empty(text.n + 1024, np.uint64))
        assert oc.dtype.itemsize == 4 and ok.dtype.itemsize == 8
        into = lambda a, b: self._sized(self.lib.zk_anchor_pileup(self.h, table.h, text.ptr, lines.ptr, int(n_reads), int(K), int(pad), a.ptr, b.ptr,
                                                                  min(a.n, b.n), C.byref(n)), n.value)
        m, (oc, ok) = self._fit(into, (oc, ok), lambda m: (self.empty(m, np.uint32), self.empty(m, np.uint64)))
        return oc.view(m), ok.view(m)

    def pileup_count(self, coords, kmers, K):
        """pairs of zk_anchor_pileup -> (coordinates u32, k-mers u64, counts u32) views: the distinct pairs, ascending by
        coordinate and then by k-mer, with the number of copies of each (zk_pileup_count)"""
        assert coords.n == kmers.n and coords.dtype.itemsize == 4 and kmers.dtype.itemsize == 8
        n = C.c_uint64(0)
        cap = coords.n
        oc, ok, cnt = self.empty(cap, np.uint32), self.empty(cap, np.uint64), self.empty(cap, np.uint32)
        self._check(self.lib.zk_pileup_count(self.h, coords.ptr, kmers.ptr, coords.n, int(K), oc.ptr, ok.ptr, cnt.ptr, cap, C.byref(n)))
        return oc.view(n.value), ok.view(n.value), cnt.view(n.value)

    # ---- counted lists made one on the device (csrc/pileup_merge.hip) -------------------------------------------
    def pileup_merge_into(self, a, b, out):
        """zk_pileup_merge of two counted lists, each (coordinates u32, k-mers u64, counts) ascending by (coordinate, k-mer) --
        a's counts u64, b's u32 or u64 -- into the three arrays of out (u32, u64, u64) -> (pairs written or, if they did not
        fit, needed; whether they fit)"""
        assert a[0].n == a[1].n == a[2].n and b[0].n == b[1].n == b[2].n
        assert a[0].dtype.itemsize == 4 and a[1].dtype.itemsize == 8 and a[2].dtype.itemsize == 8
        assert b[0].dtype.itemsize == 4 and b[1].dtype.itemsize == 8 and b[2].dtype.itemsize in (4, 8)
        assert out[0].dtype.itemsize == 4 and out[1].dtype.itemsize == 8 and out[2].dtype.itemsize == 8
        n = C.c_uint64(0)
        rc = self.lib.zk_pileup_merge(self.h, a[0].ptr, a[1].ptr, a[2].ptr, a[0].n, b[0].ptr, b[1].ptr, b[2].ptr, 8 * b[2].dtype.itemsize, b[0].n,
                                      out[0].ptr, out[1].ptr, out[2].ptr, min(o.n for o in out), C.byref(n))
        return self._sized(rc, n.value)

    def pileup_merge(self, a, b, out=None):
        """the union of two counted lists as (coordinates u32, k-mers u64, counts u64) views, the counts of a pair that both
        hold added (zk_pileup_merge).  out: three arrays to write into first; one retry with the length the entry reports when
        they are too small."""
        o = out if out is not None else (self.empty(a[0].n + b[0].n, np.uint32), self.empty(a[0].n + b[0].n, np.uint64),
                                         self.empty(a[0].n + b[0].n, np.uint64))
        n, o = self._fit(lambda *o: self.pileup_merge_into(a, b, o), o,
                         lambda n: (self.empty(n, np.uint32), self.empty(n, np.uint64), self.empty(n, np.uint64)))
        return tuple(x.view(n) for x in o)

    def narrow_counts(self, counts):
        """u64 counts -> (u32 DeviceArray of min(count, 2^32 - 1), the largest count): the counterpart of widen
        (zk_narrow_counts)"""
        assert counts.dtype.itemsize == 8
        out = self.empty(counts.n, np.uint32)
        mx = C.c_uint64(0)
        self._check(self.lib.zk_narrow_counts(self.h, counts.ptr, out.ptr, counts.n, C.byref(mx)))
        return out, mx.value

    # ---- variants called from captured read pairs (csrc/hgvs_find.hip) -----------------------------------------
    def capture_kmers_into(self, pairs, text1, lines1, n_reads, K, text2, lines2, out_baits, out_kmers):
        """zk_capture_kmers into the arrays given -> (entries written or, if they did not fit, needed; whether they fit).
        2^32 entries or more never fit: the caller passes fewer pairs."""
        assert 4 * n_reads <= lines1.n and (lines2 is None or 4 * n_reads <= lines2.n)
        assert out_baits.dtype.itemsize == 4 and out_kmers.dtype.itemsize == 8
        n = C.c_uint64(0)
        rc = self.lib.zk_capture_kmers(self.h, pairs.ptr, pairs.n, text1.ptr, lines1.ptr, text2.ptr if text2 is not None else None,
                                       lines2.ptr if lines2 is not None else None, int(n_reads), int(K), out_baits.ptr, out_kmers.ptr,
                                       min(out_baits.n, out_kmers.n), C.byref(n))
        return self._sized(rc, n.value, (ZK_ENOSPC, ZK_ERANGE))

    def capture_kmers(self, pairs, text1, lines1, n_reads, K, text2=None, lines2=None, out=None):
        """pairs of capture_hits (or a slice of them) -> (baits u32 view, k-mers u64 view): (bait, x) and (bait, rc x) for every
        window x of the pair's read in each text, in no order (zk_capture_kmers).  out: (baits, kmers) arrays to write into
        first; grown when too small."""
        ob, ok = out if out is not None else (self.empty(256 * pairs.n + 1024, np.uint32), self.empty(256 * pairs.n + 1024, np.uint64))
        def grow(n):
            if n >= 1 << 32:
                raise ZotkError(ZK_ERANGE, "zk_capture_kmers: %d entries in one call (at most 2^32 - 1); pass fewer pairs" % n)
            return self.empty(n, np.uint32), self.empty(n, np.uint64)

        n, (ob, ok) = self._fit(lambda *o: self.capture_kmers_into(pairs, text1, lines1, n_reads, K, text2, lines2, *o), (ob, ok), grow)
        return ob.view(n), ok.view(n)

    def path_scan(self, baits, kmers, counts, K, windows, out=None):
        """a counted (bait, k-mer) list as pileup_count gives it + windows = [(bait, value, mask, max_ham, min_count), ...]
        ascending by bait -> (window indices, entry indices): numpy u32 arrays of the matches, ascending
        by window and then by entry (zk_path_scan).  out: (win, entry) u32 DeviceArrays to write into first; grown when too small."""
        assert baits.n == kmers.n == counts.n and baits.dtype.itemsize == 4 and kmers.dtype.itemsize == 8 and counts.dtype.itemsize == 4
        arr = (PathWindow * max(len(windows), 1))(*[PathWindow(int(v), int(m), int(b), int(h), int(q), 0) for b, v, m, h, q in windows])
        nw = len(windows)
        n = C.c_uint64(0)
        ow, oe = out if out is not None else (self.empty(4 * nw + 1024, np.uint32), self.empty(4 * nw + 1024, np.uint32))
        into = lambda a, b: self._sized(self.lib.zk_path_scan(self.h, baits.ptr, kmers.ptr, counts.ptr, baits.n, int(K), arr, nw, a.ptr, b.ptr,
                                                              min(a.n, b.n), C.byref(n)), n.value)
        m, (ow, oe) = self._fit(into, (ow, oe), lambda m: (self.empty(m, np.uint32), self.empty(m, np.uint32)))
        return ow.to_host(m), oe.to_host(m)

    # ---- gene alleles from a k-mer set (csrc/lcp_scan.hip) -------------------------------------------------------
    def lcp_resolve(self, S, X, K, out=None):
        """ascending index k-mers S and sample k-mers X -> (L u8, Y u64) DeviceArrays of S.n entries: what the reference's
        resolveAll leaves (zk_lcp_resolve).  out: (L, Y) arrays to write into."""
        L, Y = out if out is not None else (self.empty(S.n, np.uint8), self.empty(S.n, np.uint64))
        assert L.n >= S.n and Y.n >= S.n and L.dtype.itemsize == 1 and Y.dtype.itemsize == 8
        self._check(self.lib.zk_lcp_resolve(self.h, S.ptr, S.n, X.ptr, X.n, int(K), L.ptr, Y.ptr))
        return L, Y

    def scan_place(self, L, Y, T, U, V, rec_off, n_slots, K):
        """(L, Y) of lcp_resolve and the index's T (u32[nS + 1]), U (u32), V (i32), rec_off (u64[n_rec + 1], n_slots its last
        word) -> (P u64[n_slots], Q u8[n_slots], cnt u32[n_rec * (K + 1)]) DeviceArrays (zk_scan_place)"""
        nS, n_rec = T.n - 1, rec_off.n - 1
        assert U.n == V.n and T.dtype.itemsize == 4 and U.dtype.itemsize == 4 and V.dtype.itemsize == 4 and rec_off.dtype.itemsize == 8
        P, Q, cnt = self.empty(n_slots, np.uint64), self.empty(n_slots, np.uint8), self.empty(n_rec * (int(K) + 1), np.uint32)
        self._check(self.lib.zk_scan_place(self.h, L.ptr, Y.ptr, nS, T.ptr, U.ptr, V.ptr, U.n, rec_off.ptr, n_rec, int(K), P.ptr, Q.ptr, cnt.ptr))
        return P, Q, cnt

    # ---- genome tally of `zot hgvs-index -T` (csrc/seq_tally.hip) -------------------------------------------------
    def sequence_tally(self, table, text, state, counts, n=None):
        """a piece of a FASTA record's body (uint8 DeviceArray, its first n bytes) -> counts[i] += the forward windows equal to
        key i of the table (u64 DeviceArray [n_keys], added to).  state: (value, length) of the bases the text before ended
        with, (0, 0) before a record -> (state after, windows met, first_gt: where a line starts with '>', else n)"""
        n = text.n if n is None else int(n)
        assert n <= text.n and counts.dtype.itemsize == 8 and counts.n >= table.n_keys
        st = (C.c_uint64 * 2)(int(state[0]), int(state[1]))
        nw, gt = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.zk_sequence_tally(self.h, table.h, text.ptr, n, st, counts.ptr, C.byref(nw), C.byref(gt)))
        return (int(st[0]), int(st[1])), nw.value, gt.value

    # ---- simulated read pairs of `zot spikein` (csrc/spikein.hip) ---------------------------------------------------
    def spike_zone_counts(self, cum, seed, first, count, counts):
        """the zone draws [first, first + count) added to counts (u64 DeviceArray, one per zone); cum: the inclusive cumulative
        zone lengths (u64 DeviceArray)"""
        assert cum.dtype.itemsize == 8 and counts.dtype.itemsize == 8 and counts.n >= cum.n
        self._check(self.lib.zk_spike_zone_counts(self.h, cum.ptr, cum.n, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), int(count), counts.ptr))

    def spike_pairs_into(self, text, zones, first_pair, heads, head_offs, seed, L, I, sd_q, thr_v, thr_e, first, count, out1, out2):
        """zk_spike_pairs into the two uint8 arrays given -> ((bytes of mate 1, bytes of mate 2) written or, if they did not fit,
        needed; whether they fit).  zones: u64[12 * n_zones], first_pair and head_offs: u64[n_zones + 1]."""
        nz = first_pair.n - 1
        assert zones.n == 12 * nz and head_offs.n == nz + 1 and zones.dtype.itemsize == 8 and first_pair.dtype.itemsize == 8
        assert head_offs.dtype.itemsize == 8 and text.dtype.itemsize == 1 and heads.dtype.itemsize == 1
        nb = (C.c_uint64 * 2)(0, 0)
        rc = self.lib.zk_spike_pairs(self.h, text.ptr, text.n, zones.ptr, first_pair.ptr, nz, heads.ptr, head_offs.ptr, heads.n,
                                     int(seed) & 0xFFFFFFFFFFFFFFFF, int(L), int(I), int(sd_q), int(thr_v), int(thr_e), int(first), int(count),
                                     out1.ptr, out1.n, out2.ptr, out2.n, nb)
        return self._sized(rc, (int(nb[0]), int(nb[1])))

    def spike_pairs(self, text, zones, first_pair, heads, head_offs, seed, L, I, sd_q, thr_v, thr_e, first, count, out=None):
        """-> (mate 1 text, mate 2 text) as uint8 DeviceArray views.  out: (out1, out2) buffers to write into first; grown when
        too small."""
        o1, o2 = out if out is not None else (self.empty(0, np.uint8), self.empty(0, np.uint8))
        args = (text, zones, first_pair, heads, head_offs, seed, L, I, sd_q, thr_v, thr_e, first, count)
        nb, (o1, o2) = self._fit(lambda *o: self.spike_pairs_into(*args, *o), (o1, o2),
                                 lambda nb: (self.empty(nb[0], np.uint8), self.empty(nb[1], np.uint8)))
        return o1.view(nb[0]), o2.view(nb[1])

    # ---- candidate-SNP k-mers of a set (csrc/ksnp.hip) ---------------------------------------------------------------
    def ksnp_into(self, kmers, K, out, metric=None, d=0):
        """zk_ksnp_flank (metric None) or zk_ksnp_components (KSNP_HAMMING / KSNP_LEVENSHTEIN, distance d) into the uint64 array
        given -> (k-mers written or, if they did not fit, needed; whether they fit)"""
        assert kmers.dtype.itemsize == 8 and out.dtype.itemsize == 8
        n = C.c_uint64(0)
        if metric is None:
            rc = self.lib.zk_ksnp_flank(self.h, kmers.ptr, kmers.n, int(K), out.ptr, out.n, C.byref(n))
        else:
            rc = self.lib.zk_ksnp_components(self.h, kmers.ptr, kmers.n, int(K), int(metric), min(int(d), 1 << 62), out.ptr, out.n, C.byref(n))
        return self._sized(rc, n.value)

    def ksnp(self, kmers, K, metric=None, d=0, out=None):
        """ascending k-mers of a set -> the candidate-SNP k-mers among them, ascending, as a uint64 DeviceArray view.  out: an
        array to write into first; one retry with the length the entry reports when it is too small."""
        o = out if out is not None else self.empty(max(kmers.n // 8, 1024), np.uint64)
        n, (o,) = self._fit(lambda o: self.ksnp_into(kmers, K, o, metric, d), (o,), lambda n: (self.empty(n, np.uint64),))
        return o.view(n)

    # ---- in-frame stop codons of reads placed on transcripts (csrc/stop_frames.hip) ----------------------------------
    def stop_frames_into(self, table, starts, text, lines, n_reads, K, pad, seed, first, out_tx, out_kmers):
        """zk_stop_frames into the arrays given -> (stops written or, if they did not fit, needed; whether they fit)"""
        assert 4 * n_reads <= lines.n and starts.dtype.itemsize == 4
        assert out_tx.dtype.itemsize == 4 and out_kmers.dtype.itemsize == 8
        n = C.c_uint64(0)
        rc = self.lib.zk_stop_frames(self.h, table.h, starts.ptr, starts.n, text.ptr, lines.ptr, int(n_reads), int(K), int(pad),
                                     int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), out_tx.ptr, out_kmers.ptr, min(out_tx.n, out_kmers.n), C.byref(n))
        return self._sized(rc, n.value)

    def stop_frames(self, table, starts, text, lines, n_reads, K, pad, seed, first, out=None):
        """a batch of single FASTQ reads, the first of which is read `first` of the run, against a table whose ids are anchors
        on an axis of transcripts in name order (starts: u32, position 0 of each) -> (transcript indices u32 view, k-mers u64
        view): the in-frame stops of the frame drawn for every read, in no order (zk_stop_frames).  out: (tx, kmers) arrays
        to write into first; one retry with the length the entry reports when they are too small."""
        ot, ok = out if out is not None else (self.empty(max(n_reads, 1024), np.uint32), self.empty(max(n_reads, 1024), np.uint64))
        n, (ot, ok) = self._fit(lambda *o: self.stop_frames_into(table, starts, text, lines, n_reads, K, pad, seed, first, *o), (ot, ok),
                                lambda n: (self.empty(n, np.uint32), self.empty(n, np.uint64)))
        return ot.view(n), ok.view(n)

    def stop_nearest(self, tx, kmers, K, tk, tk_offs, known):
        """counted stops ascending by (transcript, k-mer) + every transcript's distinct k-mers (tk u64 ascending per transcript,
        tk_offs u64[n_tx + 1]) + the known stops (u64 ascending) -> (distances u32, nearest k-mers u64, known flags u8)
        (zk_stop_nearest)"""
        assert tx.n == kmers.n and tx.dtype.itemsize == 4 and kmers.dtype.itemsize == 8
        assert tk.dtype.itemsize == 8 and tk_offs.dtype.itemsize == 8 and known.dtype.itemsize == 8 and tk_offs.n >= 1
        m = tx.n
        dist, near, flags = self.empty(m, np.uint32), self.empty(m, np.uint64), self.empty(m, np.uint8)
        self._check(self.lib.zk_stop_nearest(self.h, tx.ptr, kmers.ptr, m, int(K), tk.ptr, tk_offs.ptr, tk_offs.n - 1, known.ptr, known.n,
                                             dist.ptr, near.ptr, flags.ptr))
        return dist, near, flags

    # ---- exon-tuple classes hit by read pairs (csrc/fizzle.hip) -----------------------------------------------------
    def fizzle_votes_into(self, table, K, text1, lines1, text2, lines2, n_reads, single, hist, out_rec, out_cls, out_cnt):
        """zk_fizzle_votes: single (u64[2 * classes]) and hist (u64) are added to, the entries go into the three u32 arrays
        given -> (entries written or, if they did not fit, needed; whether they fit -- if not, nothing was added either)"""
        assert 4 * n_reads <= lines1.n and 4 * n_reads <= lines2.n and single.dtype.itemsize == 8 and hist.dtype.itemsize == 8
        assert single.n >= 2 * table.n_records and out_rec.dtype.itemsize == 4 and out_cls.dtype.itemsize == 4 and out_cnt.dtype.itemsize == 4
        n = C.c_uint64(0)
        rc = self.lib.zk_fizzle_votes(self.h, table.h, int(K), text1.ptr, lines1.ptr, text2.ptr, lines2.ptr, int(n_reads), table.n_records,
                                      single.ptr, hist.ptr, hist.n, out_rec.ptr, out_cls.ptr, out_cnt.ptr,
                                      min(out_rec.n, out_cls.n, out_cnt.n), C.byref(n))
        return self._sized(rc, n.value)

    def fizzle_votes(self, table, K, text1, lines1, text2, lines2, n_reads, single, hist, out=None):
        """a batch of FASTQ read pairs against a table whose every key lists its class: the records with one class are added to
        single and hist, the others come back as (records, classes, hits) u32 views, ascending by (record, class); record 2 p + o
        = orientation o of pair p (zk_fizzle_votes).  out: (rec, cls, cnt) arrays to write into first; one retry with the length
        the entry reports when they are too small."""
        o = out if out is not None else tuple(self.empty(4 * n_reads + 1024, np.uint32) for _ in range(3))
        n, o = self._fit(lambda *o: self.fizzle_votes_into(table, K, text1, lines1, text2, lines2, n_reads, single, hist, *o), o,
                         lambda n: tuple(self.empty(n, np.uint32) for _ in range(3)))
        return tuple(a.view(n) for a in o)

    # ---- candidate tandem duplications of `zot vardyger` (csrc/dup_join.hip) ---------------------------------------
    def dup_join_into(self, baits, kmers, counts, rseq, rkmer, rpos, by_second, K, min_count, cover, out_e, out_i, out_j):
        """zk_dup_join into the arrays given -> (rows written or, if they did not fit, needed; whether they fit).  cover is
        written either way."""
        assert baits.n == kmers.n == counts.n and baits.dtype.itemsize == 4 and kmers.dtype.itemsize == 8 and counts.dtype.itemsize == 4
        assert rseq.n == rkmer.n == rpos.n == by_second.n and cover.n >= rseq.n
        assert rseq.dtype.itemsize == 4 and rkmer.dtype.itemsize == 8 and rpos.dtype.itemsize == 4 and by_second.dtype.itemsize == 4
        assert cover.dtype.itemsize == 4 and out_e.dtype.itemsize == 4 and out_i.dtype.itemsize == 4 and out_j.dtype.itemsize == 4
        n = C.c_uint64(0)
        rc = self.lib.zk_dup_join(self.h, baits.ptr, kmers.ptr, counts.ptr, baits.n, rseq.ptr, rkmer.ptr, rpos.ptr, by_second.ptr, rseq.n,
                                  int(K), int(min_count), cover.ptr, out_e.ptr, out_i.ptr, out_j.ptr, min(out_e.n, out_i.n, out_j.n), C.byref(n))
        return self._sized(rc, n.value)

    def dup_join(self, baits, kmers, counts, rseq, rkmer, rpos, by_second, K, min_count, out=None):
        """a counted (bait, k-mer) list as pileup_count gives it + the occurrence table of the baits' sequences (u32 sequence,
        u64 k-mer, u32 position, ascending; by_second: its indices ascending by (sequence, second half, first half, position))
        -> (cover, entries, lefts, rights) as numpy u32 arrays: every occurrence's count, and the rows (entry index of cb,
        occurrence index of ab, occurrence index of cd) in the entry's fixed order (zk_dup_join).  out: three u32 arrays to
        write the rows into first; one retry with the length the entry reports when they are too small."""
        cover = self.empty(rseq.n, np.uint32)
        o = out if out is not None else tuple(self.empty(1024, np.uint32) for _ in range(3))
        n, o = self._fit(lambda *o: self.dup_join_into(baits, kmers, counts, rseq, rkmer, rpos, by_second, K, min_count, cover, *o), o,
                         lambda n: tuple(self.empty(n, np.uint32) for _ in range(3)))
        return (cover.to_host(),) + tuple(a.to_host(n) for a in o)

    # ---- random variants of `zot hgvs-gen` (csrc/hgvs_gen.hip) -----------------------------------------------------
    HGVS_ROW_WORDS = 6
    HGVS_TABULAR, HGVS_HEADERS, HGVS_DIRECT = 1, 2, 4

    def hgvs_draw_into(self, text, zones, first_var, type_thr, geom, geom_n, mix_thr, seed, first, count, rows, pool):
        """zk_hgvs_draw into the arrays given (rows: u64, 6 words a variant; pool: u8) -> ((rows, pool bytes) written or, if they
        did not fit, needed; whether they fit).  zones: u64[3 * n_zones], first_var: u64[n_zones + 1], type_thr: 7 ints, geom: the
        three tables in a row (u64), geom_n: their 3 lengths."""
        nz = first_var.n - 1
        assert zones.n == 3 * nz and zones.dtype.itemsize == 8 and first_var.dtype.itemsize == 8 and text.dtype.itemsize == 1
        assert geom.dtype.itemsize == 8 and geom.n >= sum(geom_n) and rows.dtype.itemsize == 8 and pool.dtype.itemsize == 1
        thr = (C.c_uint64 * 7)(*[int(t) for t in type_thr])
        gn = (C.c_uint64 * 3)(*[int(t) for t in geom_n])
        n = (C.c_uint64 * 2)(0, 0)
        rc = self.lib.zk_hgvs_draw(self.h, text.ptr, text.n, zones.ptr, first_var.ptr, nz, thr, geom.ptr, gn, int(mix_thr),
                                   int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), int(count), rows.ptr, rows.n // self.HGVS_ROW_WORDS, pool.ptr, pool.n, n)
        return self._sized(rc, (int(n[0]), int(n[1])))

    def hgvs_draw(self, text, zones, first_var, type_thr, geom, geom_n, mix_thr, seed, first, count, out=None):
        """-> (rows u64 view of 6 * count words, pool u8 view).  out: (rows, pool) buffers to write into first; grown when too
        small."""
        rows, pool = out if out is not None else (self.empty(self.HGVS_ROW_WORDS * count, np.uint64), self.empty(2 * count + 64, np.uint8))
        args = (text, zones, first_var, type_thr, geom, geom_n, mix_thr, seed, first, count)
        grow = lambda n: (rows if rows.n >= self.HGVS_ROW_WORDS * n[0] else self.empty(self.HGVS_ROW_WORDS * n[0], np.uint64),
                          pool if pool.n >= n[1] else self.empty(n[1], np.uint8))
        n, (rows, pool) = self._fit(lambda *o: self.hgvs_draw_into(*args, *o), (rows, pool), grow)
        return rows.view(self.HGVS_ROW_WORDS * n[0]), pool.view(n[1])

    def hgvs_render_into(self, rows, pool, text, zones, accs, acc_offs, names, name_offs, first_var, first, flags, out):
        """zk_hgvs_render into the uint8 array given -> (bytes written or, if they did not fit, needed; whether they fit).  names,
        name_offs and first_var may be None without HGVS_HEADERS."""
        nz = zones.n // 3
        assert rows.n % self.HGVS_ROW_WORDS == 0 and rows.dtype.itemsize == 8 and zones.dtype.itemsize == 8 and acc_offs.n == nz + 1
        assert pool.dtype.itemsize == 1 and text.dtype.itemsize == 1 and accs.dtype.itemsize == 1 and out.dtype.itemsize == 1
        if flags & self.HGVS_HEADERS:
            assert name_offs.n == nz + 1 and first_var.n == nz + 1 and names.dtype.itemsize == 1
        nb = C.c_uint64(0)
        rc = self.lib.zk_hgvs_render(self.h, rows.ptr, rows.n // self.HGVS_ROW_WORDS, pool.ptr, pool.n, text.ptr, text.n, zones.ptr, nz, accs.ptr,
                                     acc_offs.ptr, accs.n, names.ptr if names is not None else None, name_offs.ptr if name_offs is not None else None,
                                     names.n if names is not None else 0, first_var.ptr if first_var is not None else None, int(first), int(flags),
                                     out.ptr, out.n, C.byref(nb))
        return self._sized(rc, nb.value)

    def hgvs_render(self, rows, pool, text, zones, accs, acc_offs, names=None, name_offs=None, first_var=None, first=0, flags=0, out=None):
        """-> the lines as a uint8 DeviceArray view.  out: a buffer to write into first; grown when too small."""
        o = out if out is not None else self.empty(48 * (rows.n // self.HGVS_ROW_WORDS) + 64, np.uint8)
        args = (rows, pool, text, zones, accs, acc_offs, names, name_offs, first_var, first, flags)
        nb, (o,) = self._fit(lambda o: self.hgvs_render_into(*args, o), (o,), lambda nb: (self.empty(nb, np.uint8),))
        return o.view(nb)

    def capture_filter(self, stream, K, baits):
        out = self.empty(stream.n, np.uint8)
        nr, nk = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.zk_capture_filter(self.h, stream.ptr, stream.n, K, baits.ptr, baits.n, out.ptr, C.byref(nr), C.byref(nk)))
        return out, nr.value, nk.value
