// debruijn.hip -- `zot contigs` (zotmer/commands/contigs.py): the two searches the reference makes per k-mer, and the text.
//
// The reference walks the ascending k-mer array S from every index not yet seen and asks, per node, sparse.rank2 for the
// successors of x -- the entries in [y0, y0 + 3], y0 = (x << 2) & (4^K - 1) -- and sparse.rank for the reverse complement.  The
// walk depends on its order and runs on the host (hostio.cpp: zk_contig_walk); what it reads per node is
// computed here for all nodes at once, and what it keeps is turned into FASTA text here.
//   * links_check_kernel: strictly ascending, below 4^K.  One plain store of 1 by whoever finds a fault.
//   * a key directory (search.hpp) over the top `bits` key bits, about 8 keys a bucket, in the call's workspace: every search
//     below starts from two adjacent words of it.
//   * links_next_kernel: one workgroup per tile of ZK_LINKS_TILE consecutive x.  Within one first base y0 ascends with x, so the
//     successors of the tile's x of first base b lie in one ascending window of S: [the first entry >= y0 of the first such x,
//     the last entry <= y0 | 3 of the last].  Four threads find the (at most four) windows, the workgroup stages them in LDS
//     one after the other and every x is resolved there: the lower bound of y0 in its window, then "is it <= y0 | 3, and is the
//     entry after it not".  An entry after the window is above every y0 | 3 of that first base, one before it below every y0,
//     so the window's ends need no further look.  The ranges are skewed (a window holds 4 x the tile's entries where the set is
//     evenly dense, and anything where it is not): windows of more than LK_STAGE entries together are searched in global
//     memory instead, between the same ends.
//   * links_rc_kernel: rc(x) is not monotone in x: one search per element, in the bucket of the directory.  No LDS, so that
//     many waves hide the misses.
//   * contig_len_kernel, a scan, contig_write_kernel: a contig's text is len + K + digits + 9 bytes; a thread per NODE writes
//     its base (the first node of a contig: the header and its K bases, the last: the newline as well), after finding its
//     contig in the offsets by binary search.  No thread's work grows with a contig's length.
// Nothing waits on another workgroup in the link kernels and there are no atomics; the scan of the render is codec.hip's.
#include "internal.hpp"
#include "search.hpp"

namespace zk {

constexpr int LK_BLOCK = 256, LK_ITEMS = 4, LK_TILE = LK_BLOCK * LK_ITEMS;
static_assert(LK_TILE == ZK_LINKS_TILE, "the tile include/zotk.h publishes");
constexpr int LK_STAGE = 5 * LK_TILE;          // staged window entries: 40 KiB, with the tile's 8 KiB three workgroups per CU

__global__ __launch_bounds__(256) void links_check_kernel(const u64* __restrict__ k, u64 n, int K, u64* __restrict__ bad) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 x = k[i];
        if ((i > 0 && x <= k[i - 1]) || (K < 32 && (x >> (2 * K)) != 0)) *bad = 1;
    }
}

__global__ __launch_bounds__(LK_BLOCK) void links_next_kernel(const u64* __restrict__ k, u32 n, int K, KeyDir d, u32* __restrict__ next) {
    __shared__ u64 s_x[LK_TILE];
    __shared__ u64 s_win[LK_STAGE];
    __shared__ u32 s_seg[5];          // the tile's first x whose first base is >= b (tile-local)
    __shared__ u32 s_ws[4], s_we[4];  // the window of first base b in S
    __shared__ u32 s_off[5];          // ... and where it starts in s_win; s_off[4] = the entries of all four
    const int tid = threadIdx.x;
    const u64 t0 = (u64)blockIdx.x * LK_TILE;
    const u32 cnt = (u64)n - t0 < (u64)LK_TILE ? (u32)((u64)n - t0) : (u32)LK_TILE;
    const int top = 2 * K - 2;
    const u64 m = K == 32 ? ~0ull : (1ull << (2 * K)) - 1;
    u64 x[LK_ITEMS];
#pragma unroll
    for (int r = 0; r < LK_ITEMS; r++) {
        const u32 i = (u32)(r * LK_BLOCK + tid);
        x[r] = i < cnt ? k[t0 + i] : 0;
    }
#pragma unroll
    for (int r = 0; r < LK_ITEMS; r++) {
        const u32 i = (u32)(r * LK_BLOCK + tid);
        if (i < cnt) s_x[i] = x[r];
    }
    __syncthreads();
    if (tid < 5) s_seg[tid] = partition_point(0u, cnt, [&](u32 i) { return (s_x[i] >> top) < (u64)tid; });
    __syncthreads();
    if (tid < 4) {
        const u32 a = s_seg[tid], b = s_seg[tid + 1];
        u32 ws = 0, we = 0;
        if (a < b) {
            ws = dir_lower(k, d, (s_x[a] << 2) & m);
            we = dir_upper(k, d, ((s_x[b - 1] << 2) & m) | 3);
        }
        s_ws[tid] = ws;
        s_we[tid] = we;
    }
    __syncthreads();
    if (tid == 0) {
        u32 o = 0;
        for (int b = 0; b < 4; b++) { s_off[b] = o; o += s_we[b] - s_ws[b]; }
        s_off[4] = o;
    }
    __syncthreads();
    const u32 o1 = s_off[1], o2 = s_off[2], o3 = s_off[3], total = s_off[4];
    const bool staged = total <= (u32)LK_STAGE;
    if (staged) {
        for (u32 s = (u32)tid; s < total; s += LK_BLOCK) {
            const u32 b = (s >= o1 ? 1u : 0u) + (s >= o2 ? 1u : 0u) + (s >= o3 ? 1u : 0u);
            s_win[s] = k[s_ws[b] + (s - s_off[b])];
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < LK_ITEMS; r++) {
        const u32 i = (u32)(r * LK_BLOCK + tid);
        if (i >= cnt) continue;
        const u32 b = (u32)(x[r] >> top) & 3u;
        const u64 y0 = (x[r] << 2) & m, y1 = y0 | 3;
        const u32 ws = s_ws[b];
        u32 res = ZK_NO_LINK;
        if (staged) {
            const u32 off = s_off[b], end = s_off[b + 1];
            const u32 lo = lower_bound(s_win, off, end, y0);
            if (lo < end && s_win[lo] <= y1 && (lo + 1 >= end || s_win[lo + 1] > y1)) res = ws + (lo - off);
        } else {
            const u32 end = s_we[b];
            const u32 lo = lower_bound(k, ws, end, y0);
            if (lo < end && k[lo] <= y1 && (lo + 1 >= end || k[lo + 1] > y1)) res = lo;
        }
        next[t0 + i] = res;
    }
}

__global__ __launch_bounds__(256) void links_rc_kernel(const u64* __restrict__ k, u32 n, int K, KeyDir d, u32* __restrict__ rcr) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x)
        rcr[i] = dir_lower(k, d, revcomp(K, k[i]));
}

static int debruijn_links(zk_ctx* c, const u64* k, uint64_t n, int K, u32* next, u32* rcr) {
    if (n == 0) return ZK_OK;
    int bits = 1;
    while (bits < 26 && (8ull << bits) < n) bits++;
    if (bits > 2 * K) bits = 2 * K;
    const u64 nb = 1ull << bits;
    const uint64_t need = 4 * (nb + 1) + (1 << 20);
    ZK_TRY(arena_require(c, need, need));
    u32* dir;
    ZK_TRY(arena_alloc(c, 4 * (nb + 1), (void**)&dir));
    u64* bad = &c->d_scalars->links_bad;
    ZK_HIP(c, hipMemsetAsync(bad, 0, sizeof(u64), c->stream));
    hipLaunchKernelGGL(links_check_kernel, dim3(grid_cap(c, div_up(n, 256), 16)), dim3(256), 0, c->stream, k, (u64)n, K, bad);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(fetch(c, &c->h_scalars->links_bad));
    ZK_TRY(stream_sync(c));
    if (c->h_scalars->links_bad)
        return fail(c, ZK_EINVAL, "zk_debruijn_links: the k-mers are not strictly ascending, or not below 4^%d", K);
    const KeyDir d{dir, 2 * K - bits};
    ZK_TRY(key_dir_build(c, k, (u32)n, d.shift, nb, dir));
    prof_begin(c, ZK_PROF_LINKS, 12 * n);
    hipLaunchKernelGGL(links_next_kernel, dim3((u32)div_up(n, LK_TILE)), dim3(LK_BLOCK), 0, c->stream, k, (u32)n, K, d, next);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    prof_begin(c, ZK_PROF_LINKS_RC, 12 * n);
    hipLaunchKernelGGL(links_rc_kernel, dim3(grid_cap(c, div_up(n, 256), 16)), dim3(256), 0, c->stream, k, (u32)n, K, d, rcr);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    return check_device_error(c);
}

// ---------------------------------------------------------------------------------------
// zk_contig_render
// ---------------------------------------------------------------------------------------
constexpr u32 CR_HEAD = 8;                     // ">contig_"
constexpr u32 CR_LETTERS = 0x54474341u;        // "ACGT", the first letter in the low byte

__device__ __forceinline__ u8 cr_letter(u64 x, int base_from_last) { return (u8)(CR_LETTERS >> (8 * (u32)((x >> (2 * base_from_last)) & 3))); }

// len[c] = the bytes of contig c; the offsets and the nodes are checked on the way
__global__ __launch_bounds__(256) void contig_len_kernel(const u32* __restrict__ nodes, u64 n_nodes, const u64* __restrict__ offs, u64 n_contigs,
                                                         u64 n, int K, u64* __restrict__ len, u64* __restrict__ bad) {
    const u64 most = n_nodes > n_contigs ? n_nodes : n_contigs;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < most; i += (u64)gridDim.x * blockDim.x) {
        if (i < n_nodes && nodes[i] >= n) *bad = 1;
        if (i < n_contigs) {
            const u64 a = offs[i], b = offs[i + 1];
            const bool ok = a < b && b <= n_nodes && (i > 0 || a == 0) && (i + 1 < n_contigs || b == n_nodes);
            if (ok) len[i] = (b - a) + (u64)K + dec_digits(nodes[a]) + CR_HEAD + 1;
            else { len[i] = 0; *bad = 1; }
        }
    }
}

// contig c ends at incl[c]
__global__ __launch_bounds__(256) void contig_write_kernel(const u64* __restrict__ k, int K, const u32* __restrict__ nodes, u64 n_nodes,
                                                           const u64* __restrict__ offs, u64 n_contigs, const u64* __restrict__ incl,
                                                           u8* __restrict__ out) {
    for (u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x; q < n_nodes; q += (u64)gridDim.x * blockDim.x) {
        // the contig of node q: the first c with offs[c + 1] > q
        const u64 lo = partition_point(0ull, n_contigs - 1, [&](u64 c) { return offs[c + 1] <= q; });
        const u64 a = offs[lo], len = offs[lo + 1] - a, p = q - a;
        const u64 first = lo ? incl[lo - 1] : 0;
        const u64 body = incl[lo] - (len + (u64)K);          // the K bases of the first node start here
        const u32 node = nodes[q];
        const u64 x = k[node];
        if (p == 0) {
            u8* h = out + first;
            h[0] = '>'; h[1] = 'c'; h[2] = 'o'; h[3] = 'n'; h[4] = 't'; h[5] = 'i'; h[6] = 'g'; h[7] = '_';
            out[body - 1] = '\n';
            put_dec(out + body - 1, node);
            for (int j = 0; j < K; j++) out[body + j] = cr_letter(x, K - 1 - j);
        } else {
            out[body + (u64)K + p - 1] = cr_letter(x, 0);
        }
        if (p == len - 1) out[body + (u64)K + len - 1] = '\n';
    }
}

static int contig_render(zk_ctx* c, const u64* k, uint64_t n, int K, const u32* nodes, uint64_t n_nodes, const u64* offs, uint64_t n_contigs,
                         u8* out, uint64_t cap, uint64_t* n_bytes) {
    *n_bytes = 0;
    if (n_contigs == 0) return ZK_OK;
    const uint64_t need = 8 * n_contigs + (1 << 20);
    ZK_TRY(arena_require(c, need, need));
    u64* len;
    ZK_TRY(arena_alloc(c, 8 * n_contigs, (void**)&len));
    u64* bad = &c->d_scalars->render_bad;
    ZK_HIP(c, hipMemsetAsync(bad, 0, sizeof(u64), c->stream));
    const uint64_t most = n_nodes > n_contigs ? n_nodes : n_contigs;
    prof_begin(c, ZK_PROF_CONTIG_RENDER, 4 * n_nodes + 16 * n_contigs);
    hipLaunchKernelGGL(contig_len_kernel, dim3(grid_cap(c, div_up(most, 256), 16)), dim3(256), 0, c->stream, nodes, (u64)n_nodes, offs,
                       (u64)n_contigs, (u64)n, K, len, bad);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(fetch(c, &c->h_scalars->render_bad));
    uint64_t total;
    ZK_TRY(scan_total(c, len, n_contigs, &total));
    if (c->h_scalars->render_bad)
        return fail(c, ZK_EINVAL, "zk_contig_render: the offsets do not ascend from 0 to n_nodes, or a node is not below n");
    *n_bytes = total;
    if (total > cap) return no_room(c, "zk_contig_render", "bytes of text", total, cap);
    prof_begin(c, ZK_PROF_CONTIG_RENDER, 12 * n_nodes + *n_bytes);
    hipLaunchKernelGGL(contig_write_kernel, dim3(grid_cap(c, div_up(n_nodes, 256), 16)), dim3(256), 0, c->stream, k, K, nodes, (u64)n_nodes,
                       offs, (u64)n_contigs, len, out);
    prof_end(c);
    ZK_HIP(c, hipGetLastError());
    return check_device_error(c);
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_debruijn_links(zk_ctx* c, const uint64_t* d_kmers, uint64_t n, int K, uint32_t* d_next, uint32_t* d_rc) {
    ZK_ARGS(c, K >= 1 && K <= 32 && n < 0xFFFFFFFFull && (n == 0 || (d_kmers && d_next && d_rc)));
    arena_reset(c);
    return debruijn_links(c, (const u64*)d_kmers, n, K, (u32*)d_next, (u32*)d_rc);
}

int zk_contig_render(zk_ctx* c, const uint64_t* d_kmers, uint64_t n, int K, const uint32_t* d_nodes, uint64_t n_nodes, const uint64_t* d_offs,
                     uint64_t n_contigs, uint8_t* d_out, uint64_t cap, uint64_t* n_bytes) {
    ZK_ARGS(c, n_bytes && K >= 1 && K <= 32 && n < 0xFFFFFFFFull && n_contigs <= n_nodes &&
                   (n_contigs == 0 || (d_kmers && d_nodes && d_offs && n_nodes > 0)) && (cap == 0 || d_out));
    arena_reset(c);
    return contig_render(c, (const u64*)d_kmers, n, K, (const u32*)d_nodes, n_nodes, (const u64*)d_offs, n_contigs, d_out, cap, n_bytes);
}

}  // extern "C"
