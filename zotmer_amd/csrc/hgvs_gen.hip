// hgvs_gen.hip -- `zot hgvs-gen` (zotmer/commands/hgvs-gen.py): random variants over zones of a genome, as HGVS lines.
//
// The reference draws, variant after variant, a kind, a position and lengths from Python's random (genVar, hgvs-gen.py:120-171)
// and prints str(v), with the columns of -T in front (:257-271).  Here every draw is rnd(seed, tag, index) of zotmer_amd/synth.py,
// a pure function of the variant's number v in output order, so the variants [first, first + count) of any call are the same
// bits.  Two entries of include/zotk.h:
//   * zk_hgvs_draw: hgvs_draw_kernel, a thread per variant, finds the zone, the kind, the position (for a sub up to 64 tries, then
//     a walk round the zone) and the lengths -- a geometric length is a binary search of a 32-bit draw in a descending table --
//     and leaves a row and the bytes it needs in the pool in the work space; scan64_inclusive turns the bytes into offsets;
//     hgvs_fill_kernel copies the rows out with their offsets and draws the inserted bases.
//   * zk_hgvs_render: hgvs_size_kernel, a thread per row, checks the row against the tables and measures its line;
//     scan64_inclusive; hgvs_write_kernel: a workgroup takes a tile of HR_TILE rows.  A line of up to ZK_HGVS_LONG_LINE bytes is
//     formatted by one thread, a longer one -- a -T line of a long dup -- by a wave, lanes over its bases.  Where the tile's text
//     fits ZK_HGVS_TILE_BYTES both write into LDS, laid out with the phase of the output address, and the workgroup copies the
//     text out in aligned 16-byte stores; a larger tile writes straight to memory.  ZK_HGVS_DIRECT makes every tile do so: the
//     plain thread-per-line form, kept for the measurement of DESIGN.md 6s.
// No atomics; nothing waits on another workgroup but inside scan64_inclusive.
#include "internal.hpp"
#include "search.hpp"

namespace zk {

constexpr u64 HG_T_TYPE = 25, HG_T_POS = 26, HG_T_LEN = 27, HG_T_INS = 28, HG_T_MIX = 29, HG_T_BASES = 30, HG_T_ALT = 31;    // synth.py
constexpr u32 HG_SUB = 0, HG_DEL = 1, HG_INS = 2, HG_DELINS = 3, HG_DUP = 4, HG_ANI = 5, HG_AND = 6;
constexpr int HG_TRIES = 64;
constexpr u64 HG_COORD_MAX = 1ull << 62;
constexpr u64 HG_LEN_MAX = 1ull << 40;
constexpr int HG_ROW = ZK_HGVS_ROW_WORDS;

__device__ __host__ __forceinline__ u64 hg_mix64(u64 z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ u32 hg_upper(u32 ch) { return ch >= 'a' && ch <= 'z' ? ch - 32 : ch; }
__device__ __forceinline__ u32 hg_code(u32 ch) { return ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u; }
__device__ __forceinline__ u32 hg_base(u32 code) { return code == 0 ? 'A' : code == 1 ? 'C' : code == 2 ? 'G' : 'T'; }

// a zone of the table, checked: its window seq[s .. e] is text[off, off + e - s + 1)
struct HgZone { u64 off, s, e; };
__device__ __forceinline__ bool hg_zone(const u64* zones, u64 z, u64 n_text, HgZone& o) {
    o.off = zones[3 * z]; o.s = zones[3 * z + 1]; o.e = zones[3 * z + 2];
    if (o.e < o.s || o.e >= HG_COORD_MAX) return false;
    const u64 span = o.e - o.s + 1;
    return span <= n_text && o.off <= n_text - span;
}

// ---------------------------------------------------------------------------------------
// zk_hgvs_draw
// ---------------------------------------------------------------------------------------
struct DrawArgs {
    const u8* text; u64 n_text;
    const u64* zones; const u64* first; u64 nz;
    u64 thr[7];                // cumulative type thresholds, the last 2^32
    const u64* geom; u64 at[4];    // the tables of -D, -I, -U are geom[at[k], at[k + 1])
    u64 mix_thr, W;
    u64 s_type, s_pos, s_len, s_ins, s_mix, s_bases, s_alt;      // mix64(seed + tag)
    u64 v0, count;
};

// 1 + the entries of the descending table q[lo, hi) above the low 32 bits of r
__device__ __forceinline__ u64 hg_geom(const u64* q, u64 lo, u64 hi, u64 r) {
    const u64 r32 = r & 0xffffffffull;
    return 1 + partition_point(lo, hi, [=](u64 i) { return q[i] > r32; }) - lo;
}

constexpr u64 HG_BAD_TABLES = 1, HG_BAD_ACGT = 2;

// what a launch takes: one variant, row or tile per thread or workgroup, no loop, so that nothing of the arguments lives across one
constexpr u64 HG_LAUNCH = 1ull << 30;

// the row of variant v but for its pool offset, in whose place stands the alternative base of a sub -> 0 and the bytes it needs
// in the pool, or what is wrong
__device__ __forceinline__ u64 hg_draw_one(const DrawArgs& a, u64 v, u64* __restrict__ row, u64& need) {
    const u64* first = a.first;
    const u64 z = partition_point((u64)0, a.nz, [=](u64 m) { return first[m + 1] <= v; });     // the first zone whose variants end after v
    HgZone zn;
    if (z >= a.nz || first[z] > v || !hg_zone(a.zones, z, a.n_text, zn)) return HG_BAD_TABLES;
    const u64 span = zn.e - zn.s + 1;
    const u32 r = (u32)hg_mix64(a.s_type + v);
    u32 kind = 0;                                                       // the thresholds ascend and thr[6] = 2^32: the entry has checked it
#pragma unroll
    for (int k = 0; k < 6; k++) kind += (u64)r >= a.thr[k] ? 1u : 0u;
    u64 p = zn.s + hg_mix64(a.s_pos + 64 * v) % span, q = p, m = 0, aux = 0;
    if (kind == HG_SUB) {
        const u8* w = a.text + zn.off;
        u64 x = p - zn.s;
        u32 c = hg_code(hg_upper(w[x]));
        for (int t = 1; t < HG_TRIES && c > 3; t++) {
            x = hg_mix64(a.s_pos + 64 * v + t) % span;
            c = hg_code(hg_upper(w[x]));
        }
        for (u64 k = 1; k < span && c > 3; k++) {                       // round the zone once from the last try
            x = x + 1 == span ? 0 : x + 1;
            c = hg_code(hg_upper(w[x]));
        }
        if (c > 3) return HG_BAD_ACGT;
        u32 t = (u32)(hg_mix64(a.s_alt + v) % 3);
        t += t >= c ? 1u : 0u;
        p = q = zn.s + x; m = 1; aux = hg_base(t);
    } else if (kind == HG_DEL || kind == HG_DUP) {
        const bool del = kind == HG_DEL;
        const u64 l = hg_geom(a.geom, del ? a.at[0] : a.at[2], del ? a.at[1] : a.at[3], hg_mix64(a.s_len + v));
        q = p + l < zn.e ? p + l : zn.e;
    } else if (kind == HG_INS || kind == HG_ANI) {
        m = hg_geom(a.geom, a.at[1], a.at[2], hg_mix64(a.s_ins + v));
    } else {
        const u64 gl = hg_geom(a.geom, a.at[0], a.at[1], hg_mix64(a.s_len + v));
        const u64 gm = hg_geom(a.geom, a.at[1], a.at[2], hg_mix64(a.s_ins + v));
        const bool one = (hg_mix64(a.s_mix + v) & 0xffffffffull) < a.mix_thr;
        const u64 l = one ? 1 : 1 + gl;
        m = one ? 1 + gm : gm;
        q = p + l < zn.e ? p + l : zn.e;
    }
    row[0] = kind; row[1] = z; row[2] = p; row[3] = q; row[4] = m; row[5] = aux;
    need = kind == HG_SUB ? 1 : (kind == HG_INS || kind == HG_DELINS) ? m : 0;
    return 0;
}

// variant v0 + i0 + the thread's number: its row to ws, its pool bytes to need
__global__ __launch_bounds__(256) void hgvs_draw_kernel(DrawArgs a, u64 i0, u64* __restrict__ ws, u64* __restrict__ need, u64* bad) {
    const u64 i = i0 + (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.count) return;
    u64 n = 0;
    const u64 code = hg_draw_one(a, a.v0 + i, ws + HG_ROW * i, n);
    if (code) *bad = code;
    need[i] = n;
}

__global__ __launch_bounds__(256) void hgvs_fill_kernel(u64 s_bases, u64 W, u64 v0, u64 count, u64 i0, const u64* __restrict__ ws,
                                                        const u64* __restrict__ incl, u64* __restrict__ rows, u64 cap_rows,
                                                        u8* __restrict__ pool, u64 cap_pool) {
    const u64 i = i0 + (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const u64* src = ws + HG_ROW * i;
    const u64 at = i ? incl[i - 1] : 0, n = incl[i] - at;
    const u64 kind = src[0];
    if (i < cap_rows) {
        u64* row = rows + HG_ROW * i;
#pragma unroll
        for (int k = 0; k < 5; k++) row[k] = src[k];
        row[5] = at;
    }
    if (kind == HG_SUB) {
        if (at < cap_pool) pool[at] = (u8)src[5];
        return;
    }
    const u64 base = s_bases + (v0 + i) * W;
    u64 word = 0;
    for (u64 j = 0; j < n; j++) {
        if ((j & 31) == 0) word = hg_mix64(base + (j >> 5));
        if (at + j < cap_pool) pool[at + j] = (u8)hg_base((u32)(word >> (2 * (j & 31))) & 3u);
    }
}

static int hgvs_draw(zk_ctx* c, DrawArgs a, u64* rows, uint64_t cap_rows, u8* pool, uint64_t cap_pool, uint64_t n_out[2]) {
    const uint64_t n = a.count;
    const uint64_t room = (8 * HG_ROW + 8) * n + (4 << 20);
    ZK_TRY(arena_require(c, room, room));
    u64 *ws, *need;
    ZK_TRY(arena_alloc(c, 8 * HG_ROW * n, (void**)&ws));
    ZK_TRY(arena_alloc(c, 8 * n, (void**)&need));
    u64* d_bad = &c->d_scalars->hgvs_bad;
    ZK_HIP(c, hipMemsetAsync(d_bad, 0, sizeof(u64), c->stream));
    prof_begin(c, ZK_PROF_HGVS_DRAW, (8 * HG_ROW + 16) * n);
    for (u64 i0 = 0; i0 < n; i0 += HG_LAUNCH) {
        const u32 grid = (u32)div_up(n - i0 < HG_LAUNCH ? n - i0 : HG_LAUNCH, 256);
        hipLaunchKernelGGL(hgvs_draw_kernel, dim3(grid), dim3(256), 0, c->stream, a, i0, ws, need, d_bad);
        ZK_HIP(c, hipGetLastError());
    }
    prof_end(c);
    ZK_TRY(fetch(c, &c->h_scalars->hgvs_bad));
    uint64_t total;
    ZK_TRY(scan_total(c, need, n, &total));
    if (c->h_scalars->hgvs_bad == HG_BAD_ACGT)
        return fail(c, ZK_EINVAL, "zk_hgvs_draw: a substitution of [%llu, %llu) falls into a zone without a base of ACGT",
                    (unsigned long long)a.v0, (unsigned long long)(a.v0 + n));
    if (c->h_scalars->hgvs_bad)
        return fail(c, ZK_EINVAL, "zk_hgvs_draw: a variant of [%llu, %llu) has no zone in the tables, or its zone is empty or leaves the text",
                    (unsigned long long)a.v0, (unsigned long long)(a.v0 + n));
    n_out[0] = n;
    n_out[1] = total;
    if (n_out[0] > cap_rows || n_out[1] > cap_pool)
        return fail(c, ZK_ENOSPC, "zk_hgvs_draw: %llu rows and %llu pool bytes, room for %llu and %llu", (unsigned long long)n_out[0],
                    (unsigned long long)n_out[1], (unsigned long long)cap_rows, (unsigned long long)cap_pool);
    prof_begin(c, ZK_PROF_HGVS_FILL, 2 * 8 * HG_ROW * n + 8 * n + n_out[1]);
    for (u64 i0 = 0; i0 < n; i0 += HG_LAUNCH) {
        const u32 grid = (u32)div_up(n - i0 < HG_LAUNCH ? n - i0 : HG_LAUNCH, 256);
        hipLaunchKernelGGL(hgvs_fill_kernel, dim3(grid), dim3(256), 0, c->stream, a.s_bases, a.W, a.v0, a.count, i0, (const u64*)ws,
                           (const u64*)need, rows, (u64)cap_rows, pool, (u64)cap_pool);
        ZK_HIP(c, hipGetLastError());
    }
    prof_end(c);
    return check_device_error(c);
}

// ---------------------------------------------------------------------------------------
// zk_hgvs_render
// ---------------------------------------------------------------------------------------
struct RenderArgs {
    const u64* rows; u64 n;
    const u8* pool; u64 n_pool;
    const u8* text; u64 n_text;
    const u64* zones; u64 nz;
    const u8* accs; const u64* acc_offs; u64 n_accs;
    const u8* names; const u64* name_offs; u64 n_names;
    const u64* first; u64 v0;
    u32 flags;
};

// what row i says, checked against the tables
struct HgLine {
    u32 kind, alen, nlen;      // nlen > 0: the zone's `# chrom : name` line goes in front
    u64 p, q, m;
    u64 text_at;               // where base p of the chromosome lies in the text
    u64 pool_at, acc_at, name_at;
};

// CHECK: the size pass; the write pass reads the rows it has passed and tests nothing again
template <bool CHECK>
__device__ __forceinline__ bool hg_line(const RenderArgs& a, u64 i, HgLine& L) {
    const u64* row = a.rows + HG_ROW * i;
    const u64 kind = row[0], z = row[1];
    L.p = row[2]; L.q = row[3]; L.m = row[4]; L.pool_at = row[5];
    if (CHECK && (kind > HG_AND || z >= a.nz)) return false;
    HgZone zn;
    if (CHECK) { if (!hg_zone(a.zones, z, a.n_text, zn)) return false; }
    else { zn.off = a.zones[3 * z]; zn.s = a.zones[3 * z + 1]; }
    L.kind = (u32)kind;
    const u64 a0 = a.acc_offs[z], a1 = a.acc_offs[z + 1];
    if (CHECK) {
        if (L.p < zn.s || L.q < L.p || L.q > zn.e) return false;
        const bool point = kind == HG_SUB || kind == HG_INS || kind == HG_ANI;
        if (point && L.q != L.p) return false;
        if (kind == HG_DEL || kind == HG_DUP ? L.m != 0 : kind == HG_SUB ? L.m != 1 : (L.m < 1 || L.m >= HG_LEN_MAX)) return false;
        const u64 used = kind == HG_SUB ? 1 : (kind == HG_INS || kind == HG_DELINS) ? L.m : 0;
        if (used > a.n_pool || L.pool_at > a.n_pool - used) return false;
        if (a0 > a1 || a1 > a.n_accs || a1 - a0 >= (1ull << 31)) return false;
    }
    L.acc_at = a0; L.alen = (u32)(a1 - a0);
    L.text_at = zn.off + (L.p - zn.s);
    L.nlen = 0; L.name_at = 0;
    if ((a.flags & ZK_HGVS_HEADERS) && a.first[z] == a.v0 + i) {
        const u64 n0 = a.name_offs[z], n1 = a.name_offs[z + 1];
        if (CHECK && (n0 > n1 || n1 > a.n_names || n1 - n0 >= (1ull << 31))) return false;
        L.name_at = n0; L.nlen = (u32)(n1 - n0);
    }
    return true;
}

// the columns of -T: range(), size() and the lengths of wt and mut
struct HgCols { u64 r0, r1, size, wt, mut; };
__device__ __forceinline__ HgCols hg_cols(const HgLine& L) {
    HgCols c;
    const bool point = L.kind == HG_INS || L.kind == HG_ANI;
    c.r0 = L.p; c.r1 = point ? L.p : L.q + 1;
    c.wt = c.r1 - c.r0;
    c.size = L.kind == HG_DEL ? 0 : L.kind == HG_DUP ? 2 * c.wt : L.m;
    c.mut = c.size;
    return c;
}

// the positions of str(v): `<p + 1>`, `<p + 1>_<q + 1>`, or `<p>_<p + 1>` of the two insertions
__device__ __forceinline__ u64 hg_span_len(const HgLine& L) {
    if (L.kind == HG_INS || L.kind == HG_ANI) return dec_digits(L.p) + 1 + dec_digits(L.p + 1);
    return L.p == L.q ? dec_digits(L.p + 1) : dec_digits(L.p + 1) + 1 + dec_digits(L.q + 1);
}

__device__ __forceinline__ u64 hg_line_len(const RenderArgs& a, const HgLine& L) {
    u64 n = L.nlen ? 2 + (u64)L.alen + 3 + L.nlen + 1 : 0;                                      // "# " acc " : " name "\n"
    if (a.flags & ZK_HGVS_TABULAR) {
        const HgCols c = hg_cols(L);
        n += (u64)L.alen + 1 + dec_digits(c.r0) + 1 + dec_digits(c.r1) + 1 + dec_digits(c.size) + 1 + c.wt + 1 + c.mut + 1;
    }
    n += (u64)L.alen + 3 + hg_span_len(L) + 1;                                                   // acc ":g." span ... "\n"
    switch (L.kind) {
    case HG_SUB: return n + 3;
    case HG_DEL: case HG_DUP: return n + 3;
    case HG_INS: return n + 3 + L.m;
    case HG_ANI: return n + 3 + dec_digits(L.m);
    case HG_DELINS: return n + 6 + L.m;
    default: return n + 6 + dec_digits(L.m);
    }
}

// where the bytes of a tile go: into LDS, byte `pos` of the text at lds[pos - base], or straight to the output
struct HgSink {
    u8* out; u64 cap;
    u8* lds; u64 base;
    bool staged;               // (the same in every thread of the workgroup)
    __device__ __forceinline__ void put(u64 pos, u32 ch) const {
        if (staged) { const u64 o = pos - base; if (o < (u64)(ZK_HGVS_TILE_BYTES + 16)) lds[o] = (u8)ch; }
        else if (pos < cap) out[pos] = (u8)ch;
    }
};

// The line of L from byte `pos` of the text.  A thread that writes a line alone has k0 = 0, step = 1 and owns every byte; the 64
// lanes of a wave that share one have the same L and pos, k0 = the lane and step = 64: the runs of bases are spread over the
// lanes, the few bytes between them are lane 0's (few = true).
struct HgWriter {
    const RenderArgs& a; const HgSink& out; u64 pos; u32 k0, step; bool few;
    __device__ __forceinline__ void ch(u32 c) { if (few) out.put(pos, c); pos++; }
    __device__ __forceinline__ void num(u64 x) {
        const u32 d = dec_digits(x);
        if (few) for (u32 k = d; k-- > 0;) { out.put(pos + k, '0' + (u32)(x % 10)); x /= 10; }
        pos += d;
    }
    __device__ __forceinline__ void bytes(const u8* src, u64 n, bool upper) {
        for (u64 k = k0; k < n; k += step) { const u32 c = src[k]; out.put(pos + k, upper ? hg_upper(c) : c); }
        pos += n;
    }
    __device__ __forceinline__ void fill(u32 c, u64 n) {
        for (u64 k = k0; k < n; k += step) out.put(pos + k, c);
        pos += n;
    }
    __device__ __forceinline__ void line(const HgLine& L) {
        const u8* acc = a.accs + L.acc_at;
        const u8* ins = a.pool + L.pool_at;
        const u8* ref = a.text + L.text_at;
        const bool point = L.kind == HG_INS || L.kind == HG_ANI;
        if (L.nlen) { ch('#'); ch(' '); bytes(acc, L.alen, false); ch(' '); ch(':'); ch(' '); bytes(a.names + L.name_at, L.nlen, false); ch('\n'); }
        if (a.flags & ZK_HGVS_TABULAR) {
            const HgCols c = hg_cols(L);
            bytes(acc, L.alen, false); ch('\t');
            num(c.r0); ch('\t'); num(c.r1); ch('\t'); num(c.size); ch('\t');
            bytes(ref, c.wt, true); ch('\t');
            if (L.kind == HG_DUP) { bytes(ref, c.wt, true); bytes(ref, c.wt, true); }
            else if (L.kind == HG_ANI || L.kind == HG_AND) fill('N', L.m);
            else if (L.kind != HG_DEL) bytes(ins, L.m, false);
            ch('\t');
        }
        bytes(acc, L.alen, false); ch(':'); ch('g'); ch('.');
        num(point ? L.p : L.p + 1);
        if (point || L.q != L.p) { ch('_'); num(point ? L.p + 1 : L.q + 1); }
        if (L.kind == HG_SUB) { ch(hg_upper(ref[0])); ch('>'); ch(ins[0]); }
        else {
            const bool del = L.kind == HG_DEL || L.kind == HG_DELINS || L.kind == HG_AND;
            if (del) { ch('d'); ch('e'); ch('l'); }
            if (L.kind == HG_DUP) { ch('d'); ch('u'); ch('p'); }
            if (L.kind != HG_DEL && L.kind != HG_DUP) { ch('i'); ch('n'); ch('s'); }
            if (L.kind == HG_INS || L.kind == HG_DELINS) bytes(ins, L.m, false);
            if (L.kind == HG_ANI || L.kind == HG_AND) num(L.m);
        }
        ch('\n');
    }
};

__global__ __launch_bounds__(256) void hgvs_size_kernel(RenderArgs a, u64 i0, u64* __restrict__ len, u64* bad) {
    const u64 i = i0 + (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    HgLine L;
    const bool ok = hg_line<true>(a, i, L);
    if (!ok) *bad = 1;
    len[i] = ok ? hg_line_len(a, L) : 0;
}

constexpr int HR_TILE = 256;

// one tile of HR_TILE rows per workgroup; t_base = the tiles of the launches before
__global__ __launch_bounds__(HR_TILE) void hgvs_write_kernel(RenderArgs a, u64 t_base, const u64* __restrict__ incl, u8* __restrict__ out, u64 cap) {
    __shared__ __attribute__((aligned(16))) u8 lds[ZK_HGVS_TILE_BYTES + 16];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 t0 = (t_base + blockIdx.x) * HR_TILE, t1 = t0 + HR_TILE < a.n ? t0 + HR_TILE : a.n;
    const u64 start = t0 ? incl[t0 - 1] : 0, bytes = incl[t1 - 1] - start;
    const u32 phase = (u32)(((uintptr_t)out + start) & 15);
    // lds[phase, phase + bytes) is the tile's text: out + start - phase is a 16-byte boundary
    const u64 gbase = start - phase;                                   // (below 0, wrapped, when start < phase: only gbase + x with x >= phase is used)
    const HgSink sink{out, cap, lds, gbase, !(a.flags & ZK_HGVS_DIRECT) && bytes <= (u64)ZK_HGVS_TILE_BYTES};
    const u64 i = t0 + tid;
    HgLine L;
    bool on = i < t1;
    if (on) hg_line<false>(a, i, L);
    u64 at = on ? (i ? incl[i - 1] : 0) : 0;
    const bool wide = on && incl[i] - at > (u64)ZK_HGVS_LONG_LINE;
    u64 todo = __ballot(wide);                                         // the wide lines of this wave's 64 rows
    on = on && !wide;
    u32 k0 = 0, step = 1;
    // round 0: every thread its own line; then a round per wide line, the wave together
    for (;;) {
        if (on) { HgWriter w{a, sink, at, k0, step, k0 == 0}; w.line(L); }
        if (!todo) break;                                              // (the same in every lane)
        const u64 r = t0 + 64 * wave + (u64)(__ffsll((long long)todo) - 1);
        todo &= todo - 1;
        on = hg_line<false>(a, r, L);
        at = r ? incl[r - 1] : 0;
        k0 = lane; step = 64;
    }
    if (!sink.staged) return;
    __syncthreads();
    const u32 end = phase + (u32)bytes;
    for (u32 x = 16 * tid; x < end; x += 16 * HR_TILE) {
        if (x >= phase && x + 16 <= end && gbase + x + 16 <= cap) {
            *reinterpret_cast<uint4*>(out + (gbase + x)) = *reinterpret_cast<const uint4*>(lds + x);
        } else {
            const u32 lo = x > phase ? x : phase, hi = x + 16 < end ? x + 16 : end;
            for (u32 k = lo; k < hi; k++) if (gbase + k < cap) out[gbase + k] = lds[k];
        }
    }
}

static int hgvs_render(zk_ctx* c, RenderArgs a, u8* out, uint64_t cap, uint64_t* n_bytes) {
    const uint64_t n = a.n;
    const uint64_t room = 8 * n + (4 << 20);
    ZK_TRY(arena_require(c, room, room));
    u64* len;
    ZK_TRY(arena_alloc(c, 8 * n, (void**)&len));
    u64* d_bad = &c->d_scalars->hgvs_bad;
    ZK_HIP(c, hipMemsetAsync(d_bad, 0, sizeof(u64), c->stream));
    prof_begin(c, ZK_PROF_HGVS_SIZE, (8 * HG_ROW + 16) * n);
    for (u64 i0 = 0; i0 < n; i0 += HG_LAUNCH) {
        const u32 grid = (u32)div_up(n - i0 < HG_LAUNCH ? n - i0 : HG_LAUNCH, 256);
        hipLaunchKernelGGL(hgvs_size_kernel, dim3(grid), dim3(256), 0, c->stream, a, i0, len, d_bad);
        ZK_HIP(c, hipGetLastError());
    }
    prof_end(c);
    ZK_TRY(fetch(c, &c->h_scalars->hgvs_bad));
    uint64_t total;
    ZK_TRY(scan_total(c, len, n, &total));
    if (c->h_scalars->hgvs_bad)
        return fail(c, ZK_EINVAL, "zk_hgvs_render: a row of unknown kind, outside its zone (s <= p <= q <= e), with a pool range outside the pool, "
                                  "or a zone that leaves the text or whose prefix offsets are out of order");
    *n_bytes = total;
    if (*n_bytes > cap) return no_room(c, "zk_hgvs_render", "bytes of lines", *n_bytes, cap);
    prof_begin(c, ZK_PROF_HGVS_RENDER, 8 * HG_ROW * n + 8 * n + *n_bytes);
    const u64 tiles = div_up(n, HR_TILE);
    for (u64 t = 0; t < tiles; t += HG_LAUNCH / HR_TILE) {
        const u32 grid = (u32)(tiles - t < HG_LAUNCH / HR_TILE ? tiles - t : HG_LAUNCH / HR_TILE);
        hipLaunchKernelGGL(hgvs_write_kernel, dim3(grid), dim3(HR_TILE), 0, c->stream, a, t, (const u64*)len, out, (u64)cap);
        ZK_HIP(c, hipGetLastError());
    }
    prof_end(c);
    return check_device_error(c);
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_hgvs_draw(zk_ctx* c, const uint8_t* d_text, uint64_t n_text, const uint64_t* d_zones, const uint64_t* d_first, uint64_t n_zones,
                 const uint64_t type_thr[7], const uint64_t* d_geom, const uint64_t geom_n[3], uint64_t mix_thr, uint64_t seed, uint64_t first,
                 uint64_t count, uint64_t* d_rows, uint64_t cap_rows, uint8_t* d_pool, uint64_t cap_pool, uint64_t n_out[2]) {
    ZK_ARGS(c, n_out && type_thr && geom_n && count < (1ull << 40) && first < (1ull << 40) &&
                   (count == 0 || (d_zones && d_first && n_zones && (n_text == 0 || d_text))) && (cap_rows == 0 || d_rows) &&
                   (cap_pool == 0 || d_pool));
    n_out[0] = n_out[1] = 0;
    DrawArgs a;
    a.at[0] = 0;
    for (int k = 0; k < 3; k++) {
        if (geom_n[k] > ZK_HGVS_TABLE_MAX) return fail(c, ZK_EINVAL, "zk_hgvs_draw: a geometric table of %llu entries, at most %d",
                                                       (unsigned long long)geom_n[k], ZK_HGVS_TABLE_MAX);
        a.at[k + 1] = a.at[k] + geom_n[k];
    }
    if (a.at[3] && !d_geom) return fail(c, ZK_EINVAL, "zk_hgvs_draw: no geometric tables");
    for (int k = 0; k < 7; k++) {
        if (type_thr[k] > (1ull << 32) || (k && type_thr[k] < type_thr[k - 1])) return fail(c, ZK_EINVAL, "zk_hgvs_draw: a threshold above 2^32 or below the one before it");
        a.thr[k] = type_thr[k];
    }
    if (type_thr[6] != (1ull << 32) || mix_thr > (1ull << 32)) return fail(c, ZK_EINVAL, "zk_hgvs_draw: the last type threshold is not 2^32, or the delins threshold is above it");
    arena_reset(c);
    if (count == 0) return ZK_OK;
    a.text = d_text; a.n_text = n_text;
    a.zones = (const u64*)d_zones; a.first = (const u64*)d_first; a.nz = n_zones;
    a.geom = (const u64*)d_geom;
    a.mix_thr = mix_thr;
    a.W = (geom_n[1] + 2 + 31) / 32;
    a.s_type = hg_mix64(seed + HG_T_TYPE); a.s_pos = hg_mix64(seed + HG_T_POS); a.s_len = hg_mix64(seed + HG_T_LEN);
    a.s_ins = hg_mix64(seed + HG_T_INS); a.s_mix = hg_mix64(seed + HG_T_MIX); a.s_bases = hg_mix64(seed + HG_T_BASES);
    a.s_alt = hg_mix64(seed + HG_T_ALT);
    a.v0 = first; a.count = count;
    return hgvs_draw(c, a, (u64*)d_rows, cap_rows, d_pool, cap_pool, n_out);
}

int zk_hgvs_render(zk_ctx* c, const uint64_t* d_rows, uint64_t n_rows, const uint8_t* d_pool, uint64_t n_pool, const uint8_t* d_text,
                   uint64_t n_text, const uint64_t* d_zones, uint64_t n_zones, const uint8_t* d_accs, const uint64_t* d_acc_offs, uint64_t n_accs,
                   const uint8_t* d_names, const uint64_t* d_name_offs, uint64_t n_names, const uint64_t* d_first, uint64_t first, int flags,
                   uint8_t* d_out, uint64_t cap, uint64_t* n_bytes) {
    ZK_ARGS(c, n_bytes && n_rows < (1ull << 40) && first < (1ull << 40) && (flags & ~(ZK_HGVS_TABULAR | ZK_HGVS_HEADERS | ZK_HGVS_DIRECT)) == 0 &&
                   (n_rows == 0 || (d_rows && d_zones && d_acc_offs && n_zones && (n_text == 0 || d_text) && (n_pool == 0 || d_pool) &&
                                    (n_accs == 0 || d_accs))) &&
                   (n_rows == 0 || !(flags & ZK_HGVS_HEADERS) || (d_name_offs && d_first && (n_names == 0 || d_names))) && (cap == 0 || d_out));
    *n_bytes = 0;
    arena_reset(c);
    if (n_rows == 0) return ZK_OK;
    RenderArgs a;
    a.rows = (const u64*)d_rows; a.n = n_rows;
    a.pool = d_pool; a.n_pool = n_pool;
    a.text = d_text; a.n_text = n_text;
    a.zones = (const u64*)d_zones; a.nz = n_zones;
    a.accs = d_accs; a.acc_offs = (const u64*)d_acc_offs; a.n_accs = n_accs;
    a.names = d_names; a.name_offs = (const u64*)d_name_offs; a.n_names = n_names;
    a.first = (const u64*)d_first; a.v0 = first;
    a.flags = (u32)flags;
    return hgvs_render(c, a, d_out, cap, n_bytes);
}

}  // extern "C"
