// read_window.hpp -- reading k-mer windows straight from text: the lines of a FASTQ record (line_at, seq_line, strip), the
// walk of one wave over a sequence line, 64 windows per step (chunk_window, for_each_chunk, for_each_mate_chunk), and the
// windows one lane cuts on its own (point_window, roll_windows, record_of).
// Users: capture.hip (lookup, record gather, bait windows), strand_bias.hip (key kernel), hgvs_find.hip (capture k-mers),
// pileup.hip (all three), contig_spectra.hip (contig windows), seq_tally.hip (base_code only).
#pragma once
#include "search.hpp"

namespace zk {

__device__ __forceinline__ u32 base_code(u32 ch, u32& ok) {     // A0 C1 G2 T/U3 (either case); ok = in AaCcGgTtUu
    const u32 t = (ch >> 1) & 3u;
    const u32 d = (ch | 0x20u) - 0x61u;
    ok = (d <= 20u) ? ((0x180045u >> d) & 1u) : 0u;
    return t ^ (t >> 1);
}

__device__ __forceinline__ bool is_space(u32 ch) { return ch == ' ' || (ch >= 9 && ch <= 13); }   // what str.strip() strips

__device__ __forceinline__ u64 spread_bits(u32 v) {      // bit i -> bit 2i
    u64 x = v;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}
__device__ __forceinline__ u32 bits_from(u64 lo, u64 hi, int l) {   // bits l .. l+31 of hi:lo
    return l ? (u32)((lo >> l) | (hi << (64 - l))) : (u32)lo;
}

// The window of RK bases that starts at lane l of the 64-byte chunk text[c0, c0 + 64) of a sequence line ending at e
// (bytes at or past e do not count).  Each lane loads one byte of the chunk (and lanes 0-31 one of the next 32); three
// ballots per row turn the codes and validity into bit planes, from which every lane cuts its own 2*RK bits.
// Called by the whole wave (ballots).
__device__ __forceinline__ bool chunk_window(const u8* __restrict__ text, u64 c0, u64 e, int RK, int lane, u64& x) {
    u32 ok1 = 0, ok2 = 0, b1 = 0, b2 = 0;
    if (c0 + lane < e) b1 = base_code(text[c0 + lane], ok1);
    if (lane < 32 && c0 + 64 + lane < e) b2 = base_code(text[c0 + 64 + lane], ok2);
    const u64 lo0 = __ballot(ok1 && (b1 & 1u)), lo1 = __ballot(ok1 && (b1 & 2u)), lov = __ballot(ok1 != 0);
    const u64 hi0 = __ballot(ok2 && (b2 & 1u)), hi1 = __ballot(ok2 && (b2 & 2u)), hiv = __ballot(ok2 != 0);
    const u32 v = bits_from(lov, hiv, lane);
    const u32 need = RK >= 32 ? 0xffffffffu : ((1u << RK) - 1u);
    const u64 z = (spread_bits(__brev(bits_from(lo1, hi1, lane))) << 1) | spread_bits(__brev(bits_from(lo0, hi0, lane)));
    x = z >> (64 - 2 * RK);
    return (v & need) == need;
}

// ---------------------------------------------------------------------------------------
// lines: a text is located through the positions of its '\n' bytes (zk_line_ends); FASTQ record r is lines 4r .. 4r + 3
// ---------------------------------------------------------------------------------------
// line i of the text: [s, e), e at its '\n'
__device__ __forceinline__ void line_at(const u64* __restrict__ lines, u64 i, u64& s, u64& e) {
    s = i ? lines[i - 1] + 1 : 0;
    e = lines[i];
}
// the sequence line of record r (line 4r + 1), RAW: a '\r' or blanks at its ends are in it.  The window kernels of capture,
// strand and hgvs-find read this; the pile-up and the record gather strip() theirs.
__device__ __forceinline__ void seq_line(const u64* __restrict__ lines, u64 r, u64& b, u64& e) {
    b = lines[4 * r] + 1;
    e = lines[4 * r + 1];
}
// [s, e) without the white space at its ends (str.strip())
__device__ __forceinline__ void strip(const u8* __restrict__ text, u64& s, u64& e) {
    while (s < e && is_space(text[s])) s++;
    while (e > s && is_space(text[e - 1])) e--;
}

// ---------------------------------------------------------------------------------------
// the walk: one wave per read, 64 window starts per step
// ---------------------------------------------------------------------------------------
// for (u64 r = w.wave; r < n; r += w.nw): the waves of the grid stride over n items
struct WaveIds { u64 wave, nw; int lane; };
__device__ __forceinline__ WaveIds wave_ids() {
    return WaveIds{((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, ((u64)gridDim.x * blockDim.x) >> 6, (int)(threadIdx.x & 63)};
}

// f(c0, valid, x) for every 64-byte step c0 = b, b + 64, .. of the line text[b, e): lane l holds the window that starts at
// c0 + l (chunk_window).  f returns true to stop the walk, and then so does this.  Called by the whole wave; what f returns
// must be the same in every lane.
template <class F>
__device__ __forceinline__ bool for_each_chunk(const u8* __restrict__ text, u64 b, u64 e, int K, int lane, F f) {
    for (u64 c0 = b; c0 < e; c0 += 64) {
        u64 x;
        const bool valid = chunk_window(text, c0, e, K, lane, x);
        if (f(c0, valid, x)) return true;
    }
    return false;
}
// ... over the raw sequence line of record r in m1 and then, if there is one (m2.text not null), in m2.  M: a FASTQ text and
// the positions of its line ends, { text, lines } (bait_table.hpp's Mate)
template <class M, class F>
__device__ __forceinline__ bool for_each_mate_chunk(const M& m1, const M& m2, u64 r, int K, int lane, F f) {
    const int mates = m2.text ? 2 : 1;
    for (int m = 0; m < mates; m++) {
        const M mt = m ? m2 : m1;
        u64 b, e;
        seq_line(mt.lines, r, b, e);
        if (for_each_chunk(mt.text, b, e, K, lane, f)) return true;
    }
    return false;
}

// ---------------------------------------------------------------------------------------
// one-lane windows
// ---------------------------------------------------------------------------------------
// The window of K bases at stream[pos, pos + K) (n bytes in the stream): x, and xb = its reverse complement.  False where it
// leaves the stream or holds a byte that is no base.
__device__ __forceinline__ bool point_window(const u8* __restrict__ stream, u64 n, int K, u64 pos, u64& x, u64& xb) {
    if (pos + K > n) return false;
    x = 0; xb = 0;
    for (int j = 0; j < K; j++) {
        u32 ok;
        const u32 b = base_code(stream[pos + j], ok);
        if (!ok) return false;
        x = (x << 2) | b;
        xb |= (u64)(3u - b) << (2 * j);
    }
    return true;
}

// The bytes [s, s + n_bytes) of a line rolled through one k-mer register by one lane: f(j, x) for every window j that lies
// whole in them, ascending; f returns true to stop.
template <class F>
__device__ __forceinline__ void roll_windows(const u8* __restrict__ text, u64 s, u64 n_bytes, int K, F f) {
    const u64 mask = K == 32 ? ~0ull : (1ull << (2 * K)) - 1;
    u64 x = 0;
    u32 run = 0;
    for (u64 b = 0; b < n_bytes; b++) {
        u32 ok;
        const u32 code = base_code(text[s + b], ok);
        if (!ok) { run = 0; x = 0; continue; }
        x = ((x << 2) | code) & mask;
        if (++run >= (u32)K && f(b + 1 - (u64)K, x)) return;
    }
}

// the record of a position in a stream of '\n'-terminated records: the number of terminators before it (ends ascending)
__device__ __forceinline__ u32 record_of(const u64* __restrict__ ends, u64 n_ends, u64 pos) {
    return (u32)lower_bound(ends, 0ull, n_ends, pos);
}

}  // namespace zk
