// read_window.hpp -- the windows of a sequence line cut straight from FASTQ text, 64 per wave and step (capture.hip's lookup
// and strand_bias.hip's key kernel read the text the same way).
#pragma once
#include "common.hpp"

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

}  // namespace zk
