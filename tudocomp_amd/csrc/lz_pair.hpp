// lz_pair.hpp -- one item of an lz78 / lzw gamma stream: the (id, char) pair of LZ78Compressor, or the single code of LZWCompressor, as
// EliasGammaCoder::Decoder reads it.  Shared by the parse of one stream (lz78_decode.hip) and the walk of a batch
// (lz_batch_decode.hip), so that the refusal rules stay in one place.
#pragma once

#include "stream_parse.hpp"

namespace tdc {

#ifdef __HIPCC__
constexpr u32 LZD_ID_BITS = 32, LZD_CHAR_BITS = 64;               // most value bits of the id field (a factorid_t) and of the char field

// The pair that starts at bit x (read_elias_gamma<u32>, read_elias_gamma<u8>): 0 and its end, id and char; < 0: no pair there.
// NV == 1: the item is the first code alone.
template <int NV, typename Win>
__device__ __forceinline__ int lz_pair(const Win& bw, u64 x, u64 total, u64& end, u32& id, u32& ch) {
    end = x; ch = 0;
    u32 used;
    if (read_field<DEC_GAMMA>(bw, x, LZD_ID_BITS, 0u, used, id) != FIELD_READ) return -1;     // (zeros up to the end, or wider than a factorid_t)
    const u64 y = x + used;
    if (NV == 1) { end = y; return end > total ? -3 : 0; }
    const u64 v = bw.peek(y);
    u32 b2;
    if (v) b2 = (u32)__builtin_clzll(v);
    else if (bw.peek(y + 64) >> 63) b2 = 64;                      // a sign-extended 64-bit char (the reference's left-over phrase)
    else return -2;
    end = y + 2 * (u64)b2 + 1;
    if (end > total) return -3;                                   // cut off by the end of the stream
    if (b2) { const u32 k = b2 < 8 ? b2 : 8; ch = (u32)(bw.peek(end - k) >> (64 - k)); }     // the low 8 bits of the value
    return 0;
}

// the most bits an item spans; every peek of lz_pair starts inside them
template <int NV> constexpr u32 lz_pair_reach() { return field_span(DEC_GAMMA, LZD_ID_BITS, 0) + (NV == 2 ? 2 * LZD_CHAR_BITS + 1 : 0); }
#endif

}  // namespace tdc
