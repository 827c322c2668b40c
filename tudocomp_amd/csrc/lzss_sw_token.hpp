// lzss_sw_token.hpp -- one token of an lzss stream under the coders bit, gamma and delta, as the device decoders read it
// (lzss_sw_decode.hip: every bit position of one stream side by side; lzss_sw_batch.hip: one wave per stream, token after token).  The
// refusal rules of a token are here and nowhere else.
//
// Device caps (gamma / delta): a distance or length field of at most 32 value bits, a literal code of at most 8.  A wider field is no
// token here, although the host loop reads it -- no encoder writes one.
#pragma once

#include "stream_parse.hpp"

namespace tdc {

#ifdef __HIPCC__
// the device caps: most value bits of a distance or length and of a literal code, and of delta's width code in front of each (bits_for
// of the former)
constexpr u32 SWD_FIELD_BITS = 32, SWD_FIELD_WBITS = 6, SWD_LIT_BITS = 8, SWD_LIT_WBITS = 4;
// the most bits a token spans; every peek of swd_token starts inside them
constexpr u32 swd_reach(int kind) { return 1 + (kind == DEC_BIT ? 32 + 32 : 2 * field_span(kind, SWD_FIELD_BITS, SWD_FIELD_WBITS)); }

// The token that starts at bit x: 0 and its end, kind, distance, length or byte; < 0: no token (malformed, beyond a cap, or cut off by
// the end of the stream).  k = bits_for(text position), lb = bits_for(window): the widths of the two fields of a factor under bit.
template <int KIND, typename Win>
__device__ __forceinline__ int swd_token(const Win& bw, u64 x, u64 total, u32 k, u32 lb, u64& end, u32& fac, u32& dist, u32& val) {
    end = x; fac = 0; dist = 0; val = 0;
    if (x >= total) return -1;
    const u64 w = bw.peek(x);
    fac = (u32)(w >> 63);
    u64 y = x + 1;
    u32 u;
    if (KIND == DEC_BIT) {
        if (!fac) { val = (u32)((w << 1) >> 56); y += 8; }
        else {
            dist = (u32)(bw.peek(y) >> (64 - k)); y += k;
            val = (u32)(bw.peek(y) >> (64 - lb)); y += lb;
        }
    } else if (!fac) {
        if (read_field<KIND>(bw, y, SWD_LIT_BITS, SWD_LIT_WBITS, u, val) != FIELD_READ) return -2;
        y += u;
    } else {
        if (read_field<KIND>(bw, y, SWD_FIELD_BITS, SWD_FIELD_WBITS, u, dist) != FIELD_READ) return -2;
        y += u;
        if (read_field<KIND>(bw, y, SWD_FIELD_BITS, SWD_FIELD_WBITS, u, val) != FIELD_READ) return -2;
        y += u;
    }
    if (y > total) return -3;
    end = y;
    return 0;
}
#endif

}  // namespace tdc
