// stream_parse.hpp -- the parse that the device decoders of token streams share (lz78_decode.hip and through it lzw.hip,
// lzss_sw_decode.hip, repair_decode.hip); the decode-side twin of field_coder.hpp.  Where a token ends depends on the bits behind its
// first one alone, so next(x) is evaluated for every bit position from an LDS image of the stream, the token starts are the orbit of
// the first token's bit (prim.hip mark_orbit_u32), and the tokens are listed and decoded side by side, segment by segment (option
// dec_seg).
//
// What a token is, is the format's business.  A format hands the parse a Tok, a small POD passed to the kernel by value:
//   static constexpr u32 REACH                                   the most bits a token spans; every peek of at() starts inside them
//   template <class Win> bool at(const Win&, u64 x, u64& end)    does a token start at bit x, and where does it end
// The payload's bit count, payload_bits(), is decode.hpp's: FastBits there is built on it.
#pragma once

#include "../../include/tdc_gpu.h"
#include "decode.hpp"
#include "prim.hpp"

#include <type_traits>

namespace tdc {

// the coders without a table; DEC_BIT fields have widths the format knows, the other two are self-delimiting
constexpr int DEC_BIT = 0, DEC_GAMMA = 1, DEC_DELTA = 2;
inline int dec_kind(int coder) { return coder == TDC_GPU_CODER_BIT ? DEC_BIT : coder == TDC_GPU_CODER_GAMMA ? DEC_GAMMA : DEC_DELTA; }

// f(std::integral_constant<int, kind>): the one place that turns a kind chosen at run time into a template argument
template <class F>
auto with_dec_kind(int kind, F&& f) {
    switch (kind) {
        case DEC_BIT:   return f(std::integral_constant<int, DEC_BIT>{});
        case DEC_GAMMA: return f(std::integral_constant<int, DEC_GAMMA>{});
        default:        return f(std::integral_constant<int, DEC_DELTA>{});
    }
}

#ifdef __HIPCC__
// ---- one gamma / delta field (io/BitIStream.hpp:129-162): b zeros, a one, then the value in b bits (gamma), or gamma(width) and the
// value in `width` bits (delta).  vcap: most value bits; wcap: most value bits of delta's width code.  The callers' caps differ under
// delta: lzss bounds the width code by bits_for(vcap) (6 for a distance or length, 4 for a literal), repair by 6 for both.
constexpr int FIELD_READ = 0, FIELD_END = 1, FIELD_WIDE = 2;      // read | zeros up to the end of the stream | beyond a cap
// the most bits a field that is read takes; every peek of read_field starts inside them
constexpr u32 field_span(int kind, u32 vcap, u32 wcap) { return kind == DEC_DELTA ? 2 * wcap + 1 + vcap : 2 * vcap + 1; }

template <int KIND, typename Win>
__device__ __forceinline__ int read_field(const Win& bw, u64 y, u32 vcap, u32 wcap, u32& used, u32& val) {
    used = 0; val = 0;
    const u64 w = bw.peek(y);
    if (!w) return y + 64 > bw.total ? FIELD_END : FIELD_WIDE;
    u32 b = (u32)__builtin_clzll(w), u = b + 1;
    if (KIND == DEC_DELTA) {
        if (b > wcap) return FIELD_WIDE;
        const u32 width = b ? (u32)((w << (b + 1)) >> (64 - b)) : 0u;
        u += b;
        b = width;
    }
    if (b > vcap) return FIELD_WIDE;
    if (b) val = (u32)(bw.peek(y + u) >> (64 - b));
    used = u + b;
    return FIELD_READ;
}

// ---- next() for the bit positions x_in .. x_in + m - 1 (index = position - x_in); m: the token leaves the segment, or there is none
constexpr u32 STREAM_TILE = 32768;                                // bit positions per LDS image

template <class Tok>
__global__ __launch_bounds__(256) void stream_next_kernel(const Tok tok, const u32* __restrict__ s32, u64 x_in, u32 m, u64 total, u32 tiles,
                                                           u32* __restrict__ next) {
    // Stream words per image.  A tile's first bit lies in word 0, at bit 31 at most, so the last peek starts before bit
    // 31 + STREAM_TILE - 1 + REACH and touches PEEK_WORDS words from there: the + 4 is those three words and one to spare.  The
    // assert states that relation and holds for every REACH as long as NW keeps this form; what keeps the reads in bounds is a REACH
    // that is right -- one that is up to 32 bits too small still reads inside the image, and no test would see it.
    constexpr u32 NW = (STREAM_TILE + Tok::REACH + 31) / 32 + 4;
    static_assert((31 + STREAM_TILE - 1 + Tok::REACH) / 32 + BitWin::PEEK_WORDS <= NW, "a peek would read behind the LDS image");
    __shared__ u32 sw[NW];
    const u64 wmax = (total + 31) / 32 + 3;                       // (the buffer is padded with 64 zero bytes: words up to here exist)
    for (u32 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const u32 i0 = tile * STREAM_TILE;
        const u64 kb = (x_in + i0) >> 5;
        for (u32 j = threadIdx.x; j < NW; j += 256) sw[j] = (kb + j < wmax) ? __builtin_bswap32(s32[kb + j]) : 0u;
        __syncthreads();
        const BitWin bw{sw, kb, total};
        for (u32 i = threadIdx.x; i < STREAM_TILE; i += 256) {
            const u32 idx = i0 + i;
            if (idx >= m) break;
            u64 end;
            u32 r = m;
            if (tok.at(bw, x_in + idx, end)) { const u64 d = end - x_in; r = d < (u64)m ? (u32)d : m; }
            next[idx] = r;
        }
        __syncthreads();
    }
}

// ---- the segment loop from bit x_in on.
//   plan(x_in, m) -> Tok     m arrives as the most bit positions the segment may take; a format that reads a stretch with one width shortens it
//   take(x_in, idx, cnt, e2) -> the bit where the next segment starts.  idx[0 .. cnt): the offsets of the segment's tokens; e2: m + 4
//                            words of scratch.  Decodes the tokens and does the format's own checks; the segment's scratch lives until
//                            it returns.
// bad_chain: what a stream whose chain does not move is refused with.
struct SegCount { u32 segments = 0; u64 evaluated = 0; };         // segments, and the bit positions next() was evaluated for

template <class Plan, class Take>
SegCount parse_segments(Ctx& c, const u32* s32, u64 total, u64 x_in, const char* list_tick, const char* bad_chain, const DecTick& tick,
                        Plan&& plan, Take&& take) {
    hipStream_t s = c.stream;
    const u64 seg_bits = c.dec_seg ? (u64)c.dec_seg : (u64)DEC_SEG;                      // (tests shrink the segments)
    u32* d_cnt = c.arena.get<u32>(2);
    SegCount r;
    while (x_in < total) {
        u64 mm = std::min<u64>(seg_bits, total - x_in);
        const auto tok = plan(x_in, mm);
        const u32 m = (u32)mm;
        const size_t mk = c.arena.mark();
        u32* next = c.arena.get<u32>(m);
        u32* e1 = c.arena.get<u32>(m), *e2 = c.arena.get<u32>((size_t)m + 4);
        u8* mark = c.arena.get<u8>(m);
        const u32 tiles = cdiv(m, STREAM_TILE);
        stream_next_kernel<<<dec_grid((size_t)tiles * 256), 256, 0, s>>>(tok, s32, x_in, m, total, tiles, next);
        LAUNCH_CHECK();
        tick("next() of every bit");
        mark_orbit_u32(c, next, m, mark, e1, e2);
        tick("chain marking");
        u32* idx = e1;                                            // (the exit arrays are free again)
        select_by_class(c, mark, 1, m, nullptr, idx, nullptr, nullptr, d_cnt);
        const u32 cnt = c.read(d_cnt);
        tick(list_tick);
        if (cnt == 0) throw StreamFormatError{bad_chain};
        const u64 x_out = take(x_in, (const u32*)idx, cnt, e2);
        c.arena.release(mk);
        if (x_out <= x_in) throw StreamFormatError{bad_chain};
        r.segments += 1;
        r.evaluated += m;
        x_in = x_out;
    }
    return r;
}
#endif

}  // namespace tdc
