// bitsink.hpp -- writing the reference's MSB-first bit stream (io/BitOStream.hpp) on the device: the length rule of its terminator, the
// atomicOr bit writer, the accumulating sink over it, and the field writers of the four universal coders with their costs.  Every encoder
// (encode.hip, bytestages.hip, field_coder.hpp and the sources of lz78.hip, lzss_sw.hip, repair.hip) takes them from here.
#pragma once

#include "common.hpp"

namespace tdc {

// io/BitOStream.hpp:53-64 -- u = bits used in the last byte; u <= 5: u is ORed into that byte, else one more byte holds it.
inline size_t bit_stream_len(u64 total_bits) { return (size_t)(total_bits >> 3) + ((total_bits & 7) <= 5 ? 1 : 2); }
// what a stream of that length takes of its buffer: the packers write whole 64-bit words, so the bytes up to here are zeroed first
inline size_t bit_stream_padded(size_t len) { return align_up(len + 8, 8); }
// the terminator at bit total_bits of d_out, on c.stream (lz78.hip)
void bit_stream_terminator(Ctx& c, u8* d_out, u64 total_bits);

// what the kernels are instantiated for: a code table or raw literals with fixed-width fields (HuffmanCoder, ArithmeticCoder, BitCoder),
// ASCIICoder, EliasGammaCoder (coders/EliasGammaCoder.hpp:26-29), EliasDeltaCoder (coders/EliasDeltaCoder.hpp:26-29)
constexpr int ENC_TAB = 0, ENC_ASCII = 1, ENC_GAMMA = 2, ENC_DELTA = 3;

#ifdef __HIPCC__
// io/BitOStream.hpp:105-135 -- gamma(v): bits_for(v) zeros, a one, v in bits_for(v) bits; delta(v): gamma(bits_for(v)), then v in
// bits_for(v) bits.  bits_for(0) = 1.  v < 2^31: gamma takes at most 63 bits, delta 11 + 31
__device__ __forceinline__ u32 uni_bits_for(u32 v) { return v ? 32u - (u32)__builtin_clz(v) : 1u; }
template <int KIND> __device__ __forceinline__ u32 uni_cost(u32 v) {
    const u32 b = uni_bits_for(v);
    return KIND == ENC_GAMMA ? 2u * b + 1u : 2u * uni_bits_for(b) + 1u + b;
}

// number of characters ASCIICoder writes for an integer: its decimal digits and the ':'
__device__ __forceinline__ u32 ascii_int_chars(u32 v) {
    u32 d = 1;
    if (v >= 1000000000u) d = 10; else if (v >= 100000000u) d = 9; else if (v >= 10000000u) d = 8; else if (v >= 1000000u) d = 7;
    else if (v >= 100000u) d = 6; else if (v >= 10000u) d = 5; else if (v >= 1000u) d = 4; else if (v >= 100u) d = 3; else if (v >= 10u) d = 2;
    return d + 1;
}

// Append `nbits` (1..64) bits of `val` at absolute bit position `bitpos`; the stream is MSB-first, so the output is
// treated as big-endian 64-bit words.  Different threads own disjoint bit ranges of a zeroed buffer: OR is order-independent.
__device__ __forceinline__ void put_bits(u64* __restrict__ out, u64 bitpos, u64 val, u32 nbits) {
    const u64 w = bitpos >> 6;
    const u32 off = (u32)(bitpos & 63);
    const u32 avail = 64 - off;
    if (nbits <= avail) {
        const u64 x = (nbits == 64) ? val : (val << (avail - nbits));
        atomicOr((unsigned long long*)&out[w], (unsigned long long)__builtin_bswap64(x));
    } else {
        const u32 rem = nbits - avail;
        atomicOr((unsigned long long*)&out[w], (unsigned long long)__builtin_bswap64(val >> rem));
        atomicOr((unsigned long long*)&out[w + 1], (unsigned long long)__builtin_bswap64(val << (64 - rem)));
    }
}

struct BitSink {
    u64* out;
    u64 pos;     // bit position of the first pending bit
    u64 acc;     // pending bits, right-aligned
    u32 cnt;
    __device__ __forceinline__ void flush() {
        if (cnt) { put_bits(out, pos, acc, cnt); pos += cnt; cnt = 0; acc = 0; }
    }
    __device__ __forceinline__ void append(u64 v, u32 nb) {     // v < 2^nb, 0 <= nb <= 64
        if (nb == 0) return;
        if (cnt + nb > 64) flush();
        acc = (nb == 64) ? v : ((acc << nb) | v);
        cnt += nb;
    }
};

// ASCIICoder::Encoder::encode(v, Range) (ASCIICoder.hpp:33-39): decimal digits, most significant first, then ':'
__device__ __forceinline__ void append_ascii_int(BitSink& sink, u32 v) {
    u32 pw = 1000000000u;
    bool started = false;
    for (int i = 0; i < 10; ++i) {
        const u32 d = v / pw;
        if (d || started || pw == 1u) { sink.append('0' + d, 8); started = true; }
        v -= d * pw;
        pw /= 10u;
    }
    sink.append(':', 8);
}

template <int KIND> __device__ __forceinline__ void append_uni(BitSink& sink, u32 v) {
    const u32 b = uni_bits_for(v);
    if (KIND == ENC_GAMMA) sink.append((1ull << b) | v, 2u * b + 1u);                 // b zeros, the one, v: one field of at most 63 bits
    else { const u32 bb = uni_bits_for(b); sink.append((1ull << bb) | b, 2u * bb + 1u); sink.append(v, b); }
}

// The three kinds of field the token and grammar streams are made of (Coder.hpp:61-77 and the coders' overrides), each with its cost:
//   a flag                            one bit; ASCIICoder '0' / '1'
//   a byte under literal_r            8 raw bits; gamma / delta of the byte
//   an integer under a range          `width` bits (BitCoder: bits_for of the range's top); ASCIICoder digits and ':'; gamma / delta of
//                                     the value, the range ignored
template <int KIND> __device__ __forceinline__ u32 flag_cost() { return KIND == ENC_ASCII ? 8u : 1u; }
template <int KIND> __device__ __forceinline__ void append_flag(BitSink& sink, u32 b) {
    if (KIND == ENC_ASCII) sink.append('0' + b, 8); else sink.append(b, 1);
}
template <int KIND> __device__ __forceinline__ u32 byte_cost(u32 ch) { return KIND == ENC_TAB || KIND == ENC_ASCII ? 8u : uni_cost<KIND>(ch); }
template <int KIND> __device__ __forceinline__ void append_byte(BitSink& sink, u32 ch) {
    if (KIND == ENC_TAB || KIND == ENC_ASCII) sink.append(ch, 8); else append_uni<KIND>(sink, ch);
}
template <int KIND> __device__ __forceinline__ u32 int_cost(u32 v, u32 width) {
    return KIND == ENC_TAB ? width : KIND == ENC_ASCII ? 8u * ascii_int_chars(v) : uni_cost<KIND>(v);
}
template <int KIND> __device__ __forceinline__ void append_int(BitSink& sink, u32 v, u32 width) {
    if (KIND == ENC_TAB) sink.append(v, width);
    else if (KIND == ENC_ASCII) append_ascii_int(sink, v);
    else append_uni<KIND>(sink, v);
}
#endif

}  // namespace tdc
