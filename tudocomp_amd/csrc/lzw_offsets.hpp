// lzw_offsets.hpp -- lzw(coder=bit): code k is written with bits_for(k + 256) bits (Coder.hpp:61-63), a width that depends on k alone, so
// the bit offset S(k) of every code is a closed form and so is its inverse.  Shared by the single call (lzw.hip) and the batch
// (lz_batch.hip) and its decoder (lz_batch_decode.hip).
#pragma once

#include "common.hpp"

namespace tdc {

// bits in front of the first code of width w: sum_{v = 9}^{w - 1} v 2^(v - 1) = (w - 2) 2^(w - 1) - 1792  (256 codes of 9 bits, then
// 2^(v - 1) codes of v bits: code k has width bits_for(k + 256))
__host__ __device__ __forceinline__ u64 lzw_width_base(u32 w) { return ((u64)(w - 2) << (w - 1)) - 1792ull; }
__host__ __device__ __forceinline__ u32 lzw_width(u64 k) { return 64u - (u32)__builtin_clzll(k + 256); }
// S(k): the bit offset of code k
__host__ __device__ __forceinline__ u64 lzw_offset(u64 k) {
    const u32 w = lzw_width(k);
    return lzw_width_base(w) + (k - ((1ull << (w - 1)) - 256)) * w;
}
// the code that holds bit x, and its width (the inverse of S; x < S(2^32))
__host__ __device__ __forceinline__ u64 lzw_code_at(u64 x, u32& w) {
    w = 9;
    while (w < 40 && lzw_width_base(w + 1) <= x) ++w;
    return ((1ull << (w - 1)) - 256) + (x - lzw_width_base(w)) / w;
}

}  // namespace tdc
