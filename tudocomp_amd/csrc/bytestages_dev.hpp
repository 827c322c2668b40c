// bytestages_dev.hpp -- device helpers that the byte stages of the single call (bytestages.hip) and of the batch call
// (bytestages_batch.hip) share: rle's vbyte and unit head rule, mtf's summary rows.
#pragma once
#include "common.hpp"

namespace tdc {
namespace {

__host__ __device__ inline u32 vbyte_len(u64 v) { u32 l = 1; while (v >= 128) { v >>= 7; ++l; } return l; }
// util/vbyte.hpp:28-37: seven bits per byte, least significant group first, bit 7 set on every byte but the last
__device__ __forceinline__ u8* put_vbyte(u8* p, u64 v) {
    while (v >= 128) { *p++ = (u8)(0x80u | (v & 0x7Fu)); v >>= 7; }
    *p++ = (u8)v;
    return p;
}

// s[0] = the byte in front of `base`, s[1 .. 16] = the 16 bytes from `base` on (0 behind the input; the buffer has 16 bytes of slack)
__device__ __forceinline__ void load16_prev(const u8* __restrict__ in, size_t n, size_t base, u32 (&s)[17]) {
    s[0] = base > 0 && base <= n ? in[base - 1] : 0u;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (base < n) v = *(const uint4*)(in + base);
    const u32 x[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
    for (int j = 0; j < 16; ++j) s[j + 1] = (x[j >> 2] >> (8 * (j & 3))) & 255u;
}

// a unit starts at the first position, where the byte changes, and at every byte from 0x80 up
__device__ __forceinline__ bool rle_head(size_t i, u32 c, u32 prev) { return i == 0 || c != prev || c >= 0x80u; }

struct Mask256 {
    u64 m0 = 0, m1 = 0, m2 = 0, m3 = 0;
    __device__ __forceinline__ bool test_set(u32 ch) {           // true: ch was in the set already
        const u64 bit = 1ull << (ch & 63u);
        const u32 q = ch >> 6;
        const u64 cur = q == 0 ? m0 : q == 1 ? m1 : q == 2 ? m2 : m3;
        if (cur & bit) return true;
        m0 |= q == 0 ? bit : 0ull; m1 |= q == 1 ? bit : 0ull; m2 |= q == 2 ? bit : 0ull; m3 |= q == 3 ? bit : 0ull;
        return false;
    }
};
// a row = 256 bytes (64 words) of HBM: a summary (its length travels in a count array) or a complete list
struct RowWriter {
    u32* dst; u32 n = 0, acc = 0;
    __device__ __forceinline__ void push(u32 ch) {
        acc |= ch << (8 * (n & 3u));
        if ((++n & 3u) == 0) { dst[(n >> 2) - 1] = acc; acc = 0; }
    }
    __device__ __forceinline__ void finish() { if (n & 3u) dst[n >> 2] = acc; }
};
// row bytes [0, cnt) in order: those not yet in `m` go to `w`
__device__ __forceinline__ void append_new(const u32* row, u32 cnt, Mask256& m, RowWriter& w) {
    for (u32 q = 0; q * 4 < cnt; ++q) {
        const u32 x = row[q];
#pragma unroll
        for (u32 b = 0; b < 4; ++b) {
            const u32 ch = (x >> (8 * b)) & 255u;
            if (q * 4 + b < cnt && !m.test_set(ch)) w.push(ch);
        }
    }
}

}  // namespace
}  // namespace tdc
