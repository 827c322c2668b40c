// bwt_passes.hpp -- what the inverse transform of one buffer (bwt.hip) and of a batch of buffers (bwt_batch.hip) share: the hashed sampling
// of list heads, the head table and the pointer jumping over it.  The passes do not care whose rows they visit: a head table over the
// rows of many buffers laid back to back is a forest of lists, ranked in the same rounds.
// The kernels live in an unnamed namespace: every file that includes this header gets its own.
#pragma once
#include "stages.hpp"
#include "prim.hpp"

namespace tdc {

namespace {

// Row i is a list head iff mix(i) < T, and mix(i) is then its slot in the head table: a bijection of [0, 2^m) (2^m >= n) with mix(0) = 0,
// so row 0 always is one, nothing is enumerated and a walk that meets a head knows its slot.  Multiples of S would be periodic in row space.
struct Mix { u32 mask, h, T, inv_a, inv_b; };
constexpr u32 MIX_A = 0x9E3779B1u, MIX_B = 0x85EBCA6Bu;
__device__ __forceinline__ u32 mix(u32 i, const Mix& m) {
    u32 x = (i * MIX_A) & m.mask;
    x ^= x >> m.h;
    x = (x * MIX_B) & m.mask;
    return x ^ (x >> m.h);
}
__device__ __forceinline__ u32 unmix(u32 k, const Mix& m) {       // (2 h >= m: the fold is its own inverse)
    u32 x = k ^ (k >> m.h);
    x = (x * m.inv_b) & m.mask;
    x ^= x >> m.h;
    return (x * m.inv_a) & m.mask;
}
inline u32 inv_odd(u32 a) { u32 x = a; for (int i = 0; i < 6; ++i) x *= 2u - a * x; return x; }
// the sampling of n rows with one head per `sample` rows on average
inline Mix make_mix(size_t n, u32 sample) {
    Mix mx;
    const u32 mbits = (u32)bits_for(n - 1);                  // 1 .. 31
    mx.mask = (u32)((1ull << mbits) - 1); mx.h = (mbits + 1) / 2;
    mx.T = (u32)((((u64)1 << mbits) + sample - 1) / sample);
    mx.inv_a = inv_odd(MIX_A); mx.inv_b = inv_odd(MIX_B);
    return mx;
}

// head table: hrow[k] = first row of the list of slot k (NONE32: the slot has no list), hlen[k] = rows in it,
// w[k] = link << 32 | length: the slot the list runs into (NONE32: it ends its cycle) and the rows up to there
constexpr u64 W_END = (u64)NONE32 << 32;
struct Heads { u32* hrow; u32* hlen; unsigned long long* w; u32* cnt; /* [0] slots in use, [1] longest list, [2] overflow, [3] changed */ u32 cap; };

// Pointer jumping over the heads, in place: w[k] = (l, d) says "d rows from the head of k up to the head of l"; whatever state w[l] is
// read in, (l', d + d') says the same of l'.  The words are read and written whole.
__global__ void __launch_bounds__(256) bwt_jump_kernel(Heads H, u32 slots) {
    bool changed = false;
    for (u64 kk = (u64)blockIdx.x * 256 + threadIdx.x; kk < slots; kk += (u64)gridDim.x * 256) {
        const u32 k = (u32)kk;
        const u64 a = __hip_atomic_load(&H.w[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const u32 l = (u32)(a >> 32);
        if (l == NONE32) continue;
        const u64 b = __hip_atomic_load(&H.w[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&H.w[k], (unsigned long long)((b & W_END) | (u32)((u32)a + (u32)b)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        changed = true;
    }
    if (__any(changed) && lane_id() == 0) H.cnt[3] = 1u;
}

__device__ __forceinline__ void put_bytes(u8* out, size_t word, u32 acc, u32 lo, u32 hi) {      // byte lanes lo .. hi of the word at `word`
    if (lo == 0 && hi == 3) { *(u32*)(out + word) = acc; return; }
    for (u32 l = lo; l <= hi; ++l) out[word + l] = (u8)(acc >> (8 * l));
}

}  // namespace

}  // namespace tdc
