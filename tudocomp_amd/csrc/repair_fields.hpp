// repair_fields.hpp -- a Re-Pair grammar as a source of field_coder.hpp: what repair.hip (one grammar per call) and repair_batch.hip (one
// grammar per text of a batch) put through the four coders.
#pragma once

#include "bitsink.hpp"
#include "field_coder.hpp"

namespace tdc {

constexpr u32 RP_NONE = 0xFFFFFFFFu;

#ifdef __HIPCC__
// ---- a grammar through one coder (RePairCompressor.hpp:208-263): the source of field_coder.hpp -------------------------------------------
// Field 0 is the number of rules under len_r; fields 1 .. 2R are the sides of the rules -- rule i's under Range(i) --, the rest the start
// sequence under Range(R).  A symbol is the flag 0 and the byte under literal_r, or the flag 1 and x - 256 under its range.  BitCoder: 32
// bits for the count, bits_for(i) or bits_for(R) for a rule index -- a function of the field's index alone; gamma / delta ignore the
// ranges; ASCIICoder writes '0' / '1', decimal digits with ':' and the byte.
struct RpFields {
    const u64* __restrict__ rules;
    u32 R;
    const u32* __restrict__ start;
    struct Item { u32 x = 0, hi = 0; };     // hi: the top of the range; RP_NONE: the count
    template <int, bool> __device__ __forceinline__ void load(u64 j, Item& f) const {
        if (j == 0) { f.x = R; f.hi = RP_NONE; }
        else if (j <= 2ull * R) {
            const u32 i = (u32)((j - 1) >> 1);
            const u64 di = rules[i];
            f.x = ((j - 1) & 1) ? (u32)di : (u32)(di >> 32); f.hi = i;
        } else { f.x = start[j - 1 - 2ull * R]; f.hi = R; }
    }
    using Tally = NoTally;
    template <int KIND> __device__ __forceinline__ u32 bits(const Item& f) const {
        if (f.hi == RP_NONE) return int_cost<KIND>(f.x, 32u);
        return flag_cost<KIND>() + (f.x < 256u ? byte_cost<KIND>(f.x) : int_cost<KIND>(f.x - 256u, uni_bits_for(f.hi)));
    }
    template <int KIND> __device__ __forceinline__ void put(BitSink& sink, const Item& f) const {
        if (f.hi == RP_NONE) { append_int<KIND>(sink, f.x, 32u); return; }                   // :212 the number of rules under len_r
        append_flag<KIND>(sink, f.x < 256u ? 0u : 1u);
        if (f.x < 256u) append_byte<KIND>(sink, f.x);                                         // :216-218
        else append_int<KIND>(sink, f.x - 256u, uni_bits_for(f.hi));                          // :219-222
    }
};
#endif

}  // namespace tdc
