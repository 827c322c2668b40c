// field_coder.hpp -- a list of items through one coder: bits per tile of 2048 items, the scan of the tile sums, then the pack recomputes
// the costs, scans them inside the workgroup and ORs the fields into the zeroed output; the terminator behind.  For lists whose items'
// widths are not a closed form of their index (lz78.hip, lzss_sw.hip, repair.hip; lzw's BitCoder stream is one, lzw.hip).
//
// What the items are is the source's business.  A source is a small POD passed to the kernels by value:
//   struct Item                                                what the pack keeps of an item between its cost and its fields
//   template <int KIND, bool COST_ONLY> void load(u64 i, Item&) item i, field by field into a zeroed Item (COST_ONLY: what bits() does
//                                                              not read may be left out)
//   template <int KIND> u32 bits(const Item&)                  its cost under coder KIND (ENC_* of bitsink.hpp)
//   template <int KIND> void put(BitSink&, const Item&)        its fields
//   struct Tally                                               what the cost pass gathers besides the bits: note(src, item) per item,
//                                                              commit<KIND>(src) once per thread, all lanes; NoTally gathers nothing
// A thread loads its 8 items with no branch between them -- behind the end of the list the last item again, which is then not counted --,
// so the loads of one item do not wait for those of the item before; a load() without branches on what it has read keeps it that way.
#pragma once

#include "bitsink.hpp"
#include "prim.hpp"

#include <type_traits>

namespace tdc {

#ifdef __HIPCC__
constexpr int FIELD_PER_THREAD = 8, FIELD_TILE = 256 * FIELD_PER_THREAD;

struct NoTally {
    template <class Src, class Item> __device__ __forceinline__ void note(const Src&, const Item&) {}
    template <int KIND, class Src> __device__ __forceinline__ void commit(const Src&) {}
};

template <class Src, int KIND>
__global__ __launch_bounds__(256) void field_tile_bits_kernel(const Src src, u64 nitems, u64* __restrict__ tile_bits) {
    __shared__ u32 sm[4];
    const u64 i0 = (u64)blockIdx.x * FIELD_TILE + (u64)threadIdx.x * FIELD_PER_THREAD;
    typename Src::Item it[FIELD_PER_THREAD];
    typename Src::Tally tally;
    u32 sum = 0;
#pragma unroll
    for (int j = 0; j < FIELD_PER_THREAD; ++j) src.template load<KIND, true>(min(i0 + j, nitems - 1), it[j]);
#pragma unroll
    for (int j = 0; j < FIELD_PER_THREAD; ++j) {
        if (i0 + j < nitems) {
            sum += src.template bits<KIND>(it[j]);
            tally.note(src, it[j]);
        }
    }
    sum = wave_reduce_sum(sum);
    if (lane_id() == 0) sm[wave_id()] = sum;
    __syncthreads();
    if (threadIdx.x == 0) tile_bits[blockIdx.x] = (u64)sm[0] + sm[1] + sm[2] + sm[3];
    tally.template commit<KIND>(src);
}

template <class Src, int KIND>
__global__ __launch_bounds__(256) void field_pack_kernel(const Src src, u64 nitems, const u64* __restrict__ tile_off, u64* __restrict__ out) {
    __shared__ u32 sm[5];
    const u64 i0 = (u64)blockIdx.x * FIELD_TILE + (u64)threadIdx.x * FIELD_PER_THREAD;
    typename Src::Item it[FIELD_PER_THREAD];
    u32 sum = 0;
#pragma unroll
    for (int j = 0; j < FIELD_PER_THREAD; ++j) src.template load<KIND, false>(min(i0 + j, nitems - 1), it[j]);
#pragma unroll
    for (int j = 0; j < FIELD_PER_THREAD; ++j)
        if (i0 + j < nitems) sum += src.template bits<KIND>(it[j]);
    u32 total;
    const u32 excl = block_exclusive_sum<u32, 4>(sum, sm, total);
    BitSink sink;
    sink.out = out;
    sink.pos = tile_off[blockIdx.x] + excl;
    sink.acc = 0;
    sink.cnt = 0;
#pragma unroll
    for (int j = 0; j < FIELD_PER_THREAD; ++j)
        if (i0 + j < nitems) src.template put<KIND>(sink, it[j]);
    sink.flush();
}

// The items of `src` under coder KIND -> the stream in d_out, terminator included; returns its length.  One tile per workgroup:
// nitems < 2^32.  An empty list is the terminator alone (no kernel runs: they take nitems >= 1).  too_small: what is thrown when out_cap
// does not hold the stream.
// after_cost() runs on the host when the cost pass has been read back (not for an empty list), with the source's tally complete: the
// place to read the tally; false -> nothing is written, not even the zeroes, and 0 is returned.
template <int KIND, class Src, class AfterCost = std::true_type>
size_t encode_fields_as(Ctx& c, const Src& src, u64 nitems, u8* d_out, size_t out_cap, const char* too_small, AfterCost after_cost = {}) {
    if (nitems >> 32) throw HipError{hipErrorInvalidValue, "field coder: more items than one tile per workgroup takes", (int)__LINE__};
    hipStream_t s = c.stream;
    const size_t mark = c.arena.mark();
    const unsigned tiles = (unsigned)((nitems + FIELD_TILE - 1) / FIELD_TILE);
    u64 total_bits = 0;
    u64* tile_bits = nullptr;
    if (nitems) {
        tile_bits = c.arena.get<u64>((size_t)tiles + 1);
        field_tile_bits_kernel<Src, KIND><<<tiles, 256, 0, s>>>(src, nitems, tile_bits);
        LAUNCH_CHECK();
        exclusive_sum_u64(c, tile_bits, tile_bits, tiles, tile_bits + tiles);
        total_bits = c.read(tile_bits + tiles);
        if (!after_cost()) { c.arena.release(mark); return 0; }
    }
    const size_t out_len = bit_stream_len(total_bits);
    const size_t padded = bit_stream_padded(out_len);
    if (padded > out_cap) throw HipError{hipErrorOutOfMemory, too_small, (int)__LINE__};
    HIP_TRY(hipMemsetAsync(d_out, 0, padded, s));
    if (nitems) {
        field_pack_kernel<Src, KIND><<<tiles, 256, 0, s>>>(src, nitems, tile_bits, (u64*)d_out);
        LAUNCH_CHECK();
    }
    bit_stream_terminator(c, d_out, total_bits);
    HIP_TRY(hipStreamSynchronize(s));
    c.arena.release(mark);
    return out_len;
}

// the same for a coder chosen at run time (kind = ENC_*): the one place that turns a kind into a template argument
template <class Src, class AfterCost = std::true_type>
size_t encode_fields(Ctx& c, const Src& src, u64 nitems, int kind, u8* d_out, size_t out_cap, const char* too_small, AfterCost after_cost = {}) {
    switch (kind) {
        case ENC_TAB:   return encode_fields_as<ENC_TAB>(c, src, nitems, d_out, out_cap, too_small, after_cost);
        case ENC_ASCII: return encode_fields_as<ENC_ASCII>(c, src, nitems, d_out, out_cap, too_small, after_cost);
        case ENC_GAMMA: return encode_fields_as<ENC_GAMMA>(c, src, nitems, d_out, out_cap, too_small, after_cost);
        default:        return encode_fields_as<ENC_DELTA>(c, src, nitems, d_out, out_cap, too_small, after_cost);
    }
}
#endif

}  // namespace tdc
