// lz78.hip -- LZ78Compressor (compressors/LZ78Compressor.hpp:64-140) with EliasGammaCoder
// (coders/EliasGammaCoder.hpp:26-29, io/BitOStream.hpp:105-129); BASELINE.json configs[3].
//
// The LZ78 parse is inherently sequential (every step depends on the whole dictionary so far), so it stays on the
// host (option a; lz78_host.cpp).
// The coder side is data-parallel and runs on the GPU: the cost / scan / pack scheme of field_coder.hpp over the items below.
// gamma(v) = bits_for(v) zeros, "1", v in bits_for(v) bits; pair i contributes gamma(id_i) gamma(c_i).
// An item holds one or two values: lzw(coder=gamma) (lzw.hip) writes gamma(code_k) alone.
#include "stages.hpp"
#include "field_coder.hpp"

#include <vector>
#include <stdlib.h>
#include <string.h>

namespace tdc {

// (the LZ78 parse itself: lz78_host.cpp)

// The one terminator of every bit stream (bitsink.hpp).  Here, in a small code object, as before the coders were unified: a file of its
// own moved this file's first-launch load into lzw(coder=gamma)'s first call (profiles/field_coder_ab.txt).
// io/BitOStream.hpp:53-64 : u = bits used in the last byte; u <= 5: OR u into that byte, else append a byte holding u.
__global__ void terminator_kernel(u8* out, u64 total_bits) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const u64 byte = total_bits >> 3;
    const u32 u = (u32)(total_bits & 7);
    if (u <= 5) out[byte] |= (u8)u;
    else out[byte + 1] = (u8)u;
}
void bit_stream_terminator(Ctx& c, u8* d_out, u64 total_bits) {
    terminator_kernel<<<1, 64, 0, c.stream>>>(d_out, total_bits);
    LAUNCH_CHECK();
}

// ---- device: gamma coding of the items -- (id, char) pairs (PAIR), or single values --------------------------------
// The source of field_coder.hpp, for EliasGammaCoder alone.
template <bool PAIR>
struct GammaItems {
    const u32* __restrict__ ids;
    const u8* __restrict__ chars;
    struct Item { u32 id = 0, ch = 0; };
    using Tally = NoTally;
    template <int, bool> __device__ __forceinline__ void load(u64 i, Item& it) const { it.id = ids[i]; if (PAIR) it.ch = chars[i]; }
    template <int> __device__ __forceinline__ u32 bits(const Item& it) const {
        return 2 * uni_bits_for(it.id) + 1 + (PAIR ? 2 * uni_bits_for(it.ch) + 1 : 0);
    }
    // gamma(v): write_unary(bits_for(v)) = b zeros then a one, followed by v in b bits: one field of 2b + 1 bits, or two for an id of 32
    // bits, which the sink could not take as one
    // One value per item: the sink is a cursor with nothing pending -- the one and the value go straight to their place behind the b
    // zeros the cleared buffer already holds, one atomicOr per item and no flush behind a lane-dependent branch (measured: the
    // accumulating form costs lzw(coder=gamma) 10 %, and wins 23 % for pairs, profiles/field_coder_ab.txt).
    template <int> __device__ __forceinline__ void put(BitSink& sink, const Item& it) const {
        const u32 b1 = uni_bits_for(it.id);
        if (!PAIR) { put_bits(sink.out, sink.pos + b1, (1ull << b1) | it.id, b1 + 1); sink.pos += 2 * b1 + 1; return; }
        if (b1 < 32) sink.append((1ull << b1) | it.id, 2 * b1 + 1);
        else { sink.append(0, b1); sink.append((1ull << b1) | it.id, b1 + 1); }
        if (PAIR) append_uni<ENC_GAMMA>(sink, it.ch);
    }
};

// items (device; d_chars == NULL: one value per item) -> gamma bit stream in d_out (zeroed here); returns the stream length in bytes
size_t gamma_encode_items(Ctx& c, const u32* d_ids, const u8* d_chars, size_t z, u8* d_out, size_t out_cap) {
    const char* too_small = "gamma coder: output buffer too small";
    if (d_chars) return encode_fields_as<ENC_GAMMA>(c, GammaItems<true>{ d_ids, d_chars }, (u64)z, d_out, out_cap, too_small);
    return encode_fields_as<ENC_GAMMA>(c, GammaItems<false>{ d_ids, d_chars }, (u64)z, d_out, out_cap, too_small);
}

size_t lz78_gamma_encode(Ctx& c, const u32* d_ids, const u8* d_chars, size_t z, u8* d_out, size_t out_cap) {
    if (!d_chars) throw HipError{hipErrorInvalidValue, "lz78: pairs need their chars", (int)__LINE__};
    return gamma_encode_items(c, d_ids, d_chars, z, d_out, out_cap);
}

}  // namespace tdc
