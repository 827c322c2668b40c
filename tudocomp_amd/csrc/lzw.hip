// lzw.hip -- LZWCompressor (compressors/LZWCompressor.hpp:39-133, lzw/LZWDecoding.hpp:12-99) with BitCoder (coders/BitCoder.hpp) or
// EliasGammaCoder: the coder and the decoder on the device.  The parse is sequential and stays on the host
// (lzw_host.cpp).
//
// coder=bit: code k is written with bits_for(k + 256) bits (Coder.hpp:61-63), a width that depends on k alone, so the bit offset of
// every code is a closed form (lzw_offset) and so is its inverse (lzw_code_at): neither direction needs a cost pass, a scan or a guess.
//   pack:  one thread per 64-bit OUTPUT word gathers the at most 8 codes that touch it -- every word is written once, whole: no zeroed
//          buffer and no atomics (the put_bits / atomicOr scheme of field_coder.hpp was not built: it would add a memset of the output and
//          up to two atomics per code for the same bytes).
//   parse: the payload bit count fixes the number of codes; one thread per code reads its at most two words and validates it.
// coder=gamma: gamma(code) per phrase -- the gamma items of lz78.hip with one value per item, and on the way back the
// next() / orbit parse of lz78_decode.hip with one code per item.
//
// Decoding: dictionary entry 256 + j is phrase j plus the first byte of phrase j + 1, and those bytes are adjacent in the text.  A code
// c >= 256 is therefore the copy (start_k, start_{c - 256}, len_{c - 256} + 1), a code below 256 a literal; KwKwK (c = 255 + k) is the
// same copy overlapping its own first byte.  Lengths by pointer jumping over k -> c_k - 256, starts by one scan, the text by the shared
// reference resolver: expand_phrases() of lz78_decode.hip.  Code k must be <= 255 + k ("invalid compressed code" otherwise, :72-76).
#include "stages.hpp"
#include "bitsink.hpp"
#include "prim.hpp"
#include "decode.hpp"
#include "lzw_offsets.hpp"
#include "../host/tdc_coders.hpp"

#include <stdexcept>
#include <vector>

namespace tdc {

namespace {

// (S(k), its inverse and the widths: lzw_offsets.hpp)

// output word j = stream bits [64 j, 64 j + 64): the codes that touch it, MSB first; zeros behind code z - 1
__global__ __launch_bounds__(256) void lzw_bit_pack_kernel(const u32* __restrict__ codes, u64 z, u64* __restrict__ out, u64 words) {
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 j = (u64)blockIdx.x * 256 + threadIdx.x; j < words; j += stride) {
    const u64 b0 = j * 64;
    u32 w;
    u64 k = lzw_code_at(b0, w);
    u64 s = lzw_width_base(w) + (k - ((1ull << (w - 1)) - 256)) * w;      // S(k) <= b0
    u64 word = 0;
    while (k < z && s < b0 + 64) {
        const int shift = 64 - (int)((long long)(s + w) - (long long)b0);  // of the code's last bit inside this word
        const u64 c = codes[k];
        word |= shift >= 0 ? c << shift : c >> -shift;                      // (bits in front of the word fall off the top)
        s += w; ++k;
        if (k + 256 == (1ull << w)) ++w;
    }
    out[j] = __builtin_bswap64(word);
    }
}

struct LzwScalars { u32 err; u32 pad; };

// code k from its closed-form offset; invalid (c > 255 + k): err, and 0 in its place
__global__ __launch_bounds__(256) void lzw_bit_codes_kernel(const u32* __restrict__ s32, u64 total, u64 z, u32* __restrict__ codes,
                                                             LzwScalars* __restrict__ sc) {
    const BitWinG bw{s32, total};
    const u64 stride = (u64)gridDim.x * 256;
    bool bad = false;
    for (u64 k = (u64)blockIdx.x * 256 + threadIdx.x; k < z; k += stride) {
        const u32 w = lzw_width(k);
        const u64 c = bw.peek(lzw_offset(k)) >> (64 - w);
        const bool late = c > 255 + k;
        codes[k] = late ? 0u : (u32)c;
        bad = bad || late;
    }
    if (__any(bad) && lane_id() == 0) atomicOr(&sc->err, 1u);
}

// the path of small streams (option dec_parse): the host loop of tdc_coders.hpp, which restates lzw::decode_step
struct VecSink { std::vector<u8> v; void put(u8 c) { v.push_back(c); } };
size_t lzw_decode_host(const u8* stream, size_t len, bool bit, Sink& out, size_t* need, DecodeStats* st) {
    VecSink text;
    try { tdc_amd::lzw_decode(stream, len, bit, text); }
    catch (const std::runtime_error&) { throw StreamFormatError{"lzw: corrupt stream (invalid, malformed or cut-off code)"}; }
    catch (const std::length_error&) { throw DecodeTooLarge{0xFFFFFFFFull}; }
    (void)st;
    if (need) *need = text.v.size();
    u8* dst = decode_dest(out, text.v.size());
    if (!text.v.empty()) memcpy(dst, text.v.data(), text.v.size());
    return text.v.size();
}

}  // namespace

size_t lzw_bit_encode(Ctx& c, const u32* d_codes, size_t z, u8* d_out, size_t out_cap) {
    const u64 total_bits = lzw_offset(z);
    const size_t out_len = bit_stream_len(total_bits);
    const size_t padded = bit_stream_padded(out_len);
    if (padded > out_cap) throw HipError{hipErrorOutOfMemory, "lzw: output buffer too small", (int)__LINE__};
    const u64 words = padded / 8;
    lzw_bit_pack_kernel<<<dec_grid(words), 256, 0, c.stream>>>(d_codes, (u64)z, (u64*)d_out, words);
    LAUNCH_CHECK();
    bit_stream_terminator(c, d_out, total_bits);
    HIP_TRY(hipStreamSynchronize(c.stream));
    return out_len;
}

size_t lzw_encode(Ctx& c, const u32* d_codes, size_t z, bool bit, u8* d_out, size_t out_cap) {
    return bit ? lzw_bit_encode(c, d_codes, z, d_out, out_cap) : gamma_encode_items(c, d_codes, nullptr, z, d_out, out_cap);
}

size_t decode_lzw(Ctx& c, const u8* stream, size_t len, bool bit, Sink& out, size_t* need, DecodeStats* st) {
    DecodeStats local;
    if (!st) st = &local;
    *st = DecodeStats();
    const u64 total = FastBits(stream, len).total;                                     // (throws for a cut-off terminator)
    if (total == 0) { decode_dest(out, 0); if (need) *need = 0; return 0; }             // the empty text's stream: no codes
    // option dec_parse: 1 = the device for streams of LZW_DEVICE_MIN bytes and more, 2 = always, 0 = the host loop
    if (!c.dec_parse || (c.dec_parse < 2 && len < LZW_DEVICE_MIN)) return lzw_decode_host(stream, len, bit, out, need, st);
    st->device_parse = 1;
    hipStream_t s = c.stream;
    const DecTick tick = dec_ticker(c, "lzw decode");
    const size_t slack = (size_t)16 << 20;
    const u32* s32 = nullptr;
    auto upload = [&] {
        void* d_stream = c.arena.get<u8>(len + 64);
        HIP_TRY(hipMemcpyAsync(d_stream, stream, len, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync((u8*)d_stream + len, 0, 64, s));
        s32 = (const u32*)d_stream;                                                      // (arena allocations are 256-byte aligned)
        tick("upload");
    };
    u32* codes = nullptr;
    size_t z = 0;
    if (bit) {
        // the codes are as many as fit the payload exactly: S(z) = total (a rest is a code cut off by the end of the stream)
        u32 w;
        const u64 zz = lzw_code_at(total, w);
        if (lzw_offset(zz) != total) throw StreamFormatError{"corrupt stream: cut-off code"};
        if (zz > 0xFFFFFFFEull) throw DecodeTooLarge{zz};                               // (more codes than 2^32 - 2: more bytes)
        z = (size_t)zz;
        c.ensure_arena(len + 64 + z * (4 + 28) + 2 * slack);                            // (z is known: the codes and what expand_phrases takes per code)
        upload();
        codes = c.arena.get<u32>(z);
        LzwScalars* d_sc = (LzwScalars*)c.arena.alloc(sizeof(LzwScalars));
        HIP_TRY(hipMemsetAsync(d_sc, 0, sizeof(LzwScalars), s));
        lzw_bit_codes_kernel<<<std::min<unsigned>(dec_grid(z), 16384u), 256, 0, s>>>(s32, total, (u64)z, codes, d_sc);
        LAUNCH_CHECK();
        const LzwScalars h = c.read(d_sc);
        tick("code decode");
        if (h.err) throw StreamFormatError{"corrupt stream: invalid compressed code"};
    } else {
        // a code an encoder writes takes 3 bits at least; the decoder also reads "1" as the code 0, so a stream may hold up to `total`
        // codes: the arrays are sized for the first and the parse starts over with room for the second where it has to
        const u64 seg_bits = c.dec_seg ? (u64)c.dec_seg : (u64)DEC_SEG;
        const size_t seg = (size_t)std::min<u64>(seg_bits, total);
        u64 zcap = std::min<u64>(total / 3 + 2, 0xFFFFFFFEull);
        for (;;) {
            c.ensure_arena(len + 64 + zcap * 4 + seg * 13 + slack);
            upload();
            codes = c.arena.get<u32>(zcap);
            try { z = parse_gamma_items(c, s32, total, 1, 255, zcap, codes, nullptr, tick); break; }
            catch (const DecodeItemOverflow& e) {
                if (zcap >= 0xFFFFFFFEull) throw DecodeTooLarge{e.items};
                zcap = std::min<u64>(total, 0xFFFFFFFEull);
            }
        }
    }
    st->factors = z;
    return expand_phrases(c, codes, nullptr, z, true, "lzw decode: the caller's buffer is too small for the text", out, need, st, tick);
}

}  // namespace tdc
