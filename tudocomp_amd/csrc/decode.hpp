// decode.hpp -- pieces of the lcpcomp decoder (decode.hip) that the other device decoders share: the MSB-first bit readers with the
// reference's terminator rule, the device reference resolver behind every parse, the arena's move and the stage log.  The parse of
// the token streams itself (lz78, lzw, lzss, repair) is stream_parse.hpp.
#pragma once
#include "stages.hpp"

#include <algorithm>
#include <functional>
#include <initializer_list>
#include <utility>

namespace tdc {

constexpr size_t DEC_SEG = (size_t)1 << 30; // bit positions per segment of the chain marking (option dec_seg overrides it)

// Workgroups (of 256 threads) of a one-dimensional launch over `items` work-items, for kernels that loop with a grid stride: at most
// DEC_MAX_BLOCKS, so that the dispatch grid (work-items, a 32-bit field) stays below 2^32 for every size the decoders take -- texts of up
// to 2^32 - 2 bytes, factor lists of up to 64 work-items per factor.  Launches that fit keep their one-item-per-thread shape.
constexpr unsigned DEC_MAX_BLOCKS = (1u << 24) - 1;
static_assert((unsigned long long)DEC_MAX_BLOCKS * 256ull < (1ull << 32), "dispatch grid must stay below 2^32 work-items");
inline unsigned dec_grid(size_t items) { return (unsigned)std::min<size_t>((items + 255) / 256, DEC_MAX_BLOCKS); }

// The reference's terminator rule (io/BitIStream.hpp:27-63, :191-193): the low 3 bits of the last byte give the number of valid bits
// of the final data byte (6 and 7 live in an extra byte).  A stream of one byte holds the bits its low three bits announce, whatever
// their number.
inline u64 payload_bits(const u8* in, size_t n) {
    if (n == 0) return 0;
    const unsigned fb = in[n - 1] & 7u;
    if (n == 1) return fb;
    return fb >= 6 ? 8ull * (n - 2) + fb : 8ull * (n - 1) + fb;
}

// MSB-first reader over the reference's bit stream; a one-byte stream that announces 6 or 7 bits is refused
struct FastBits {
    const u8* p;
    size_t nbytes;
    u64 total = 0, pos = 0;
    FastBits(const u8* in, size_t n) : p(in), nbytes(n), total(payload_bits(in, n)) {
        if (n == 1 && total >= 6) throw StreamFormatError{"truncated stream"};
    }
    bool eof() const { return pos >= total; }
    // next 57 bits, left-aligned in the result's top bits (zeros beyond the end, like BitIStream::read_bit at eof)
    u64 peek() const {
        const size_t byte = (size_t)(pos >> 3);
        u64 w = 0;
        if (byte + 8 <= nbytes) { u64 t; memcpy(&t, p + byte, 8); w = __builtin_bswap64(t); }
        else for (size_t i = 0; i < 8; ++i) w = (w << 8) | (byte + i < nbytes ? p[byte + i] : 0);
        w <<= (pos & 7);
        if (pos + 57 > total) {                               // mask the bits behind the end of the stream
            const u64 valid = total > pos ? total - pos : 0;
            w = valid == 0 ? 0 : (w & (~0ull << (64 - valid)));
        }
        return w;
    }
    u64 read(unsigned bits) {                                 // bits <= 57
        if (bits == 0) return 0;
        const u64 v = peek() >> (64 - bits);
        pos += bits;
        return v;
    }
    u64 read_compressed_int() {                               // io/BitIStream.hpp:174-188, 7-bit groups
        u64 v = 0; unsigned i = 0; bool more;
        do { more = read(1) != 0; v |= read(7) << (7 * i++); } while (more && i < 10);
        return v;
    }
};

// 64 stream bits from absolute bit position x on (MSB first), zeros behind `total` (BitIStream reads zeros at eof).  `words` are the
// stream's 32-bit words, byte-swapped so that bit 31 of word k is stream bit 32 k; word index kb is words[0].
struct BitWin {
    static constexpr u32 PEEK_WORDS = 3;                         // a peek at bit x touches the words of bits x .. x + 95 at most
    const u32* words; u64 kb; u64 total;
    __device__ __forceinline__ u64 peek(u64 x) const {
        if (x >= total) return 0ull;
        const u64 k = (x >> 5) - kb;
        const u32 sh = (u32)x & 31u;
        const u64 hi = ((u64)words[k] << 32) | words[k + 1];
        u64 w = sh ? (hi << sh) | (u64)(words[k + 2] >> (32 - sh)) : hi;
        if (x + 64 > total) w &= ~0ull << (64 - (total - x));
        return w;
    }
};
// the same over the stream in global memory (bytes; the buffer is padded with 16 zero bytes)
struct BitWinG {
    const u32* s32; u64 total;
    __device__ __forceinline__ u64 peek(u64 x) const {
        if (x >= total) return 0ull;
        const u64 k = x >> 5;
        const u32 sh = (u32)x & 31u;
        const u32 a = __builtin_bswap32(s32[k]), b = __builtin_bswap32(s32[k + 1]), c = __builtin_bswap32(s32[k + 2]);
        const u64 hi = ((u64)a << 32) | b;
        u64 w = sh ? (hi << sh) | (u64)(c >> (32 - sh)) : hi;
        if (x + 64 > total) w &= ~0ull << (64 - (total - x));
        return w;
    }
};

// where a decoded text of n bytes goes: out.into if set (HipError hipErrorOutOfMemory if n > out.cap), else a buffer allocated here
// (out.owned; the sink frees it unless it is released to the caller)
u8* decode_dest(Sink& o, size_t n);
// Resolves the reference forest of n text positions on the device and downloads the text into decode_dest(out, n).  d_text (n + 64
// bytes) holds the literals at their positions; the factor list (d_pos, d_src, d_len: z entries, length 0 allowed) copies
// text[d_src[i] + j] to d_pos[i] + j, j < d_len[i], every source in front of its target.  d_ref: n entries of scratch, d_changed: one
// word.  st->rounds receives the number of pointer-jumping rounds.  n < 2^32 - 1 (positions and NONE32 share the u32 range).
void resolve_and_download(Ctx& c, size_t n, u8* d_text, u32* d_ref, const u32* d_pos, const u32* d_src, const u32* d_len, size_t z,
                          u32* d_changed, Sink& out, DecodeStats* st);

// option dec_log: the time since the previous call, on stderr under `who` (synchronises the stream); nothing without the option.
// The second form has the caller's own option decide (bwt_log).
using DecTick = std::function<void(const char*)>;
DecTick dec_ticker(Ctx& c, const char* who);
DecTick dec_ticker(Ctx& c, const char* who, bool on);
// The arena is too small for what follows: the live arrays (pointer, bytes) travel to the host and back into an arena of `bytes`;
// the pointers are updated, everything else in the arena is gone.
void regrow_arena(Ctx& c, size_t bytes, std::initializer_list<std::pair<void**, size_t>> live);

// ---- what the LZ78 and the LZW decoder share (lz78_decode.hip) ---------------------------------------------------------------------
// Items of nv self-delimiting gamma codes (2: LZ78's (id, char) pairs, 1: one LZW code) from bit 0 of the uploaded stream s32 (padded
// with 64 zero bytes) to bit `total`, by the segment loop of stream_parse.hpp.  ids[k] (and chars[k], nv == 2) receive item k; item k
// must hold an id <= k + slack.  Returns the number of items.  Malformed input: StreamFormatError; more than zcap items:
// DecodeItemOverflow, before anything is written behind zcap.
struct DecodeItemOverflow { u64 items; };
size_t parse_gamma_items(Ctx& c, const u32* s32, u64 total, int nv, u32 slack, size_t zcap, u32* ids, u8* chars, const DecTick& tick);
// Phrases -> text.  LZ78 (lzw = false): phrase k is phrase ids[k] - 1 (none for 0) followed by chars[k].  LZW: phrase k is the byte
// ids[k] below 256, else phrase ids[k] - 256 and the byte behind it in the text.  Lengths by pointer jumping over the links, starts by
// one 64-bit scan, then the factor list and the literals go to resolve_and_download.  Returns the text length, *need (nullable) as
// decode_lz78_gamma; DecodeTooLarge above 2^32 - 2 bytes before anything of that size is allocated; `who` names the caller where
// out.into is too small.  ids / chars lie in the arena, nothing above them is live.
size_t expand_phrases(Ctx& c, u32* ids, u8* chars, size_t z, bool lzw, const char* who, Sink& out, size_t* need, DecodeStats* st,
                      const DecTick& tick);
// The first stage of expand_phrases alone, for any forest of links that point backwards (the batch of lz_batch_decode.hip: the items of
// many streams with their links rebased): J[k] = NONE32 << 32 | len_k for z >= 1 items, where ids[k] >= base links item k to item
// ids[k] - base (base: 1 for LZ78 ids, 256 for LZW codes) and a smaller value links nowhere.  d_changed: one word.  Returns the number
// of pointer-jumping rounds; it synchronises once per round.
u32 phrase_lengths(Ctx& c, const u32* ids, size_t z, u32 base, u64* J, u32* d_changed);

}  // namespace tdc
