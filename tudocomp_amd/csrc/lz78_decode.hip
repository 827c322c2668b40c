// lz78_decode.hip -- LZ78Compressor::decompress (compressors/LZ78Compressor.hpp:142-160, lz78::Decompressor :16-37) with
// EliasGammaCoder::Decoder (coders/EliasGammaCoder.hpp:31-42: io/BitIStream.hpp:129-156 read_unary + read_int), on the device.
//
// The stream is a sequence of pairs gamma(id_k) gamma(c_k), gamma(v) = b zeros, a one, then v in b bits.  Every gamma
// code is self-delimiting, so "where does the pair that starts at bit x end" depends on the bits behind x alone: next(x) is
// evaluated for every bit position, the pair starts are the orbit of position 0 under next() (prim.hip mark_orbit_u32, the general
// marking of the lcpcomp parse in decode.hip), and the pairs are decoded side by side.  Streams of more bit positions than one segment
// (2^30, option dec_seg) take several segments; the exit of one is the entry of the next.  The next() kernel, the segment loop and
// the gamma reader are stream_parse.hpp's; lz_pair is the format.
//
// Phrase k is phrase id_k (1-based, 0 = the empty phrase) followed by c_k, so len_k = 1 + len_{id_k - 1} (1 for id_k = 0).  Ids point
// backwards: pointer jumping over the parent links gives every length in O(log depth) rounds, a 64-bit exclusive scan gives every
// phrase's text position start_k.  Phrase k is then the factor (start_k, start_{id_k - 1}, len_k - 1) plus the literal c_k at
// start_k + len_k - 1 -- exactly what decode.hip's reference resolver (resolve_and_download) takes.
//
// Semantics of the reference decoder: the id field is read as a factorid_t (u32), the char field as a uliteral_t (its low 8 bits: a
// sign-extended 64-bit left-over char decodes to its byte), pairs are read until the stream ends.  Rejected (StreamFormatError): a
// pair cut off by the end of the stream (the reference loops forever on a cut-off unary code), an id field of more than 32 bits, a
// char field of more than 64 bits (no encoder writes one; it bounds the work of a candidate), and id_k > k (a phrase that does not
// exist yet).  A decoded length above 2^32 - 2 throws DecodeTooLarge before anything of the text's size is allocated.
//
// lzw streams (lzw.hip) are the same two problems with other constants, so both halves are shared (decode.hpp):
// parse_gamma_items() parses items of one gamma code as well as pairs, expand_phrases() takes the LZW link rule (code - 256, a literal
// below that) beside the LZ78 one.
#include "stages.hpp"
#include "prim.hpp"
#include "stream_parse.hpp"
#include "lz_pair.hpp"

namespace tdc {

namespace {

#ifndef TDC_LZD_HOPS
#define TDC_LZD_HOPS 16
#endif

// (the item reader lz_pair<NV>: lz_pair.hpp)

// what stream_next_kernel asks (stream_parse.hpp)
template <int NV>
struct LzTok {
    static constexpr u32 REACH = lz_pair_reach<NV>();
    template <typename Win>
    __device__ __forceinline__ bool at(const Win& bw, u64 x, u64& end) const {
        u32 id, ch;
        return lz_pair<NV>(bw, x, bw.total, end, id, ch) == 0;
    }
};

struct LzScalars { u64 exit_bit; u32 err; u32 pad; };

// the pairs of a segment (offsets idx[0 .. cnt)), global pair index k0 + j: id, char, validation (id <= k + slack: 0 for LZ78, where
// id k is the newest phrase; 255 for LZW, whose code 256 + j names phrase j); the last one reports the exit
template <int NV>
__global__ __launch_bounds__(256) void lz_pairs_kernel(const u32* __restrict__ s32, u64 x_in, const u32* __restrict__ idx, u32 cnt, u64 total,
                                                        u64 k0, u32 slack, u32* __restrict__ ids, u8* __restrict__ chars,
                                                        LzScalars* __restrict__ sc) {
    const BitWinG bw{s32, total};
    for (u32 j = blockIdx.x * 256 + threadIdx.x; j < cnt; j += gridDim.x * 256) {
        const u64 x = x_in + idx[j];
        const u64 k = k0 + j;
        u64 end; u32 id, ch;
        const int st = lz_pair<NV>(bw, x, total, end, id, ch);
        const bool late = (u64)id > k + slack;
        if (st < 0) atomicOr(&sc->err, 1u);
        else if (late) atomicOr(&sc->err, 2u);
        ids[k] = (st < 0 || late) ? 0u : id;
        if (NV == 2) chars[k] = (u8)ch;
        if (j == cnt - 1) sc->exit_bit = end;
    }
}

// J[k] = (link << 32) | acc: len_k = acc + len(link), link = NONE32 once acc is the length
// (the per-phrase kernels loop with a grid stride: up to 2^32 - 2 phrases, launched with dec_grid())
// base: the value that names phrase 0 -- 1 for LZ78 ids, 256 for LZW codes; smaller values link nowhere
__global__ void lz_link_kernel(const u32* __restrict__ ids, size_t z, u32 base, u64* __restrict__ J) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < z; k += stride) {
        const u32 id = ids[k];
        J[k] = ((u64)(id >= base ? id - base : NONE32) << 32) | 1ull;
    }
}

// one round of in-place pointer jumping over the links, up to HOPS of them per phrase.  Every (link, acc) word a thread can read is
// a valid statement about its phrase (the words are read and written whole), so unsynchronised rounds are safe, as in decode.hip.
__global__ __launch_bounds__(256) void lz_len_jump_kernel(u64* J, size_t z, u32* __restrict__ changed) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    bool any = false;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < z; k += stride) {
        const u64 v = __hip_atomic_load(J + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        u32 t = (u32)(v >> 32);
        if (t == NONE32) continue;
        u32 acc = (u32)v;
        bool open = true;
#pragma unroll
        for (int h = 0; h < TDC_LZD_HOPS; ++h) {
            const u64 w = __hip_atomic_load(J + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            acc += (u32)w;
            t = (u32)(w >> 32);
            if (t == NONE32) { open = false; break; }
        }
        __hip_atomic_store(J + k, ((u64)t << 32) | acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        any = any || open;
    }
    if (__any(any) && lane_id() == 0) atomicOr(changed, 1u);
}

__global__ void lz_len_kernel(const u64* __restrict__ J, size_t z, u64* __restrict__ L) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < z; k += stride) L[k] = (u32)J[k];
}

// phrase k -> factor (start_k, start_{id_k - 1}, len_k - 1); S = the phrase starts (n <= 2^32 - 2: they fit 32 bits)
// LZW: code c >= 256 -> the factor (start_k, start_{c - 256}, len_k), one byte longer than its source phrase (a KwKwK code overlaps its
// own first byte); a literal code is a factor of length 0
template <bool LZW>
__global__ void lz_factor_kernel(const u32* __restrict__ ids, const u64* __restrict__ J, const u64* __restrict__ S, size_t z,
                                 u32* __restrict__ fpos, u32* __restrict__ fsrc, u32* __restrict__ flen) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < z; k += stride) {
        const u32 id = ids[k];
        fpos[k] = (u32)S[k];
        if (LZW) {
            fsrc[k] = id >= 256u ? (u32)S[id - 256u] : 0u;
            flen[k] = id >= 256u ? (u32)J[k] : 0u;
        } else {
            fsrc[k] = id ? (u32)S[id - 1] : 0u;
            flen[k] = (u32)J[k] - 1u;
        }
    }
}

// the literal of phrase k at its last text position
__global__ void lz_literal_kernel(const u32* __restrict__ fpos, const u32* __restrict__ flen, const u8* __restrict__ chars, size_t z,
                                  u8* __restrict__ text) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < z; k += stride) text[(size_t)fpos[k] + flen[k]] = chars[k];
}
// LZW: a code below 256 is its byte
__global__ void lzw_literal_kernel(const u32* __restrict__ fpos, const u32* __restrict__ codes, size_t z, u8* __restrict__ text) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < z; k += stride)
        if (codes[k] < 256u) text[fpos[k]] = (u8)codes[k];
}

template <int NV>
size_t parse_items(Ctx& c, const u32* s32, u64 total, u32 slack, size_t zcap, u32* ids, u8* chars, const DecTick& tick) {
    constexpr bool PAIR = NV == 2;
    hipStream_t s = c.stream;
    LzScalars* d_sc = (LzScalars*)c.arena.alloc(sizeof(LzScalars));
    HIP_TRY(hipMemsetAsync(d_sc, 0, sizeof(LzScalars), s));
    size_t z = 0;
    parse_segments(c, s32, total, 0, PAIR ? "pair list" : "code list", PAIR ? "corrupt stream: pair chain" : "corrupt stream: code chain", tick,
        [](u64, u64&) { return LzTok<NV>{}; },
        [&](u64 x_in, const u32* idx, u32 cnt, u32*) {
            if (z + cnt > zcap) throw DecodeItemOverflow{z + cnt};
            const unsigned g = std::min<u32>(cdiv(cnt, 256), 4096u);
            lz_pairs_kernel<NV><<<g, 256, 0, s>>>(s32, x_in, idx, cnt, total, (u64)z, slack, ids, chars, d_sc);
            LAUNCH_CHECK();
            const LzScalars h = c.read(d_sc);
            tick(PAIR ? "pair decode" : "code decode");
            z += cnt;
            if (h.err & 1u) throw StreamFormatError{PAIR ? "corrupt stream: malformed or cut-off pair" : "corrupt stream: malformed or cut-off code"};
            if (h.err & 2u) throw StreamFormatError{PAIR ? "corrupt stream: phrase id out of range" : "corrupt stream: invalid compressed code"};
            return h.exit_bit;
        });
    return z;
}

}  // namespace

size_t parse_gamma_items(Ctx& c, const u32* s32, u64 total, int nv, u32 slack, size_t zcap, u32* ids, u8* chars, const DecTick& tick) {
    return nv == 2 ? parse_items<2>(c, s32, total, slack, zcap, ids, chars, tick) : parse_items<1>(c, s32, total, slack, zcap, ids, chars, tick);
}

u32 phrase_lengths(Ctx& c, const u32* ids, size_t z, u32 base, u64* J, u32* d_changed) {
    hipStream_t s = c.stream;
    lz_link_kernel<<<dec_grid(z), 256, 0, s>>>(ids, z, base, J);
    LAUNCH_CHECK();
    unsigned g = cdiv(z, 256 * 8); if (g > 16384) g = 16384;
    u32 len_rounds = 0;
    for (u32 round = 0;; ++round) {
        if (round > 40) throw HipError{hipErrorUnknown, "phrase lengths did not converge", (int)__LINE__};   // depth < 2^32
        HIP_TRY(hipMemsetAsync(d_changed, 0, sizeof(u32), s));
        lz_len_jump_kernel<<<g, 256, 0, s>>>(J, z, d_changed);
        LAUNCH_CHECK();
        len_rounds = round + 1;
        if (c.read(d_changed) == 0) break;
    }
    return len_rounds;
}

size_t expand_phrases(Ctx& c, u32* ids, u8* chars, size_t z, bool lzw, const char* who, Sink& out, size_t* need, DecodeStats* st,
                      const DecTick& tick) {
    hipStream_t s = c.stream;
    const size_t slack = (size_t)16 << 20;
    const size_t zc = lzw ? 0 : z;                                                      // bytes of chars[] that live on
    u32* d_cnt = c.arena.get<u32>(2);
    // ---- phrase lengths (pointer jumping), starts (64-bit scan), factor list
    {
        const size_t need1 = c.arena.mark() + z * 28 + slack;
        if (c.arena.size < need1) {
            void* pi = ids; void* pc = chars;
            regrow_arena(c, need1, {{&pi, z * 4}, {&pc, zc}});
            ids = (u32*)pi; chars = (u8*)pc;
            d_cnt = c.arena.get<u32>(2);
        }
    }
    u32* fpos = c.arena.get<u32>(z), *fsrc = c.arena.get<u32>(z), *flen = c.arena.get<u32>(z);
    const size_t mkB = c.arena.mark();
    u64* J = c.arena.get<u64>(z);
    u64* S = c.arena.get<u64>(z);
    u64* d_total = c.arena.get<u64>(1);
    const u32 len_rounds = phrase_lengths(c, ids, z, lzw ? 256u : 1u, J, d_cnt);
    lz_len_kernel<<<dec_grid(z), 256, 0, s>>>(J, z, S);
    LAUNCH_CHECK();
    exclusive_sum_u64(c, S, S, z, d_total);
    const u64 n = c.read(d_total);
    tick("phrase lengths + starts");
    if (need) *need = (size_t)n;
    if (n > 0xFFFFFFFEull) throw DecodeTooLarge{n};                                     // checked before any text-sized allocation
    if (out.into && n > out.cap) throw HipError{hipErrorOutOfMemory, who, (int)__LINE__};
    if (lzw) lz_factor_kernel<true><<<dec_grid(z), 256, 0, s>>>(ids, J, S, z, fpos, fsrc, flen);
    else lz_factor_kernel<false><<<dec_grid(z), 256, 0, s>>>(ids, J, S, z, fpos, fsrc, flen);
    LAUNCH_CHECK();
    c.arena.release(mkB);
    tick("factor list");

    // ---- text: literals, then the shared reference resolver
    {
        const size_t need2 = c.arena.mark() + (size_t)n * 5 + (size_t)n / 8 + slack;
        if (c.arena.size < need2) {
            void* pp = fpos; void* ps = fsrc; void* pl = flen; void* pc = chars; void* pi = ids;
            regrow_arena(c, need2, {{&pp, z * 4}, {&ps, z * 4}, {&pl, z * 4}, {&pc, zc}, {&pi, lzw ? z * 4 : 0}});
            fpos = (u32*)pp; fsrc = (u32*)ps; flen = (u32*)pl; chars = (u8*)pc; ids = (u32*)pi;
            d_cnt = c.arena.get<u32>(2);
        }
    }
    u8* d_text = c.arena.get<u8>((size_t)n + 64);
    u32* d_ref = c.arena.get<u32>((size_t)n);
    if (lzw) lzw_literal_kernel<<<dec_grid(z), 256, 0, s>>>(fpos, ids, z, d_text);
    else lz_literal_kernel<<<dec_grid(z), 256, 0, s>>>(fpos, flen, chars, z, d_text);
    LAUNCH_CHECK();
    tick("literals");
    resolve_and_download(c, (size_t)n, d_text, d_ref, fpos, fsrc, flen, z, d_cnt, out, st);
    st->rounds += len_rounds;
    tick("references + download");
    return (size_t)n;
}

size_t decode_lz78_gamma(Ctx& c, const u8* stream, size_t len, Sink& out, size_t* need, DecodeStats* st) {
    DecodeStats local;
    if (!st) st = &local;
    *st = DecodeStats();
    const u64 total = FastBits(stream, len).total;                                     // (throws for a cut-off terminator)
    if (total == 0) { decode_dest(out, 0); if (need) *need = 0; return 0; }             // the empty text's stream: no pairs
    hipStream_t s = c.stream;
    const DecTick tick = dec_ticker(c, "lz78 decode");
    // a pair takes 2 bits at least ("1" "1": id 0, char 0), and more than 2^32 - 2 pairs decode to more than 2^32 - 2 bytes
    const u64 zcap = std::min<u64>(total / 2 + 1, 0xFFFFFFFEull);
    const u64 seg_bits = c.dec_seg ? (u64)c.dec_seg : (u64)DEC_SEG;
    const size_t seg = (size_t)std::min<u64>(seg_bits, total);
    const size_t slack = (size_t)16 << 20;
    c.ensure_arena(len + 64 + zcap * 5 + seg * 13 + slack);
    void* d_stream = c.arena.get<u8>(len + 64);
    u32* ids = c.arena.get<u32>(zcap);
    u8* chars = c.arena.get<u8>(zcap + 64);
    HIP_TRY(hipMemcpyAsync(d_stream, stream, len, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync((u8*)d_stream + len, 0, 64, s));
    tick("upload");
    size_t z;
    try { z = parse_gamma_items(c, (const u32*)d_stream, total, 2, 0, zcap, ids, chars, tick); }    // (arena allocations are 256-byte aligned)
    catch (const DecodeItemOverflow& e) { throw DecodeTooLarge{e.items}; }              // (more pairs than 2^32 - 2: more bytes)
    st->factors = z;
    return expand_phrases(c, ids, chars, z, false, "lz78 decode: the caller's buffer is too small for the text", out, need, st, tick);
}

}  // namespace tdc
