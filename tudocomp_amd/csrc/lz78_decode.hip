// lz78_decode.hip -- LZ78Compressor::decompress (compressors/LZ78Compressor.hpp:142-160, lz78::Decompressor :16-37) with
// EliasGammaCoder::Decoder (coders/EliasGammaCoder.hpp:31-42: io/BitIStream.hpp:129-156 read_unary + read_int), on the device.
//
// The stream is a sequence of pairs gamma(id_k) gamma(c_k), gamma(v) = b zeros, a one, then v in b bits.  Every gamma
// code is self-delimiting, so "where does the pair that starts at bit x end" depends on the bits behind x alone: next(x) is
// evaluated for every bit position, the pair starts are the orbit of position 0 under next() (prim.hip mark_orbit_u32, the general
// marking of the lcpcomp parse in decode.hip), and the pairs are decoded side by side.  Streams of more bit positions than one segment
// (2^30, option dec_seg) take several segments; the exit of one is the entry of the next.
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
#include "stages.hpp"
#include "prim.hpp"
#include "decode.hpp"

#include <chrono>
#include <vector>

namespace tdc {

namespace {

constexpr u32 LZD_TILE = 32768;                                   // bit positions per workgroup of the next() pass
constexpr u32 LZD_REACH = 2 * 32 + 1 + 2 * 64 + 1 + 64;           // bits behind a candidate that lz_pair may peek at (pair + window)
constexpr u32 LZD_NW = (LZD_TILE + LZD_REACH + 31) / 32 + 4;      // stream words per workgroup
#ifndef TDC_LZD_HOPS
#define TDC_LZD_HOPS 16
#endif

// The pair that starts at bit x (read_elias_gamma<u32>, read_elias_gamma<u8>): 0 and its end, id and char; < 0: no pair there.
template <typename Win>
__device__ __forceinline__ int lz_pair(const Win& bw, u64 x, u64 total, u64& end, u32& id, u32& ch) {
    end = x; id = 0; ch = 0;
    const u64 w = bw.peek(x);                                     // (zeros behind the end of the stream)
    if (w == 0) return -1;
    const u32 b1 = (u32)__builtin_clzll(w);
    if (b1 > 32) return -1;                                       // id field wider than a factorid_t
    if (b1) id = (u32)(bw.peek(x + b1 + 1) >> (64 - b1));
    const u64 y = x + 2 * b1 + 1;
    const u64 v = bw.peek(y);
    u32 b2;
    if (v) b2 = (u32)__builtin_clzll(v);
    else if (bw.peek(y + 64) >> 63) b2 = 64;                      // a sign-extended 64-bit char (the reference's left-over phrase)
    else return -2;
    end = y + 2 * (u64)b2 + 1;
    if (end > total) return -3;                                   // cut off by the end of the stream
    if (b2) { const u32 k = b2 < 8 ? b2 : 8; ch = (u32)(bw.peek(end - k) >> (64 - k)); }     // the low 8 bits of the value
    return 0;
}

// next() for the bit positions x_in .. x_in + m - 1 (index = position - x_in); m: the pair leaves the segment, or there is no pair
__global__ __launch_bounds__(256) void lz_next_kernel(const u32* __restrict__ s32, u64 x_in, u32 m, u64 total, u32* __restrict__ next) {
    __shared__ u32 sw[LZD_NW];
    const u32 i0 = blockIdx.x * LZD_TILE;
    const u64 kb = (x_in + i0) >> 5;
    const u64 wmax = (total + 31) / 32 + 3;                       // (the buffer is padded: words up to here exist)
    for (u32 k = threadIdx.x; k < LZD_NW; k += 256) sw[k] = (kb + k < wmax) ? __builtin_bswap32(s32[kb + k]) : 0u;
    __syncthreads();
    const BitWin bw{sw, kb, total};
    for (u32 i = threadIdx.x; i < LZD_TILE; i += 256) {
        const u32 idx = i0 + i;
        if (idx >= m) break;
        u64 end; u32 id, ch;
        u32 r = m;
        if (lz_pair(bw, x_in + idx, total, end, id, ch) == 0) { const u64 d = end - x_in; r = d < (u64)m ? (u32)d : m; }
        next[idx] = r;
    }
}

struct LzScalars { u64 exit_bit; u32 err; u32 pad; };

// the pairs of a segment (offsets idx[0 .. cnt)), global pair index k0 + j: id, char, validation; the last one reports the exit
__global__ __launch_bounds__(256) void lz_pairs_kernel(const u32* __restrict__ s32, u64 x_in, const u32* __restrict__ idx, u32 cnt, u64 total,
                                                        u64 k0, u32* __restrict__ ids, u8* __restrict__ chars, LzScalars* __restrict__ sc) {
    const BitWinG bw{s32, total};
    for (u32 j = blockIdx.x * 256 + threadIdx.x; j < cnt; j += gridDim.x * 256) {
        const u64 x = x_in + idx[j];
        const u64 k = k0 + j;
        u64 end; u32 id, ch;
        const int st = lz_pair(bw, x, total, end, id, ch);
        if (st < 0) atomicOr(&sc->err, 1u);
        else if ((u64)id > k) atomicOr(&sc->err, 2u);
        ids[k] = (st < 0 || (u64)id > k) ? 0u : id;
        chars[k] = (u8)ch;
        if (j == cnt - 1) sc->exit_bit = end;
    }
}

// J[k] = (link << 32) | acc: len_k = acc + len(link), link = NONE32 once acc is the length
// (the per-phrase kernels loop with a grid stride: up to 2^32 - 2 phrases, launched with dec_grid())
__global__ void lz_link_kernel(const u32* __restrict__ ids, size_t z, u64* __restrict__ J) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < z; k += stride) {
        const u32 id = ids[k];
        J[k] = ((u64)(id ? id - 1 : NONE32) << 32) | 1ull;
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
__global__ void lz_factor_kernel(const u32* __restrict__ ids, const u64* __restrict__ J, const u64* __restrict__ S, size_t z,
                                 u32* __restrict__ fpos, u32* __restrict__ fsrc, u32* __restrict__ flen) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < z; k += stride) {
        const u32 id = ids[k];
        fpos[k] = (u32)S[k];
        fsrc[k] = id ? (u32)S[id - 1] : 0u;
        flen[k] = (u32)J[k] - 1u;
    }
}

// the literal of phrase k at its last text position
__global__ void lz_literal_kernel(const u32* __restrict__ fpos, const u32* __restrict__ flen, const u8* __restrict__ chars, size_t z,
                                  u8* __restrict__ text) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < z; k += stride) text[(size_t)fpos[k] + flen[k]] = chars[k];
}

// The arena is too small for what follows: the live arrays travel to the host and back into an arena of `bytes` (the size this call
// would have needed without moving, so that the next call of the same size on this context does not move again).
void regrow_arena(Ctx& c, size_t bytes, std::initializer_list<std::pair<void**, size_t>> live) {
    std::vector<std::vector<u8>> keep;
    for (const auto& a : live) {
        keep.emplace_back(a.second);
        if (a.second) HIP_TRY(hipMemcpyAsync(keep.back().data(), *a.first, a.second, hipMemcpyDeviceToHost, c.stream));
    }
    HIP_TRY(hipStreamSynchronize(c.stream));
    c.ensure_arena(bytes);
    size_t i = 0;
    for (const auto& a : live) {
        *a.first = c.arena.alloc(a.second + 64);
        if (a.second) HIP_TRY(hipMemcpyAsync(*a.first, keep[i].data(), a.second, hipMemcpyHostToDevice, c.stream));
        ++i;
    }
    HIP_TRY(hipStreamSynchronize(c.stream));
}

}  // namespace

size_t decode_lz78_gamma(Ctx& c, const u8* stream, size_t len, Sink& out, size_t* need, DecodeStats* st) {
    DecodeStats local;
    if (!st) st = &local;
    *st = DecodeStats();
    const u64 total = FastBits(stream, len).total;                                     // (throws for a cut-off terminator)
    if (total == 0) { decode_dest(out, 0); if (need) *need = 0; return 0; }             // the empty text's stream: no pairs
    hipStream_t s = c.stream;
    const bool dlog = c.dec_log != 0;                                                    // stage times on stderr (synchronises)
    auto t_last = std::chrono::steady_clock::now();
    auto tick = [&](const char* what) {
        if (!dlog) return;
        (void)hipStreamSynchronize(s);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "lz78 decode: %-26s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    };
    // a pair takes 2 bits at least ("1" "1": id 0, char 0), and more than 2^32 - 2 pairs decode to more than 2^32 - 2 bytes
    const u64 zcap = std::min<u64>(total / 2 + 1, 0xFFFFFFFEull);
    const u64 seg_bits = c.dec_seg ? (u64)c.dec_seg : (u64)DEC_SEG;                      // (tests shrink the segments)
    const size_t seg = (size_t)std::min<u64>(seg_bits, total);
    const size_t slack = (size_t)16 << 20;
    c.ensure_arena(len + 64 + zcap * 5 + seg * 13 + slack);
    void* d_stream = c.arena.get<u8>(len + 64);
    u32* ids = c.arena.get<u32>(zcap);
    u8* chars = c.arena.get<u8>(zcap + 64);
    LzScalars* d_sc = (LzScalars*)c.arena.alloc(sizeof(LzScalars));
    u32* d_cnt = c.arena.get<u32>(2);
    HIP_TRY(hipMemcpyAsync(d_stream, stream, len, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync((u8*)d_stream + len, 0, 64, s));
    HIP_TRY(hipMemsetAsync(d_sc, 0, sizeof(LzScalars), s));
    const u32* s32 = (const u32*)d_stream;                                              // (arena allocations are 256-byte aligned)
    tick("upload");

    // ---- pair starts and pairs, segment by segment
    size_t z = 0;
    u64 x_in = 0;
    while (x_in < total) {
        const u32 m = (u32)std::min<u64>(seg_bits, total - x_in);
        const size_t mk = c.arena.mark();
        u32* next = c.arena.get<u32>(m);
        u32* e1 = c.arena.get<u32>(m), *e2 = c.arena.get<u32>(m);
        u8* mark = c.arena.get<u8>(m);
        lz_next_kernel<<<cdiv(m, LZD_TILE), 256, 0, s>>>(s32, x_in, m, total, next);
        LAUNCH_CHECK();
        tick("next() of every bit");
        mark_orbit_u32(c, next, m, mark, e1, e2);
        tick("chain marking");
        u32* idx = e1;                                                                  // (the exit arrays are free again)
        select_by_class(c, mark, 1, m, nullptr, idx, nullptr, nullptr, d_cnt);
        const u32 cnt = c.read(d_cnt);
        tick("pair list");
        if (cnt == 0) throw StreamFormatError{"corrupt stream: pair chain"};
        if (z + cnt > zcap) throw DecodeTooLarge{z + cnt};                              // (more pairs than 2^32 - 2: more bytes)
        lz_pairs_kernel<<<std::min<u32>(cdiv(cnt, 256), 4096u), 256, 0, s>>>(s32, x_in, idx, cnt, total, (u64)z, ids, chars, d_sc);
        LAUNCH_CHECK();
        const LzScalars h = c.read(d_sc);
        tick("pair decode");
        c.arena.release(mk);
        z += cnt;
        if (h.err & 1u) throw StreamFormatError{"corrupt stream: malformed or cut-off pair"};
        if (h.err & 2u) throw StreamFormatError{"corrupt stream: phrase id out of range"};
        if (h.exit_bit >= total) break;
        if (h.exit_bit <= x_in) throw StreamFormatError{"corrupt stream: pair chain"};
        x_in = h.exit_bit;
    }
    st->factors = z;

    // ---- phrase lengths (pointer jumping), starts (64-bit scan), factor list
    {
        const size_t need1 = c.arena.mark() + z * 28 + slack;
        if (c.arena.size < need1) {
            void* pi = ids; void* pc = chars;
            regrow_arena(c, need1, {{&pi, z * 4}, {&pc, z}});
            ids = (u32*)pi; chars = (u8*)pc;
            d_cnt = c.arena.get<u32>(2);
        }
    }
    u32* fpos = c.arena.get<u32>(z), *fsrc = c.arena.get<u32>(z), *flen = c.arena.get<u32>(z);
    const size_t mkB = c.arena.mark();
    u64* J = c.arena.get<u64>(z);
    u64* S = c.arena.get<u64>(z);
    u64* d_total = c.arena.get<u64>(1);
    lz_link_kernel<<<dec_grid(z), 256, 0, s>>>(ids, z, J);
    LAUNCH_CHECK();
    unsigned g = cdiv(z, 256 * 8); if (g > 16384) g = 16384;
    u32 len_rounds = 0;
    for (u32 round = 0;; ++round) {
        if (round > 40) throw HipError{hipErrorUnknown, "lz78 decode: phrase lengths did not converge", (int)__LINE__};   // depth < 2^32
        HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(u32), s));
        lz_len_jump_kernel<<<g, 256, 0, s>>>(J, z, d_cnt);
        LAUNCH_CHECK();
        len_rounds = round + 1;
        if (c.read(d_cnt) == 0) break;
    }
    lz_len_kernel<<<dec_grid(z), 256, 0, s>>>(J, z, S);
    LAUNCH_CHECK();
    exclusive_sum_u64(c, S, S, z, d_total);
    const u64 n = c.read(d_total);
    tick("phrase lengths + starts");
    if (need) *need = (size_t)n;
    if (n > 0xFFFFFFFEull) throw DecodeTooLarge{n};                                     // checked before any text-sized allocation
    if (out.into && n > out.cap) throw HipError{hipErrorOutOfMemory, "lz78 decode: the caller's buffer is too small for the text", (int)__LINE__};
    lz_factor_kernel<<<dec_grid(z), 256, 0, s>>>(ids, J, S, z, fpos, fsrc, flen);
    LAUNCH_CHECK();
    c.arena.release(mkB);
    tick("factor list");

    // ---- text: literals, then the shared reference resolver
    {
        const size_t need2 = c.arena.mark() + (size_t)n * 5 + (size_t)n / 8 + slack;
        if (c.arena.size < need2) {
            void* pp = fpos; void* ps = fsrc; void* pl = flen; void* pc = chars;
            regrow_arena(c, need2, {{&pp, z * 4}, {&ps, z * 4}, {&pl, z * 4}, {&pc, z}});
            fpos = (u32*)pp; fsrc = (u32*)ps; flen = (u32*)pl; chars = (u8*)pc;
            d_cnt = c.arena.get<u32>(2);
        }
    }
    u8* d_text = c.arena.get<u8>((size_t)n + 64);
    u32* d_ref = c.arena.get<u32>((size_t)n);
    lz_literal_kernel<<<dec_grid(z), 256, 0, s>>>(fpos, flen, chars, z, d_text);
    LAUNCH_CHECK();
    tick("literals");
    resolve_and_download(c, (size_t)n, d_text, d_ref, fpos, fsrc, flen, z, d_cnt, out, st);
    st->rounds += len_rounds;
    tick("references + download");
    return (size_t)n;
}

}  // namespace tdc
