// lzss_sw_batch.hip -- lzss over many independent texts in one call, both directions ("Batches").
//
// Compression is ONE pass over the concatenation of the texts, not a loop over them.  off[0 .. count] are the texts' borders (off[0] = 0,
// off[count] = n, ascending; equal neighbours: an empty text, which owns no position).
//   match kernel   the tile scheme of lzss_sw.hip.  A tile may hold a piece of one text or thousands of texts: the texts of a tile are
//                  found once per tile (two searches over off[]), their borders staged in LDS, and every lane finds its own text among
//                  them.  Candidates and look-ahead are those of the position INSIDE its text: s in [max(start, p - w), p), L(p) from the
//                  text's own length -- the image's bytes of the neighbouring texts lie in LDS but are never compared beyond L.  The
//                  kernel also notes bits_for(p - start), the width of the distance under BitCoder, beside the factor.
//   the parse      no factor crosses a text's end, so next(p) <= end of p's text and the orbit of position 0 over the concatenation
//                  passes through the first position of every non-empty text: one mark_orbit_u32, one select_by_class.
//   placement      cost of every token (the field costs of bitsink.hpp) | 64-bit scan: every token's bit in the concatenated stream |
//                  per text: the bit of its first token (a search over the token positions) -> its bit count -> its 8-byte aligned slot
//                  | scan over the texts: out_off | pack: every token at its bit, rebased to its stream | one terminator per text.
// A text whose lengths BitCoder would truncate gets a flag in the cost pass, a slot of 0 bytes, and is skipped by the pack.
//
// Decompression: the streams are independent, so one wave takes one stream (workgroups of one wave, in a grid-stride over the
// streams) and walks its tokens in order.  Two launches: a sizes pass (text length and verdict of every stream), and behind the scan
// over the texts a write pass.  All 64 lanes decode the same token from an LDS window of the stream (uniform control flow, broadcast
// reads; swd_token of lzss_sw_token.hpp, so the refusal rules are the single decoder's), lane 0 writes a literal, the 64 lanes copy a
// factor: byte j comes from source byte j, or j mod distance where the source overlaps the target -- always a byte in front of the
// token, written by an earlier token, behind a workgroup barrier.  Every loop is bounded by the stream's own bit count (a token takes at
// least one bit); the write pass writes inside the slot the sizes pass assigned and nowhere else.
#include "stages.hpp"
#include "bitsink.hpp"
#include "prim.hpp"
#include "decode.hpp"
#include "lzss_sw_token.hpp"

#include <algorithm>

namespace tdc {

namespace {

// ---- compression ---------------------------------------------------------------------------------------------------------------------
constexpr u32 SWB_TILE = 4096;                                        // positions per workgroup, as SW_TILE of lzss_sw.hip
constexpr u32 SWB_LDS_WORDS = (SWB_TILE + 3 * LZSS_SW_MAX_WINDOW) / 8 + 2;
constexpr u32 SWB_OFFS = 2048;                                        // borders of a tile staged in LDS; a tile with more searches off[] itself

// fac[p] of the batch: length (13 bits) | distance << 13 (13 bits) | (bits_for(p - start) - 1) << 26; 0: a literal
__device__ __forceinline__ u32 swb_len(u32 f) { return f & 0x1FFFu; }
__device__ __forceinline__ u32 swb_dist(u32 f) { return (f >> 13) & 0x1FFFu; }
__device__ __forceinline__ u32 swb_width(u32 f) { return (f >> 26) + 1u; }

// the 8 bytes from byte i of the image on, byte i in the low bits
__device__ __forceinline__ u64 swb_word(const u64* img, u32 i) {
    const u32 k = i >> 3, sh = (i & 7u) * 8u;
    const u64 a = img[k];
    return sh ? (a >> sh) | (img[k + 1] << (64u - sh)) : a;
}

// the largest j in [lo, hi] with tab[j] <= p, for ascending tab with tab[lo] <= p: among equal borders the last one, so a position's
// text is never an empty one
__device__ __forceinline__ u32 swb_text_of(const u32* tab, u32 lo, u32 hi, u32 p) {
    while (lo < hi) {
        const u32 mid = lo + (hi - lo + 1) / 2;
        if (tab[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void swb_match_kernel(const u8* __restrict__ text, u64 n, const u32* __restrict__ off, u32 count, u32 w, u32 t,
                                                         u32 tiles, u32* __restrict__ next, u32* __restrict__ fac) {
    __shared__ u64 img[SWB_LDS_WORDS];
    __shared__ u32 soff[SWB_OFFS];
    __shared__ u32 srng[2];
    const u8* imgb = (const u8*)img;
    const u32 wpad = (w + 7u) & ~7u;
    const u32 words = (wpad + SWB_TILE + 2u * w + 15u) >> 3;
    for (u32 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const u64 t0 = (u64)tile * SWB_TILE;
        if (threadIdx.x == 0) {                                       // the texts of the first and of the last position of the tile
            const u64 last = (t0 + SWB_TILE < n ? t0 + SWB_TILE : n) - 1;
            const u32 j0 = swb_text_of(off, 0, count, (u32)t0);
            srng[0] = j0;
            srng[1] = swb_text_of(off, j0, count, (u32)last);       // (off[count] = n > last: at most count - 1)
        }
        for (u32 k = threadIdx.x; k < words; k += 256) {
            const long long g = (long long)t0 - (long long)wpad + 8ll * k;
            u64 v = 0;
            if (g >= 0 && (u64)g + 8 <= n) v = *(const u64*)(text + g);
            else if (g >= 0) { for (u32 b = 0; b < 8 && (u64)g + b < n; ++b) v |= (u64)text[g + b] << (8u * b); }
            img[k] = v;
        }
        __syncthreads();
        const u32 j0 = srng[0], j1 = srng[1];
        const bool staged = j1 - j0 + 2u <= SWB_OFFS;                 // the borders off[j0 .. j1 + 1]
        if (staged) {
            for (u32 k = threadIdx.x; k < j1 - j0 + 2u; k += 256) soff[k] = off[j0 + k];
        }
        __syncthreads();
        const u32* tab = staged ? (const u32*)soff : off + j0;
        for (u32 k = threadIdx.x; k < SWB_TILE; k += 256) {
            const u64 p = t0 + k;
            if (p >= n) break;
            const u32 j = swb_text_of(tab, 0, j1 - j0, (u32)p);
            const u32 start = tab[j], nk = tab[j + 1] - start, q = (u32)p - start;      // the text's start and length, p inside it
            u32 end = nk;
            if (nk >= 2u * w) { const u32 o = q > w ? q - w : 0u; end = (o < nk - 2u * w ? o : nk - 2u * w) + 2u * w; }
            const u32 L = end - q;
            const u32 ip = k + wpad;
            const u32 cand = q < w ? q : w;                           // sources p - cand .. p - 1: none in front of the text
            const u32 is = ip - cand;
            u32 best = 0, bdist = 0;
            if (cand) {
                const u64 P = swb_word(img, ip);
                u64 S = swb_word(img, is);
                for (u32 c = 0; c < cand; ++c) {
                    u64 x = S ^ P;
                    u32 jj;
                    if (x) jj = (u32)__builtin_ctzll(x) >> 3;
                    else {
                        jj = 8;
                        while (jj < L) {
                            x = swb_word(img, is + c + jj) ^ swb_word(img, ip + jj);
                            if (x) { jj += (u32)__builtin_ctzll(x) >> 3; break; }
                            jj += 8;
                        }
                    }
                    jj = jj < L ? jj : L;                             // (what matched beyond L may be a neighbour's bytes: dropped here)
                    if (jj >= t && jj > best) { best = jj; bdist = cand - c; if (best == L) break; }
                    S = (S >> 8) | ((u64)imgb[is + c + 8] << 56);
                }
            }
            next[p] = (u32)p + (best ? best : 1u);                    // <= the text's end
            fac[p] = best ? ((uni_bits_for(q) - 1u) << 26) | (bdist << 13) | best : 0u;
        }
        __syncthreads();
    }
}

struct SwbScalars { unsigned long long factors; };

struct SwbTok { u32 pos, f, ch; };
__device__ __forceinline__ SwbTok swb_load(const u8* __restrict__ text, const u32* __restrict__ tokpos, const u32* __restrict__ fac, u64 i) {
    SwbTok tk;
    tk.pos = tokpos[i]; tk.f = fac[tk.pos]; tk.ch = text[tk.pos];
    return tk;
}
// LZSSSlidingWindowCompressor.hpp:85-95, as SwTokens of lzss_sw.hip: the distance under Range(0, p - start), the length under Range(0, window)
template <int KIND> __device__ __forceinline__ u32 swb_bits(const SwbTok& tk, u32 wbits) {
    return flag_cost<KIND>() + (tk.f ? int_cost<KIND>(swb_dist(tk.f), swb_width(tk.f)) + int_cost<KIND>(swb_len(tk.f), wbits) : byte_cost<KIND>(tk.ch));
}
template <int KIND> __device__ __forceinline__ void swb_put(BitSink& sink, const SwbTok& tk, u32 wbits) {
    append_flag<KIND>(sink, tk.f ? 1u : 0u);
    if (!tk.f) append_byte<KIND>(sink, tk.ch);
    else { append_int<KIND>(sink, swb_dist(tk.f), swb_width(tk.f)); append_int<KIND>(sink, swb_len(tk.f), wbits); }
}

// cost[i]: the bits of token i; the factors are counted, and the text of a length that BitCoder would truncate is flagged
template <int KIND>
__global__ __launch_bounds__(256) void swb_cost_kernel(const u8* __restrict__ text, const u32* __restrict__ tokpos, const u32* __restrict__ fac, u64 ntok,
                                                        const u32* __restrict__ off, u32 count, u32 wbits, u64* __restrict__ cost,
                                                        u32* __restrict__ flag, SwbScalars* __restrict__ sc) {
    const u64 stride = (u64)gridDim.x * 256;
    u32 nfac = 0;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < ntok; i += stride) {
        const SwbTok tk = swb_load(text, tokpos, fac, i);
        cost[i] = swb_bits<KIND>(tk, wbits);
        nfac += tk.f ? 1u : 0u;
        if (KIND == ENC_TAB && tk.f && (swb_len(tk.f) >> wbits)) flag[swb_text_of(off, 0, count, tk.pos)] = 1u;
    }
    nfac = wave_reduce_sum(nfac);
    if (lane_id() == 0 && nfac) atomicAdd(&sc->factors, (unsigned long long)nfac);
}

// Per text k: gfirst[k] = the bit, in the concatenated token stream, of the first token at or behind off[k] (the text's first token; for
// an empty text the next text's, so its bit count is 0), gfirst[count] = all bits; slot[k] = the bytes its stream takes in the output,
// rounded up to 8 (0 for a flagged text).
__device__ __forceinline__ u64 swb_first_bit(const u32* __restrict__ tokpos, u64 ntok, const u64* __restrict__ gpos, u64 total, u32 p) {
    u64 lo = 0, hi = ntok;                                            // the first token with tokpos >= p
    while (lo < hi) { const u64 mid = lo + (hi - lo) / 2; if (tokpos[mid] < p) lo = mid + 1; else hi = mid; }
    return lo < ntok ? gpos[lo] : total;
}
__global__ __launch_bounds__(256) void swb_slots_kernel(const u32* __restrict__ off, u32 count, const u32* __restrict__ tokpos, u64 ntok,
                                                         const u64* __restrict__ gpos, const u64* __restrict__ d_total, const u32* __restrict__ flag,
                                                         u64* __restrict__ gfirst, u64* __restrict__ slot) {
    const u64 total = *d_total;
    for (u32 k = blockIdx.x * 256 + threadIdx.x; k < count; k += gridDim.x * 256) {
        const u64 a = swb_first_bit(tokpos, ntok, gpos, total, off[k]);
        const u64 b = off[k + 1] == off[k] ? a : swb_first_bit(tokpos, ntok, gpos, total, off[k + 1]);
        gfirst[k] = a;
        if (k == count - 1) gfirst[count] = b;
        const u64 tb = b - a;
        const u64 len = (tb >> 3) + ((tb & 7) <= 5 ? 1 : 2);        // bit_stream_len
        slot[k] = flag[k] ? 0ull : (len + 7) & ~7ull;
    }
}

// Every token at its bit of its text's stream: gpos[i] - gfirst[k] behind byte ooff[k].  A thread packs 8 tokens in a row through one
// sink, which it seats anew where the next token does not continue the pending bits: at a text's first token.
template <int KIND>
__global__ __launch_bounds__(256) void swb_pack_kernel(const u8* __restrict__ text, const u32* __restrict__ tokpos, const u32* __restrict__ fac, u64 ntok,
                                                        const u32* __restrict__ off, u32 count, u32 wbits, const u64* __restrict__ gpos,
                                                        const u64* __restrict__ gfirst, const u64* __restrict__ ooff, const u32* __restrict__ flag,
                                                        u64* __restrict__ out) {
    const u64 i0 = ((u64)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i0 >= ntok) return;
    BitSink sink;
    sink.out = out; sink.pos = 0; sink.acc = 0; sink.cnt = 0;
    u32 k = 0, kend = 0;                                              // the text of the token before and its end
    u64 delta = 0;
    bool skip = false;
    for (u32 j = 0; j < 8 && i0 + j < ntok; ++j) {
        const SwbTok tk = swb_load(text, tokpos, fac, i0 + j);
        if (j == 0 || tk.pos >= kend) {
            k = swb_text_of(off, j == 0 ? 0u : k + 1u, count, tk.pos);
            kend = off[k + 1];
            delta = 8ull * ooff[k] - gfirst[k];
            skip = flag[k] != 0u;
        }
        if (skip) continue;
        const u64 at = gpos[i0 + j] + delta;
        if (at != sink.pos + sink.cnt) { sink.flush(); sink.pos = at; }
        swb_put<KIND>(sink, tk, wbits);
    }
    sink.flush();
}

// io/BitOStream.hpp:53-64 for every stream, as terminator_kernel of lz78.hip
__global__ __launch_bounds__(256) void swb_terminators_kernel(const u64* __restrict__ gfirst, const u64* __restrict__ ooff, const u32* __restrict__ flag,
                                                               u32 count, u8* __restrict__ out) {
    for (u32 k = blockIdx.x * 256 + threadIdx.x; k < count; k += gridDim.x * 256) {
        if (flag[k]) continue;
        const u64 tb = gfirst[k + 1] - gfirst[k];
        u8* o = out + ooff[k] + (tb >> 3);
        const u32 u = (u32)(tb & 7);
        if (u <= 5) o[0] |= (u8)u; else o[1] = (u8)u;
    }
}

template <class F>
void with_enc_kind(int kind, F&& f) {
    switch (kind) {
        case ENC_TAB:   f(std::integral_constant<int, ENC_TAB>{}); break;
        case ENC_ASCII: f(std::integral_constant<int, ENC_ASCII>{}); break;
        case ENC_GAMMA: f(std::integral_constant<int, ENC_GAMMA>{}); break;
        default:        f(std::integral_constant<int, ENC_DELTA>{}); break;
    }
}

}  // namespace

void lzss_sw_batch_sizes(Ctx& c, const u8* d_text, size_t n, size_t count, u32 window, u32 threshold, int kind, LzssSwBatch& B) {
    if (kind < 0 || kind > 3 || window == 0 || window > LZSS_SW_MAX_WINDOW || n > 0xFFFFFFFEull || count == 0 || count > 0xFFFFFFFEull)
        throw HipError{hipErrorInvalidValue, "lzss batch: coder, window, text length or count out of range", (int)__LINE__};
    hipStream_t s = c.stream;
    B.ntok = 0; B.factors = 0; B.tokpos = nullptr; B.fac = nullptr; B.gpos = nullptr;
    HIP_TRY(hipMemsetAsync(B.flag, 0, count * sizeof(u32), s));
    if (n == 0) {                                                     // empty texts only: no token, every stream is the terminator
        HIP_TRY(hipMemsetAsync(B.gfirst, 0, (count + 1) * sizeof(u64), s));
        HIP_TRY(hipMemsetAsync(B.ooff, 0, (count + 1) * sizeof(u64), s));
        u64* d_total = c.arena.get<u64>(1);
        HIP_TRY(hipMemsetAsync(d_total, 0, sizeof(u64), s));
        swb_slots_kernel<<<dec_grid(count), 256, 0, s>>>(B.off, (u32)count, nullptr, 0, nullptr, d_total, B.flag, B.gfirst, B.ooff);
        LAUNCH_CHECK();
        exclusive_sum_u64(c, B.ooff, B.ooff, count, B.ooff + count);
        return;
    }
    u64* wide = c.arena.get<u64>(n);                                  // next and a scratch array of the orbit; then the tokens' bits
    u32* next = (u32*)wide, *s2 = next + n;
    u32* fac = c.arena.get<u32>(n);
    u32* s1 = c.arena.get<u32>(n);
    u8* mark = c.arena.get<u8>(n);
    u32* d_cnt = c.arena.get<u32>(1);
    u64* d_total = c.arena.get<u64>(1);
    SwbScalars* d_sc = (SwbScalars*)c.arena.alloc(sizeof(SwbScalars));
    HIP_TRY(hipMemsetAsync(d_sc, 0, sizeof(SwbScalars), s));
    const size_t tiles = (n + SWB_TILE - 1) / SWB_TILE;
    swb_match_kernel<<<dec_grid(tiles * 256), 256, 0, s>>>(d_text, (u64)n, B.off, (u32)count, window, threshold ? threshold : 1u, (u32)tiles, next, fac);
    LAUNCH_CHECK();
    mark_orbit_u32(c, next, n, mark, s1, s2);
    select_by_class(c, mark, 1, n, nullptr, s1, nullptr, nullptr, d_cnt);
    const size_t ntok = c.read(d_cnt);
    const u32 wbits = bits_for(window);
    with_enc_kind(kind, [&](auto K) {
        swb_cost_kernel<decltype(K)::value><<<dec_grid(ntok), 256, 0, s>>>(d_text, s1, fac, (u64)ntok, B.off, (u32)count, wbits, wide, B.flag, d_sc);
    });
    LAUNCH_CHECK();
    exclusive_sum_u64(c, wide, wide, ntok, d_total);
    swb_slots_kernel<<<dec_grid(count), 256, 0, s>>>(B.off, (u32)count, s1, (u64)ntok, wide, d_total, B.flag, B.gfirst, B.ooff);
    LAUNCH_CHECK();
    exclusive_sum_u64(c, B.ooff, B.ooff, count, B.ooff + count);
    B.ntok = ntok; B.tokpos = s1; B.fac = fac; B.gpos = wide;
    B.factors = c.read(&d_sc->factors);
}

void lzss_sw_batch_pack(Ctx& c, const u8* d_text, size_t count, u32 window, int kind, const LzssSwBatch& B, u8* d_out, size_t used) {
    hipStream_t s = c.stream;
    if (used) HIP_TRY(hipMemsetAsync(d_out, 0, used, s));
    if (B.ntok) {
        const u32 wbits = bits_for(window);
        const unsigned blocks = (unsigned)((B.ntok + 2047) / 2048);
        with_enc_kind(kind, [&](auto K) {
            swb_pack_kernel<decltype(K)::value><<<blocks, 256, 0, s>>>(d_text, B.tokpos, B.fac, (u64)B.ntok, B.off, (u32)count, wbits, B.gpos, B.gfirst,
                                                                       B.ooff, B.flag, (u64*)d_out);
        });
        LAUNCH_CHECK();
    }
    swb_terminators_kernel<<<dec_grid(count), 256, 0, s>>>(B.gfirst, B.ooff, B.flag, (u32)count, d_out);
    LAUNCH_CHECK();
}

// ---- decompression -------------------------------------------------------------------------------------------------------------------
namespace {

constexpr u64 SWB_TEXT_MAX = 0xFFFFFFFEull;
constexpr u32 SWB_WIN = 260;                                          // stream words a wave holds in LDS at a time

// Stream k = blob[s_off[k] - sub, + s_len[k]) (the blob is padded with 64 zero bytes).  WRITE = false, the sizes pass: tlen[k] and
// status[k] of every stream, the factor tokens of the accepted ones counted.  WRITE = true: the text of every accepted stream into
// out[ooff[k], + tlen[k]).
template <int KIND, bool WRITE>
__global__ __launch_bounds__(64) void swb_decode_kernel(const u8* __restrict__ blob, u64 sub, const u64* __restrict__ s_off, const u64* __restrict__ s_len,
                                                         u32 count, u32 lb, u32* __restrict__ tlen, int* __restrict__ status,
                                                         const u64* __restrict__ ooff, u8* __restrict__ out, unsigned long long* __restrict__ factors) {
    constexpr u32 REACH = swd_reach(KIND);
    static_assert(31 + REACH + 32 * BitWin::PEEK_WORDS <= 16 * SWB_WIN, "a refilled window must hold a token and leave half of itself for progress");
    __shared__ u32 win[SWB_WIN];
    const u32 lane = threadIdx.x;
    for (u32 sidx = blockIdx.x; sidx < count; sidx += gridDim.x) {
        if (WRITE && (status[sidx] != 0 || tlen[sidx] == 0u)) continue;
        const u64 len = s_len[sidx], b = s_off[sidx] - sub;
        u64 total = 0;                                                // payload_bits (decode.hpp)
        if (len) {
            const u32 fb = blob[b + len - 1] & 7u;
            total = len == 1 ? fb : fb >= 6 ? 8ull * (len - 2) + fb : 8ull * (len - 1) + fb;
        }
        // the stream's words start at the 4-byte border in front of it: its bits are [skew, T) of them
        const u32* s32 = (const u32*)(blob + (b & ~3ull));
        const u64 skew = 8ull * (b & 3ull), T = skew + total;
        const u64 wmax = (T + 31) / 32 + 3;                           // words that exist (the pad behind the blob)
        const u64 nk = WRITE ? (u64)tlen[sidx] : 0ull;
        u8* dst = WRITE ? out + ooff[sidx] : nullptr;
        u64 x = skew, p = 0, kb = 0, nfac = 0;
        bool loaded = false, dirty = false;
        int verdict = 0;
        while (x < T) {                                               // every turn takes at least one bit
            if (!loaded || x + REACH + 32 * BitWin::PEEK_WORDS > (kb + SWB_WIN) * 32) {
                __syncthreads();
                kb = x >> 5;
                for (u32 j = lane; j < SWB_WIN; j += 64) win[j] = kb + j < wmax ? __builtin_bswap32(s32[kb + j]) : 0u;
                __syncthreads();
                loaded = true;
                dirty = false;                                        // (the barrier also published the text so far)
            }
            const BitWin bw{win, kb, T};
            u64 end; u32 fac, dist, val;
            if (swd_token<KIND>(bw, x, T, uni_bits_for((u32)p), lb, end, fac, dist, val) != 0) { verdict = TDC_GPU_ERR_ARG; break; }
            if (fac) {
                if (dist == 0u || (u64)dist > p) { verdict = TDC_GPU_ERR_ARG; break; }      // never in front of the stream's own text
                if ((u64)val > SWB_TEXT_MAX - p) { verdict = TDC_GPU_ERR_TOO_LARGE; break; }
                if (WRITE && val) {
                    if (dirty) __syncthreads();                       // the source bytes were written by earlier tokens
                    const u8* src = dst + (p - dist);
                    const bool periodic = dist < val;
                    for (u64 j = lane; j < (u64)val && p + j < nk; j += 64) dst[p + j] = src[periodic ? (u32)j % dist : (u32)j];
                    dirty = true;
                }
                p += val;
                ++nfac;
            } else {
                if (p >= SWB_TEXT_MAX) { verdict = TDC_GPU_ERR_TOO_LARGE; break; }
                if (WRITE) {
                    if (lane == 0 && p < nk) dst[p] = (u8)val;
                    dirty = true;
                }
                p += 1;
            }
            x = end;
        }
        if (!WRITE && lane == 0) {
            status[sidx] = verdict;
            tlen[sidx] = verdict ? 0u : (u32)p;
            if (!verdict && nfac) atomicAdd(factors, (unsigned long long)nfac);
        }
    }
}

__global__ __launch_bounds__(256) void swb_widen_kernel(const u32* __restrict__ in, u32 count, u64* __restrict__ out) {
    for (u32 k = blockIdx.x * 256 + threadIdx.x; k < count; k += gridDim.x * 256) out[k] = in[k];
}

// workgroups of one wave: as many as there are streams, up to what keeps every CU busy several times over
unsigned swb_decode_grid(size_t count) { return (unsigned)std::min<size_t>(count, (size_t)1 << 16); }

}  // namespace

void lzss_sw_batch_decode_sizes(Ctx& c, int kind, u32 window, size_t count, LzssSwBatchDec& D) {
    if (count == 0 || count > 0xFFFFFFFEull) throw HipError{hipErrorInvalidValue, "lzss batch decode: count out of range", (int)__LINE__};
    hipStream_t s = c.stream;
    const u32 lb = bits_for(window);
    HIP_TRY(hipMemsetAsync(D.factors, 0, sizeof(u64), s));
    with_dec_kind(kind, [&](auto K) {
        swb_decode_kernel<decltype(K)::value, false><<<swb_decode_grid(count), 64, 0, s>>>(D.blob, D.sub, D.s_off, D.s_len, (u32)count, lb, D.tlen, D.status,
                                                                                           nullptr, nullptr, (unsigned long long*)D.factors);
        return 0;
    });
    LAUNCH_CHECK();
    swb_widen_kernel<<<dec_grid(count), 256, 0, s>>>(D.tlen, (u32)count, D.ooff);
    LAUNCH_CHECK();
    exclusive_sum_u64(c, D.ooff, D.ooff, count, D.ooff + count);
}

void lzss_sw_batch_decode_write(Ctx& c, int kind, u32 window, size_t count, const LzssSwBatchDec& D, u8* d_text) {
    hipStream_t s = c.stream;
    const u32 lb = bits_for(window);
    with_dec_kind(kind, [&](auto K) {
        swb_decode_kernel<decltype(K)::value, true><<<swb_decode_grid(count), 64, 0, s>>>(D.blob, D.sub, D.s_off, D.s_len, (u32)count, lb, D.tlen, D.status,
                                                                                          D.ooff, d_text, nullptr);
        return 0;
    });
    LAUNCH_CHECK();
}

}  // namespace tdc
