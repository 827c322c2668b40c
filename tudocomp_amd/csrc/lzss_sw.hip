// lzss_sw.hip -- lzss = LZSSSlidingWindowCompressor (compressors/LZSSSlidingWindowCompressor.hpp:39-118): the sliding-window LZ77
// factorization on the device.  The host loop that specifies it: lzss_sw_host.cpp.
//
// Whether position p starts a factor, and which one, depends only on the text within `window` bytes in front of p and at most
// 2 * window bytes behind it (the closed form of the reference's buffer, stated in lzss_sw_host.cpp), so one lane computes it for every
// position without knowing the positions in front of it:
//   match kernel   a workgroup takes SW_TILE positions; their text, the window in front and the look-ahead behind -- [t0 - w,
//                  t0 + SW_TILE + 2w) -- go into LDS.  One lane per position walks the sources s ascending (the reference's order, and
//                  its strict `>`: the smallest s among the longest matches wins) and compares 8-byte words; the word of s + 1 is the
//                  word of s shifted by one byte with one new byte from LDS, so a candidate costs one LDS byte read until a whole word
//                  matches.  A lane stops as soon as best == L(p): nothing can beat it, and runs or periodic texts, whose first
//                  candidate already reaches L, cost one candidate per position instead of w.
//   the parse      next(p) = p + max(1, len(p)); the tokens are the orbit of position 0 (mark_orbit_u32), listed by select_by_class.
// The tokens then go through lzss_sw_encode_tokens: the cost pass, scan, pack and terminator of field_coder.hpp over SwTokens below.
//
// Worst case of the match kernel: n * w * L / 8 word compares, on texts built so that many candidates match almost to L.
#include "stages.hpp"
#include "field_coder.hpp"
#include "decode.hpp"

#include <algorithm>

namespace tdc {

namespace {

// positions per workgroup; with the largest window the LDS image is 4096 (window, 8-byte aligned) + SW_TILE + 2 * 4096 (look-ahead) bytes
// = 16 KiB, plus one word that the last 8-byte read reaches into
constexpr u32 SW_TILE = 4096;
constexpr u32 SW_LDS_WORDS = (SW_TILE + 3 * LZSS_SW_MAX_WINDOW) / 8 + 2;

// the 8 bytes from byte i of the image on, byte i in the low bits
__device__ __forceinline__ u64 sw_word(const u64* img, u32 i) {
    const u32 k = i >> 3, sh = (i & 7u) * 8u;
    const u64 a = img[k];
    return sh ? (a >> sh) | (img[k + 1] << (64u - sh)) : a;
}

__global__ __launch_bounds__(256) void lzss_sw_match_kernel(const u8* __restrict__ text, u64 n, u32 w, u32 t, u32 tiles,
                                                             u32* __restrict__ next, u32* __restrict__ fac) {
    __shared__ u64 img[SW_LDS_WORDS];
    const u8* imgb = (const u8*)img;
    const u32 wpad = (w + 7u) & ~7u;                                  // the image starts 8-byte aligned in the text: at t0 - wpad
    const u32 words = (wpad + SW_TILE + 2u * w + 15u) >> 3;           // <= SW_LDS_WORDS - 1; reads reach byte wpad + SW_TILE + 2w + 5
    for (u32 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const u64 t0 = (u64)tile * SW_TILE;
        for (u32 k = threadIdx.x; k < words; k += 256) {
            const long long g = (long long)t0 - (long long)wpad + 8ll * k;      // text position of the word's first byte
            u64 v = 0;
            if (g >= 0 && (u64)g + 8 <= n) v = *(const u64*)(text + g);
            else if (g >= 0) { for (u32 b = 0; b < 8 && (u64)g + b < n; ++b) v |= (u64)text[g + b] << (8u * b); }   // zeros behind the text
            img[k] = v;
        }
        __syncthreads();
        for (u32 k = threadIdx.x; k < SW_TILE; k += 256) {
            const u64 p = t0 + k;
            if (p >= n) break;
            u64 end = n;
            if (n >= 2ull * w) { const u64 off = p > w ? p - w : 0; end = (off < n - 2ull * w ? off : n - 2ull * w) + 2ull * w; }
            const u32 L = (u32)(end - p);
            const u32 ip = k + wpad;                                  // p in the image
            const u32 cand = p < w ? (u32)p : w;                      // sources p - cand .. p - 1
            const u32 is = ip - cand;
            u32 best = 0, bdist = 0;
            if (cand) {
                const u64 P = sw_word(img, ip);
                u64 S = sw_word(img, is);
                for (u32 c = 0; c < cand; ++c) {
                    u64 x = S ^ P;
                    u32 j;
                    if (x) j = (u32)__builtin_ctzll(x) >> 3;
                    else {
                        j = 8;
                        while (j < L) {
                            x = sw_word(img, is + c + j) ^ sw_word(img, ip + j);
                            if (x) { j += (u32)__builtin_ctzll(x) >> 3; break; }
                            j += 8;
                        }
                    }
                    j = j < L ? j : L;
                    if (j >= t && j > best) { best = j; bdist = cand - c; if (best == L) break; }
                    S = (S >> 8) | ((u64)imgb[is + c + 8] << 56);
                }
            }
            next[p] = (u32)(p + (best ? best : 1u));
            fac[p] = best ? (bdist << 16) | best : 0u;               // (distance <= 4096, length <= 8191)
        }
        __syncthreads();
    }
}

// the factors among the tokens: cls[i] = 1 where token i is one
__global__ __launch_bounds__(256) void lzss_sw_factor_class_kernel(const u32* __restrict__ tokpos, const u32* __restrict__ fac, u64 ntok,
                                                                    u8* __restrict__ cls) {
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < ntok; i += stride) cls[i] = fac[tokpos[i]] ? 1 : 0;
}
__global__ __launch_bounds__(256) void lzss_sw_factor_emit_kernel(const u32* __restrict__ fac, u64 z, const u32* __restrict__ pos,
                                                                   u32* __restrict__ src, u32* __restrict__ len) {
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < z; i += stride) {
        const u32 p = pos[i], f = fac[p];
        src[i] = p - (f >> 16);
        len[i] = f & 0xFFFFu;
    }
}

// ---- the tokens through one coder (LZSSSlidingWindowCompressor.hpp:85-95): the source of field_coder.hpp ------------------------------
// Token i starts at text position tokpos[i]; fac[p] = distance << 16 | length, 0 for a literal.  A literal is the flag 0 and the byte
// under literal_r; a factor the flag 1, the distance under Range(0, p) and the length under Range(0, window).  BitCoder: bits_for(p) and
// wbits = bits_for(window) bits (the one field whose width depends on where the token stands: hence a cost pass over the tokens instead of
// closed-form offsets); gamma / delta ignore the ranges; ASCIICoder writes '0' / '1', decimal digits with ':' and the byte.
// The cost pass also counts the factors and finds the longest one, and whether BitCoder would drop bits of a length.
struct SwScalars { unsigned long long factors; u32 flen_max, trunc; };

struct SwTokens {
    const u8* __restrict__ text;
    const u32* __restrict__ tokpos;
    const u32* __restrict__ fac;
    u32 wbits;
    SwScalars* sc;
    struct Item { u32 pos = 0, f = 0, ch = 0; };     // ch: the byte at pos (read for a factor too: no branch on f between the loads)
    template <int KIND, bool COST_ONLY> __device__ __forceinline__ void load(u64 i, Item& it) const {
        it.pos = tokpos[i]; it.f = fac[it.pos];
        if (!COST_ONLY || KIND == ENC_GAMMA || KIND == ENC_DELTA) it.ch = text[it.pos];       // (bit and ascii: every byte costs 8 bits)
    }
    template <int KIND> __device__ __forceinline__ u32 bits(const Item& it) const {
        return flag_cost<KIND>() + (it.f ? int_cost<KIND>(it.f >> 16, uni_bits_for(it.pos)) + int_cost<KIND>(it.f & 0xFFFFu, wbits) : byte_cost<KIND>(it.ch));
    }
    template <int KIND> __device__ __forceinline__ void put(BitSink& sink, const Item& it) const {
        append_flag<KIND>(sink, it.f ? 1u : 0u);
        if (!it.f) append_byte<KIND>(sink, it.ch);                                                  // :94-95
        else { append_int<KIND>(sink, it.f >> 16, uni_bits_for(it.pos)); append_int<KIND>(sink, it.f & 0xFFFFu, wbits); }     // :87-89
    }
    struct Tally {
        u32 nfac = 0, lmax = 0;
        __device__ __forceinline__ void note(const SwTokens&, const Item& it) { nfac += it.f ? 1u : 0u; lmax = max(lmax, it.f & 0xFFFFu); }
        template <int KIND> __device__ __forceinline__ void commit(const SwTokens& src) {
            nfac = wave_reduce_sum(nfac);
            lmax = wave_reduce_max(lmax);
            if (lane_id() == 0) {
                if (nfac) atomicAdd(&src.sc->factors, (unsigned long long)nfac);
                if (lmax) atomicMax(&src.sc->flen_max, lmax);
                if (KIND == ENC_TAB && (lmax >> src.wbits)) atomicOr(&src.sc->trunc, 1u);      // write_int would drop the length's top bits
            }
        }
    };
};

}  // namespace

// lzss (LZSSSlidingWindowCompressor.hpp:85-95; kind 0 = BitCoder, 1 = ASCIICoder, 2 = EliasGammaCoder, 3 = EliasDeltaCoder): no header, and
// every token covers at least one text byte, so the worst case is n times the costliest token.  A literal is the flag and the byte: 1 + 8
// bits, '0' and the byte = 16, 1 + gamma(255) = 1 + 17, 1 + delta(255) = 1 + 17.  A factor is the flag, a distance <= w and a length
// <= 2w - 1 (both coders' costs grow with the value):
//   bit    1 + bits_for(p) + bits_for(w) <= 1 + bits_for(n) + bits_for(w)
//   ascii  8 * (1 + digits(w) + 1 + digits(2w - 1) + 1)
//   gamma  1 + (2 bits_for(w) + 1) + (2 bits_for(2w - 1) + 1)
//   delta  1 + delta_bits(w) + delta_bits(2w - 1),  delta_bits(v) = 2 bits_for(bits_for(v)) + 1 + bits_for(v)
// + 2: the terminator (the count of the last byte's bits, in that byte or in one of its own).
size_t lzss_sw_bound(size_t n, u32 window, int kind) {
    if (kind < 0 || kind > 3 || window == 0 || window > LZSS_SW_MAX_WINDOW || n > 0xFFFFFFFEull) return 0;
    const u64 w = window, l = 2 * w - 1;
    auto digits = [](u64 v) { u64 d = 1; while (v >= 10) { v /= 10; ++d; } return d; };
    auto delta_bits = [](u64 v) { return 2 * (u64)bits_for(bits_for(v)) + 1 + bits_for(v); };
    u64 lit, fac;
    switch (kind) {
        case 0:  lit = 9;  fac = 1 + (u64)bits_for(n) + bits_for(w); break;
        case 1:  lit = 16; fac = 8 * (1 + digits(w) + 1 + digits(l) + 1); break;
        case 2:  lit = 18; fac = 1 + (2 * (u64)bits_for(w) + 1) + (2 * (u64)bits_for(l) + 1); break;
        default: lit = 18; fac = 1 + delta_bits(w) + delta_bits(l); break;
    }
    return (size_t)(((u64)n * std::max(lit, fac) + 7) / 8 + 2);
}

size_t lzss_sw_encode_tokens(Ctx& c, const u8* d_text, const u32* tokpos, const u32* fac, size_t ntok, u32 window, int kind,
                             u8* d_out, size_t out_cap, LzssSwStats* st) {
    LzssSwStats local;
    if (!st) st = &local;
    *st = LzssSwStats();
    if (kind < 0 || kind > 3) throw HipError{hipErrorInvalidValue, "lzss: no such coder", (int)__LINE__};
    const size_t mark = c.arena.mark();
    SwScalars* d_sc = nullptr;                                                                      // (an empty list: no cost pass, no tally)
    if (ntok) {
        d_sc = (SwScalars*)c.arena.alloc(sizeof(SwScalars));
        HIP_TRY(hipMemsetAsync(d_sc, 0, sizeof(SwScalars), c.stream));
    }
    const size_t len = encode_fields(c, SwTokens{ d_text, tokpos, fac, bits_for(window), d_sc }, (u64)ntok, kind, d_out, out_cap,
                                     "lzss: output buffer too small", [&] {
        const SwScalars h = c.read(d_sc);
        st->factors = h.factors; st->flen_max = h.flen_max; st->truncates = h.trunc != 0;
        return !st->truncates;                                                                      // BitCoder would truncate: nothing is packed
    });
    c.arena.release(mark);
    return len;
}

size_t lzss_sw_tokens(Ctx& c, const u8* d_text, size_t n, u32 window, u32 threshold, u32** tokpos, u32** fac_out) {
    *tokpos = nullptr; *fac_out = nullptr;
    if (n == 0) return 0;
    if (window == 0 || window > LZSS_SW_MAX_WINDOW || n > 0xFFFFFFFEull) throw HipError{hipErrorInvalidValue, "lzss: window or text length out of range", (int)__LINE__};
    hipStream_t s = c.stream;
    u32* next = c.arena.get<u32>(n);
    u32* fac = c.arena.get<u32>(n);
    u32* s1 = c.arena.get<u32>(n), *s2 = c.arena.get<u32>(n);
    u8* mark = c.arena.get<u8>(n);
    u32* d_cnt = c.arena.get<u32>(1);
    const size_t tiles = (n + SW_TILE - 1) / SW_TILE;                 // < 2^20
    lzss_sw_match_kernel<<<dec_grid(tiles * 256), 256, 0, s>>>(d_text, (u64)n, window, threshold ? threshold : 1u, (u32)tiles, next, fac);
    LAUNCH_CHECK();
    mark_orbit_u32(c, next, n, mark, s1, s2);
    select_by_class(c, mark, 1, n, nullptr, s1, nullptr, nullptr, d_cnt);      // (s1 is free again: the token positions)
    const size_t ntok = c.read(d_cnt);
    *tokpos = s1; *fac_out = fac;
    return ntok;
}

size_t lzss_sw_factor_list(Ctx& c, const u32* tokpos, const u32* fac, size_t ntok, u32* d_pos, u32* d_src, u32* d_len) {
    if (ntok == 0) return 0;
    hipStream_t s = c.stream;
    const size_t mark0 = c.arena.mark();
    u8* cls = c.arena.get<u8>(ntok);
    u32* d_cnt = c.arena.get<u32>(1);
    lzss_sw_factor_class_kernel<<<dec_grid(ntok), 256, 0, s>>>(tokpos, fac, (u64)ntok, cls);
    LAUNCH_CHECK();
    select_by_class(c, cls, 1, ntok, tokpos, d_pos, nullptr, nullptr, d_cnt);
    const size_t z = c.read(d_cnt);
    if (z) {
        lzss_sw_factor_emit_kernel<<<dec_grid(z), 256, 0, s>>>(fac, (u64)z, d_pos, d_src, d_len);
        LAUNCH_CHECK();
    }
    c.arena.release(mark0);
    return z;
}

}  // namespace tdc
