// lzss_sw_decode.hip -- LZSSSlidingWindowCompressor::decompress (compressors/LZSSSlidingWindowCompressor.hpp:120-143) for the coders
// BitCoder, EliasGammaCoder and EliasDeltaCoder, on the device.  The host loop that specifies it:
// lzss_sw_host.cpp (tdc_lzss_sw_decode); it also keeps the ascii streams and the streams below the threshold of option dec_parse.
//
// The stream has no header: tokens until it ends, a literal = flag 0 + the byte, a factor = flag 1 + (p - s) + the length, p the text
// position of the token.  Under gamma / delta every field is self-delimiting, so where the token that starts at bit x ends depends on
// the bits behind x alone -- the parse of stream_parse.hpp: next(x) for every bit position, the orbit of the first bit, the tokens
// decoded side by side, segment by segment.  Under bit the distance takes bits_for(p) bits, which is constant while p stays in
// [2^(k-1), 2^k): the segment loop carries the text position beside the bit position, evaluates next() with k = bits_for(p_in) for the
// whole segment, and lets the first token whose text position has reached 2^k end the segment -- it and everything behind it are
// dropped, the next segment starts at its bit and its position with k + 1.  At most 32 such cuts per stream; a segment is shortened up
// front to what the rest of the stretch is expected to hold (the bits per text position of the segment before), so that little is
// parsed twice.
//
// Per segment: next() from an LDS image of the stream words | mark_orbit_u32 | select_by_class -> the token list | every token read
// from global memory (kind, distance, length or byte) | a 64-bit exclusive scan of the advances (1, or the length) -> text positions |
// validation (distance 0 or above the position, malformed or cut-off token) and the cut.  The token records (position, distance,
// length / byte: 12 bytes, and a class byte) stay on the device between the parse and the text pass, so the stream is parsed once; the
// text length is the scan's total and is judged before anything of its size is allocated.  Literals go to their positions, the factors
// (pos, pos - dist, len) to resolve_and_download, which takes sources that overlap their targets.
//
// Device caps (gamma / delta): a distance or length field of at most 32 value bits, a literal code of at most 8.  A wider field is no
// token here, although the host loop reads it -- no encoder writes one; the caps bound how far next() looks behind a bit position
// (SwdTok::REACH).
#include "stages.hpp"
#include "prim.hpp"
#include "stream_parse.hpp"
#include "lzss_sw_token.hpp"

#include <stdio.h>
#include <vector>

namespace tdc {

namespace {

constexpr u64 SWD_TEXT_MAX = 0xFFFFFFFEull;
constexpr u8 SWD_LIT = 0, SWD_FAC = 1, SWD_BAD = 2;               // class byte of a token
// what stream_next_kernel asks (stream_parse.hpp); a factor is the longer token
template <int KIND>
struct SwdTok {
    static constexpr u32 REACH = swd_reach(KIND);
    u32 k, lb;
    template <typename Win>
    __device__ __forceinline__ bool at(const Win& bw, u64 x, u64& end) const {
        u32 fac, dist, val;
        return swd_token<KIND>(bw, x, bw.total, k, lb, end, fac, dist, val) == 0;
    }
};

// first_bad / cut: index of the first refused token / of the first token at or behind 2^k in the segment's list (NONE32: none);
// cut_x / cut_p: that token's bit offset in the segment and its text position; exit_bit: where the last listed token ends;
// sum: text positions the listed tokens produce
struct SwdScalars { u64 exit_bit; u64 sum; u64 cut_p; u32 first_bad; u32 cut; u32 cut_x; u32 pad; };

// the tokens of a segment (offsets idx[0 .. cnt)): class, distance, length or byte, and the text positions each one produces
template <int KIND>
__global__ __launch_bounds__(256) void swd_tokens_kernel(const u32* __restrict__ s32, u64 x_in, const u32* __restrict__ idx, u32 cnt, u64 total,
                                                          u32 k, u32 lb, u32* __restrict__ tdist, u32* __restrict__ tval, u8* __restrict__ cls,
                                                          u64* __restrict__ adv, SwdScalars* __restrict__ sc) {
    const BitWinG bw{s32, total};
    for (u32 j = blockIdx.x * 256 + threadIdx.x; j < cnt; j += gridDim.x * 256) {
        u64 end; u32 fac, dist, val;
        const int st = swd_token<KIND>(bw, x_in + idx[j], total, k, lb, end, fac, dist, val);
        const bool ok = st == 0;
        tdist[j] = ok ? dist : 0u;
        tval[j] = ok ? val : 0u;
        cls[j] = !ok ? SWD_BAD : fac ? SWD_FAC : SWD_LIT;
        adv[j] = !ok ? 0ull : fac ? (u64)val : 1ull;
        if (j == cnt - 1) sc->exit_bit = end;
    }
}

// pos[j]: the exclusive scan of the advances.  Text positions, the checks that need them, and the cut at lim = 2^k (0: none).
__global__ __launch_bounds__(256) void swd_place_kernel(const u32* __restrict__ idx, const u64* __restrict__ pos, u32 cnt, u64 p_in, u64 lim,
                                                         const u32* __restrict__ tdist, u8* __restrict__ cls, u32* __restrict__ tpos,
                                                         SwdScalars* __restrict__ sc) {
    for (u32 j = blockIdx.x * 256 + threadIdx.x; j < cnt; j += gridDim.x * 256) {
        const u64 p = p_in + pos[j];
        const u8 cl = cls[j];
        const u32 d = tdist[j];
        const bool bad = cl == SWD_BAD || (cl == SWD_FAC && (d == 0u || (u64)d > p));
        if (bad) { cls[j] = SWD_BAD; atomicMin(&sc->first_bad, j); }
        tpos[j] = (u32)p;                                         // (read only once the text length has passed its check)
        if (lim && p >= lim && (j == 0 || p_in + pos[j - 1] < lim)) { sc->cut = j; sc->cut_x = idx[j]; sc->cut_p = p; }
    }
}

// factor i of the list = token fidx[i]
__global__ __launch_bounds__(256) void swd_factor_kernel(const u32* __restrict__ fidx, size_t zf, const u32* __restrict__ tpos,
                                                          const u32* __restrict__ tdist, const u32* __restrict__ tval, u32* __restrict__ fpos,
                                                          u32* __restrict__ fsrc, u32* __restrict__ flen) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < zf; i += stride) {
        const u32 j = fidx[i], p = tpos[j];
        fpos[i] = p; fsrc[i] = p - tdist[j]; flen[i] = tval[j];
    }
}

__global__ __launch_bounds__(256) void swd_literal_kernel(const u32* __restrict__ tpos, const u32* __restrict__ tval, const u8* __restrict__ cls,
                                                           size_t z, size_t n, u8* __restrict__ text) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < z; j += stride)
        if (cls[j] == SWD_LIT && (size_t)tpos[j] < n) text[tpos[j]] = (u8)tval[j];
}

struct SwdParse { size_t z = 0; u64 n = 0; SegCount seg; };

// The segments of the stream (stream_parse.hpp).  tpos / tdist / tval / cls: zcap entries each.  More tokens than zcap:
// DecodeItemOverflow, before anything is written behind zcap.
template <int KIND>
SwdParse swd_parse(Ctx& c, const u32* s32, u64 total, u32 lb, size_t zcap, u32* tpos, u32* tdist, u32* tval, u8* cls, const DecTick& tick) {
    hipStream_t s = c.stream;
    SwdScalars* d_sc = (SwdScalars*)c.arena.alloc(sizeof(SwdScalars));
    SwdParse r;
    u64 p_in = 0, lim = 0;
    u32 k = 0;
    double rate = 9.0;                                            // bits per text position, as the segment before had them (bit: a literal's)
    r.seg = parse_segments(c, s32, total, 0, "token list", "corrupt stream: token chain", tick,
        [&](u64, u64& mm) {
            k = 0; lim = 0;
            if (KIND == DEC_BIT) {
                k = bits_for(p_in);                               // (p_in <= 2^32 - 2: k <= 32)
                if (k < 32) {
                    lim = 1ull << k;
                    const double est = (double)(lim - p_in) * rate * (1.0 + 1.0 / 64) + 4096.0;     // what the rest of the stretch should hold
                    if (est < (double)mm) mm = (u64)est;
                }
            }
            return SwdTok<KIND>{k, lb};
        },
        [&](u64 x_in, const u32* idx, u32 cnt, u32* e2) {
            if (r.z + cnt > zcap) throw DecodeItemOverflow{r.z + cnt};
            u64* adv = (u64*)e2;                                  // (a token takes 2 bits at least: cnt <= m / 2 + 1 entries fit m + 4 words)
            HIP_TRY(hipMemsetAsync(d_sc, 0xFF, sizeof(SwdScalars), s));
            const unsigned g = dec_grid(cnt);
            swd_tokens_kernel<KIND><<<g, 256, 0, s>>>(s32, x_in, idx, cnt, total, k, lb, tdist + r.z, tval + r.z, cls + r.z, adv, d_sc);
            LAUNCH_CHECK();
            exclusive_sum_u64(c, adv, adv, cnt, &d_sc->sum);
            swd_place_kernel<<<g, 256, 0, s>>>(idx, adv, cnt, p_in, lim, tdist + r.z, cls + r.z, tpos + r.z, d_sc);
            LAUNCH_CHECK();
            const SwdScalars h = c.read(d_sc);
            tick("token decode + positions");
            const u32 keep = h.cut < cnt ? h.cut : cnt;           // the tokens in front of the cut
            if (h.first_bad < keep) {
                // the host loop meets the tokens one by one: a text that has outgrown the format in front of the refused token is what it reports
                const u64 p_bad = p_in + c.read(adv + h.first_bad);
                if (p_bad > SWD_TEXT_MAX) throw DecodeTooLarge{p_bad};
                throw StreamFormatError{"corrupt stream: malformed or cut-off token, or a factor source out of range"};
            }
            // every token in front of x_out was read, and the cut is not the first one (p_in < 2^k): x_out > x_in
            u64 x_out, p_out;
            if (h.cut < cnt) { x_out = x_in + h.cut_x; p_out = h.cut_p; }
            else { x_out = h.exit_bit; p_out = p_in + h.sum; }
            r.z += keep;
            if (p_out > p_in) rate = std::max(0.01, (double)(x_out - x_in) / (double)(p_out - p_in));
            p_in = p_out;
            if (p_in > SWD_TEXT_MAX) throw DecodeTooLarge{p_in};    // (also keeps bits_for(p_in) <= 32)
            return x_out;
        });
    r.n = p_in;
    return r;
}

}  // namespace

bool decode_lzss_sw(Ctx& c, const u8* stream, size_t len, int kind, u32 window, Sink& out, size_t* need, DecodeStats* st, size_t* n_out) {
    DecodeStats local;
    if (!st) st = &local;
    *st = DecodeStats();
    *n_out = 0;
    // option dec_parse: 1 = the device for streams of 1 MiB and more, 2 = every stream, 0 = the host loop
    if (!c.dec_parse || (c.dec_parse < 2 && len < ((size_t)1 << 20))) return false;
    const u64 total = payload_bits(stream, len);
    if (total == 0) { decode_dest(out, 0); if (need) *need = 0; return true; }           // no token: the empty text
    hipStream_t s = c.stream;
    const DecTick tick = dec_ticker(c, "lzss decode");
    const u32 lb = bits_for(window);
    const u64 seg_bits = c.dec_seg ? (u64)c.dec_seg : (u64)DEC_SEG;
    const size_t seg = (size_t)std::min<u64>(seg_bits, total);
    const size_t slack = (size_t)16 << 20;
    // Tokens per stream bit.  bit: a literal takes 9 bits, and so does a factor from text position 2^(7 - lb) on; the shortest factor,
    // in front of position 2, takes 2 + lb >= 3, and so may the tokens a segment lists behind its cut, read with the narrower width
    // (they count until the cut is known) -- one per 8 bits leaves room for those.  gamma / delta: an encoder's shortest token is a
    // literal below 2 in 4 bits, the shortest the decoder reads "0" "1", the byte 0, in 2.  The arrays are sized for the first figure
    // and the parse starts over with room for the second where a stream needs it.
    u64 zcap = kind == DEC_BIT ? total / 8 + 4096 : total / 4 + 2;
    const u64 zmax = kind == DEC_BIT ? total / 3 + 4096 : total / 2 + 2;
    SwdParse P;
    u32* tpos = nullptr, *tdist = nullptr, *tval = nullptr;
    u8* cls = nullptr;
    for (;;) {
        if (zcap > 0xFFFFFFFEull) return false;                   // (token indices are 32-bit: the host loop has the verdict)
        // + 24 bytes per stream byte: room for the text pass (16 bytes per token for the factor list, 5 1/8 per text byte) of a stream that
        // does not expand much -- with the segment's scratch, free again by then; where it does not fit, the records move (regrow_arena)
        c.ensure_arena(len + 64 + (size_t)zcap * 13 + 1024 + seg * 13 + 64 + len * 24 + 2 * slack);
        void* d_stream = c.arena.get<u8>(len + 64);
        HIP_TRY(hipMemcpyAsync(d_stream, stream, len, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync((u8*)d_stream + len, 0, 64, s));
        tick("upload");
        tpos = c.arena.get<u32>(zcap); tdist = c.arena.get<u32>(zcap); tval = c.arena.get<u32>(zcap);
        cls = c.arena.get<u8>(zcap);
        try {                                                     // (arena allocations are 256-byte aligned)
            P = with_dec_kind(kind, [&](auto K) { return swd_parse<decltype(K)::value>(c, (const u32*)d_stream, total, lb, (size_t)zcap, tpos, tdist, tval, cls, tick); });
            break;
        }
        catch (const DecodeItemOverflow&) {
            if (zcap >= zmax) throw HipError{hipErrorUnknown, "lzss decode: more tokens than the stream can hold", (int)__LINE__};
            zcap = zmax;
        }
    }
    st->device_parse = 1;
    const size_t z = P.z, n = (size_t)P.n;
    if (c.dec_log)
        fprintf(stderr, "lzss decode: %u segments, next() evaluated for %llu bit positions (%.4f of the stream's %llu), %zu tokens\n", P.seg.segments,
                (unsigned long long)P.seg.evaluated, (double)P.seg.evaluated / (double)total, (unsigned long long)total, z);
    if (need) *need = n;
    *n_out = n;
    if (out.into && n > out.cap) throw HipError{hipErrorOutOfMemory, "lzss decode: the caller's buffer is too small for the text", (int)__LINE__};
    if (n == 0) { decode_dest(out, 0); return true; }              // (factors of length 0 only)

    // ---- the factor list, the literals, then the shared reference resolver
    u32* d_cnt = c.arena.get<u32>(2);
    {
        const size_t need2 = c.arena.mark() + z * 16 + n * 5 + n / 8 + 2 * slack;
        if (c.arena.size < need2) {
            void* a = tpos; void* b = tdist; void* v = tval; void* k = cls;
            regrow_arena(c, z * 29 + n * 5 + n / 8 + 2 * slack, {{&a, z * 4}, {&b, z * 4}, {&v, z * 4}, {&k, z}});
            tpos = (u32*)a; tdist = (u32*)b; tval = (u32*)v; cls = (u8*)k;
            d_cnt = c.arena.get<u32>(2);
        }
    }
    u32* fidx = c.arena.get<u32>(z);
    select_by_class(c, cls, SWD_FAC, z, nullptr, fidx, nullptr, nullptr, d_cnt);
    const size_t zf = c.read(d_cnt);
    st->factors = zf;
    u32* fpos = c.arena.get<u32>(zf + 1), *fsrc = c.arena.get<u32>(zf + 1), *flen = c.arena.get<u32>(zf + 1);
    if (zf) {
        swd_factor_kernel<<<dec_grid(zf), 256, 0, s>>>(fidx, zf, tpos, tdist, tval, fpos, fsrc, flen);
        LAUNCH_CHECK();
    }
    tick("factor list");
    u8* d_text = c.arena.get<u8>(n + 64);
    u32* d_ref = c.arena.get<u32>(n);
    swd_literal_kernel<<<dec_grid(z), 256, 0, s>>>(tpos, tval, cls, z, n, d_text);
    LAUNCH_CHECK();
    tick("literals");
    if (zf == 0) {                                                 // literals only: the text is complete
        HIP_TRY(hipMemcpyAsync(decode_dest(out, n), d_text, n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    } else resolve_and_download(c, n, d_text, d_ref, fpos, fsrc, flen, zf, d_cnt, out, st);
    tick("references + download");
    return true;
}

}  // namespace tdc
