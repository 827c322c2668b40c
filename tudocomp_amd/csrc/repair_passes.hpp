// repair_passes.hpp -- what the single decoder of repair streams (repair_decode.hip) and the batch decoder (repair_batch_decode.hip) share:
// the token reader with the device caps -- the refusal rules stand here and nowhere else --, and the passes that turn a grammar, or a forest
// of grammars, into literals and a factor list.  The passes do not care whose rules they visit: sym[2 k], sym[2 k + 1] are the sides of
// rule k, sym[2 R + j] is start symbol j, a symbol below 256 is a byte and 256 + v names rule v < k (a side) or v < R (a start symbol).
// The kernels live in an unnamed namespace: every file that includes this header gets its own.
#pragma once
#include "stages.hpp"
#include "prim.hpp"
#include "stream_parse.hpp"

namespace tdc {

namespace {

constexpr u64 RPD_TEXT_MAX = 0xFFFFFFFEull;
constexpr u32 RPD_NONE = 0xFFFFFFFFu;
constexpr u32 RPD_BATCH = 8;                                      // rounds per read-back of the change flags
// class of a token: read, refused by the host loop too (a field of zeros up to the end of the stream, a cut-off token), beyond a device cap
constexpr int RPD_OK = FIELD_READ, RPD_BAD = FIELD_END, RPD_WIDE = FIELD_WIDE;
// the device caps: most value bits of an index and of a literal code, and of delta's width code in front of either
constexpr u32 RPD_INDEX_BITS = 32, RPD_LIT_BITS = 8, RPD_WBITS = 6;

// The token that starts at bit x: class, end, flag (1: a rule index) and value.  w: width of an index under bit.  A token cut off by the
// end of the stream is RPD_BAD.
template <int KIND, typename Win>
__device__ __forceinline__ int rpd_token(const Win& bw, u64 x, u64 total, u32 w, u64& end, u32& rule, u32& val) {
    end = x; rule = 0; val = 0;
    if (x >= total) return RPD_BAD;
    const u64 win = bw.peek(x);
    rule = (u32)(win >> 63);
    u64 y = x + 1;
    if (KIND == DEC_BIT) {
        if (!rule) { val = (u32)((win << 1) >> 56); y += 8; }
        else { val = (u32)(bw.peek(y) >> (64 - w)); y += w; }
    } else {
        u32 used;
        const int st = read_field<KIND>(bw, y, rule ? RPD_INDEX_BITS : RPD_LIT_BITS, RPD_WBITS, used, val);
        if (st != RPD_OK) return st;
        y += used;
    }
    if (y > total) return RPD_BAD;
    end = y;
    return RPD_OK;
}

// what stream_next_kernel asks (stream_parse.hpp); an index is the longer token
template <int KIND>
struct RpdTok {
    static constexpr u32 REACH = 1 + (KIND == DEC_BIT ? 32 : field_span(KIND, RPD_INDEX_BITS, RPD_WBITS));
    u32 w;
    template <typename Win>
    __device__ __forceinline__ bool at(const Win& bw, u64 x, u64& end) const {
        u32 rule, val;
        return rpd_token<KIND>(bw, x, bw.total, w, end, rule, val) == RPD_OK;
    }
};

// ---- the grammar's passes ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rpd_adv_kernel(const u32* __restrict__ start, u32 m, const u32* __restrict__ len, u64* __restrict__ adv) {
    for (u32 j = blockIdx.x * 256 + threadIdx.x; j < m; j += gridDim.x * 256) {
        const u32 c = start[j];
        adv[j] = c < 256u ? 1ull : (u64)len[c - 256u];
    }
}

// first[k]: the leftmost text position at which rule k is expanded
__global__ __launch_bounds__(256) void rpd_first_start_kernel(const u32* __restrict__ start, u32 m, const u64* __restrict__ pos, u32* first) {
    for (u32 j = blockIdx.x * 256 + threadIdx.x; j < m; j += gridDim.x * 256) {
        const u32 c = start[j];
        if (c >= 256u) atomicMin(&first[c - 256u], (u32)pos[j]);
    }
}

__global__ __launch_bounds__(256) void rpd_first_kernel(const u32* __restrict__ sym, u32 R, const u32* __restrict__ len, u32* first,
                                                         u32* __restrict__ changed) {
    bool any = false;
    for (u32 k = blockIdx.x * 256 + threadIdx.x; k < R; k += gridDim.x * 256) {
        const u32 f = first[k];
        if (f == RPD_NONE) continue;
        const u32 l = sym[2 * (size_t)k], r = sym[2 * (size_t)k + 1];
        if (l >= 256u) any |= atomicMin(&first[l - 256u], f) > f;
        if (r >= 256u) {
            const u32 q = f + (l < 256u ? 1u : len[l - 256u]);    // (rule k occurs: its length, and so q, is below n)
            any |= atomicMin(&first[r - 256u], q) > q;
        }
    }
    if (any) *changed = 1u;
}

// item i: start symbol i (i < m) or side (i - m) & 1 of rule (i - m) / 2.  false: a side of a rule that never occurs.
__device__ __forceinline__ bool rpd_item(size_t i, const u32* __restrict__ sym, const u64* __restrict__ pos, const u32* __restrict__ len,
                                         const u32* __restrict__ first, u32 R, u32 m, u32& c, u32& q) {
    if (i < m) { c = sym[2 * (size_t)R + i]; q = (u32)pos[i]; return true; }
    const size_t t = i - m;
    const u32 f = first[t >> 1];
    if (f == RPD_NONE) return false;
    c = sym[t];
    q = f;
    if (t & 1) { const u32 l = sym[t - 1]; q += l < 256u ? 1u : len[l - 256u]; }
    return true;
}

// literals go to the text; cls[i] = 1 where item i is a factor
__global__ __launch_bounds__(256) void rpd_item_kernel(const u32* __restrict__ sym, const u64* __restrict__ pos, const u32* __restrict__ len,
                                                        const u32* __restrict__ first, u32 R, u32 m, size_t n, u8* __restrict__ text,
                                                        u8* __restrict__ cls) {
    const size_t items = (size_t)m + 2 * (size_t)R, stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += stride) {
        u32 c, q;
        u8 cl = 0;
        if (rpd_item(i, sym, pos, len, first, R, m, c, q)) {
            if (c < 256u) { if ((size_t)q < n) text[q] = (u8)c; }
            else cl = first[c - 256u] != q;
        }
        cls[i] = cl;
    }
}

// factor i of the list = item fidx[i]: its rule's first occurrence is the source
__global__ __launch_bounds__(256) void rpd_factor_kernel(const u32* __restrict__ fidx, size_t zf, const u32* __restrict__ sym,
                                                          const u64* __restrict__ pos, const u32* __restrict__ len, const u32* __restrict__ first,
                                                          u32 R, u32 m, u32* __restrict__ fpos, u32* __restrict__ fsrc, u32* __restrict__ flen) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < zf; i += stride) {
        u32 c = 256u, q = 0;
        (void)rpd_item(fidx[i], sym, pos, len, first, R, m, c, q);
        fpos[i] = q; fsrc[i] = first[c - 256u]; flen[i] = len[c - 256u];
    }
}

// Rounds of `launch(flag)` until one leaves its flag at 0; RPD_BATCH rounds per read-back.  Returns the rounds that ran, the quiet one
// included; 0: `cap` rounds did not reach it.
template <typename Launch>
u32 rpd_rounds(Ctx& c, u32* d_flags, u32 cap, Launch&& launch) {
    u32 rounds = 0;
    while (rounds < cap) {
        const u32 b = std::min(RPD_BATCH, cap - rounds);
        HIP_TRY(hipMemsetAsync(d_flags, 0, RPD_BATCH * sizeof(u32), c.stream));
        for (u32 i = 0; i < b; ++i) { launch(d_flags + i); LAUNCH_CHECK(); }
        u32 h[RPD_BATCH];
        c.read_n(d_flags, h, (size_t)RPD_BATCH);
        for (u32 i = 0; i < b; ++i) { ++rounds; if (!h[i]) return rounds; }
    }
    return 0;
}

}  // namespace

}  // namespace tdc
