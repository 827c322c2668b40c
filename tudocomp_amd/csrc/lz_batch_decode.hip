// lz_batch_decode.hip -- many lzw or lz78 streams decoded in one call ("Batch decoder").
//
// expand_phrases() (lz78_decode.hip) does not care whose items it expands: links that point backwards, lengths by pointer jumping,
// starts by one scan, the text by the shared resolver.  The item lists of all streams of a batch, laid back to back with their links
// rebased to global item indices, are such a forest, and its text is the texts back to back.  So the batch is ONE pass:
//   bits      per stream: the payload bits from its last one or two bytes (payload_bits / FastBits of decode.hpp, the cut-off
//             terminator refused as the host loop refuses it).
//   items     lzw + bit: the bit count fixes the number of codes (lzw_code_at; a rest is a cut-off code), a scan gives item_off, and
//             one flat launch reads every code of every stream at skew + S(j) of its own stream: no sequential work at all.
//             gamma (lzw and lz78): the item borders of one stream are sequential, so one wave takes one stream (workgroups of one
//             wave, an LDS window of the stream: the shape of swb_decode_kernel in lzss_sw_batch.hip) and walks it twice -- for the
//             count and the verdict, and behind the scan to write ids (and chars) at item_off[k] + j.  The reader is lz_pair<NV>.
//   one forest  the linking items are written rebased (lzw c >= 256 -> c + item_off[k], lz78 id >= 1 -> id + item_off[k]); item j is
//             validated against ITS stream's count (c <= 255 + j, id <= j), so nothing in front of a stream's own items is reachable.
//             phrase_lengths() | the items of refused streams get length 0 | 64-bit scan | per stream: the difference of the scan at its
//             borders is its text length (above 2^32 - 2: refused) | scan of the accepted lengths: ooff | factor list, every position
//             moved from the scan of all items to its stream's slot.
// The host reads ooff, status and the item count once, decides, and only then allocates anything text-sized (api_decompress.hip).
//
// Words other threads of the same launch write are never read (a stream's status is set by atomicMin in the code kernel and read in
// later launches only); every loop of a walk takes at least one bit per turn, so a damaged stream ends after at most its bit count.
#include "stages.hpp"
#include "prim.hpp"
#include "decode.hpp"
#include "lz_pair.hpp"
#include "lzw_offsets.hpp"

#include <algorithm>

namespace tdc {

namespace {

constexpr u64 LZB_TEXT_MAX = 0xFFFFFFFEull;
constexpr u32 LZB_WIN = 260;                                          // stream words a wave holds in LDS at a time

// bits[k] = payload_bits of stream k, status[k] = ERR_ARG for a one-byte stream that announces 6 or 7 bits (FastBits).  BIT: cnt[k] = the
// codes that fit the payload exactly, S(z) = bits (a rest: a code cut off by the end of the stream); else 0 (the walk counts).
template <bool BIT>
__global__ __launch_bounds__(256) void lzb_bits_kernel(const u8* __restrict__ blob, u64 sub, const u64* __restrict__ s_off, const u64* __restrict__ s_len,
                                                        u32 count, u64* __restrict__ bits, int* __restrict__ status, u64* __restrict__ cnt) {
    for (u32 k = blockIdx.x * 256 + threadIdx.x; k < count; k += gridDim.x * 256) {
        const u64 len = s_len[k];
        u64 total = 0, z = 0;
        int st = 0;
        if (len) {
            const u32 fb = blob[s_off[k] - sub + len - 1] & 7u;
            total = len == 1 ? fb : fb >= 6 ? 8ull * (len - 2) + fb : 8ull * (len - 1) + fb;
            if (len == 1 && fb >= 6) { st = TDC_GPU_ERR_ARG; total = 0; }
        }
        if (BIT && total) {
            u32 w;
            z = lzw_code_at(total, w);
            if (lzw_offset(z) != total) { st = TDC_GPU_ERR_ARG; z = 0; }
            else if (z > LZB_TEXT_MAX) { st = TDC_GPU_ERR_TOO_LARGE; z = 0; }      // (more codes than 2^32 - 2: more bytes)
        }
        bits[k] = total; status[k] = st; cnt[k] = z;
    }
}

// the largest k in [0, hi] with tab[k] <= i, for ascending tab with tab[0] <= i: among equal borders the last one, so an item's stream
// is never an empty one
__device__ __forceinline__ u32 lzb_stream_of(const u64* __restrict__ tab, u32 hi, u64 i) {
    u32 lo = 0;
    while (lo < hi) {
        const u32 mid = lo + (hi - lo + 1) / 2;
        if (tab[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// lzw + bit: item i of the batch is code j = i - item_off[k] of its stream k, at bit skew + S(j) from the 4-byte border in front of the
// stream (lzw_bit_codes_kernel of lzw.hip for many streams).  c > 255 + j: 0 in its place, and the stream is refused.
__global__ __launch_bounds__(256) void lzb_bit_codes_kernel(const u8* __restrict__ blob, u64 sub, const u64* __restrict__ s_off, const u64* __restrict__ bits,
                                                             const u64* __restrict__ item_off, u32 count, u64 z, u32* __restrict__ ids,
                                                             u32* __restrict__ owner, int* status) {
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < z; i += stride) {
        const u32 k = lzb_stream_of(item_off, count, i);              // (item_off[count] = z > i: at most count - 1)
        const u64 io = item_off[k], j = i - io;
        const u64 b = s_off[k] - sub;
        const u64 skew = 8ull * (b & 3ull);
        const BitWinG bw{(const u32*)(blob + (b & ~3ull)), skew + bits[k]};
        const u32 w = lzw_width(j);
        const u64 c = bw.peek(skew + lzw_offset(j)) >> (64 - w);
        const bool late = c > 255 + j;
        if (late) atomicMin(&status[k], (int)TDC_GPU_ERR_ARG);
        ids[i] = late ? 0u : c >= 256 ? (u32)(c + io) : (u32)c;       // (c + io <= 255 + i < 2^32)
        owner[i] = k;
    }
}

// gamma: one wave walks one stream.  WRITE = false: cnt[k] and the verdict of every stream the bits kernel left open -- item j must hold
// an id <= j + slack (0 for LZ78, where id j is the newest phrase; 255 for LZW, whose code 256 + j names phrase j), counted from the
// stream's own first item; a refused stream has no items.  WRITE = true (cnt = item_off, scanned): the items of the accepted streams at
// item_off[k] + j, a link (id >= base) rebased by item_off[k].
template <int NV, bool WRITE>
__global__ __launch_bounds__(64) void lzb_walk_kernel(const u8* __restrict__ blob, u64 sub, const u64* __restrict__ s_off, const u64* __restrict__ bits,
                                                       u32 count, u32 slack, u32 base, int* status, u64* cnt, u32* __restrict__ ids,
                                                       u8* __restrict__ chars, u32* __restrict__ owner) {
    constexpr u32 REACH = lz_pair_reach<NV>();
    static_assert(31 + REACH + 32 * BitWin::PEEK_WORDS <= 16 * LZB_WIN, "a refilled window must hold an item and leave half of itself for progress");
    __shared__ u32 win[LZB_WIN];
    const u32 lane = threadIdx.x;
    for (u32 sidx = blockIdx.x; sidx < count; sidx += gridDim.x) {
        const u64 total = bits[sidx];
        if (status[sidx] != 0 || total == 0) continue;
        const u64 io = WRITE ? cnt[sidx] : 0ull, zk = WRITE ? cnt[sidx + 1] - io : 0ull;
        if (WRITE && zk == 0) continue;
        // the stream's words start at the 4-byte border in front of it: its bits are [skew, T) of them
        const u64 b = s_off[sidx] - sub;
        const u32* s32 = (const u32*)(blob + (b & ~3ull));
        const u64 skew = 8ull * (b & 3ull), T = skew + total;
        const u64 wmax = (T + 31) / 32 + 3;                           // words that exist (the pad behind the blob)
        u64 x = skew, kb = 0, j = 0;
        bool loaded = false;
        int verdict = 0;
        while (x < T) {                                               // every turn takes at least one bit
            if (!loaded || x + REACH + 32 * BitWin::PEEK_WORDS > (kb + LZB_WIN) * 32) {
                __syncthreads();
                kb = x >> 5;
                for (u32 q = lane; q < LZB_WIN; q += 64) win[q] = kb + q < wmax ? __builtin_bswap32(s32[kb + q]) : 0u;
                __syncthreads();
                loaded = true;
            }
            const BitWin bw{win, kb, T};
            u64 end; u32 id, ch;
            if (lz_pair<NV>(bw, x, T, end, id, ch) != 0 || (u64)id > j + slack) { verdict = TDC_GPU_ERR_ARG; break; }
            if (WRITE) {
                if (j >= zk) break;                                   // (never: the first walk counted the same items)
                if (lane == (u32)(j & 63u)) {
                    ids[io + j] = id >= base ? id + (u32)io : id;     // (id + io <= 255 + the item's global index < 2^32)
                    if (NV == 2) chars[io + j] = (u8)ch;
                    owner[io + j] = sidx;
                }
            }
            ++j;
            x = end;
        }
        if (!WRITE && lane == 0) {
            if (verdict) status[sidx] = verdict;
            cnt[sidx] = verdict ? 0ull : j;
        }
    }
}

// the length of every item, 0 for the items of a refused stream
__global__ __launch_bounds__(256) void lzb_len_kernel(const u64* __restrict__ J, const u32* __restrict__ owner, const int* __restrict__ status, u64 z,
                                                       u64* __restrict__ L) {
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < z; i += stride) L[i] = status[owner[i]] ? 0ull : (u64)(u32)J[i];
}

// per stream: its text length is the difference of the scan S (z + 1 entries) at its borders; above 2^32 - 2: refused.  ooff[k] = the
// accepted length (scanned next); the items of the accepted streams are counted.
__global__ __launch_bounds__(256) void lzb_sizes_kernel(const u64* __restrict__ S, const u64* __restrict__ item_off, u32 count, int* __restrict__ status,
                                                         u64* __restrict__ ooff, unsigned long long* __restrict__ factors) {
    const u32 rounds = (count + gridDim.x * 256 - 1) / (gridDim.x * 256);
    for (u32 r = 0; r < rounds; ++r) {                                // (whole waves stay together for the reduction)
        const u32 k = (r * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        unsigned long long nf = 0;
        if (k < count) {
            const u64 a = item_off[k], b = item_off[k + 1];
            u64 tl = S[b] - S[a];
            if (status[k]) tl = 0;
            else if (tl > LZB_TEXT_MAX) { status[k] = TDC_GPU_ERR_TOO_LARGE; tl = 0; }
            else nf = b - a;
            ooff[k] = tl;
        }
        nf = wave_reduce_sum(nf);
        if (lane_id() == 0 && nf) atomicAdd(factors, nf);
    }
}

// Item i of an accepted stream k -> its factor and its literal, every position moved from the scan over all items to the stream's slot:
// position = S[i] - S[item_off[k]] + ooff[k].  LZ78: the factor (start_i, start_{id - 1}, len_i - 1) and the char behind it.  LZW: a code
// >= 256 is the factor (start_i, start_{c - 256}, len_i), a smaller one the literal at start_i.  The items of a refused stream: fpos =
// NONE32 and length 0 -- no factor, no literal.
template <bool LZW>
__global__ __launch_bounds__(256) void lzb_factor_kernel(const u32* __restrict__ ids, const u8* __restrict__ chars, const u32* __restrict__ owner,
                                                          const u64* __restrict__ J, const u64* __restrict__ S, const u64* __restrict__ item_off,
                                                          const u64* __restrict__ ooff, const int* __restrict__ status, u64 z,
                                                          u32* __restrict__ fpos, u32* __restrict__ fsrc, u32* __restrict__ flen, u8* __restrict__ lit) {
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < z; i += stride) {
        const u32 k = owner[i];
        if (status[k]) { fpos[i] = NONE32; fsrc[i] = 0u; flen[i] = 0u; lit[i] = 0; continue; }
        const u64 delta = ooff[k] - S[item_off[k]];
        const u32 id = ids[i];
        fpos[i] = (u32)(S[i] + delta);
        if (LZW) {
            const bool link = id >= 256u;
            fsrc[i] = link ? (u32)(S[id - 256u] + delta) : 0u;
            flen[i] = link ? (u32)J[i] : 0u;
            lit[i] = (u8)id;
        } else {
            fsrc[i] = id ? (u32)(S[id - 1u] + delta) : 0u;
            flen[i] = (u32)J[i] - 1u;
            lit[i] = chars[i];
        }
    }
}

// LZ78: the char of item i at its last text position; LZW: a literal code (the items without a factor) at its position
template <bool LZW>
__global__ __launch_bounds__(256) void lzb_literal_kernel(const u32* __restrict__ fpos, const u32* __restrict__ flen, const u8* __restrict__ lit, u64 z,
                                                           u8* __restrict__ text) {
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < z; i += stride) {
        const u32 p = fpos[i], l = flen[i];
        if (p == NONE32) continue;
        if (LZW) { if (l == 0u) text[p] = lit[i]; }
        else text[(size_t)p + l] = lit[i];
    }
}

// workgroups of one wave: as many as there are streams, up to what keeps every CU busy several times over
unsigned lzb_walk_grid(size_t count) { return (unsigned)std::min<size_t>(count, (size_t)1 << 16); }

template <bool WRITE>
void lzb_walk(Ctx& c, bool lzw, size_t count, const LzBatchDec& D, u32* ids, u8* chars, u32* owner) {
    const unsigned g = lzb_walk_grid(count);
    if (lzw) lzb_walk_kernel<1, WRITE><<<g, 64, 0, c.stream>>>(D.blob, D.sub, D.s_off, D.bits, (u32)count, 255u, 256u, D.status, D.item_off, ids, chars, owner);
    else lzb_walk_kernel<2, WRITE><<<g, 64, 0, c.stream>>>(D.blob, D.sub, D.s_off, D.bits, (u32)count, 0u, 1u, D.status, D.item_off, ids, chars, owner);
    LAUNCH_CHECK();
}

}  // namespace

void lz_batch_decode_count(Ctx& c, bool lzw, bool bit, size_t count, LzBatchDec& D) {
    if (count == 0 || count > 0xFFFFFFFEull || (bit && !lzw)) throw HipError{hipErrorInvalidValue, "lz batch decode: count or coder out of range", (int)__LINE__};
    hipStream_t s = c.stream;
    if (bit) lzb_bits_kernel<true><<<dec_grid(count), 256, 0, s>>>(D.blob, D.sub, D.s_off, D.s_len, (u32)count, D.bits, D.status, D.item_off);
    else lzb_bits_kernel<false><<<dec_grid(count), 256, 0, s>>>(D.blob, D.sub, D.s_off, D.s_len, (u32)count, D.bits, D.status, D.item_off);
    LAUNCH_CHECK();
    if (!bit) lzb_walk<false>(c, lzw, count, D, nullptr, nullptr, nullptr);
    exclusive_sum_u64(c, D.item_off, D.item_off, count, D.item_off + count);
}

u32 lz_batch_decode_sizes(Ctx& c, bool lzw, bool bit, size_t count, LzBatchDec& D, LzBatchItems& I, u32* d_changed) {
    hipStream_t s = c.stream;
    const size_t z = I.z;
    if (z == 0 || z >= 0xFFFFFFFEull - 256) throw HipError{hipErrorInvalidValue, "lz batch decode: item count out of range", (int)__LINE__};
    if (bit) {
        lzb_bit_codes_kernel<<<std::min<unsigned>(dec_grid(z), 16384u), 256, 0, s>>>(D.blob, D.sub, D.s_off, D.bits, D.item_off, (u32)count, (u64)z, I.ids,
                                                                                    I.owner, D.status);
        LAUNCH_CHECK();
    } else lzb_walk<true>(c, lzw, count, D, I.ids, I.chars, I.owner);
    const u32 rounds = phrase_lengths(c, I.ids, z, lzw ? 256u : 1u, I.J, d_changed);
    lzb_len_kernel<<<dec_grid(z), 256, 0, s>>>(I.J, I.owner, D.status, (u64)z, I.S);
    LAUNCH_CHECK();
    exclusive_sum_u64(c, I.S, I.S, z, I.S + z);
    HIP_TRY(hipMemsetAsync(D.factors, 0, sizeof(u64), s));
    lzb_sizes_kernel<<<dec_grid(count), 256, 0, s>>>(I.S, D.item_off, (u32)count, D.status, D.ooff, (unsigned long long*)D.factors);
    LAUNCH_CHECK();
    exclusive_sum_u64(c, D.ooff, D.ooff, count, D.ooff + count);
    if (lzw) lzb_factor_kernel<true><<<dec_grid(z), 256, 0, s>>>(I.ids, I.chars, I.owner, I.J, I.S, D.item_off, D.ooff, D.status, (u64)z, I.fpos, I.fsrc, I.flen, I.lit);
    else lzb_factor_kernel<false><<<dec_grid(z), 256, 0, s>>>(I.ids, I.chars, I.owner, I.J, I.S, D.item_off, D.ooff, D.status, (u64)z, I.fpos, I.fsrc, I.flen, I.lit);
    LAUNCH_CHECK();
    return rounds;
}

void lz_batch_decode_literals(Ctx& c, bool lzw, const LzBatchItems& I, u8* d_text) {
    if (lzw) lzb_literal_kernel<true><<<dec_grid(I.z), 256, 0, c.stream>>>(I.fpos, I.flen, I.lit, (u64)I.z, d_text);
    else lzb_literal_kernel<false><<<dec_grid(I.z), 256, 0, c.stream>>>(I.fpos, I.flen, I.lit, (u64)I.z, d_text);
    LAUNCH_CHECK();
}

}  // namespace tdc
