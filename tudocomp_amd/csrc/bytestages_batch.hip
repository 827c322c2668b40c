// bytestages_batch.hip -- rle, mtf and encode(huff) over a batch of independent texts (DESIGN.md section 5.3 "Batches").
//
// Layout  Text k lies at off[k], a multiple of 16, with len[k] bytes (bytestages_batch.hpp).  A kernel's unit of work is a TILE of one
//         text: text k has ceil(len[k] / tile) of them, tb[] is the exclusive sum of those counts, and the workgroup of global tile t
//         finds its text as the largest k with tb[k] <= t (a binary search; an empty text has no tile and is never found).  Inside
//         its text a tile sits where the single call's tile sits, so the kernels below are the single call's kernels with a text's
//         base and length in place of the buffer's -- position 0 of a text is "the first position" of every rule: no run reaches
//         over a border, no byte in front of a text is consulted, every text starts from the list 0 .. 255.
// rle     The one thing a unit needs from far away is where the next unit starts.  Per tile: whether it holds a unit head and where
//         its first one is; a running maximum over the tiles in reverse order names the next tile with a head, and if that tile is
//         another text's, the unit ends with its text (the first tile of every text has a head at position 0).
// mtf     Chunks of MTF_CHUNK bytes of one text.  A summary row carries a flag "closed": its range starts at its text's first chunk.
//         The scan is the single call's Hillis-Steele scan over groups of 256 with the segmented operator -- a closed row takes
//         nothing from the rows in front of it -- on as many levels as the chunk count needs; the list in front of a chunk is its
//         group's prefix, then (if that is not closed) the list in front of the group, else 0 .. 255.
// huff    Histograms of all texts in one pass (count x 256 counters), one read-back, the tables built on the host (the tie order of
//         libstdc++ is the format) on a few threads, one upload; bits per tile, one scan, sizes per text, then headers, pack and
//         terminators.  A code word may be longer than 32 bits (depth 33 needs Fib(35) = 9.2 M symbols, and rle can lengthen a text
//         of 2^20 bytes to 11.5 M), so the device table keeps 64-bit words: 2304 bytes per text with the lengths as bytes.
//
// Nothing reads what the arena held before: every array is written before it is read, and the bytes between two texts are masked by
// the text's length wherever a 16-byte load covers them.
#include "bytestages_batch.hpp"
#include "bytestages_dev.hpp"
#include "stages.hpp"
#include "bitsink.hpp"
#include "prim.hpp"
#include "huffman_host.hpp"

#include <algorithm>
#include <chrono>
#include <memory>
#include <thread>
#include <vector>

namespace tdc {
namespace {

constexpr u32 COPY_TILE = 4096;
constexpr u32 CLOSED = 1u << 16, CNT_MASK = 0x1FFu;          // a summary's count word: bytes in the row | CLOSED

inline u32 bsb_grid(u64 blocks) { return (u32)std::min<u64>(std::max<u64>(blocks, 1), BSB_MAX_BLOCKS); }
inline u32 bsb_grid256(u64 items) { return bsb_grid((items + 255) / 256); }

// the largest k with tb[k] <= t, for t < tb[count] (tb[0] = 0, not decreasing)
__device__ __forceinline__ u32 text_of(const u64* __restrict__ tb, u32 count, u64 t) {
    u32 lo = 0, hi = count;
    while (hi - lo > 1) {
        const u32 mid = lo + (hi - lo) / 2;
        if (tb[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}
// the same for a workgroup: one search, handed on through `slot` (the caller's barrier at the end of its turn frees the slot)
__device__ __forceinline__ u32 block_text_of(const u64* __restrict__ tb, u32 count, u64 t, u32* slot) {
    if (threadIdx.x == 0) *slot = text_of(tb, count, t);
    __syncthreads();
    return *slot;
}

// ---- layout ------------------------------------------------------------------------------------------------------------------------
// pad[k] = len[k] rounded up to 16 (pad != NULL), tiles[k] = ceil(len[k] / tile) (tiles != NULL)
__global__ void __launch_bounds__(256) bsb_layout_kernel(const u64* __restrict__ len, u64 count, u32 tile, u64* __restrict__ pad, u64* __restrict__ tiles) {
    for (u64 k = (u64)blockIdx.x * 256 + threadIdx.x; k < count; k += (u64)gridDim.x * 256) {
        const u64 n = len[k];
        if (pad) pad[k] = (n + 15) & ~(u64)15;
        if (tiles) tiles[k] = (n + tile - 1) / tile;
    }
}

__global__ void __launch_bounds__(256) bsb_copy_kernel(const u8* __restrict__ src, const u64* __restrict__ soff, u8* __restrict__ dst, const u64* __restrict__ doff,
                                                       const u64* __restrict__ len, const u64* __restrict__ tb, u32 count, u64 T) {
    __shared__ u32 slot;
    for (u64 tile = blockIdx.x; tile < T; tile += gridDim.x) {
        const u32 k = block_text_of(tb, count, tile, &slot);
        const u64 n = len[k], base = (tile - tb[k]) * COPY_TILE;
        const u8* s = src + soff[k];
        u8* d = dst + doff[k];
#pragma unroll 4
        for (u32 b = 0; b < COPY_TILE / 256; ++b) {
            const u64 j = base + b * 256 + threadIdx.x;
            if (j < n) d[j] = s[j];
        }
        __syncthreads();
    }
}

// out[k] = E[tb[k + 1]] - E[tb[k]]: what the tiles of text k add up to (E: exclusive sums over the tiles, T + 1 entries)
__global__ void __launch_bounds__(256) bsb_text_sum_kernel(const u64* __restrict__ E, const u64* __restrict__ tb, u64 count, u64* __restrict__ out) {
    for (u64 k = (u64)blockIdx.x * 256 + threadIdx.x; k < count; k += (u64)gridDim.x * 256) out[k] = E[tb[k + 1]] - E[tb[k]];
}

// ---- rle ---------------------------------------------------------------------------------------------------------------------------
// rev[T - 1 - tile] = T - tile if the tile holds a unit head, else 0 (an inclusive maximum over it names the next tile with a head);
// fho[tile] = where its first head lies in the tile
__global__ void __launch_bounds__(256) rleb_first_head_kernel(const u8* __restrict__ in, const u64* __restrict__ off, const u64* __restrict__ len,
                                                              const u64* __restrict__ tb, u32 count, u32 T, u32* __restrict__ rev, u32* __restrict__ fho) {
    __shared__ u32 wmin[4];
    __shared__ u32 slot;
    for (u32 tile = blockIdx.x; tile < T; tile += gridDim.x) {
        const u32 k = block_text_of(tb, count, tile, &slot);
        const size_t n = (size_t)len[k];
        const size_t tile_base = (size_t)(tile - tb[k]) * RLE_TILE, base = tile_base + (size_t)threadIdx.x * RLE_PER_THREAD;
        u32 s[17];
        load16_prev(in + off[k], n, base, s);
        u32 fh = NONE32;
#pragma unroll
        for (int j = 15; j >= 0; --j) if (base + j < n && rle_head(base + j, s[j + 1], s[j])) fh = (u32)(base + j);
        fh = wave_reduce_min(fh);
        if (lane_id() == 0) wmin[wave_id()] = fh;
        __syncthreads();
        if (threadIdx.x == 0) {
            const u32 m = min(min(wmin[0], wmin[1]), min(wmin[2], wmin[3]));
            rev[T - 1 - tile] = m == NONE32 ? 0u : T - tile;
            fho[tile] = m == NONE32 ? 0u : (u32)(m - tile_base);
        }
        __syncthreads();
    }
}

// EMIT = false: bytes the units that start in the tile emit -> tile_bytes[tile];  true: tile_bytes[] holds the exclusive sums, write them
// (text k's output starts at ooff[k]; its tiles' outputs follow each other)
template <bool EMIT>
__global__ void __launch_bounds__(256) rleb_tile_kernel(const u8* __restrict__ in, const u64* __restrict__ off, const u64* __restrict__ len,
                                                        const u64* __restrict__ tb, u32 count, u32 T, u64 o, u32 lo, const u32* __restrict__ revmax,
                                                        const u32* __restrict__ fho, u64* __restrict__ tile_bytes, const u64* __restrict__ ooff,
                                                        u8* __restrict__ out) {
    __shared__ u32 wsuf[4];
    __shared__ u32 sm[5];
    __shared__ u32 slot;
    const int lane = lane_id(), w = wave_id();
    for (u32 tile = blockIdx.x; tile < T; tile += gridDim.x) {
        const u32 k = block_text_of(tb, count, tile, &slot);
        const u64 tb0 = tb[k];
        const size_t n = (size_t)len[k];
        const size_t base = (size_t)(tile - tb0) * RLE_TILE + (size_t)threadIdx.x * RLE_PER_THREAD;
        u32 s[17];
        load16_prev(in + off[k], n, base, s);
        u32 fh = NONE32;
#pragma unroll
        for (int j = 15; j >= 0; --j) if (base + j < n && rle_head(base + j, s[j + 1], s[j])) fh = (u32)(base + j);
        // where the next unit behind this thread's 16 positions starts: suffix minimum over the threads behind it, then the tiles behind
        // (~fh turns the minimum into a maximum with 0 as "none": fh < 2^32 - 1)
        const u32 v = fh == NONE32 ? 0u : ~fh;
        u32 r = (u32)__shfl((int)v, 63 - lane, 64);
        r = wave_inclusive_max(r);
        const u32 suf = (u32)__shfl((int)r, 63 - lane, 64);          // maximum over the lanes >= lane
        u32 ex = (u32)__shfl_down((int)suf, 1, 64);
        if (lane == 63) ex = 0;
        if (lane == 0) wsuf[w] = suf;
        __syncthreads();
        for (int w2 = w + 1; w2 < 4; ++w2) if (ex == 0) ex = wsuf[w2];
        u32 next;
        if (ex) next = ~ex;
        else {
            next = (u32)n;                                            // no head behind it in its text: the unit ends with the text
            const u32 q = tile + 1 < T ? revmax[T - 2 - tile] : 0u;
            if (q) {
                const u32 t2 = T - q;                                 // the next tile with a head
                if (t2 < tb[k + 1]) next = (u32)((size_t)(t2 - tb0) * RLE_TILE + fho[t2]);
            }
        }
        u32 ln[16];
#pragma unroll
        for (int j = 15; j >= 0; --j) {
            ln[j] = 0;
            if (base + j < n && rle_head(base + j, s[j + 1], s[j])) { ln[j] = next - (u32)(base + j); next = (u32)(base + j); }
        }
        u32 bytes = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (!ln[j]) continue;
            const u32 ch = s[j + 1];
            if (ch >= 0x80u) bytes += (base + j > 0 && s[j] == ch) ? 1 + lo : 1;
            else bytes += ln[j] == 1 ? 1 : 2 + vbyte_len((u64)(ln[j] - 2) + o);
        }
        u32 total;
        const u32 pre = block_exclusive_sum<u32, 4>(bytes, sm, total);        // (ends with a barrier: wsuf and slot are free again)
        if (!EMIT) {
            if (threadIdx.x == 0) tile_bytes[tile] = total;
            continue;
        }
        u8* p = out + ooff[k] + (tile_bytes[tile] - tile_bytes[tb0]) + pre;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (!ln[j]) continue;
            const u32 ch = s[j + 1];
            *p++ = (u8)ch;
            if (ch >= 0x80u) { if (base + j > 0 && s[j] == ch) p = put_vbyte(p, o); }
            else if (ln[j] > 1) { *p++ = (u8)ch; p = put_vbyte(p, (u64)(ln[j] - 2) + o); }
        }
    }
}

// ---- mtf ---------------------------------------------------------------------------------------------------------------------------
// summary of chunk g: its distinct bytes, last occurrence first; CLOSED if it is its text's first chunk.  ctext[g] = its text
__global__ void __launch_bounds__(256) mtfb_summary_kernel(const u8* __restrict__ in, const u64* __restrict__ off, const u64* __restrict__ len,
                                                           const u64* __restrict__ cb, u32 count, u32 M, u32* __restrict__ rows, u32* __restrict__ cnt,
                                                           u32* __restrict__ ctext) {
    for (u64 gg = (u64)blockIdx.x * 256 + threadIdx.x; gg < M; gg += (u64)gridDim.x * 256) {
        const u32 g = (u32)gg;
        const u32 k = text_of(cb, count, g);
        ctext[g] = k;
        const u32 tc = g - (u32)cb[k];
        const size_t n = (size_t)len[k], start = (size_t)tc * MTF_CHUNK;
        const u8* p = in + off[k];
        Mask256 m;
        RowWriter w{rows + (size_t)g * 64};
        for (int q = MTF_CHUNK / 16 - 1; q >= 0 && w.n < 256; --q) {
            const size_t p0 = start + (size_t)q * 16;
            if (p0 >= n) continue;
            const uint4 v = *(const uint4*)(p + p0);
            const u32 x[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
            for (int b = 15; b >= 0; --b) {
                const u32 ch = (x[b >> 2] >> (8 * (b & 3))) & 255u;
                if (p0 + b < n && !m.test_set(ch)) w.push(ch);
            }
        }
        w.finish();
        cnt[g] = w.n | (tc == 0 ? CLOSED : 0u);
    }
}

// Segmented inclusive scan of the summaries inside every group of 256 rows (Hillis-Steele, rows ping-pong between A and B; eight rounds
// end in A): row g becomes the summary of rows [max(first of the group, the last text start at or in front of g), g], CLOSED if a text
// starts in that range.  The last row of a group is the group's item one level up.
__global__ void __launch_bounds__(256) mtfb_scan_kernel(u32* rowsA, u32* cntA, u32* rowsB, u32* cntB, u32 M, u32* __restrict__ up_rows,
                                                        u32* __restrict__ up_cnt) {
    const u32 t = threadIdx.x;
    const u32 groups = (M + 255) / 256;
    for (u32 grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const u32 g = grp * 256 + t;
        const bool valid = g < M;
        u32 *src = rowsA, *scnt = cntA, *dst = rowsB, *dcnt = cntB;
        for (u32 d = 1; d < 256; d <<= 1) {
            if (valid) {
                Mask256 m;
                RowWriter w{dst + (size_t)g * 64};
                const u32 c0 = scnt[g];
                u32 closed = c0 & CLOSED;
                append_new(src + (size_t)g * 64, c0 & CNT_MASK, m, w);                      // the later rows first
                if (t >= d && !closed) {                                                     // what the earlier ones add
                    const u32 c1 = scnt[g - d];
                    append_new(src + (size_t)(g - d) * 64, c1 & CNT_MASK, m, w);
                    closed = c1 & CLOSED;
                }
                w.finish();
                dcnt[g] = w.n | closed;
            }
            __syncthreads();
            u32* x = src; src = dst; dst = x;
            x = scnt; scnt = dcnt; dcnt = x;
        }
        if (valid && (t == 255 || g == M - 1)) {
            const u32 c0 = cntA[g];
            for (u32 q = 0; q * 4 < (c0 & CNT_MASK); ++q) up_rows[(size_t)grp * 64 + q] = rowsA[(size_t)g * 64 + q];
            up_cnt[grp] = c0;
        }
    }
}

// every byte value not yet in `m`, ascending: what is left of the list 0 .. 255
__device__ __forceinline__ void append_identity(Mask256& m, RowWriter& w) {
    for (u32 ch = 0; ch < 256; ++ch) if (!m.test_set(ch)) w.push(ch);
}

// list in front of item i = the prefix of its group in front of it, then -- unless a text starts in that prefix -- what is left of
// the list in front of the group (parent == nullptr: there is no level above), else of 0 .. 255
__global__ void __launch_bounds__(256) mtfb_down_kernel(const u32* __restrict__ parent, const u32* __restrict__ rows, const u32* __restrict__ cnt, u32 M,
                                                        u32* __restrict__ lists) {
    for (u64 ii = (u64)blockIdx.x * 256 + threadIdx.x; ii < M; ii += (u64)gridDim.x * 256) {
        const u32 i = (u32)ii;
        Mask256 m;
        RowWriter w{lists + (size_t)i * 64};
        bool closed = false;
        if (i & 255u) {
            const u32 c0 = cnt[i - 1];
            append_new(rows + (size_t)(i - 1) * 64, c0 & CNT_MASK, m, w);
            closed = (c0 & CLOSED) != 0;
        }
        if (parent && !closed) append_new(parent + (size_t)(i >> 8) * 64, 256, m, w);
        else append_identity(m, w);
        w.finish();
    }
}

// One workgroup per group of 256 chunks.  Entry j of thread t's list lives at byte j * 256 + (t & 63) * 4 + (t >> 6): the lanes of a wave
// hit 64 different banks whatever their j, the four waves share the words.
__global__ void __launch_bounds__(256) mtfb_encode_kernel(const u8* __restrict__ in, u8* __restrict__ out, const u64* __restrict__ off,
                                                          const u64* __restrict__ len, const u64* __restrict__ cb, const u32* __restrict__ ctext, u32 M,
                                                          const u32* __restrict__ group_lists, const u32* __restrict__ rows, const u32* __restrict__ cnt) {
    __shared__ u8 lds[65536];
    const u32 t = threadIdx.x;
    const u32 groups = (M + 255) / 256;
    u8* L = lds + (t & 63u) * 4 + (t >> 6);
    for (u32 grp = blockIdx.x; grp < groups; grp += gridDim.x) {      // (no barrier: a thread touches its own column of the LDS only)
        const u32 g = grp * 256 + t;
        if (g >= M) continue;
        const u32 k = ctext[g];
        const u32 tc = g - (u32)cb[k];
        {
            Mask256 m;
            u32 kk = 0;
            auto take = [&](const u32* __restrict__ row, u32 c) {
                for (u32 q = 0; q * 4 < c; ++q) {
                    const u32 x = row[q];
#pragma unroll
                    for (u32 b = 0; b < 4; ++b) {
                        const u32 ch = (x >> (8 * b)) & 255u;
                        if (q * 4 + b < c && !m.test_set(ch)) { L[kk * 256] = (u8)ch; ++kk; }
                    }
                }
            };
            bool closed = tc == 0;                                    // a text's first chunk starts from 0 .. 255
            if (!closed && t) {
                const u32 c0 = cnt[g - 1];
                take(rows + (size_t)(g - 1) * 64, c0 & CNT_MASK);
                closed = (c0 & CLOSED) != 0;
            }
            if (!closed) take(group_lists + (size_t)grp * 64, 256);
            else for (u32 ch = 0; ch < 256; ++ch) if (!m.test_set(ch)) { L[kk * 256] = (u8)ch; ++kk; }
        }
        const size_t n = (size_t)len[k], start = (size_t)tc * MTF_CHUNK;
        const u8* pi = in + off[k];
        u8* po = out + off[k];
        for (u32 q = 0; q < MTF_CHUNK / 16; ++q) {
            const size_t p0 = start + (size_t)q * 16;
            if (p0 >= n) break;
            const uint4 v = *(const uint4*)(pi + p0);
            const u32 x[4] = { v.x, v.y, v.z, v.w };
            u32 y[4] = { 0, 0, 0, 0 };
#pragma unroll
            for (u32 b = 0; b < 16; ++b) {
                const u32 ch = (x[b >> 2] >> (8 * (b & 3))) & 255u;
                u32 j = 0;
                if (p0 + b < n) {
                    u32 prev = ch;
                    for (;;) {                                        // the plain loop: shift the entries in front of ch back by one
                        const u32 e = L[j * 256];
                        L[j * 256] = (u8)prev;
                        if (e == ch || j == 255) break;
                        prev = e;
                        ++j;
                    }
                }
                y[b >> 2] |= j << (8 * (b & 3));
            }
            if (p0 + 16 <= n) *(uint4*)(po + p0) = make_uint4(y[0], y[1], y[2], y[3]);
            else for (u32 b = 0; p0 + b < n; ++b) po[p0 + b] = (u8)(y[b >> 2] >> (8 * (b & 3)));
        }
    }
}

// ---- encode(huff) --------------------------------------------------------------------------------------------------------------------
struct HuffDevB { u64 code[256]; u8 len[256]; };

__global__ void __launch_bounds__(256) huffb_hist_kernel(const u8* __restrict__ in, const u64* __restrict__ off, const u64* __restrict__ len,
                                                         const u64* __restrict__ tb, u32 count, u32 T, u32* __restrict__ hist) {
    __shared__ u32 h[256];
    __shared__ u32 slot;
    for (u32 tile = blockIdx.x; tile < T; tile += gridDim.x) {
        h[threadIdx.x] = 0;
        const u32 k = block_text_of(tb, count, tile, &slot);         // (its barrier also publishes the zeros)
        const size_t n = (size_t)len[k];
        const size_t base = (size_t)(tile - tb[k]) * HUFF_TILE + (size_t)threadIdx.x * HUFF_PER_THREAD;
        if (base < n) {
            const uint4 v = *(const uint4*)(in + off[k] + base);
            const u32 x[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
            for (u32 b = 0; b < 16; ++b) if (base + b < n) atomicAdd(&h[(x[b >> 2] >> (8 * (b & 3))) & 255u], 1u);
        }
        __syncthreads();
        const u32 c = h[threadIdx.x];
        if (c) atomicAdd(&hist[(size_t)k * 256 + threadIdx.x], c);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) huffb_tile_bits_kernel(const u8* __restrict__ in, const u64* __restrict__ off, const u64* __restrict__ len,
                                                              const u64* __restrict__ tb, u32 count, u32 T, const HuffDevB* __restrict__ tab,
                                                              u64* __restrict__ tile_bits) {
    __shared__ u32 cl[256];
    __shared__ u32 sm[5];
    __shared__ u32 slot;
    for (u32 tile = blockIdx.x; tile < T; tile += gridDim.x) {
        const u32 k = block_text_of(tb, count, tile, &slot);
        cl[threadIdx.x] = tab[k].len[threadIdx.x];
        __syncthreads();
        const size_t n = (size_t)len[k];
        const size_t base = (size_t)(tile - tb[k]) * HUFF_TILE + (size_t)threadIdx.x * HUFF_PER_THREAD;
        u32 bits = 0;
        if (base < n) {
            const uint4 v = *(const uint4*)(in + off[k] + base);
            const u32 x[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
            for (u32 b = 0; b < 16; ++b) if (base + b < n) bits += cl[(x[b >> 2] >> (8 * (b & 3))) & 255u];
        }
        u32 total;
        (void)block_exclusive_sum<u32, 4>(bits, sm, total);           // (ends with a barrier)
        if (threadIdx.x == 0) tile_bits[tile] = total;
    }
}

// per text: the bits of its stream (header + codes) and its length in bytes; a refused text has neither
__global__ void __launch_bounds__(256) huffb_sizes_kernel(const u64* __restrict__ E, const u64* __restrict__ tb, u64 count, const u32* __restrict__ hbits,
                                                          const int* __restrict__ status, u64* __restrict__ tbits, u64* __restrict__ out_len) {
    for (u64 k = (u64)blockIdx.x * 256 + threadIdx.x; k < count; k += (u64)gridDim.x * 256) {
        const u64 bits = (u64)hbits[k] + (E[tb[k + 1]] - E[tb[k]]);
        const bool ok = status[k] == 0;
        tbits[k] = ok ? bits : 0;
        out_len[k] = ok ? (bits >> 3) + ((bits & 7) <= 5 ? 1 : 2) : 0;      // bit_stream_len
    }
}

// the header of every accepted text, in whole words (the image is zero behind its last bit): one wave per text
__global__ void __launch_bounds__(256) huffb_header_kernel(const u64* __restrict__ hdr, const u64* __restrict__ hoff, const u32* __restrict__ hbits,
                                                           const int* __restrict__ status, u64 count, const u64* __restrict__ ooff, u8* __restrict__ out) {
    const u32 lane = lane_id();
    for (u64 k = (u64)blockIdx.x * 4 + wave_id(); k < count; k += (u64)gridDim.x * 4) {
        if (status[k] != 0) continue;
        const u32 words = (hbits[k] + 63) / 64;
        u64* dst = (u64*)(out + ooff[k]);
        for (u32 w = lane; w < words; w += 64) dst[w] = hdr[hoff[k] + w];
    }
}

__global__ void __launch_bounds__(256) huffb_pack_kernel(const u8* __restrict__ in, const u64* __restrict__ off, const u64* __restrict__ len,
                                                         const u64* __restrict__ tb, u32 count, u32 T, const HuffDevB* __restrict__ tab,
                                                         const u64* __restrict__ E, const u32* __restrict__ hbits, const u64* __restrict__ ooff,
                                                         u8* __restrict__ out) {
    __shared__ u64 code[256];
    __shared__ u32 cl[256];
    __shared__ u32 sm[5];
    __shared__ u32 slot;
    for (u32 tile = blockIdx.x; tile < T; tile += gridDim.x) {
        const u32 k = block_text_of(tb, count, tile, &slot);
        code[threadIdx.x] = tab[k].code[threadIdx.x];
        cl[threadIdx.x] = tab[k].len[threadIdx.x];
        __syncthreads();
        const u64 tb0 = tb[k];
        const size_t n = (size_t)len[k];
        const size_t base = (size_t)(tile - tb0) * HUFF_TILE + (size_t)threadIdx.x * HUFF_PER_THREAD;
        u32 x[4] = { 0, 0, 0, 0 };
        u32 bits = 0;
        if (base < n) {
            const uint4 v = *(const uint4*)(in + off[k] + base);
            x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
#pragma unroll
            for (u32 b = 0; b < 16; ++b) if (base + b < n) bits += cl[(x[b >> 2] >> (8 * (b & 3))) & 255u];
        }
        u32 total;
        const u32 pre = block_exclusive_sum<u32, 4>(bits, sm, total);
        if (base < n) {
            BitSink sink;
            sink.out = (u64*)(out + ooff[k]);                         // (a multiple of 16: no two streams share a word)
            sink.pos = (u64)hbits[k] + (E[tile] - E[tb0]) + pre;
            sink.acc = 0;
            sink.cnt = 0;
#pragma unroll
            for (u32 b = 0; b < 16; ++b) {
                const u32 ch = (x[b >> 2] >> (8 * (b & 3))) & 255u;
                if (base + b < n) sink.append(code[ch], cl[ch]);       // (nothing behind the text)
            }
            sink.flush();
        }
        __syncthreads();                                              // the tables and the slot are free again
    }
}

// io/BitOStream.hpp:53-64, per text (bit_stream_terminator)
__global__ void __launch_bounds__(256) huffb_terminator_kernel(const u64* __restrict__ tbits, const int* __restrict__ status, u64 count,
                                                               const u64* __restrict__ ooff, u8* __restrict__ out) {
    for (u64 k = (u64)blockIdx.x * 256 + threadIdx.x; k < count; k += (u64)gridDim.x * 256) {
        if (status[k] != 0) continue;
        const u64 bits = tbits[k];
        u8* p = out + ooff[k] + (bits >> 3);
        const u32 u = (u32)(bits & 7);
        if (u <= 5) p[0] |= (u8)u;
        else p[1] = (u8)u;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
// exclusive sums of a[0 .. n) in place, the total behind them at a[n]; returns the total
u64 scan_in_place(Ctx& c, u64* a, size_t n) {
    if (n == 0) { HIP_TRY(hipMemsetAsync(a, 0, sizeof(u64), c.stream)); return 0; }
    exclusive_sum_u64(c, a, a, n, a + n);
    return c.read(a + n);
}
// tb[] for tiles of `tile` bytes (count + 1 entries from the arena); T = the number of tiles
u64* make_tiles(Ctx& c, const u64* d_len, size_t count, u32 tile, u64* T) {
    u64* tb = c.arena.get<u64>(count + 1);
    bsb_layout_kernel<<<bsb_grid256(count), 256, 0, c.stream>>>(d_len, count, tile, nullptr, tb);
    LAUNCH_CHECK();
    *T = scan_in_place(c, tb, count);
    return tb;
}
// the sum of a device array (scratch: n + 1 entries from the arena)
u64 device_sum(Ctx& c, const u64* a, size_t n) {
    u64* tmp = c.arena.get<u64>(n + 1);
    exclusive_sum_u64(c, a, tmp, n, tmp + n);
    return c.read(tmp + n);
}

}  // namespace

void batch_layout(Ctx& c, BatchLay& lay, size_t count) {
    lay.off = c.arena.get<u64>(count + 1);
    bsb_layout_kernel<<<bsb_grid256(count), 256, 0, c.stream>>>(lay.len, count, 1, lay.off, nullptr);
    LAUNCH_CHECK();
    lay.padded = scan_in_place(c, lay.off, count);
}

void batch_relayout(Ctx& c, const u8* src, const u64* soff, u8* dst, const u64* doff, const u64* len, size_t count) {
    u64 T;
    const u64* tb = make_tiles(c, len, count, COPY_TILE, &T);
    if (!T) return;
    bsb_copy_kernel<<<bsb_grid(T), 256, 0, c.stream>>>(src, soff, dst, doff, len, tb, (u32)count, T);
    LAUNCH_CHECK();
}

BatchLay rle_encode_batch(Ctx& c, const BatchLay& in, size_t count, u64 offset, const BatchSizesHook& hook) {
    hipStream_t s = c.stream;
    BatchLay r;
    r.len = c.arena.get<u64>(count);
    u64 T64;
    const u64* tb = make_tiles(c, in.len, count, RLE_TILE, &T64);
    const u32 T = (u32)T64;                                   // (at most 2^32 / 4096 + 2^31 tiles)
    u32* rev = c.arena.get<u32>((size_t)T + 1);
    u32* fho = c.arena.get<u32>((size_t)T + 1);
    u64* E = c.arena.get<u64>((size_t)T + 1);
    const u32 lo = vbyte_len(offset);
    if (T) {
        rleb_first_head_kernel<<<bsb_grid(T), 256, 0, s>>>(in.d, in.off, in.len, tb, (u32)count, T, rev, fho);
        LAUNCH_CHECK();
        inclusive_max_u32(c, rev, rev, T);
        rleb_tile_kernel<false><<<bsb_grid(T), 256, 0, s>>>(in.d, in.off, in.len, tb, (u32)count, T, offset, lo, rev, fho, E, nullptr, nullptr);
        LAUNCH_CHECK();
    }
    r.total = scan_in_place(c, E, T);
    if (r.total > STAGE_MAX_BYTES) throw StageTooLarge{r.total};
    bsb_text_sum_kernel<<<bsb_grid256(count), 256, 0, s>>>(E, tb, count, r.len);
    LAUNCH_CHECK();
    if (hook) hook(r.len);
    batch_layout(c, r, count);
    r.d = c.arena.get<u8>(r.padded + 64);
    if (T) {
        rleb_tile_kernel<true><<<bsb_grid(T), 256, 0, s>>>(in.d, in.off, in.len, tb, (u32)count, T, offset, lo, rev, fho, E, r.off, r.d);
        LAUNCH_CHECK();
    }
    return r;
}

BatchLay mtf_encode_batch(Ctx& c, const BatchLay& in, size_t count, const BatchSizesHook& hook) {
    hipStream_t s = c.stream;
    if (hook) hook(in.len);                                   // (the lengths are the input's)
    BatchLay r = in;
    r.d = c.arena.get<u8>(in.padded + 64);
    u64 M64;
    const u64* cb = make_tiles(c, in.len, count, MTF_CHUNK, &M64);
    if (!M64) return r;
    // level 0: chunks; level l + 1: groups of 256 items of level l, until one group holds a level (at least two levels: the encoder
    // takes a list per group of chunks)
    std::vector<u32> M{ (u32)M64 };
    while (M.size() < 2 || M.back() > 256) M.push_back(cdiv(M.back(), 256));
    const size_t L = M.size();
    std::vector<u32*> rowsA(L), rowsB(L), cntA(L), cntB(L), lists(L, nullptr);
    for (size_t l = 0; l < L; ++l) {
        rowsA[l] = c.arena.get<u32>((size_t)M[l] * 64); rowsB[l] = c.arena.get<u32>((size_t)M[l] * 64);
        cntA[l] = c.arena.get<u32>(M[l]); cntB[l] = c.arena.get<u32>(M[l]);
        if (l) lists[l] = c.arena.get<u32>((size_t)M[l] * 64);
    }
    u32* top_row = c.arena.get<u32>(64);                      // (the top level is one group: its item is nobody's)
    u32* top_cnt = c.arena.get<u32>(1);
    u32* ctext = c.arena.get<u32>(M[0]);
    mtfb_summary_kernel<<<bsb_grid256(M[0]), 256, 0, s>>>(in.d, in.off, in.len, cb, (u32)count, M[0], rowsA[0], cntA[0], ctext);
    LAUNCH_CHECK();
    for (size_t l = 0; l < L; ++l) {
        const bool top = l + 1 == L;
        mtfb_scan_kernel<<<bsb_grid(cdiv(M[l], 256)), 256, 0, s>>>(rowsA[l], cntA[l], rowsB[l], cntB[l], M[l], top ? top_row : rowsA[l + 1], top ? top_cnt : cntA[l + 1]);
        LAUNCH_CHECK();
    }
    for (size_t l = L - 1; l >= 1; --l) {
        mtfb_down_kernel<<<bsb_grid256(M[l]), 256, 0, s>>>(l + 1 == L ? nullptr : lists[l + 1], rowsA[l], cntA[l], M[l], lists[l]);
        LAUNCH_CHECK();
    }
    mtfb_encode_kernel<<<bsb_grid(M[1]), 256, 0, s>>>(in.d, r.d, in.off, in.len, cb, ctext, M[0], lists[1], rowsA[0], cntA[0]);
    LAUNCH_CHECK();
    return r;
}

BatchLay huff_literals_batch(Ctx& c, const BatchLay& in, size_t count, const int* d_status, const int32_t* status, u32 threads, BatchHuffInfo* info,
                             const BatchSizesHook& hook) {
    if (!c.huff_ok) throw HipError{hipErrorUnknown, "encode(huff): the Huffman self-check of this build failed", (int)__LINE__};
    hipStream_t s = c.stream;
    BatchLay r;
    r.len = c.arena.get<u64>(count);
    u64 T64;
    const u64* tb = make_tiles(c, in.len, count, HUFF_TILE, &T64);
    const u32 T = (u32)T64;
    // histograms of all texts, one read-back
    u32* d_hist = c.arena.get<u32>(count * 256);
    HIP_TRY(hipMemsetAsync(d_hist, 0, count * 256 * sizeof(u32), s));
    if (T) {
        huffb_hist_kernel<<<bsb_grid(T), 256, 0, s>>>(in.d, in.off, in.len, tb, (u32)count, T, d_hist);
        LAUNCH_CHECK();
    }
    std::unique_ptr<u32[]> hist(new u32[count * 256]);
    c.read_n(d_hist, hist.get(), count * 256);
    // the tables and headers of the accepted texts, on the host: worker j takes the texts [j, j + 1) * per and writes their headers, each
    // padded with zeros to whole words, into a buffer of its own
    const auto t0 = std::chrono::steady_clock::now();
    const u32 hw = std::max(1u, std::thread::hardware_concurrency());
    u32 workers = threads ? std::min(threads, 16u) : std::min(16u, hw);
    workers = (u32)std::min<size_t>(workers, (count + 255) / 256);    // (a thread is not worth fewer than 256 tables)
    std::unique_ptr<HuffDevB[]> tab(new HuffDevB[count]);
    std::vector<u32> hbits(count);
    std::vector<u64> hoff(count + 1);
    std::vector<std::vector<u8>> part(workers);
    const size_t per = (count + workers - 1) / workers;
    auto build = [&](u32 j) {
        std::vector<u8>& buf = part[j];
        for (size_t k = j * per; k < std::min(count, (j + 1) * per); ++k) {
            hoff[k] = buf.size() / 8;                                 // (in its worker's buffer for now)
            hbits[k] = 0;
            if (status[k] != 0) { memset(&tab[k], 0, sizeof(HuffDevB)); continue; }
            HuffTable ht;
            build_huffman_table(hist.get() + k * 256, &ht);
            HostBitWriter w;
            write_huffman_header(w, ht);
            for (int i = 0; i < 256; ++i) {                          // (sigma <= 1: eight raw bits per byte, HuffmanCoder.hpp:562-569)
                tab[k].code[i] = ht.sigma <= 1 ? (u64)i : ht.code_of[i];
                tab[k].len[i] = ht.sigma <= 1 ? (u8)8 : ht.len_of[i];
            }
            hbits[k] = (u32)w.nbits;
            buf.insert(buf.end(), w.bytes.begin(), w.bytes.end());
            buf.resize((buf.size() + 7) / 8 * 8, 0);
        }
    };
    if (workers <= 1) build(0);
    else {
        std::vector<std::thread> pool;
        for (u32 j = 0; j < workers; ++j) pool.emplace_back(build, j);
        for (auto& t : pool) t.join();
    }
    std::vector<u8> hdr;
    for (u32 j = 0; j < workers; ++j) {
        const u64 base = hdr.size() / 8;
        for (size_t k = j * per; k < std::min(count, (j + 1) * per); ++k) hoff[k] += base;
        hdr.insert(hdr.end(), part[j].begin(), part[j].end());
    }
    hoff[count] = hdr.size() / 8;
    if (info) { info->ms_tables = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(); info->threads = workers; }
    // one upload each of the tables, the headers, their places and their bits
    HuffDevB* d_tab = (HuffDevB*)c.arena.alloc(count * sizeof(HuffDevB));
    u64* d_hdr = c.arena.get<u64>(hdr.size() / 8 + 1);
    u64* d_hoff = c.arena.get<u64>(count + 1);
    u32* d_hbits = c.arena.get<u32>(count);
    HIP_TRY(hipMemcpyAsync(d_tab, tab.get(), count * sizeof(HuffDevB), hipMemcpyHostToDevice, s));
    if (!hdr.empty()) HIP_TRY(hipMemcpyAsync(d_hdr, hdr.data(), hdr.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_hoff, hoff.data(), (count + 1) * sizeof(u64), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_hbits, hbits.data(), count * sizeof(u32), hipMemcpyHostToDevice, s));
    u64* E = c.arena.get<u64>((size_t)T + 1);
    u64* tbits = c.arena.get<u64>(count);
    if (T) {
        huffb_tile_bits_kernel<<<bsb_grid(T), 256, 0, s>>>(in.d, in.off, in.len, tb, (u32)count, T, d_tab, E);
        LAUNCH_CHECK();
    }
    (void)scan_in_place(c, E, T);                                     // (synchronises: the host buffers above are free)
    huffb_sizes_kernel<<<bsb_grid256(count), 256, 0, s>>>(E, tb, count, d_hbits, d_status, tbits, r.len);
    LAUNCH_CHECK();
    r.total = device_sum(c, r.len, count);
    if (r.total > STAGE_MAX_BYTES) throw StageTooLarge{r.total};
    if (hook) hook(r.len);
    batch_layout(c, r, count);
    r.d = c.arena.get<u8>(r.padded + 64);
    HIP_TRY(hipMemsetAsync(r.d, 0, r.padded, s));
    huffb_header_kernel<<<bsb_grid((count + 3) / 4), 256, 0, s>>>(d_hdr, d_hoff, d_hbits, d_status, count, r.off, r.d);
    LAUNCH_CHECK();
    if (T) {
        huffb_pack_kernel<<<bsb_grid(T), 256, 0, s>>>(in.d, in.off, in.len, tb, (u32)count, T, d_tab, E, d_hbits, r.off, r.d);
        LAUNCH_CHECK();
    }
    huffb_terminator_kernel<<<bsb_grid256(count), 256, 0, s>>>(tbits, d_status, count, r.off, r.d);
    LAUNCH_CHECK();
    return r;
}

}  // namespace tdc
