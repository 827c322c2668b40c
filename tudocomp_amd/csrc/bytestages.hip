// bytestages.hip -- rle, mtf and encode(huff) on the device: the stages behind bwt in the reference's bwtzip chain.
//   rle:  a "unit" is a maximal run of equal bytes below 0x80, or ONE byte from 0x80 up (the reference compares a signed char with
//         peek(): such bytes never extend a run).  A unit emits at most 2 + 10 bytes, so one position costs one thread a bounded
//         amount of work whatever the input; the only thing a unit needs from far away is where the next unit starts, and that is a
//         suffix minimum over the first unit heads of the tiles.
//   mtf:  the list in front of a chunk is "the distinct bytes in front of it, latest occurrence first, then the untouched rest of
//         0 .. 255".  The first part (a summary of at most 256 bytes) composes associatively: summaries per chunk, scanned over groups
//         of 256 on three levels, then every thread starts from its true list and runs the plain loop on its chunk.
//   huff: histogram -> host table (huffman_host.cpp: the tie order of libstdc++ is the format) -> bits per tile -> scan -> pack.
#include "bytestages.hpp"
#include "bytestages_dev.hpp"
#include "stages.hpp"
#include "bitsink.hpp"
#include "prim.hpp"
#include "huffman_host.hpp"

#include <vector>

namespace tdc {
namespace {

// ---- rle ------------------------------------------------------------------------------------------------------------------------------

// first unit head of every tile as n - position (0: the tile has none), tiles in REVERSE order: an inclusive maximum over that array is
// the suffix minimum of the positions
__global__ void __launch_bounds__(256) rle_first_head_kernel(const u8* __restrict__ in, size_t n, u32 ntiles, u32* __restrict__ rev) {
    __shared__ u32 wmin[4];
    const u32 tile = blockIdx.x;
    const size_t base = (size_t)tile * RLE_TILE + (size_t)threadIdx.x * RLE_PER_THREAD;
    u32 s[17];
    load16_prev(in, n, base, s);
    u32 fh = NONE32;
#pragma unroll
    for (int j = 15; j >= 0; --j) if (base + j < n && rle_head(base + j, s[j + 1], s[j])) fh = (u32)(base + j);
    fh = wave_reduce_min(fh);
    if (lane_id() == 0) wmin[wave_id()] = fh;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u32 m = min(min(wmin[0], wmin[1]), min(wmin[2], wmin[3]));
        rev[ntiles - 1 - tile] = m == NONE32 ? 0u : (u32)(n - m);
    }
}

// EMIT = false: bytes the units that start in the tile emit -> tile_bytes[tile];  true: tile_bytes[] holds the exclusive sums, write them
template <bool EMIT>
__global__ void __launch_bounds__(256) rle_tile_kernel(const u8* __restrict__ in, size_t n, u64 o, u32 lo, const u32* __restrict__ revmax, u32 ntiles,
                                                       u64* __restrict__ tile_bytes, u8* __restrict__ out) {
    __shared__ u32 wsuf[4];
    __shared__ u32 sm[5];
    const u32 tile = blockIdx.x;
    const int lane = lane_id(), w = wave_id();
    const size_t base = (size_t)tile * RLE_TILE + (size_t)threadIdx.x * RLE_PER_THREAD;
    u32 s[17];
    load16_prev(in, n, base, s);
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
        const u32 q = tile + 1 < ntiles ? revmax[ntiles - 2 - tile] : 0u;
        next = q ? (u32)(n - q) : (u32)n;
    }
    u32 len[16];
#pragma unroll
    for (int j = 15; j >= 0; --j) {
        len[j] = 0;
        if (base + j < n && rle_head(base + j, s[j + 1], s[j])) { len[j] = next - (u32)(base + j); next = (u32)(base + j); }
    }
    u32 bytes = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (!len[j]) continue;
        const u32 ch = s[j + 1];
        if (ch >= 0x80u) bytes += (base + j > 0 && s[j] == ch) ? 1 + lo : 1;
        else bytes += len[j] == 1 ? 1 : 2 + vbyte_len((u64)(len[j] - 2) + o);
    }
    u32 total;
    const u32 pre = block_exclusive_sum<u32, 4>(bytes, sm, total);
    if (!EMIT) {
        if (threadIdx.x == 0) tile_bytes[tile] = total;
        return;
    }
    u8* p = out + tile_bytes[tile] + pre;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (!len[j]) continue;
        const u32 ch = s[j + 1];
        *p++ = (u8)ch;
        if (ch >= 0x80u) { if (base + j > 0 && s[j] == ch) p = put_vbyte(p, o); }
        else if (len[j] > 1) { *p++ = (u8)ch; p = put_vbyte(p, (u64)(len[j] - 2) + o); }
    }
}

// ---- mtf ------------------------------------------------------------------------------------------------------------------------------
// summary of chunk g: its distinct bytes, last occurrence first
__global__ void __launch_bounds__(256) mtf_summary_kernel(const u8* __restrict__ in, size_t n, u32 M, u32* __restrict__ rows, u32* __restrict__ cnt) {
    const u32 g = blockIdx.x * 256 + threadIdx.x;
    if (g >= M) return;
    const size_t start = (size_t)g * MTF_CHUNK;
    Mask256 m;
    RowWriter w{rows + (size_t)g * 64};
    for (int q = MTF_CHUNK / 16 - 1; q >= 0 && w.n < 256; --q) {
        const size_t p0 = start + (size_t)q * 16;
        if (p0 >= n) continue;
        const uint4 v = *(const uint4*)(in + p0);
        const u32 x[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
        for (int b = 15; b >= 0; --b) {
            const u32 ch = (x[b >> 2] >> (8 * (b & 3))) & 255u;
            if (p0 + b < n && !m.test_set(ch)) w.push(ch);
        }
    }
    w.finish();
    cnt[g] = w.n;
}

// Inclusive scan of the summaries inside every group of 256 rows (Hillis-Steele, rows ping-pong between A and B; eight rounds end in A):
// row g becomes the summary of rows [first of the group, g].  The last row of a group is the group's summary one level up.
__global__ void __launch_bounds__(256) mtf_scan_kernel(u32* rowsA, u32* cntA, u32* rowsB, u32* cntB, u32 M, u32* __restrict__ up_rows,
                                                       u32* __restrict__ up_cnt) {
    const u32 t = threadIdx.x;
    const u32 g = blockIdx.x * 256 + t;
    const bool valid = g < M;
    u32 *src = rowsA, *scnt = cntA, *dst = rowsB, *dcnt = cntB;
    for (u32 d = 1; d < 256; d <<= 1) {
        if (valid) {
            Mask256 m;
            RowWriter w{dst + (size_t)g * 64};
            append_new(src + (size_t)g * 64, scnt[g], m, w);                               // the later rows first
            if (t >= d) append_new(src + (size_t)(g - d) * 64, scnt[g - d], m, w);          // what the earlier ones add
            w.finish();
            dcnt[g] = w.n;
        }
        __syncthreads();
        u32* x = src; src = dst; dst = x;
        x = scnt; scnt = dcnt; dcnt = x;
    }
    if (valid && (t == 255 || g == M - 1)) {
        const u32 k = cntA[g];
        for (u32 q = 0; q * 4 < k; ++q) up_rows[(size_t)blockIdx.x * 64 + q] = rowsA[(size_t)g * 64 + q];
        up_cnt[blockIdx.x] = k;
    }
}

// list in front of item i = the summary of the items in front of it inside its group, then what is left of the list in front of the group
// (parent == nullptr: 0, 1, ..., 255)
__global__ void __launch_bounds__(256) mtf_down_kernel(const u32* __restrict__ parent, const u32* __restrict__ rows, const u32* __restrict__ cnt, u32 M,
                                                       u32* __restrict__ lists) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    Mask256 m;
    RowWriter w{lists + (size_t)i * 64};
    if (i & 255u) append_new(rows + (size_t)(i - 1) * 64, cnt[i - 1], m, w);
    if (parent) append_new(parent + (size_t)(i >> 8) * 64, 256, m, w);
    else for (u32 ch = 0; ch < 256; ++ch) if (!m.test_set(ch)) w.push(ch);
    w.finish();
}

// One workgroup per group of 256 chunks.  Entry j of thread t's list lives at byte j * 256 + (t & 63) * 4 + (t >> 6): the lanes of a wave
// hit 64 different banks whatever their j, the four waves share the words.
__global__ void __launch_bounds__(256) mtf_encode_kernel(const u8* __restrict__ in, size_t n, u32 M, const u32* __restrict__ tile_lists,
                                                         const u32* __restrict__ rows, const u32* __restrict__ cnt, u8* __restrict__ out) {
    __shared__ u8 lds[65536];
    const u32 t = threadIdx.x;
    const u32 g = blockIdx.x * 256 + t;
    if (g >= M) return;                                           // (no barrier below)
    u8* L = lds + (t & 63u) * 4 + (t >> 6);
    {
        Mask256 m;
        u32 k = 0;
        auto take = [&](const u32* __restrict__ row, u32 c) {
            for (u32 q = 0; q * 4 < c; ++q) {
                const u32 x = row[q];
#pragma unroll
                for (u32 b = 0; b < 4; ++b) {
                    const u32 ch = (x >> (8 * b)) & 255u;
                    if (q * 4 + b < c && !m.test_set(ch)) { L[k * 256] = (u8)ch; ++k; }
                }
            }
        };
        if (t) take(rows + (size_t)(g - 1) * 64, cnt[g - 1]);
        take(tile_lists + (size_t)blockIdx.x * 64, 256);
    }
    const size_t start = (size_t)g * MTF_CHUNK;
    for (u32 q = 0; q < MTF_CHUNK / 16; ++q) {
        const size_t p0 = start + (size_t)q * 16;
        if (p0 >= n) break;
        const uint4 v = *(const uint4*)(in + p0);
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
        if (p0 + 16 <= n) *(uint4*)(out + p0) = make_uint4(y[0], y[1], y[2], y[3]);
        else for (u32 b = 0; p0 + b < n; ++b) out[p0 + b] = (u8)(y[b >> 2] >> (8 * (b & 3)));
    }
}

// ---- encode(huff) -----------------------------------------------------------------------------------------------------------------------
struct HuffDev { u64 code[256]; u32 len[256]; };

__global__ void __launch_bounds__(256) huff_tile_bits_kernel(const u8* __restrict__ in, size_t n, const HuffDev* __restrict__ T, u64* __restrict__ tile_bits) {
    __shared__ u32 len[256];
    __shared__ u32 sm[5];
    len[threadIdx.x] = T->len[threadIdx.x];
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * HUFF_TILE + (size_t)threadIdx.x * HUFF_PER_THREAD;
    u32 bits = 0;
    if (base < n) {
        const uint4 v = *(const uint4*)(in + base);
        const u32 x[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
        for (u32 b = 0; b < 16; ++b) if (base + b < n) bits += len[(x[b >> 2] >> (8 * (b & 3))) & 255u];
    }
    u32 total;
    (void)block_exclusive_sum<u32, 4>(bits, sm, total);
    if (threadIdx.x == 0) tile_bits[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) huff_pack_kernel(const u8* __restrict__ in, size_t n, const HuffDev* __restrict__ T, const u64* __restrict__ tile_off,
                                                        u64 base_bits, u64* __restrict__ out) {
    __shared__ u64 code[256];
    __shared__ u32 len[256];
    __shared__ u32 sm[5];
    code[threadIdx.x] = T->code[threadIdx.x];
    len[threadIdx.x] = T->len[threadIdx.x];
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * HUFF_TILE + (size_t)threadIdx.x * HUFF_PER_THREAD;
    u32 x[4] = { 0, 0, 0, 0 };
    u32 bits = 0;
    if (base < n) {
        const uint4 v = *(const uint4*)(in + base);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
#pragma unroll
        for (u32 b = 0; b < 16; ++b) if (base + b < n) bits += len[(x[b >> 2] >> (8 * (b & 3))) & 255u];
    }
    u32 total;
    const u32 pre = block_exclusive_sum<u32, 4>(bits, sm, total);
    if (base >= n) return;
    BitSink sink;
    sink.out = out;
    sink.pos = base_bits + tile_off[blockIdx.x] + pre;
    sink.acc = 0;
    sink.cnt = 0;
#pragma unroll
    for (u32 b = 0; b < 16; ++b) {
        const u32 ch = (x[b >> 2] >> (8 * (b & 3))) & 255u;
        if (base + b < n) sink.append(code[ch], len[ch]);           // (nothing behind the input)
    }
    sink.flush();
}

}  // namespace

u64 rle_bound(u64 n, u64 offset) { return n ? 1 + (n - 1) * (u64)(1 + vbyte_len(offset)) : 0; }
// a code is at most 64 bits long (the packer's word; 2^32 symbols reach 46), the header at most 2 + 2 * 256 + 256 + 4 bytes
u64 huff_literals_bound(u64 n) { return 8 * n + 1024; }
// tile tables of 8 bytes per 4096, or mtf's rows: 2 x 256 bytes per chunk of 1024 and their counts, the levels above, the tile lists
// (encode(sle) states its own: sle_literals_scratch_bound in encode.hip -- up to 38 bytes per input byte for the k-mer count at k = 7)
u64 stage_scratch_bound(u64 n) { return n / 2 + n / 64 + ((u64)1 << 20); }

StageOut rle_encode_device(Ctx& c, const u8* d_in, size_t n, u64 offset) {
    StageOut r;
    if (n == 0) { r.d = c.arena.get<u8>(64); return r; }
    hipStream_t s = c.stream;
    const u32 ntiles = cdiv(n, RLE_TILE);
    u32* rev = c.arena.get<u32>(ntiles);
    u64* tile_bytes = c.arena.get<u64>((size_t)ntiles + 1);
    u64* d_total = tile_bytes + ntiles;
    const u32 lo = vbyte_len(offset);
    rle_first_head_kernel<<<ntiles, 256, 0, s>>>(d_in, n, ntiles, rev);
    LAUNCH_CHECK();
    inclusive_max_u32(c, rev, rev, ntiles);
    rle_tile_kernel<false><<<ntiles, 256, 0, s>>>(d_in, n, offset, lo, rev, ntiles, tile_bytes, nullptr);
    LAUNCH_CHECK();
    exclusive_sum_u64(c, tile_bytes, tile_bytes, ntiles, d_total);
    r.len = c.read(d_total);
    if (r.len > STAGE_MAX_BYTES) throw StageTooLarge{r.len};
    r.d = c.arena.get<u8>(r.len + 64);
    rle_tile_kernel<true><<<ntiles, 256, 0, s>>>(d_in, n, offset, lo, rev, ntiles, tile_bytes, r.d);
    LAUNCH_CHECK();
    return r;
}

StageOut mtf_encode_device(Ctx& c, const u8* d_in, size_t n) {
    StageOut r;
    r.len = n;
    r.d = c.arena.get<u8>(n + 64);
    if (n == 0) return r;
    hipStream_t s = c.stream;
    // level 0: chunks, level 1: groups of 256 chunks (one workgroup of the encoder each), level 2: groups of 256 of those (at most 64 for 2^32 bytes)
    const u32 M0 = cdiv(n, MTF_CHUNK), M1 = cdiv(M0, 256), M2 = cdiv(M1, 256);
    u32 *rowsA[3], *rowsB[3], *cntA[3], *cntB[3];
    const u32 M[3] = { M0, M1, M2 };
    for (int l = 0; l < 3; ++l) {
        rowsA[l] = c.arena.get<u32>((size_t)M[l] * 64); rowsB[l] = c.arena.get<u32>((size_t)M[l] * 64);
        cntA[l] = c.arena.get<u32>(M[l]); cntB[l] = c.arena.get<u32>(M[l]);
    }
    u32* top_row = c.arena.get<u32>((size_t)cdiv(M2, 256) * 64);
    u32* top_cnt = c.arena.get<u32>(cdiv(M2, 256));
    u32* lists2 = c.arena.get<u32>((size_t)M2 * 64);
    u32* lists1 = c.arena.get<u32>((size_t)M1 * 64);
    mtf_summary_kernel<<<cdiv(M0, 256), 256, 0, s>>>(d_in, n, M0, rowsA[0], cntA[0]);
    LAUNCH_CHECK();
    for (int l = 0; l < 3; ++l) {
        mtf_scan_kernel<<<cdiv(M[l], 256), 256, 0, s>>>(rowsA[l], cntA[l], rowsB[l], cntB[l], M[l], l < 2 ? rowsA[l + 1] : top_row, l < 2 ? cntA[l + 1] : top_cnt);
        LAUNCH_CHECK();
    }
    mtf_down_kernel<<<cdiv(M2, 256), 256, 0, s>>>(nullptr, rowsA[2], cntA[2], M2, lists2);
    LAUNCH_CHECK();
    mtf_down_kernel<<<cdiv(M1, 256), 256, 0, s>>>(lists2, rowsA[1], cntA[1], M1, lists1);
    LAUNCH_CHECK();
    mtf_encode_kernel<<<M1, 256, 0, s>>>(d_in, n, M0, lists1, rowsA[0], cntA[0], r.d);
    LAUNCH_CHECK();
    return r;
}

StageOut huff_literals_device(Ctx& c, const u8* d_in, size_t n) {
    if (!c.huff_ok) throw HipError{hipErrorUnknown, "encode(huff): the Huffman self-check of this build failed", (int)__LINE__};
    hipStream_t s = c.stream;
    StageOut r;
    u32 hist[256] = {0};
    if (n) {
        u32* d_hist = c.arena.get<u32>(256);
        HIP_TRY(hipMemsetAsync(d_hist, 0, 256 * sizeof(u32), s));
        text_histogram_add(c, d_in, n, d_hist);
        c.read_n(d_hist, hist, 256);
    }
    HuffTable ht;
    build_huffman_table(hist, &ht);
    HostBitWriter hw;
    write_huffman_header(hw, ht);
    std::vector<HuffDev> tab(1);
    for (int i = 0; i < 256; ++i) {                              // (sigma <= 1: eight raw bits per byte, HuffmanCoder.hpp:562-569)
        tab[0].code[i] = ht.sigma <= 1 ? (u64)i : ht.code_of[i];
        tab[0].len[i] = ht.sigma <= 1 ? 8u : ht.len_of[i];
    }
    const u32 ntiles = cdiv(n, HUFF_TILE);
    u64 total_bits = hw.nbits;
    HuffDev* d_tab = (HuffDev*)c.arena.alloc(sizeof(HuffDev));
    u64* tile_bits = c.arena.get<u64>((size_t)ntiles + 1);
    if (n) {
        HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), sizeof(HuffDev), hipMemcpyHostToDevice, s));
        huff_tile_bits_kernel<<<ntiles, 256, 0, s>>>(d_in, n, d_tab, tile_bits);
        LAUNCH_CHECK();
        exclusive_sum_u64(c, tile_bits, tile_bits, ntiles, tile_bits + ntiles);
        total_bits += c.read(tile_bits + ntiles);
    }
    r.len = bit_stream_len(total_bits);
    if (r.len > STAGE_MAX_BYTES) throw StageTooLarge{r.len};
    const size_t padded = bit_stream_padded(r.len);
    r.d = c.arena.get<u8>(padded + 64);
    HIP_TRY(hipMemsetAsync(r.d, 0, padded, s));
    HIP_TRY(hipMemcpyAsync(r.d, hw.bytes.data(), hw.bytes.size(), hipMemcpyHostToDevice, s));
    if (n) {
        huff_pack_kernel<<<ntiles, 256, 0, s>>>(d_in, n, d_tab, tile_bits, hw.nbits, (u64*)r.d);
        LAUNCH_CHECK();
    }
    bit_stream_terminator(c, r.d, total_bits);
    HIP_TRY(hipStreamSynchronize(s));                            // (the header and the table live on this frame)
    return r;
}

}  // namespace tdc
