// bytestages_decode.hip -- the decoders of rle, mtf, encode(huff) and encode(sle) on the device.  The host loops of
// host/tdc_coders.hpp (rle_decode, mtf_decode, huff_decode_literals, sle_decode_literals) are the specification, including what they refuse.
//   mtf:  the moves of a chunk of ranks do not depend on what the list holds.  Run on the identity list, a chunk of 1 KiB yields its
//         permutation (the list it leaves behind, 256 bytes) and for every rank the index into the list the chunk STARTS from.
//         Permutations compose associatively, (a o b)[j] = a[b[j]]: reduced over groups of 256 on three levels, brought back down as the
//         list in front of every chunk, and the output is the gather out[i] = list[chunk of i][index i].
//   huff: next(x) = x + length of the code at bit x.  A chain can enter a tile of 2048 bit positions only within the first `longest`
//         offsets: the tile scheme of tile_chain.hpp (exits per tile in LDS, entries of every tile), then codes per tile -> 64-bit scan
//         -> one byte per code.  No per-bit array in HBM.
//   sle:  encode(sle) is a prefix code as well, and the length of a code follows from its first three bits: the same kernels and driver
//         as huff under another Code policy, without a table in the exit pass; a code stands for 1 or k bytes, so the count pass adds
//         up bytes, not codes.
//   rle:  the parse carries one bit of state ("this data byte equals the previous data byte": a vbyte follows), a token is at most 1 + 10
//         bytes long: the same tile scheme with the 2 x 11 states (offset, eq).  Run lengths -> 64-bit scan; every token writes its bytes
//         up to the next 256-byte border of the output itself and leaves (end, byte) at the first border it covers; a maximum scan over
//         the borders tells every 256-byte piece of the output which run fills it.  No thread loops over a run.
// Every pass is bounded by its tile: a thread walks at most one tile (2048 bit positions, 512 bytes) or one group of 512 table rows.
// Scratch comes from the TOP of the arena (the caller releases it once the output exists), the output from the bottom.
#include "bytestages.hpp"
#include "decode.hpp"
#include "prim.hpp"
#include "tile_chain.hpp"
#include "../host/tdc_coders.hpp"

#include <vector>

namespace tdc {
namespace {

// the output of a stage, from the bottom of the arena
u8* stage_out(Ctx& c, u64 len) {
    const size_t off = align_up(c.arena.top, 256);
    if (off + len + 64 > c.arena.size - c.arena.top_hi) throw StageArenaShort{len, c.arena.top_hi};
    return c.arena.get<u8>((size_t)len + 64);
}

// ---- mtf --------------------------------------------------------------------------------------------------------------------------------
// One thread per chunk; entry j of thread t's list at byte j * 256 + (t & 63) * 4 + (t >> 6) as in mtf_encode_kernel (the lanes of a wave
// hit 64 different banks whatever their j).  sym[i] = index into the list in front of the chunk, rows[g] = the list chunk g leaves
// behind when it starts from 0 .. 255.
__global__ void __launch_bounds__(256) mtf_dec_chunk_kernel(const u8* __restrict__ in, size_t n, u32 M, u8* __restrict__ sym, u8* __restrict__ rows) {
    __shared__ u8 lds[65536];
    const u32 t = threadIdx.x;
    const u32 g = blockIdx.x * 256 + t;
    u8* L = lds + (t & 63u) * 4 + (t >> 6);
    for (u32 j = 0; j < 256; ++j) L[j * 256] = (u8)j;
    if (g < M) {
        const size_t start = (size_t)g * MTF_CHUNK;
        for (u32 q = 0; q < MTF_CHUNK / 16; ++q) {
            const size_t p0 = start + (size_t)q * 16;
            if (p0 >= n) break;
            const uint4 v = *(const uint4*)(in + p0);
            const u32 x[4] = { v.x, v.y, v.z, v.w };
            u32 y[4] = { 0, 0, 0, 0 };
#pragma unroll
            for (u32 b = 0; b < 16; ++b) {
                const u32 r = (x[b >> 2] >> (8 * (b & 3))) & 255u;
                u32 ch = 0;
                if (p0 + b < n) {
                    ch = L[r * 256];
                    u32 prev = ch;
                    for (u32 j = 0; j <= r; ++j) {                // the plain loop: the entries in front of rank r move back by one
                        const u32 e = L[j * 256];
                        L[j * 256] = (u8)prev;
                        prev = e;
                    }
                }
                y[b >> 2] |= ch << (8 * (b & 3));
            }
            if (p0 + 16 <= n) *(uint4*)(sym + p0) = make_uint4(y[0], y[1], y[2], y[3]);
            else for (u32 b = 0; p0 + b < n; ++b) sym[p0 + b] = (u8)(y[b >> 2] >> (8 * (b & 3)));
        }
    }
    __syncthreads();
    const u32 g0 = blockIdx.x * 256;
    for (u32 r = 0; r < 256 && g0 + r < M; ++r) rows[(size_t)(g0 + r) * 256 + t] = lds[t * 256 + (r & 63u) * 4 + (r >> 6)];
}

// One wave per group of up to 256 rows, lane l holds bytes 4 l .. 4 l + 3 of the running list.
// DOWN = false: out[group] = row[first] o ... o row[last] (the group's row one level up)
// DOWN = true:  out[g] = the list in front of item g = (list in front of the group: parent[group], or 0 .. 255) o (rows in front of g)
template <bool DOWN>
__global__ void __launch_bounds__(64) mtf_perm_kernel(const u32* __restrict__ rows, u32 M, const u32* __restrict__ parent, u32* __restrict__ out) {
    __shared__ u32 cur32[64];
    const u8* cur = (const u8*)cur32;
    const u32 lane = threadIdx.x, grp = blockIdx.x;
    const u32 g0 = grp * 256, g1 = min(g0 + 256, M);
    u32 w = (DOWN && parent) ? parent[(size_t)grp * 64 + lane] : 0x03020100u + 0x04040404u * lane;
    for (u32 g = g0; g < g1; ++g) {
        if (DOWN) out[(size_t)g * 64 + lane] = w;
        cur32[lane] = w;
        __syncthreads();
        const u32 r = rows[(size_t)g * 64 + lane];
        w = (u32)cur[r & 255u] | ((u32)cur[(r >> 8) & 255u] << 8) | ((u32)cur[(r >> 16) & 255u] << 16) | ((u32)cur[r >> 24] << 24);
        __syncthreads();
    }
    if (!DOWN) out[(size_t)grp * 64 + lane] = w;
}

// io[i] = list in front of the chunk of i [io[i]]: 4096 bytes (four chunks) per workgroup and round
__global__ void __launch_bounds__(256) mtf_dec_gather_kernel(u8* io, size_t n, const u32* __restrict__ lists, u32 M, u32 ntiles) {
    __shared__ u32 L32[256];
    const u8* L = (const u8*)L32;
    const u32 t = threadIdx.x;
    for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        __syncthreads();
        L32[t] = tile * 4 + (t >> 6) < M ? lists[(size_t)tile * 256 + t] : 0u;
        __syncthreads();
        const size_t p = (size_t)tile * 4096 + (size_t)t * 16;
        if (p >= n) continue;
        const uint4 v = *(const uint4*)(io + p);
        const u32 x[4] = { v.x, v.y, v.z, v.w };
        u32 y[4] = { 0, 0, 0, 0 };
        const u8* Lc = L + (t >> 6) * 256;
#pragma unroll
        for (u32 b = 0; b < 16; ++b) y[b >> 2] |= (u32)Lc[(x[b >> 2] >> (8 * (b & 3))) & 255u] << (8 * (b & 3));
        if (p + 16 <= n) *(uint4*)(io + p) = make_uint4(y[0], y[1], y[2], y[3]);
        else for (u32 b = 0; p + b < n; ++b) io[p + b] = (u8)(y[b >> 2] >> (8 * (b & 3)));
    }
}

// ---- encode(huff) -----------------------------------------------------------------------------------------------------------------------
constexpr u32 HD_LUT_BITS = 12;
constexpr u32 HD_T = 2048;                  // bit positions per tile
constexpr u32 HD_CH = 16384;                // bit positions per workgroup of the exit pass
// HuffmanCoder::Decoder as the host builds it (coders/HuffmanCoder.hpp:581-597); lut: code length | symbol << 4 for the codes that end
// inside 12 bits, 0: the canonical walk decides
struct HuffDecTab {
    u16 lut[1 << HD_LUT_BITS];
    u64 first[256];
    u16 prefix[256];
    u8 numl[256];
    u8 order[256];
    u32 longest, sigma, pad0, pad1;
};
static_assert(sizeof(HuffDecTab) % 4 == 0, "copied word by word");

// huffman_decode (HuffmanCoder.hpp:377-397) at bit x with the host loop's arithmetic: code length (0: no code of the table) and symbol
template <typename Win>
__device__ __forceinline__ u32 hd_code(const HuffDecTab* T, const Win& bw, u64 x, u32& sym) {
    u64 w = bw.peek(x);
    const u32 e = T->lut[w >> (64 - HD_LUT_BITS)];
    if (e) { sym = e >> 4; return e & 15u; }
    u64 value = 0; u32 length = 0;
    do {
        if (length && !(length & 63u)) w = bw.peek(x + length);
        value = (value << 1) + ((w >> (63 - (length & 63u))) & 1u);
        ++length;
    } while (length <= T->longest && value < T->first[length - 1]);
    if (length > T->longest) return 0u;
    --length;
    const u64 off = value - T->first[length];
    if (off >= T->numl[length] || (u64)T->prefix[length] + off >= T->sigma) return 0u;
    sym = T->order[T->prefix[length] + off];
    return length + 1;
}

// ---- prefix-code streams: encode(huff) and encode(sle) ----------------------------------------------------------------------------------
// What a code is, is the coder's business.  A coder hands the two kernels a Code, a small POD passed by value (as Tok in
// stream_parse.hpp):
//   Tab, g                                the table of the walk as the host builds it, and its copy on the device
//   exit_tab() / walk_tab()               what the pass keeps in LDS beside the stream image: staged here, complete behind the next barrier
//   len(T, bw, x)                         the length of the code at bit x < total; 0: none, the chain ends there
//   put<EMIT>(T, bw, x, dst, m)           the code at x: its length, 0: an error of the stream.  m = the bytes it stands for, written
//                                         to dst[0 .. m) if EMIT
struct HuffCode {
    typedef HuffDecTab Tab;
    const HuffDecTab* g;
    __device__ __forceinline__ const HuffDecTab* exit_tab() const {
        __shared__ HuffDecTab T;
        for (u32 k = threadIdx.x; k < sizeof(HuffDecTab) / 4; k += blockDim.x) ((u32*)&T)[k] = ((const u32*)g)[k];
        return &T;
    }
    __device__ __forceinline__ const HuffDecTab* walk_tab() const { return exit_tab(); }
    template <typename Win>
    __device__ __forceinline__ u32 len(const HuffDecTab* T, const Win& bw, u64 x) const { u32 sym; return hd_code(T, bw, x, sym); }
    template <bool EMIT, typename Win>
    __device__ __forceinline__ u32 put(const HuffDecTab* T, const Win& bw, u64 x, u8* dst, u32& m) const {   // a code outside the table is the error
        u32 sym;
        const u32 d = hd_code(T, bw, x, sym);
        m = 1;
        if (!d) return 0u;
        if (EMIT) *dst = (u8)sym;
        return d;
    }
};

// s32: the stream's words (nw32 of them readable), hb: first bit of the body, total: bits in front of the terminator
template <class Code>
__global__ void __launch_bounds__(256) code_exit_kernel(const Code code, const u32* __restrict__ s32, u64 nw32, u64 hb, u64 total, u32 LA, u32 nchunks,
                                                        u32 ntiles, u16* __restrict__ exit0) {
    __shared__ u32 sw[HD_CH / 32 + 16];
    __shared__ u8 nxl[HD_CH];                                  // next(x) - x; 0: no code starts at x
    const auto T = code.exit_tab();
    for (u32 chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        __syncthreads();
        const u64 a0 = hb + (u64)chunk * HD_CH;
        const u64 kb = a0 >> 5;
        for (u32 k = threadIdx.x; k < HD_CH / 32 + 16; k += 256) sw[k] = kb + k < nw32 ? __builtin_bswap32(s32[kb + k]) : 0u;
        __syncthreads();
        const BitWin bw{sw, kb, total};
        for (u32 i = threadIdx.x; i < HD_CH; i += 256) nxl[i] = (u8)(a0 + i < total ? code.len(T, bw, a0 + i) : 0u);
        __syncthreads();
        tile_exits<HD_T, HD_CH / HD_T>(nxl, LA, chunk * (HD_CH / HD_T), ntiles, exit0);
    }
}

// the codes of every tile from its entry: EMIT = false adds up the bytes they stand for (tcount[t]; *err |= 1 for a code that
// Code::put refuses), EMIT = true: tcount[] holds the exclusive sums, the bytes go to out
template <class Code, bool EMIT>
__global__ void __launch_bounds__(256) code_walk_kernel(const Code code, const u32* __restrict__ s32, u64 hb, u64 total, const u16* __restrict__ tile_entry,
                                                        u32 ntiles, u64* __restrict__ tcount, u8* __restrict__ out, u32* __restrict__ err) {
    const auto T = code.walk_tab();
    __syncthreads();
    const BitWinG bw{s32, total};
    for (u32 t = blockIdx.x * 256 + threadIdx.x; t < ntiles; t += gridDim.x * 256) {
        const u32 e = tile_entry[t];
        u64 cnt = 0;
        if (e != DX_NONE) {
            u64 x = hb + (u64)t * HD_T + e;
            const u64 tile_end = min(hb + (u64)(t + 1) * HD_T, total);
            u8* dst = EMIT ? out + tcount[t] : nullptr;
            for (u32 guard = 0; x < tile_end && guard <= HD_T; ++guard) {
                u32 m;
                const u32 d = code.template put<EMIT>(T, bw, x, EMIT ? dst + cnt : nullptr, m);
                if (!d) { if (!EMIT) atomicOr(err, 1u); break; }
                cnt += m;
                x += d;
            }
        }
        if (!EMIT) tcount[t] = cnt;
    }
}
// header bit 0 (sigma <= 1): eight raw bits per byte from bit 1 on, zeros behind the end
__global__ void __launch_bounds__(256) hd_raw_kernel(const u32* __restrict__ s32, u64 total, u64 count, u8* __restrict__ out) {
    const BitWinG bw{s32, total};
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < count; i += (u64)gridDim.x * 256) out[i] = (u8)(bw.peek(1 + 8 * i) >> 56);
}

// what hd_code does with a window whose first 12 bits are p, as far as those 12 bits decide it
u16 hd_lut_entry(const HuffDecTab& T, u32 p) {
    u64 value = 0; u32 length = 0;
    do {
        if (length == HD_LUT_BITS) return 0;
        value = (value << 1) + ((p >> (HD_LUT_BITS - 1 - length)) & 1u);
        ++length;
    } while (length <= T.longest && value < T.first[length - 1]);
    if (length > T.longest) return 0;
    --length;
    const u64 off = value - T.first[length];
    if (off >= T.numl[length] || (u64)T.prefix[length] + off >= T.sigma) return 0;
    return (u16)((length + 1) | ((u32)T.order[T.prefix[length] + off] << 4));
}

// The header as huff_decode_literals and HuffmanCoder::Decoder read it, from the first `pre_len` bytes of the stream (`whole`: that is
// all of it).  0: refused, 1: no table (sigma <= 1), 2: table in T, -1: the header does not end inside the prefix.  hb: first body bit.
int hd_parse_header(const u8* pre, size_t pre_len, bool whole, u64 total, HuffDecTab& T, u64& hb) {
    if (!(pre[0] & 0x80u)) { hb = 1; return 1; }
    const u64 lim = whole ? ~0ull : 8ull * (pre_len - 2);
    {
        tdc_amd::BitIStream probe(pre, pre_len);
        u64 need = 1, used = 1;
        auto group = [&] {
            u64 v = 0; unsigned i = 0; bool more;
            do { more = probe.read_bit(); v |= probe.read_int(7) << (7 * i++); used += 8; } while (more && used <= lim);
            need += 8; for (u64 x = v >> 7; x; x >>= 7) need += 8;
            return v;
        };
        probe.read_bit();
        const u64 longest = group() & 0xFF;
        for (u64 i = 0; i < longest && need <= total && used <= lim; ++i) (void)group();
        const u64 sigma = need <= total && used <= lim ? group() : 0;
        if (!whole && (used > lim || need + 8 * std::min<u64>(sigma, 256) > lim)) return -1;
        need += 8 * sigma;
        if (need > total || !longest || sigma > 256) return 0;
    }
    tdc_amd::BitIStream in(pre, pre_len);
    u64 used = 1;
    auto cint = [&] {
        u64 v = 0; unsigned i = 0; bool more;
        do { more = in.read_bit(); v |= in.read_int(7) << (7 * i++); used += 8; } while (more && used <= lim);
        return v;
    };
    in.read_bit();
    memset(&T, 0, sizeof(T));
    T.longest = (u32)(cint() & 0xFF);
    if (!T.longest) return 0;
    for (u32 i = 0; i < T.longest; ++i) T.numl[i] = (u8)cint();
    const u64 sigma = cint();
    if (!whole && used + 8 * std::min<u64>(sigma, 256) > lim) return -1;
    if (sigma > 256) return 0;
    T.sigma = (u32)sigma;
    for (u64 i = 0; i < sigma; ++i) T.order[i] = (u8)in.read_int(8);
    used += 8 * sigma;
    T.first[T.longest - 1] = 0;
    for (u32 i = T.longest - 1; i > 0; --i) T.first[i - 1] = (T.first[i] + T.numl[i]) / 2;
    u32 acc = 0;
    for (u32 l = 0; l < T.longest; ++l) { T.prefix[l] = (u16)acc; acc += T.numl[l]; }
    for (u32 p = 0; p < (1u << HD_LUT_BITS); ++p) T.lut[p] = hd_lut_entry(T, p);
    hb = std::min(used, total);                               // (BitIStream reads zeros at the end and stays there)
    return 2;
}

// ---- encode(sle) ------------------------------------------------------------------------------------------------------------------------
// A pure prefix-code stream behind the ranking: the length of a code follows from its first three bits and sigma_bits
// (tdc_amd::sle_code_len), so next(x) needs no table; a rank stands for 1 or k bytes.  The kernels of encode(huff) with the same
// tile and chunk sizes; the states are the first LA = longest code (at most 13) offsets of a tile.
struct SleDecTab { u64 ent[tdc_amd::SLE_MAX_SIGMA]; };      // rank -> its bytes (first byte most significant) | their number << 56
static_assert(sizeof(SleDecTab) % 4 == 0, "copied word by word");

struct SleCode {
    typedef SleDecTab Tab;
    const SleDecTab* g;
    u32 sb, sigma;
    __device__ __forceinline__ int exit_tab() const { return 0; }                              // (sb is all the exit pass needs)
    __device__ __forceinline__ const u64* walk_tab() const {
        __shared__ SleDecTab T;
        for (u32 k = threadIdx.x; k < sizeof(SleDecTab) / 4; k += blockDim.x) ((u32*)&T)[k] = ((const u32*)g)[k];
        return T.ent;
    }
    template <typename Win>
    __device__ __forceinline__ u32 len(int, const Win& bw, u64 x) const {                      // 0: cut off by the end of the stream
        const u32 d = tdc_amd::sle_code_len(sb, (u32)(bw.peek(x) >> 61));
        return x + d > bw.total ? 0u : d;
    }
    template <bool EMIT, typename Win>
    __device__ __forceinline__ u32 put(const u64* T, const Win& bw, u64 x, u8* dst, u32& m) const {   // cut off, or a rank outside the ranking: the error
        const u64 w = bw.peek(x);
        const u32 d = tdc_amd::sle_code_len(sb, (u32)(w >> 61));                               // >= 1
        const u32 rank = tdc_amd::sle_code_rank(sb, d, (u32)(w >> (64 - d)));
        if (x + d > bw.total || rank >= sigma) return 0u;
        const u64 ent = T[rank];
        m = (u32)(ent >> 56);
        if (EMIT) for (u32 j = 0; j < m; ++j) dst[j] = (u8)(ent >> (8 * (m - 1 - j)));
        return d;
    }
};

// ---- rle --------------------------------------------------------------------------------------------------------------------------------
constexpr u32 RLD_T = 512;                  // input bytes per tile
constexpr u32 RLD_TOK = 11;                 // longest token: the data byte and a vbyte of ten
constexpr u32 RLD_S = 2 * RLD_TOK;          // states: (offset into the tile) * 2 + eq
constexpr u32 RLD_WT = 64;                  // tiles per workgroup: 32 KiB of the input in LDS ...
constexpr u32 RLD_STRIDE = RLD_T + 4;       // ... every tile shifted by one bank against its neighbour
constexpr u32 RLD_LDS = RLD_WT * RLD_STRIDE + RLD_STRIDE;
constexpr u32 RLD_OT = 256;                 // output bytes per piece of the fill
constexpr u64 RLD_CLAMP = 1ull << 33;       // run lengths and tile sums saturate here (anything above 2^32 - 2 is refused)

// the workgroup's input bytes [base, base + RLD_WT * RLD_T + 16) in LDS
struct RldWin {
    const u8* lds; u64 base;
    __device__ __forceinline__ u32 at(u64 p) const { const u32 rel = (u32)(p - base); return lds[(rel >> 9) * RLD_STRIDE + (rel & (RLD_T - 1))]; }
};
__device__ __forceinline__ void rld_load(const u8* __restrict__ in, u64 n, u64 base, u8* lds) {
    for (u32 k = threadIdx.x; k < (RLD_WT * RLD_T + 16) / 4; k += blockDim.x) {
        const u32 rel = k * 4;
        const u64 p = base + rel;
        *(u32*)(lds + (rel >> 9) * RLD_STRIDE + (rel & (RLD_T - 1))) = p < n ? *(const u32*)(in + p) : 0u;      // (16 readable bytes behind n)
    }
}
// the token at data byte x < n in state eq: its output length (saturated), where the next token starts and in which state.
// false: a vbyte that runs off the end or past ten bytes, or below the offset (rle_decode, read_vbyte)
__device__ __forceinline__ bool rld_token(const RldWin& w, u64 n, u64 x, u32 eq, u64 offset, u64& len, u64& nx, u32& neq) {
    const u32 ch = w.at(x);
    nx = x + 1;
    len = 1;
    if (eq) {
        u64 v = 0;
        for (u32 k = 0;; ++k) {
            if (nx >= n || k == 10) return false;
            const u32 b = w.at(nx++);
            v |= (u64)(b & 0x7Fu) << (7 * k);
            if (!(b & 0x80u)) break;
        }
        if (v < offset) return false;
        len = 1 + min(v - offset, RLD_CLAMP);
    }
    neq = nx < n && w.at(nx) == ch;
    return true;
}

__global__ void __launch_bounds__(256) rld_exit_kernel(const u8* __restrict__ in, u64 n, u64 offset, u32 ntiles, u32 nblocks, u16* __restrict__ exit0) {
    __shared__ __attribute__((aligned(16))) u8 lds[RLD_LDS];
    for (u32 blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        __syncthreads();
        const u64 base = (u64)blk * RLD_WT * RLD_T;
        rld_load(in, n, base, lds);
        __syncthreads();
        const RldWin w{lds, base};
        for (u32 k = threadIdx.x; k < RLD_WT * RLD_S; k += 256) {
            const u32 tt = k & (RLD_WT - 1), st = k / RLD_WT;
            const u32 tile = blk * RLD_WT + tt;
            if (tile >= ntiles) continue;
            const u64 tend = base + (u64)(tt + 1) * RLD_T;
            u64 x = base + (u64)tt * RLD_T + (st >> 1);
            u32 eq = st & 1u, res = DX_NONE;
            for (u32 guard = 0; guard <= RLD_T; ++guard) {
                if (x >= tend) { res = (u32)(x - tend) * 2 + eq; break; }
                if (x >= n) break;
                u64 len, nx; u32 neq;
                if (!rld_token(w, n, x, eq, offset, len, nx, neq)) break;
                x = nx; eq = neq;
            }
            exit0[(size_t)tile * RLD_S + st] = (u16)res;
        }
    }
}

// the tokens of every tile from its entry.  EMIT = false: tsum[t] = bytes they decode to (saturated), *err |= 1 for a malformed token.
// EMIT = true: tsum[] holds the exclusive sums; a token writes its bytes up to the next RLD_OT border and, if it goes on behind it,
// leaves (end | byte << 40) and its mark at that border
template <bool EMIT>
__global__ void __launch_bounds__(RLD_WT) rld_walk_kernel(const u8* __restrict__ in, u64 n, u64 offset, const u16* __restrict__ tile_entry, u32 ntiles,
                                                          u32 nblocks, u64* __restrict__ tsum, u8* __restrict__ out, u32* __restrict__ head,
                                                          u64* __restrict__ info, u32* __restrict__ err) {
    __shared__ __attribute__((aligned(16))) u8 lds[RLD_LDS];
    for (u32 blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        __syncthreads();
        const u64 base = (u64)blk * RLD_WT * RLD_T;
        rld_load(in, n, base, lds);
        __syncthreads();
        const RldWin w{lds, base};
        const u32 tile = blk * RLD_WT + threadIdx.x;
        if (tile >= ntiles) continue;
        const u32 e = tile_entry[tile];
        u64 sum = 0;
        if (e != DX_NONE) {
            const u64 tend = min(base + (u64)(threadIdx.x + 1) * RLD_T, n);
            u64 x = base + (u64)threadIdx.x * RLD_T + (e >> 1);
            u32 eq = e & 1u;
            u64 p = EMIT ? tsum[tile] : 0;
            for (u32 guard = 0; x < tend && guard <= RLD_T; ++guard) {
                u64 len, nx; u32 neq;
                if (!rld_token(w, n, x, eq, offset, len, nx, neq)) { if (!EMIT) atomicOr(err, 1u); break; }
                if (EMIT) {
                    const u32 ch = w.at(x);
                    const u64 end = p + len, border = (p + RLD_OT - 1) & ~(u64)(RLD_OT - 1);
                    for (u64 q = p; q < min(end, border); ++q) out[q] = (u8)ch;
                    if (border < end) { const u64 ot = border / RLD_OT; head[ot] = (u32)ot + 1; info[ot] = end | ((u64)ch << 40); }
                    p = end;
                } else sum = min(sum + len, RLD_CLAMP);
                x = nx; eq = neq;
            }
        }
        if (!EMIT) tsum[tile] = sum;
    }
}
// hmax[ot] - 1 = the border at which the run that covers border ot left its (end, byte): 16 bytes per thread
__global__ void __launch_bounds__(256) rld_fill_kernel(const u32* __restrict__ hmax, const u64* __restrict__ info, u64 total, u8* __restrict__ out) {
    const u64 items = (total + 15) / 16;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < items; i += (u64)gridDim.x * 256) {
        const u64 pos = i * 16, ot = pos / RLD_OT;
        const u32 h = hmax[ot];
        if (!h) continue;
        const u64 inf = info[h - 1];
        const u64 lim = min(inf & ((1ull << 40) - 1), (ot + 1) * RLD_OT);
        if (pos >= lim) continue;
        const u32 ch = (u32)(inf >> 40) & 255u;
        if (pos + 16 <= lim) { const u32 x = ch * 0x01010101u; *(uint4*)(out + pos) = make_uint4(x, x, x, x); }
        else for (u64 q = pos; q < lim; ++q) out[q] = (u8)ch;
    }
}

}  // namespace

// mtf: rows of 256 bytes per chunk of 1 KiB and their lists (n / 2), the levels above (n / 8 covers them many times).  The tile tables of
// huff and sle (2 x longest + 10 bytes per 2048 bits of input, entries and levels above included) fit into the same 5 n / 8 up to a longest
// code of 75 bits: every table an encoder writes (2^32 symbols reach 46 bits) and sle's 13.  A header may claim up to 255: those tables
// take 2 n, are NOT covered here, and reach the driver through StageArenaShort::scratch_bytes.  rle: 2 x 22 + 10 bytes per 512 bytes of
// input and 12 bytes per 256 bytes of output (out / 16).
u64 stage_decode_scratch_bound(u64 n, u64 out) { return n / 2 + n / 8 + out / 16 + ((u64)4 << 20); }

StageOut mtf_decode_device(Ctx& c, const u8* d_in, size_t n) {
    StageOut r;
    r.len = n;
    r.d = stage_out(c, n);
    if (n == 0) return r;
    hipStream_t s = c.stream;
    const u32 M0 = cdiv(n, MTF_CHUNK), M1 = cdiv(M0, 256), M2 = cdiv(M1, 256);       // M2 <= 64
    u32* rows0 = (u32*)c.arena.alloc_top((size_t)M0 * 256);
    u32* rows1 = (u32*)c.arena.alloc_top((size_t)M1 * 256);
    u32* rows2 = (u32*)c.arena.alloc_top((size_t)M2 * 256);
    u32* lists2 = (u32*)c.arena.alloc_top((size_t)M2 * 256);
    u32* lists1 = (u32*)c.arena.alloc_top((size_t)M1 * 256);
    u32* lists0 = (u32*)c.arena.alloc_top((size_t)M0 * 256);
    mtf_dec_chunk_kernel<<<M1, 256, 0, s>>>(d_in, n, M0, r.d, (u8*)rows0);
    LAUNCH_CHECK();
    mtf_perm_kernel<false><<<M1, 64, 0, s>>>(rows0, M0, nullptr, rows1);
    LAUNCH_CHECK();
    mtf_perm_kernel<false><<<M2, 64, 0, s>>>(rows1, M1, nullptr, rows2);
    LAUNCH_CHECK();
    mtf_perm_kernel<true><<<1, 64, 0, s>>>(rows2, M2, nullptr, lists2);
    LAUNCH_CHECK();
    mtf_perm_kernel<true><<<M2, 64, 0, s>>>(rows1, M1, lists2, lists1);
    LAUNCH_CHECK();
    mtf_perm_kernel<true><<<M1, 64, 0, s>>>(rows0, M0, lists1, lists0);
    LAUNCH_CHECK();
    const u32 ntiles = cdiv(n, 4096);
    mtf_dec_gather_kernel<<<std::min<u32>(ntiles, 1u << 16), 256, 0, s>>>(r.d, n, lists0, M0, ntiles);
    LAUNCH_CHECK();
    return r;
}

// The body of a prefix-code stream behind its parsed header: bits [hb, total) of the n bytes at s32, no code longer than LA; `tab`
// (alive until this returns) goes up and becomes code.g.
template <class Code>
StageOut code_decode_device(Ctx& c, Code code, const typename Code::Tab& tab, const u32* s32, size_t n, u64 hb, u64 total, u32 LA) {
    typedef typename Code::Tab Tab;
    hipStream_t s = c.stream;
    StageOut r;
    const u64 m = total - hb;
    if (m == 0) { r.d = stage_out(c, 0); return r; }
    const u32 ntiles = cdiv(m, HD_T), nchunks = cdiv(m, HD_CH);
    Tab* d_tab = (Tab*)c.arena.alloc_top(sizeof(Tab));
    u32* d_err = (u32*)c.arena.alloc_top(256);
    u64* tcount = (u64*)c.arena.alloc_top(((size_t)ntiles + 1) * 8);
    u16* exit0 = (u16*)c.arena.alloc_top((size_t)ntiles * LA * 2);
    HIP_TRY(hipMemcpyAsync(d_tab, &tab, sizeof(Tab), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_err, 0, 4, s));
    code.g = d_tab;
    code_exit_kernel<Code><<<std::min<u32>(nchunks, DEC_MAX_BLOCKS), 256, 0, s>>>(code, s32, ((u64)n + 60) / 4, hb, total, LA, nchunks, ntiles, exit0);
    LAUNCH_CHECK();
    const u16* entry = dx_entries(c, exit0, ntiles, LA, c.arena.alloc_top(dx_entries_scratch(ntiles, LA)));
    code_walk_kernel<Code, false><<<dec_grid(ntiles), 256, 0, s>>>(code, s32, hb, total, entry, ntiles, tcount, nullptr, d_err);
    LAUNCH_CHECK();
    exclusive_sum_u64(c, tcount, tcount, ntiles, tcount + ntiles);
    const u32 err = c.read(d_err);                              // (synchronises: the table lives on the caller's frame)
    r.len = c.read(tcount + ntiles);
    if (err) throw StreamFormatError{"pipeline: malformed stream"};
    if (r.len > STAGE_MAX_BYTES) throw StageTooLarge{r.len};
    r.d = stage_out(c, r.len);
    code_walk_kernel<Code, true><<<dec_grid(ntiles), 256, 0, s>>>(code, s32, hb, total, entry, ntiles, tcount, r.d, d_err);
    LAUNCH_CHECK();
    return r;
}

StageOut huff_decode_device(Ctx& c, const u8* d_in, size_t n) {
    const StreamFormatError bad{"pipeline: malformed stream"};
    if (!n) throw bad;
    hipStream_t s = c.stream;
    constexpr size_t PRE = 4096;
    std::vector<u8> pre(std::min(n, PRE) + 2);
    u8 tail[2] = { 0, 0 };
    HIP_TRY(hipMemcpyAsync(pre.data(), d_in, std::min(n, PRE), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(tail, d_in + (n >= 2 ? n - 2 : 0), n >= 2 ? 2 : 1, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const unsigned u = (n >= 2 ? tail[1] : tail[0]) & 7u;
    if (u >= 6 && n < 2) throw bad;
    const u64 total = u >= 6 ? (u64)(n - 2) * 8 + u : (u64)(n - 1) * 8 + u;
    if (total < 1) throw bad;
    std::vector<HuffDecTab> tab(1);
    u64 hb = 0;
    const int kind = hd_parse_header(pre.data(), std::min(n, PRE), n <= PRE, total, tab[0], hb);
    if (kind < 0) throw StageHostOnly{};
    if (kind == 0) throw bad;
    const u32* s32 = (const u32*)d_in;                          // (arena allocations are 256-byte aligned, 64 bytes of slack behind n)
    if (kind == 1) {
        StageOut r;
        r.len = (total - 1 + 7) / 8;
        if (r.len > STAGE_MAX_BYTES) throw StageTooLarge{r.len};
        r.d = stage_out(c, r.len);
        if (r.len) { hd_raw_kernel<<<dec_grid(r.len), 256, 0, s>>>(s32, total, r.len, r.d); LAUNCH_CHECK(); }
        return r;
    }
    return code_decode_device(c, HuffCode{nullptr}, tab[0], s32, n, hb, total, tab[0].longest);
}

StageOut sle_decode_device(Ctx& c, const u8* d_in, size_t n, u32 kmer) {
    const StreamFormatError bad{"pipeline: malformed stream"};
    if (!n) throw bad;
    if (kmer == 0) kmer = 3;
    hipStream_t s = c.stream;
    constexpr size_t PRE = 16384;                               // the longest ranking tdc_amd::sle_parse_ranking accepts ends in front of it
    static_assert(PRE >= tdc_amd::SLE_MAX_HEADER_BYTES + 16, "the ranking is parsed from the first PRE bytes");
    std::vector<u8> pre(std::min(n, PRE));
    u8 last = 0;
    HIP_TRY(hipMemcpyAsync(pre.data(), d_in, pre.size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&last, d_in + n - 1, 1, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    tdc_amd::SleRanking R;
    try { tdc_amd::sle_parse_ranking(pre.data(), pre.size(), tdc_amd::sle_total_bits(n, last), kmer, R); }
    catch (const std::runtime_error&) { throw bad; }
    std::vector<SleDecTab> tab(1);
    memset(&tab[0], 0, sizeof(SleDecTab));
    for (u32 i = 0; i < R.sigma; ++i) tab[0].ent[i] = R.ent[i];
    // (arena allocations are 256-byte aligned, 64 bytes of slack behind n); LA: the longest code
    return code_decode_device(c, SleCode{nullptr, R.sb, R.sigma}, tab[0], (const u32*)d_in, n, R.body, R.total, tdc_amd::sle_code_len(R.sb, 7));
}

StageOut rle_decode_device(Ctx& c, const u8* d_in, size_t n, u64 offset) {
    StageOut r;
    if (n == 0) { r.d = stage_out(c, 0); return r; }
    hipStream_t s = c.stream;
    const u32 ntiles = cdiv(n, RLD_T), nblocks = cdiv(ntiles, RLD_WT);
    u32* d_err = (u32*)c.arena.alloc_top(256);
    u64* tsum = (u64*)c.arena.alloc_top(((size_t)ntiles + 1) * 8);
    u16* exit0 = (u16*)c.arena.alloc_top((size_t)ntiles * RLD_S * 2);
    HIP_TRY(hipMemsetAsync(d_err, 0, 4, s));
    rld_exit_kernel<<<std::min<u32>(nblocks, DEC_MAX_BLOCKS), 256, 0, s>>>(d_in, n, offset, ntiles, nblocks, exit0);
    LAUNCH_CHECK();
    const u16* entry = dx_entries(c, exit0, ntiles, RLD_S, c.arena.alloc_top(dx_entries_scratch(ntiles, RLD_S)));
    rld_walk_kernel<false><<<std::min<u32>(nblocks, DEC_MAX_BLOCKS), RLD_WT, 0, s>>>(d_in, n, offset, entry, ntiles, nblocks, tsum, nullptr, nullptr, nullptr, d_err);
    LAUNCH_CHECK();
    exclusive_sum_u64(c, tsum, tsum, ntiles, tsum + ntiles);
    const u32 err = c.read(d_err);
    r.len = c.read(tsum + ntiles);
    if (err) throw StreamFormatError{"pipeline: malformed stream"};
    if (r.len > STAGE_MAX_BYTES) throw StageTooLarge{r.len};
    r.d = stage_out(c, r.len);
    const size_t nout = (size_t)(r.len / RLD_OT) + 1;
    u32* head = (u32*)c.arena.alloc_top(nout * 4);
    u64* info = (u64*)c.arena.alloc_top(nout * 8);
    HIP_TRY(hipMemsetAsync(head, 0, nout * 4, s));
    rld_walk_kernel<true><<<std::min<u32>(nblocks, DEC_MAX_BLOCKS), RLD_WT, 0, s>>>(d_in, n, offset, entry, ntiles, nblocks, tsum, r.d, head, info, d_err);
    LAUNCH_CHECK();
    inclusive_max_u32(c, head, head, nout);
    rld_fill_kernel<<<dec_grid((size_t)((r.len + 15) / 16)), 256, 0, s>>>(head, info, r.len, r.d);
    LAUNCH_CHECK();
    return r;
}

}  // namespace tdc
