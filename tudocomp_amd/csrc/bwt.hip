// bwt.hip -- the bwt compressor (compressors/BWTCompressor.hpp, ds/bwt.hpp of the reference) on the device; DESIGN.md section 5.2.
//   forward: one gather over the suffix array, bwt[i] = T[SA[i] - 1] (T[n - 1] where SA[i] = 0), chunk by chunk in front of the download;
//   inverse: LF[i] = C[b[i]] + #{j < i : b[j] = b[i]} by one pass of a stable 8-bit counting sort that keeps only the destination index,
//            then list ranking of the one n-cycle of LF with sampled heads (Helman-JaJa): bounded walks from every head to the next one,
//            pointer jumping over the heads, and a second walk that writes the text.  The reference walks LF one byte at a time.
#include "stages.hpp"
#include "prim.hpp"
#include "decode.hpp"
#include "bwt_passes.hpp"

namespace tdc {
namespace {

// ---- forward ------------------------------------------------------------------------------------------------------------------------
// rows [a, b) of the transform, four rows per work-item (a is a multiple of 4: one aligned word of output per item)
__global__ void __launch_bounds__(256) bwt_gather_kernel(const u8* __restrict__ text, const u32* __restrict__ sa, size_t a, size_t b, size_t n,
                                                         u8* __restrict__ out) {
    const size_t items = (b - a + 3) / 4;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < items; g += (size_t)gridDim.x * 256) {
        const size_t i = a + g * 4;
        if (i + 4 <= b) {
            const uint4 s = *(const uint4*)(sa + i);
            const u32 c0 = text[s.x ? s.x - 1 : n - 1], c1 = text[s.y ? s.y - 1 : n - 1], c2 = text[s.z ? s.z - 1 : n - 1], c3 = text[s.w ? s.w - 1 : n - 1];
            *(u32*)(out + i) = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
        } else {
            for (size_t j = i; j < b; ++j) { const u32 p = sa[j]; out[j] = text[p ? p - 1 : n - 1]; }
        }
    }
}

// ---- inverse: LF ----------------------------------------------------------------------------------------------------------------------
constexpr int LF_NW = 4, LF_ITEMS = 16;
constexpr u32 LF_TILE = LF_NW * 64 * LF_ITEMS;          // 4096 rows per tile; wave w ranks rows [w * 1024, (w + 1) * 1024) of it

// tile histograms, symbol-major: hist[c * ntiles + tile] -- the exclusive scan of the whole table is then C[c] + the number of c in the
// tiles in front, the base of the stable rank
__global__ void __launch_bounds__(256) bwt_tile_hist_kernel(const u8* __restrict__ b, size_t n, u32 ntiles, u32* __restrict__ hist) {
    __shared__ u32 h[LF_NW][256];
    const int w = wave_id();
    for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (int i = threadIdx.x; i < LF_NW * 256; i += 256) (&h[0][0])[i] = 0;
        __syncthreads();
        const size_t base = (size_t)tile * LF_TILE + (size_t)threadIdx.x * 16;
        if (base + 16 <= n) {
            const uint4 v = *(const uint4*)(b + base);
            const u32 x[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) atomicAdd(&h[w][(x[k] >> (8 * j)) & 255u], 1u);
        } else {
            for (size_t i = base; i < n && i < base + 16; ++i) atomicAdd(&h[w][b[i]], 1u);
        }
        __syncthreads();
        const u32 t = threadIdx.x;
        hist[(size_t)t * ntiles + tile] = h[0][t] + h[1][t] + h[2][t] + h[3][t];
        __syncthreads();
    }
}

// The ranking of one pass of the LSD radix sort (prim.hip) without its scatter: LF[i] is written in row order.
__global__ void __launch_bounds__(256) bwt_lf_kernel(const u8* __restrict__ b, size_t n, u32 ntiles, const u32* __restrict__ base, u32* __restrict__ lf) {
    __shared__ u32 wcnt[LF_NW][256];
    __shared__ unsigned long long match[LF_NW * 256];
    const int lane = lane_id(), w = wave_id();
    const u64 lanebit = 1ull << lane;
    const u64 lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    unsigned long long* M = match + w * 256;
    u32* mycnt = wcnt[w];
    for (int i = threadIdx.x; i < LF_NW * 256; i += 256) match[i] = 0ull;
    for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (int i = threadIdx.x; i < LF_NW * 256; i += 256) (&wcnt[0][0])[i] = 0;
        __syncthreads();
        const size_t row0 = (size_t)tile * LF_TILE + (size_t)w * (64 * LF_ITEMS) + lane;
        u32 pk[LF_ITEMS];                                  // byte << 16 | rank inside the wave's part of the tile (< 1024)
#pragma unroll
        for (int j = 0; j < LF_ITEMS; ++j) {
            const size_t idx = row0 + (size_t)j * 64;
            const bool valid = idx < n;
            const u32 d = valid ? (u32)b[idx] : 0u;
            const u64 peers = wave_match_peel<4, 8>(M, d, valid, lanebit);
            const u32 prefix = lds_load(&mycnt[d]);
            const u32 rank = (u32)__popcll(peers & lt_mask);
            pk[j] = (d << 16) | (prefix + rank);
            if (valid && rank == 0) lds_store(&mycnt[d], prefix + (u32)__popcll(peers));
        }
        __syncthreads();
        {   // thread t = byte value t: where the rows of every wave with that byte start
            const u32 t = threadIdx.x;
            u32 run = base[(size_t)t * ntiles + tile];
#pragma unroll
            for (int i = 0; i < LF_NW; ++i) { const u32 cnt = wcnt[i][t]; wcnt[i][t] = run; run += cnt; }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < LF_ITEMS; ++j) {
            const size_t idx = row0 + (size_t)j * 64;
            if (idx < n) lf[idx] = wcnt[w][pk[j] >> 16] + (pk[j] & 0xFFFFu);
        }
        __syncthreads();
    }
}

// ---- inverse: list ranking ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) bwt_heads_init_kernel(Heads H, Mix m, u32 n) {
    for (u64 kk = (u64)blockIdx.x * 256 + threadIdx.x; kk < m.T; kk += (u64)gridDim.x * 256) {
        const u32 k = (u32)kk;
        const u32 row = unmix(k, m);
        H.hrow[k] = row < n ? row : NONE32;
        H.hlen[k] = 0;
        H.w[k] = W_END;
    }
}

// First walk, slots [lo, hi): follow LF from the head until row 0 (the cycle is cut there), a head, or max_steps steps -- then the row
// reached becomes a head of its own behind the hashed slots, for the next launch.  Every list is at most max_steps rows long, the lists
// are disjoint (LF is a permutation whatever the input), so at most n / max_steps slots are appended and all launches together read n rows.
__global__ void __launch_bounds__(256) bwt_walk1_kernel(const u32* __restrict__ lf, Heads H, Mix m, u32 lo, u32 hi, u32 max_steps) {
    u32 longest = 0;
    for (u64 kk = (u64)lo + (u64)blockIdx.x * 256 + threadIdx.x; kk < hi; kk += (u64)gridDim.x * 256) {
        const u32 k = (u32)kk;
        u32 cur = H.hrow[k];
        if (cur == NONE32) continue;
        u32 steps = 0, link = NONE32;
        for (;;) {
            cur = lf[cur];
            ++steps;
            if (cur == 0) break;
            const u32 g = mix(cur, m);
            if (g < m.T) { link = g; break; }
            if (steps == max_steps) {
                const u32 id = atomicAdd(&H.cnt[0], 1u);
                if (id < H.cap) { H.hrow[id] = cur; link = id; }
                else atomicOr(&H.cnt[2], 1u);
                break;
            }
        }
        H.hlen[k] = steps;
        H.w[k] = ((u64)link << 32) | steps;
        longest = max(longest, steps);
    }
    longest = wave_reduce_max(longest);
    if (lane_id() == 0 && longest) atomicMax(&H.cnt[1], longest);
}

// Second walk: the head of slot k starts `n - w[k]` rows behind row 0; the row t behind row 0 puts its byte at n - 2 - t (the last row
// of the cycle holds the 0 that ends the text).  The byte of a row is the c with C[c] <= LF[row] < C[c + 1]: one gather per step.
// Positions fall by one per step: the bytes are collected into aligned words.
__global__ void __launch_bounds__(256) bwt_walk2_kernel(const u32* __restrict__ lf, Heads H, u32 slots, const u32* __restrict__ Ctab, u32 n,
                                                        u8* __restrict__ out) {
    __shared__ u32 C[257];
    for (int i = threadIdx.x; i < 257; i += 256) C[i] = Ctab[i];
    __syncthreads();
    for (u64 kk = (u64)blockIdx.x * 256 + threadIdx.x; kk < slots; kk += (u64)gridDim.x * 256) {
        const u32 k = (u32)kk;
        u32 cur = H.hrow[k];
        if (cur == NONE32) continue;
        const u32 len = H.hlen[k];
        const u32 r = n - (u32)H.w[k];
        u32 acc = 0, hi = 0;
        bool open = false;                                 // a word is being filled: byte lanes (pos & 3) .. hi are in acc
        size_t pos = 0;
        for (u32 j = 0; j < len; ++j) {
            const u32 nxt = lf[cur];
            u32 c = 0;
#pragma unroll
            for (u32 s = 128; s; s >>= 1) if (C[c + s] <= nxt) c += s;
            const u32 t = r + j;
            if (t > n - 2) { out[n - 1] = (u8)c; break; }   // (the row of the 0: the last step of the last list)
            pos = (size_t)n - 2 - t;
            const u32 ln = (u32)pos & 3u;
            if (!open) { open = true; hi = ln; acc = 0; }
            acc |= c << (8 * ln);
            if (ln == 0) { put_bytes(out, pos, acc, 0, hi); open = false; }
            cur = nxt;
        }
        if (open) put_bytes(out, pos & ~(size_t)3, acc, (u32)pos & 3u, hi);
    }
}

bool host_pinned(const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeHost;
}

}  // namespace

// bwt[i] = T[SA[i] - 1] into d_out (n + 64 bytes).  host_dst (nullable) page-locked and the text of 128 MiB or more: chunk k is downloaded
// there on the copy stream while chunk k + 1 is gathered, c.stream waits for the last copy, and the function returns true.
bool bwt_gather(Ctx& c, const u8* d_text, const u32* d_sa, size_t n, u8* d_out, u8* host_dst) {
    constexpr size_t CH = (size_t)64 << 20;
    const bool chunked = host_dst && n >= 2 * CH && host_pinned(host_dst) && (n + CH - 1) / CH <= Ctx::CHUNK_EVENTS;
    if (!chunked) {
        bwt_gather_kernel<<<dec_grid((n + 3) / 4), 256, 0, c.stream>>>(d_text, d_sa, 0, n, n, d_out);
        LAUNCH_CHECK();
        return false;
    }
    size_t q = 0;
    for (size_t a = 0; a < n; a += CH, ++q) {
        const size_t b = std::min(n, a + CH);
        bwt_gather_kernel<<<dec_grid((b - a + 3) / 4), 256, 0, c.stream>>>(d_text, d_sa, a, b, n, d_out);
        LAUNCH_CHECK();
        HIP_TRY(hipEventRecord(c.ev_chunk[q], c.stream));
        HIP_TRY(hipStreamWaitEvent(c.copy_stream, c.ev_chunk[q], 0));
        HIP_TRY(hipMemcpyAsync(host_dst + a, d_out + a, b - a, hipMemcpyDeviceToHost, c.copy_stream));
    }
    c.wait_for(c.stream, c.copy_stream);
    return true;
}

// upper bound of what bwt_inverse takes from the arena for a transform of n bytes (hashed slots: at most 2 n / sample + 1)
size_t bwt_inverse_arena(size_t n) { return 6 * n + (size_t)cdiv(n, LF_TILE) * 1024 + (2 * n / BWT_SAMPLE + n / BWT_SAMPLE + 4) * 16 + ((size_t)16 << 20); }

// decode_bwt (ds/bwt.hpp:77-98) with the complete C table.  Returns the text length (0 for inputs of at most one byte).
size_t bwt_inverse(Ctx& c, const u8* bwt, size_t len, u32 sample, u32 max_steps, Sink& out, u32* host_lf, BwtInvStats* st, bool on_device) {
    BwtInvStats local;
    if (!st) st = &local;
    *st = BwtInvStats();
    if (len <= 1) { decode_dest(out, 0); return 0; }
    if (len >= 0x7FFFFFFFull) throw DecodeTooLarge{(u64)len};
    if (out.into && out.cap < len) throw HipError{hipErrorOutOfMemory, "decompress: output buffer too small", (int)__LINE__};
    const size_t n = len;
    const u32 S = sample ? sample : BWT_SAMPLE;
    const u32 M = max_steps ? max_steps : (u32)std::min<u64>((u64)BWT_STEPS_PER_SAMPLE * S, 0x7FFFFFFFull);
    st->sample = S; st->max_steps = M;
    hipStream_t s = c.stream;
    const bool dlog = c.bwt_log != 0;                       // stage times on stderr (synchronises)
    const DecTick tick = dec_ticker(c, "bwt", dlog);

    const Mix mx = make_mix(n, S);
    const u32 ntiles = cdiv(n, LF_TILE);
    const size_t cap = (size_t)mx.T + n / M + 2;             // hashed slots + one per max_steps rows walked
    // (on_device: the transform lies in the arena already, what is needed comes from the room above it)
    if (!on_device) c.ensure_arena(6 * n + (size_t)ntiles * 1024 + cap * 16 + ((size_t)16 << 20));
    u8* d_b = on_device ? const_cast<u8*>(bwt) : c.arena.get<u8>(n + 64);
    u32* d_lf = c.arena.get<u32>(n);
    u8* d_out = c.arena.get<u8>(n + 64);
    u32* d_tab = c.arena.get<u32>(257);
    Heads H;
    H.cnt = c.arena.get<u32>(4);
    H.hrow = c.arena.get<u32>(cap); H.hlen = c.arena.get<u32>(cap); H.w = (unsigned long long*)c.arena.get<u64>(cap);
    H.cap = (u32)std::min<size_t>(cap, 0xFFFFFFFEull);
    if (!on_device) HIP_TRY(hipMemcpyAsync(d_b, bwt, n, hipMemcpyHostToDevice, s));
    tick("upload");

    // C from the byte histogram; exactly one 0 byte
    u32 hist[256];
    {
        const size_t mk = c.arena.mark();
        u32* d_hist = c.arena.get<u32>(256);
        HIP_TRY(hipMemsetAsync(d_hist, 0, 256 * sizeof(u32), s));
        text_histogram_add(c, d_b, n, d_hist);
        c.read_n(d_hist, hist, 256);
        c.arena.release(mk);
    }
    if (hist[0] != 1) throw StreamFormatError{"bwt: the buffer must hold exactly one 0 byte"};
    u32 Ctab[257];
    Ctab[0] = 0;
    for (int i = 0; i < 256; ++i) Ctab[i + 1] = Ctab[i] + hist[i];
    HIP_TRY(hipMemcpyAsync(d_tab, Ctab, sizeof(Ctab), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));                        // (Ctab lives on this frame)
    tick("histogram");

    {   // LF
        const size_t mk = c.arena.mark();
        u32* d_th = c.arena.get<u32>((size_t)ntiles * 256);
        bwt_tile_hist_kernel<<<dec_grid((size_t)ntiles * 256), 256, 0, s>>>(d_b, n, ntiles, d_th);
        LAUNCH_CHECK();
        exclusive_sum_u32(c, d_th, d_th, (size_t)ntiles * 256, nullptr);
        bwt_lf_kernel<<<dec_grid((size_t)ntiles * 256), 256, 0, s>>>(d_b, n, ntiles, d_th, d_lf);
        LAUNCH_CHECK();
        HIP_TRY(hipStreamSynchronize(s));                    // (the scan's scratch goes back to the arena)
        c.arena.release(mk);
    }
    if (host_lf) HIP_TRY(hipMemcpyAsync(host_lf, d_lf, n * sizeof(u32), hipMemcpyDeviceToHost, s));
    tick("LF");

    // first walk, launch by launch until no list is left open
    const u32 init[4] = { mx.T, 0, 0, 0 };
    HIP_TRY(hipMemcpyAsync(H.cnt, init, sizeof(init), hipMemcpyHostToDevice, s));
    bwt_heads_init_kernel<<<dec_grid(mx.T), 256, 0, s>>>(H, mx, (u32)n);
    LAUNCH_CHECK();
    u32 lo = 0, hi = mx.T;
    u32 hc[4];
    while (lo < hi) {
        bwt_walk1_kernel<<<dec_grid(hi - lo), 256, 0, s>>>(d_lf, H, mx, lo, hi, M);
        LAUNCH_CHECK();
        st->launches++;
        c.read_n(H.cnt, hc, 4);
        if (hc[2] || hc[0] > H.cap) throw HipError{hipErrorUnknown, "bwt: head table overflow", (int)__LINE__};
        lo = hi; hi = hc[0];
    }
    const u32 slots = hi;
    st->longest = hc[1];
    tick("first walk");

    // ranks of the heads; a list that does not end (a cycle without row 0) is still changing when the bound is reached
    const u32 bound = (u32)bits_for(slots) + 2;
    bool converged = false;
    while (st->rounds < bound) {
        HIP_TRY(hipMemsetAsync(H.cnt + 3, 0, sizeof(u32), s));
        bwt_jump_kernel<<<dec_grid(slots), 256, 0, s>>>(H, slots);
        LAUNCH_CHECK();
        st->rounds++;
        if (c.read(H.cnt + 3) == 0) { converged = true; break; }
    }
    const u64 w0 = c.read((const u64*)H.w);
    tick("head ranking");
    if (!converged || w0 != (W_END | (u64)n)) throw StreamFormatError{"bwt: the LF mapping of the buffer is not one cycle (not a Burrows-Wheeler transform)"};
    if (dlog || st != &local) {
        // heads in use = slots whose row lies inside the text; counted on the host from hrow only when somebody asks
        std::vector<u32> hr(slots);
        HIP_TRY(hipMemcpyAsync(hr.data(), H.hrow, (size_t)slots * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        u64 used = 0;
        for (u32 r : hr) used += r != NONE32;
        st->heads = used;
    }

    bwt_walk2_kernel<<<dec_grid(slots), 256, 0, s>>>(d_lf, H, slots, d_tab, (u32)n, d_out);
    LAUNCH_CHECK();
    tick("second walk");
    u8* dst = decode_dest(out, n);
    HIP_TRY(hipMemcpyAsync(dst, d_out, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    tick("download");
    if (dlog) fprintf(stderr, "bwt:      n %zu sample %u max_steps %u heads %llu launches %u rounds %u longest %u\n", n, S, M,
                      (unsigned long long)st->heads, st->launches, st->rounds, st->longest);
    return n;
}

}  // namespace tdc
