// lz_batch.hip -- lzw and lz78 over many independent texts in one call, parsed ON THE DEVICE ("Batches"): the
// kernels, the stage functions and the entry points of include/tdc_gpu.h.
//
// The LZ78 / LZW parse of ONE text is sequential and the single calls run it on the host.  Across texts the parses
// are independent: one wave takes one text (workgroups of one wave, as the batch decoder of lzss_sw_batch.hip: barriers at the wave's
// own pace, no deadlock against a neighbour with another trip count), and thousands of waves run side by side.
//   the table      every text owns 2^b >= 2 (n_k + 1) 64-bit words of the arena, zeroed by the call: open addressing, linear probing.  A
//                  word is  key << 31 | tag << 25 | child id, key = parent id << 8 | byte: the EXACT key (a child id is never 0, so an
//                  empty word is 0).  A node lives at the
//                  hash of the STRING it spells (lz78_host.cpp), which needs no memory access: the 64 lanes hash the next 64 prefixes of
//                  the phrase (lane d: text[i .. i + d + 1), two polynomial hashes by a prefix sum across the wave) and all probe at
//                  once.  The tag, 6 more bits of that hash, lets a lane pass over foreign words on its own, before it knows its parent.
//   the walk       lane d's word must hold the key (child id lane d - 1 found, byte d): one ballot, and the phrase ends at the first
//                  lane that does not.  That lane either sits on an empty word -- the node is new and goes there -- or on a foreign word
//                  with its tag (1 in 64 collisions), and it alone probes on.  A phrase deeper than 64 takes another turn.  A phrase thus
//                  costs about one memory latency, not one per byte.  Exactness rests on the key compare alone; the hash (and option
//                  lz_batch_hash_bits, which leaves only k bits of it) only says where a node lives.  Ids are insertion order.
//   the items      z_k <= n_k, so text k's items go to items[off[k] + j]: no item count is needed before the parse, and the packers
//                  find a text's items without a search.  The wave notes each item's bit under EliasGammaCoder (ibit) and sums them;
//                  under BitCoder the bit count is S(z_k) (lzw_offsets.hpp).
//   placement      per text: its bits -> its 8-byte aligned slot (0 for a refused text) | 64-bit scan: out_off | one read-back | pack |
//                  one terminator per text, as lzss_sw_batch.hip.  lzw + bit: one thread per OUTPUT word gathers its codes
//                  (lzw_bit_pack_kernel's scheme; the word's text by a search over out_off).  gamma: a workgroup per text, a thread
//                  packs 8 items in a row through one BitSink seated at the first one's bit.
#include "api.hpp"
#include "bitsink.hpp"
#include "decode.hpp"
#include "lzw_offsets.hpp"

#include <algorithm>
#include <vector>

namespace tdc {

namespace {

constexpr u32 LZB_TEXT_MAX = 0x1FFFF00u;         // 2^25 - 256 bytes per text: ids stay below 2^25 (lzw: 255 + z), a key below 2^33
constexpr u32 LZB_ID_MASK = 0x1FFFFFFu;
constexpr u32 LZB_B1 = 0x9E3779B1u, LZB_B2 = 0x85EBCA6Bu;             // the bases of the two polynomial hashes (odd)
constexpr u32 lzb_pow64(u32 b) { for (int i = 0; i < 6; ++i) b *= b; return b; }

struct LzbParse {
    const u8* __restrict__ text; const u32* __restrict__ off; u32 count;
    u64* tab; const u64* __restrict__ tab_off;      // text k: tab[tab_off[k], tab_off[k + 1]), a power of two of words
    u32 hash_bits;
    u32* items; u8* chars; u32* ibit;               // n each, text k's from off[k] on; chars: lz78; ibit: nullable
    u32* z; u64* gbits; int* status;                // per text: items, their bits under gamma, the verdict
};

// The table's words are read by lanes that did not write them: agent-scope accesses (never the scalar cache), and a workgroup barrier
// -- the wave's own -- between an insert and the next phrase's probes.
__device__ __forceinline__ u64 lzb_ld(u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void lzb_st(u64* p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ u32 lzb_tag(u64 w) { return ((u32)w >> 25) & 0x3Fu; }
__device__ __forceinline__ u64 lzb_mix(u32 a, u32 b) {
    u64 x = ((u64)a << 32) | b;
    x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32; x *= 0x94D049BB133111EBull; x ^= x >> 29;
    return x;
}
// From `slot` on: the first word that is empty or carries `tag`.  false: all mask + 1 words have been passed over -- the load stays at or
// below 1/2 (z_k <= n_k nodes in >= 2 (n_k + 1) words), so an empty word always ends the run; the bound only keeps a broken table from
// spinning, and the text then gets TDC_GPU_ERR_INTERNAL.
__device__ __forceinline__ bool lzb_probe(u64* T, u32 mask, u32 tag, u32& slot, u32& tries, u64& w) {
    while (tries <= mask) {
        w = lzb_ld(T + slot);
        if (!w || lzb_tag(w) == tag) return true;
        slot = (slot + 1) & mask; ++tries;
    }
    return false;
}

// Termination: a text's loop runs once per phrase and every phrase moves i forward by at least one byte (lz78: the matched bytes and
// the new one; lzw: at least the root's byte).  A phrase takes turns of 64 depths; a turn either ends the phrase or moves p0 forward by
// 64, and a turn at p0 >= n has no valid lane and ends it.  Inside a turn the verify loop leaves `first` where it is or moves it up, and
// while it stays, lane `first` passes over at least one word per round: at most 64 (mask + 1) rounds (lzb_probe).
template <bool LZW>
__global__ __launch_bounds__(64) void lzb_parse_kernel(const LzbParse P) {
    const u32 lane = threadIdx.x;
    u32 pw1 = 1, pw2 = 1;                                             // B^lane
    for (u32 t = 0; t < lane; ++t) { pw1 *= LZB_B1; pw2 *= LZB_B2; }
    for (u32 k = blockIdx.x; k < P.count; k += gridDim.x) {
        const u32 start = P.off[k], n = P.off[k + 1] - start;
        if (n > LZB_TEXT_MAX) {
            if (lane == 0) { P.z[k] = 0; P.gbits[k] = 0; P.status[k] = TDC_ERR_TOO_LARGE; }
            continue;
        }
        u64* T = P.tab + P.tab_off[k];
        const u32 cap = (u32)(P.tab_off[k + 1] - P.tab_off[k]), mask = cap - 1;       // cap >= 2
        const u32 shift = 64u - (u32)__builtin_ctz(cap);
        const u32 hmask = P.hash_bits ? (1u << P.hash_bits) - 1u : 0xFFFFFFFFu;
        const u8* tx = P.text + start;
        u32* it = P.items + start;
        u8* ch = LZW ? nullptr : P.chars + start;
        u32* ib = P.ibit ? P.ibit + start : nullptr;
        u32 i = 0, z = 0, next_id = LZW ? 256u : 1u;
        u64 nbits = 0;
        int verdict = 0;
        while (i < n) {                                               // one phrase per turn of this loop
            u32 node, parent = 0, p0, ha, hb, ma, mb;                 // the node reached, the one above it, the next byte to match
            if (LZW) { node = tx[i]; p0 = i + 1; ha = hb = node + 1u; ma = LZB_B1; mb = LZB_B2; }
            else { node = 0; p0 = i; ha = hb = 0; ma = mb = 1; }
            u32 id = 0, cc = 0;                                       // the item of this phrase
            for (;;) {                                                // 64 depths per turn
                const u32 p = p0 + lane;
                const bool valid = p < n;
                const u32 c = valid ? tx[p] : 0u;
                // (byte + 1: a run of zero bytes must not hash to the same word at every depth)
                const u32 h1 = ha + ma * wave_inclusive_sum_u32((c + 1u) * pw1), h2 = hb + mb * wave_inclusive_sum_u32((c + 1u) * pw2);
                const u64 x = lzb_mix(h1, h2);
                const u32 tag = (u32)x & 0x3Fu;
                u32 slot = ((u32)(x >> shift) & hmask) & mask, tries = 0;
                u64 w = 0;
                bool ok = valid ? lzb_probe(T, mask, tag, slot, tries, w) : true;
                u32 first;
                for (;;) {
                    u32 prev = __shfl_up((u32)w & LZB_ID_MASK, 1, 64);
                    if (lane == 0) prev = node;
                    const bool hit = valid && ok && w && (w >> 31) == (((u64)prev << 8) | c);
                    const u64 miss = ~__ballot(hit);
                    first = miss ? (u32)__builtin_ctzll(miss) : 64u;
                    const bool foreign = lane == first && valid && ok && w;             // its tag, another key
                    if (!__ballot(foreign)) break;
                    if (foreign) { slot = (slot + 1) & mask; ++tries; ok = lzb_probe(T, mask, tag, slot, tries, w); }
                }
                if (__ballot(!ok)) { verdict = TDC_ERR_INTERNAL; break; }
                const u32 val = (u32)w & LZB_ID_MASK;
                const u32 last = first ? __shfl(val, (int)first - 1, 64) : node;       // the node `first` depths further down
                const u32 above = first >= 2 ? __shfl(val, (int)first - 2, 64) : first == 1 ? node : parent;
                if (first == 64) {                                    // all of them matched: the next 64 depths
                    node = last; parent = above; p0 += 64;
                    ha = __shfl(h1, 63, 64); hb = __shfl(h2, 63, 64); ma *= lzb_pow64(LZB_B1); mb *= lzb_pow64(LZB_B2);
                    continue;
                }
                const u32 e = p0 < n ? (n - p0 < 64u ? n - p0 : 64u) : 0u;           // the valid lanes
                if (first < e) {                                      // lane `first` found no node: the new one goes where it looked
                    cc = __shfl(c, (int)first, 64);
                    if (lane == first) lzb_st(T + slot, ((((u64)last << 8) | cc) << 31) | ((u64)tag << 25) | next_id);
                    ++next_id;
                    id = last;
                    i = p0 + first + (LZW ? 0u : 1u);                 // lzw: the next phrase starts AT the byte that did not match
                    __syncthreads();                                  // the insert, before any lane probes again
                } else {                                              // the text ended inside the dictionary: the left-over phrase
                    id = LZW ? last : above;                          // lzw: the node it stands in; lz78: (parent id, last byte)
                    cc = tx[n - 1];
                    if (!LZW && cc >= 0x80u) verdict = TDC_ERR_UNSUPPORTED;           // the single call's refusal (api_compress.hip)
                    i = n;
                }
                break;
            }
            if (verdict == TDC_ERR_INTERNAL) break;
            if (lane == 0) {
                it[z] = id;
                if (!LZW) ch[z] = (u8)cc;
                if (ib) ib[z] = (u32)nbits;                           // (fewer than 2^25 items of at most 84 bits)
            }
            nbits += 2u * uni_bits_for(id) + 1u + (LZW ? 0u : 2u * uni_bits_for(cc) + 1u);
            ++z;
        }
        if (lane == 0) { P.z[k] = z; P.gbits[k] = nbits; P.status[k] = verdict; }
    }
}

// per text: its bit count and the bytes its stream takes in the output, rounded up to 8 (0 for a refused text)
__global__ __launch_bounds__(256) void lzb_slots_kernel(const u32* __restrict__ z, const u64* __restrict__ gbits, const int* __restrict__ status, u32 count,
                                                         int bit, u64* __restrict__ tbits, u64* __restrict__ slot) {
    for (u32 k = blockIdx.x * 256 + threadIdx.x; k < count; k += gridDim.x * 256) {
        const u64 tb = bit ? lzw_offset(z[k]) : gbits[k];
        const u64 len = (tb >> 3) + ((tb & 7) <= 5 ? 1 : 2);        // bit_stream_len
        tbits[k] = tb;
        slot[k] = status[k] ? 0ull : (len + 7) & ~7ull;
    }
}

// lzw + bit.  Output word j = bits [64 jl, 64 jl + 64) of the stream of its text k, the last k with ooff[k] <= 8 j: a refused text has
// an empty slot and is never the last one.  The codes that touch the word, MSB first; zeros behind code z_k - 1 (lzw_bit_pack_kernel).
__global__ __launch_bounds__(256) void lzb_bit_pack_kernel(const u32* __restrict__ items, const u32* __restrict__ off, const u32* __restrict__ zs,
                                                            const u64* __restrict__ ooff, u32 count, u64* __restrict__ out, u64 words) {
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 j = (u64)blockIdx.x * 256 + threadIdx.x; j < words; j += stride) {
        u32 lo = 0, hi = count - 1;
        while (lo < hi) {
            const u32 mid = lo + (hi - lo + 1) / 2;
            if (ooff[mid] <= 8 * j) lo = mid; else hi = mid - 1;
        }
        const u32* codes = items + off[lo];
        const u64 z = zs[lo], b0 = (j - ooff[lo] / 8) * 64;
        u32 w;
        u64 k = lzw_code_at(b0, w);
        u64 s = lzw_width_base(w) + (k - ((1ull << (w - 1)) - 256)) * w;      // S(k) <= b0
        u64 word = 0;
        while (k < z && s < b0 + 64) {
            const int shift = 64 - (int)((long long)(s + w) - (long long)b0);  // of the code's last bit inside this word
            const u64 c = codes[k];
            word |= shift >= 0 ? c << shift : c >> -shift;                      // (bits in front of the word fall off the top)
            s += w; ++k;
            if (k + 256 == (1ull << w)) ++w;
        }
        out[j] = __builtin_bswap64(word);
    }
}

// gamma: gamma(code) per lzw item, gamma(id) gamma(char) per lz78 item (GammaItems of lz78.hip).  A workgroup per text; a thread packs 8
// items in a row through one sink, seated at the bit of its first one inside the text's stream.  The output is zeroed.
template <bool PAIR>
__global__ __launch_bounds__(256) void lzb_gamma_pack_kernel(const u32* __restrict__ items, const u8* __restrict__ chars, const u32* __restrict__ ibit,
                                                              const u32* __restrict__ off, const u32* __restrict__ zs, const u64* __restrict__ ooff,
                                                              const int* __restrict__ status, u32 count, u64* __restrict__ out) {
    for (u32 k = blockIdx.x; k < count; k += gridDim.x) {
        if (status[k]) continue;
        const u32 z = zs[k], base = off[k];
        const u64 bit0 = 8ull * ooff[k];
        for (u32 j0 = threadIdx.x * 8; j0 < z; j0 += 2048) {
            BitSink sink;
            sink.out = out; sink.pos = bit0 + ibit[base + j0]; sink.acc = 0; sink.cnt = 0;
            for (u32 j = j0; j < j0 + 8 && j < z; ++j) {
                append_uni<ENC_GAMMA>(sink, items[base + j]);
                if (PAIR) append_uni<ENC_GAMMA>(sink, chars[base + j]);
            }
            sink.flush();
        }
    }
}

// io/BitOStream.hpp:53-64 for every stream, as swb_terminators_kernel
__global__ __launch_bounds__(256) void lzb_terminators_kernel(const u64* __restrict__ tbits, const u64* __restrict__ ooff, const int* __restrict__ status,
                                                               u32 count, u8* __restrict__ out) {
    for (u32 k = blockIdx.x * 256 + threadIdx.x; k < count; k += gridDim.x * 256) {
        if (status[k]) continue;
        const u64 tb = tbits[k];
        u8* o = out + ooff[k] + (tb >> 3);
        const u32 u = (u32)(tb & 7);
        if (u <= 5) o[0] |= (u8)u; else o[1] = (u8)u;
    }
}

// tdc_gpu_lz_parse_batch: the items of the texts back to back.  zoff = the scan of the item counts (0 for a text without a parse)
__global__ __launch_bounds__(256) void lzb_counts_kernel(const u32* __restrict__ z, const int* __restrict__ status, u32 count, u64* __restrict__ zoff) {
    for (u32 k = blockIdx.x * 256 + threadIdx.x; k < count; k += gridDim.x * 256)
        zoff[k] = status[k] == TDC_ERR_TOO_LARGE || status[k] == TDC_ERR_INTERNAL ? 0ull : z[k];
}
__global__ __launch_bounds__(256) void lzb_compact_kernel(const u32* __restrict__ items, const u8* __restrict__ chars, const u32* __restrict__ off,
                                                           const u64* __restrict__ zoff, u32 count, u32* __restrict__ d_items, u8* __restrict__ d_chars) {
    for (u32 k = blockIdx.x; k < count; k += gridDim.x) {
        const u32 base = off[k];
        const u64 to = zoff[k], z = zoff[k + 1] - to;
        for (u64 j = threadIdx.x; j < z; j += 256) {
            d_items[to + j] = items[base + j];
            if (chars) d_chars[to + j] = chars[base + j];
        }
    }
}

// workgroups of one wave (the parse) or one per text (the gamma pack): as many as there are texts, up to what keeps every CU busy
// several times over
unsigned lzb_text_grid(size_t count) { return (unsigned)std::min<size_t>(count, (size_t)1 << 16); }

// the words of text k's table: the power of two from 2 (n + 1) on; none for a text the parse refuses
u64 lzb_table_words(u64 n) {
    if (n > LZB_TEXT_MAX) return 0;
    u64 cap = 2;
    while (cap < 2 * (n + 1)) cap <<= 1;
    return cap;
}

// the device side of one batch: what the caller uploaded, and what the parse leaves in the arena
struct LzBatch {
    const u8* text = nullptr; const u32* off = nullptr;
    u32* items = nullptr; u8* chars = nullptr; u32* ibit = nullptr;
    u32* z = nullptr; u64* gbits = nullptr; int* status = nullptr; u64* tbits = nullptr; u64* ooff = nullptr;
};

// what the host knows before the device is asked: the borders as 32-bit words, every text's table, and the arena they need
struct LzbPlan { std::vector<u32> off32; std::vector<u64> toff; u64 words = 0; };
void lz_batch_plan(Ctx& c, const uint64_t* in_off, size_t count, LzbPlan& L) {
    const size_t n = (size_t)in_off[count];
    L.off32.resize(count + 1); L.toff.resize(count + 1);
    for (size_t k = 0; k <= count; ++k) {
        L.off32[k] = (u32)in_off[k];
        L.toff[k] = L.words;
        if (k < count) L.words += lzb_table_words(in_off[k + 1] - in_off[k]);
    }
    // the text, 8 bytes and (lz78) a char per position, the tables (at most 32 bytes per position), 48 bytes per text, the output or the
    // items once more (at most 11 bytes per position)
    reserve_arena(c, 21 * n + 8 * (size_t)L.words + 56 * (count + 1) + ((size_t)64 << 20));
}

// uploads the texts and their borders (*e_up: the event behind them), zeroes the tables and runs the parse (count >= 1).  Enqueued only:
// the plan must outlive the caller's first read-back.
void lz_batch_parse(Ctx& c, const uint8_t* in, size_t n, size_t count, const LzbPlan& L, bool lzw, bool want_ibit, LzBatch& B, Events& ev, int* e_up) {
    hipStream_t s = c.stream;
    B.text = upload_plain(c, in, n);
    u32* d_off = c.arena.get<u32>(count + 1);
    u64* d_toff = c.arena.get<u64>(count + 1);
    HIP_TRY(hipMemcpyAsync(d_off, L.off32.data(), (count + 1) * sizeof(u32), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_toff, L.toff.data(), (count + 1) * sizeof(u64), hipMemcpyHostToDevice, s));
    *e_up = ev.tick();
    B.off = d_off;
    B.items = c.arena.get<u32>(n + 1);
    B.chars = lzw ? nullptr : c.arena.get<u8>(n + 1);
    B.ibit = want_ibit ? c.arena.get<u32>(n + 1) : nullptr;
    B.z = c.arena.get<u32>(count); B.gbits = c.arena.get<u64>(count); B.status = c.arena.get<int>(count);
    B.tbits = c.arena.get<u64>(count); B.ooff = c.arena.get<u64>(count + 1);
    u64* tab = c.arena.get<u64>((size_t)L.words + 1);
    if (L.words) HIP_TRY(hipMemsetAsync(tab, 0, (size_t)L.words * sizeof(u64), s));
    LzbParse P;
    P.text = B.text; P.off = d_off; P.count = (u32)count; P.tab = tab; P.tab_off = d_toff; P.hash_bits = (u32)c.lz_batch_hash_bits;
    P.items = B.items; P.chars = B.chars; P.ibit = B.ibit; P.z = B.z; P.gbits = B.gbits; P.status = B.status;
    if (lzw) lzb_parse_kernel<true><<<lzb_text_grid(count), 64, 0, s>>>(P);
    else lzb_parse_kernel<false><<<lzb_text_grid(count), 64, 0, s>>>(P);
    LAUNCH_CHECK();
}

int lz_batch_coder(bool lzw, int coder) {        // 1: BitCoder, 0: EliasGammaCoder, -1: not taken -- the coders of the single calls
    if (coder == TDC_GPU_CODER_GAMMA) return 0;
    return lzw && coder == TDC_GPU_CODER_BIT ? 1 : -1;
}

// what can be said of the arguments without a device; throws ArgError
void lz_batch_check_offsets(const uint64_t* in_off, size_t count) {
    if (in_off[0] != 0) throw ArgError{TDC_GPU_ERR_ARG, "lz batch: in_off[0] must be 0"};
    for (size_t k = 0; k < count; ++k)
        if (in_off[k + 1] < in_off[k]) throw ArgError{TDC_GPU_ERR_ARG, "lz batch: in_off must not decrease"};
    if (in_off[count] > 0xFFFFFFFEull || count > 0xFFFFFFFEull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "lz batch: the texts must be at most 2^32 - 2 bytes in all"};
}
void lz_batch_check(bool lzw, const uint8_t* in, const uint64_t* in_off, size_t count, int coder, const uint8_t* out, const uint64_t* out_off,
                    const uint64_t* out_len, const int32_t* status) {
    if (!in_off || !out_off || (count && (!out || !out_len || !status))) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
    if (lz_batch_coder(lzw, coder) < 0)
        throw ArgError{TDC_GPU_ERR_UNSUPPORTED, lzw ? "lzw: only coder=bit and coder=gamma are built" : "lz78: only coder=gamma is built"};
    lz_batch_check_offsets(in_off, count);
    if (!in && in_off[count]) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
}

// the worst case of a text of n bytes: n items, every field at its widest for such a text, and the terminator
size_t lz_batch_text_bound(u64 n, bool lzw, bool bit) {
    const u64 bits = !lzw ? n * (2 * bits_for(n) + 1 + 17) : bit ? lzw_offset(n) : n * (2 * bits_for(n + 255) + 1);
    return bit_stream_len(bits);
}
size_t lz_batch_bound(const uint64_t* in_off, size_t count, bool lzw, int coder) {
    const int bit = lz_batch_coder(lzw, coder);
    if (!in_off || in_off[0] != 0 || bit < 0) return 0;
    size_t sum = 0;
    for (size_t k = 0; k < count; ++k) {
        if (in_off[k + 1] < in_off[k]) return 0;
        sum += align_up(lz_batch_text_bound(in_off[k + 1] - in_off[k], lzw, bit != 0), 8);
    }
    return in_off[count] > 0xFFFFFFFEull ? 0 : sum;
}

void lz_compress_batch(tdc_gpu_ctx* ctx, bool lzw, const uint8_t* in, const uint64_t* in_off, size_t count, int coder, uint8_t* out, size_t out_cap,
                       uint64_t* out_off, uint64_t* out_len, int32_t* status, tdc_gpu_stats* stats) {
    const bool bit = lz_batch_coder(lzw, coder) == 1;
    Ctx& c = ctx->c;
    if (stats) memset(stats, 0, sizeof(*stats));
    out_off[0] = 0;
    if (count == 0) return;
    const size_t n = (size_t)in_off[count];
    hipStream_t s = c.stream;
    LzbPlan L;
    lz_batch_plan(c, in_off, count, L);
    Events ev(c);
    const int e0 = ev.tick();
    int e1 = e0;
    LzBatch B;
    lz_batch_parse(c, in, n, count, L, lzw, !bit, B, ev, &e1);
    lzb_slots_kernel<<<dec_grid(count), 256, 0, s>>>(B.z, B.gbits, B.status, (u32)count, bit ? 1 : 0, B.tbits, B.ooff);
    LAUNCH_CHECK();
    exclusive_sum_u64(c, B.ooff, B.ooff, count, B.ooff + count);
    // the sizes: where every stream goes, its bits, its items and the texts that are refused
    std::vector<u64> tbits(count);
    std::vector<u32> z(count);
    c.read_n(B.ooff, (u64*)out_off, count + 1);
    c.read_n(B.tbits, tbits.data(), count);
    c.read_n(B.z, z.data(), count);
    c.read_n(B.status, (int*)status, count);
    u64 factors = 0;
    for (size_t k = 0; k < count; ++k) {
        out_len[k] = status[k] ? 0 : bit_stream_len(tbits[k]);
        if (!status[k]) factors += z[k];
    }
    const int e2 = ev.tick();
    const size_t used = (size_t)out_off[count];
    if (used > out_cap) throw ArgError{TDC_GPU_ERR_OOM, "lz batch: output buffer too small (out_off[count] holds the required size)"};
    u8* d_out = c.arena.get<u8>(used + 8);
    if (used) {
        if (bit) {
            lzb_bit_pack_kernel<<<dec_grid(used / 8), 256, 0, s>>>(B.items, B.off, B.z, B.ooff, (u32)count, (u64*)d_out, (u64)(used / 8));
        } else {
            HIP_TRY(hipMemsetAsync(d_out, 0, used, s));
            if (lzw) lzb_gamma_pack_kernel<false><<<lzb_text_grid(count), 256, 0, s>>>(B.items, B.chars, B.ibit, B.off, B.z, B.ooff, B.status, (u32)count, (u64*)d_out);
            else lzb_gamma_pack_kernel<true><<<lzb_text_grid(count), 256, 0, s>>>(B.items, B.chars, B.ibit, B.off, B.z, B.ooff, B.status, (u32)count, (u64*)d_out);
        }
        LAUNCH_CHECK();
    }
    lzb_terminators_kernel<<<dec_grid(count), 256, 0, s>>>(B.tbits, B.ooff, B.status, (u32)count, d_out);
    LAUNCH_CHECK();
    const int e3 = ev.tick();
    if (used) HIP_TRY(hipMemcpyAsync(out, d_out, used, hipMemcpyDeviceToHost, s));
    const int e4 = ev.tick();
    if (stats) {
        stats->n = n; stats->out_len = used; stats->factors = factors; stats->arena_bytes = c.arena.high;
        ev.span(&stats->ms_h2d, e0, e1); ev.span(&stats->ms_factorize, e1, e2); ev.span(&stats->ms_encode, e2, e3);
        ev.span(&stats->ms_d2h, e3, e4); ev.span(&stats->ms_total, e0, e4);
    }
    ev.finish();
}

void lz_parse_batch(tdc_gpu_ctx* ctx, bool lzw, const uint8_t* in, const uint64_t* in_off, size_t count, uint32_t* items, uint8_t* chars,
                    uint64_t* item_off, int32_t* status) {
    Ctx& c = ctx->c;
    item_off[0] = 0;
    if (count == 0) return;
    hipStream_t s = c.stream;
    LzbPlan L;
    lz_batch_plan(c, in_off, count, L);
    Events ev(c);
    int e1 = 0;
    LzBatch B;
    lz_batch_parse(c, in, (size_t)in_off[count], count, L, lzw, false, B, ev, &e1);
    lzb_counts_kernel<<<dec_grid(count), 256, 0, s>>>(B.z, B.status, (u32)count, B.ooff);
    LAUNCH_CHECK();
    exclusive_sum_u64(c, B.ooff, B.ooff, count, B.ooff + count);
    c.read_n(B.ooff, (u64*)item_off, count + 1);
    c.read_n(B.status, (int*)status, count);
    const size_t total = (size_t)item_off[count];
    u32* d_items = c.arena.get<u32>(total + 1);
    u8* d_chars = lzw ? nullptr : c.arena.get<u8>(total + 1);
    lzb_compact_kernel<<<lzb_text_grid(count), 256, 0, s>>>(B.items, B.chars, B.off, B.ooff, (u32)count, d_items, d_chars);
    LAUNCH_CHECK();
    if (total) {
        HIP_TRY(hipMemcpyAsync(items, d_items, total * sizeof(u32), hipMemcpyDeviceToHost, s));
        if (!lzw) HIP_TRY(hipMemcpyAsync(chars, d_chars, total, hipMemcpyDeviceToHost, s));
    }
    ev.finish();
}

int compress_batch_entry(tdc_gpu_ctx* ctx, bool lzw, const uint8_t* in, const uint64_t* in_off, size_t count, int coder, uint8_t* out, size_t out_cap,
                         uint64_t* out_off, uint64_t* out_len, int32_t* status, tdc_gpu_stats* stats) {
    try { lz_batch_check(lzw, in, in_off, count, coder, out, out_off, out_len, status); }      // (before the context: no device needed)
    catch (const ArgError& e) { if (ctx) ctx->last_error = e.msg; return e.code; }
    return guarded(ctx, [&] { lz_compress_batch(ctx, lzw, in, in_off, count, coder, out, out_cap, out_off, out_len, status, stats); });
}

}  // namespace

}  // namespace tdc

using namespace tdc;

extern "C" {

size_t tdc_gpu_lzw_batch_bound(const uint64_t* in_off, size_t count, int coder) { return lz_batch_bound(in_off, count, true, coder); }
size_t tdc_gpu_lz78_batch_bound(const uint64_t* in_off, size_t count, int coder) { return lz_batch_bound(in_off, count, false, coder); }

int tdc_gpu_lzw_compress_batch(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* in_off, size_t count, int coder, uint8_t* out, size_t out_cap,
                               uint64_t* out_off, uint64_t* out_len, int32_t* status, tdc_gpu_stats* stats) {
    return compress_batch_entry(ctx, true, in, in_off, count, coder, out, out_cap, out_off, out_len, status, stats);
}

int tdc_gpu_lz78_compress_batch(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* in_off, size_t count, int coder, uint8_t* out, size_t out_cap,
                                uint64_t* out_off, uint64_t* out_len, int32_t* status, tdc_gpu_stats* stats) {
    return compress_batch_entry(ctx, false, in, in_off, count, coder, out, out_cap, out_off, out_len, status, stats);
}

int tdc_gpu_lz_parse_batch(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* in_off, size_t count, int lzw, uint32_t* items, uint8_t* chars,
                           uint64_t* item_off, int32_t* status) {
    try {
        if (!in_off || !item_off || (count && !status)) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
        lz_batch_check_offsets(in_off, count);
        if (in_off[count] && (!in || !items || (!lzw && !chars))) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
    } catch (const ArgError& e) { if (ctx) ctx->last_error = e.msg; return e.code; }
    return guarded(ctx, [&] { lz_parse_batch(ctx, lzw != 0, in, in_off, count, items, chars, item_off, status); });
}

}  // extern "C"
