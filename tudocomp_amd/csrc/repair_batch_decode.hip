// repair_batch_decode.hip -- many repair streams decoded in one call ("Batch decoder").
//
// The grammar passes of repair_decode.hip (repair_passes.hpp) do not care whose rules they visit: the rules of all streams, laid back to
// back with their references rebased to global rule indices, are one forest of backward references, and its text is the texts back to
// back.  So the batch is ONE pass:
//   bits      per stream: the payload bits from its last one or two bytes (payload_bits / FastBits of decode.hpp; the stream of no bytes
//             and the cut-off terminator are refused here).
//   walks     the token borders of one stream are sequential, so one wave takes one stream (workgroups of one wave, an LDS window of the
//             stream: the shape of lzb_walk_kernel) and walks it twice -- for R_k, the number of start symbols m_k and the verdict, and
//             behind the two scans to write the symbols.  The walk reads everything, the count field included; the token reader is
//             rpd_token with its caps, and a token beyond a cap is refused like a cut-off one: there is no host loop to hand it to.
//   one forest  side s of rule i of stream k goes to sym[2 (rule_off[k] + i) + s], start symbol j to sym[2 R + start_off[k] + j], a
//             reference to rule v becomes 256 + rule_off[k] + v.  An index is checked against ITS stream (v < i, v < R_k), so nothing in
//             front of a stream's own rules is reachable.
//   lengths   in the STRICT schedule: a round reads only the lengths of the round before (two buffers), so round r makes exactly the
//             rules of height r known and the rules still unknown after `cap` rounds are exactly those higher than cap -- the verdict
//             on a deep grammar is a function of the stream and the option alone.  A stream that owns such a rule is refused.
//   nothing   the start symbols of a refused stream keep their slots.  They are overwritten with 256 + R, the rule behind the last one,
//             whose length is 0 -- they advance the scan by nothing -- and (once the scan is done) placed at position 0, where that
//             rule's first occurrence then lies as well: the item pass classes them as a rule AT its first occurrence, which writes
//             nothing and makes no factor.  Rule R has no sides in sym, so nothing is seeded from it; the rules of a refused stream are
//             never seeded, and their sides make no items.
//   sizes     advances of all start symbols | 64-bit scan | per stream: the difference at its borders is its text length (above 2^32 - 2:
//             refused) | scan of the accepted lengths: ooff | the start symbols move from the scan over all of them to their text's slot.
// The host reads ooff, status and the rule count once, decides, and only then allocates anything text-sized (api_decompress.hip); first
// occurrences, items, the factor list and the resolver follow as in the single decoder, with global positions.
//
// Words other threads of the same launch write are never read, but for the atomicMin of the first-occurrence pass (repair_passes.hpp);
// every turn of a walk takes at least one bit, so a damaged stream ends in a verdict after at most its bit count.
#include "repair_passes.hpp"
#include "bitsink.hpp"

#include <algorithm>

namespace tdc {

namespace {

constexpr u32 RBD_WIN = 260;                                          // stream words a wave holds in LDS at a time

// bits[k] = payload_bits of stream k; ERR_ARG for the stream of no bytes and for a one-byte stream that announces 6 or 7 bits (FastBits).
// No stream has tokens yet.
__global__ __launch_bounds__(256) void rbd_bits_kernel(const u8* __restrict__ blob, u64 sub, const u64* __restrict__ s_off, const u64* __restrict__ s_len,
                                                        u32 count, u64* __restrict__ bits, int* __restrict__ status, u64* __restrict__ rule_off,
                                                        u64* __restrict__ start_off) {
    for (u32 k = blockIdx.x * 256 + threadIdx.x; k < count; k += gridDim.x * 256) {
        const u64 len = s_len[k];
        u64 total = 0;
        int st = 0;
        if (!len) st = TDC_GPU_ERR_ARG;
        else {
            const u32 fb = blob[s_off[k] - sub + len - 1] & 7u;
            total = len == 1 ? fb : fb >= 6 ? 8ull * (len - 2) + fb : 8ull * (len - 1) + fb;
            if (len == 1 && fb >= 6) { st = TDC_GPU_ERR_ARG; total = 0; }
        }
        bits[k] = total; status[k] = st; rule_off[k] = 0; start_off[k] = 0;
    }
}

// the largest k in [0, hi] with tab[k] <= i, for ascending tab with tab[0] <= i: among equal borders the last one, so a rule's stream is
// never one without rules
__device__ __forceinline__ u32 rbd_stream_of(const u64* __restrict__ tab, u32 hi, u64 i) {
    u32 lo = 0;
    while (lo < hi) {
        const u32 mid = lo + (hi - lo + 1) / 2;
        if (tab[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// One wave walks one stream: the count field (32 bits under bit, one code under gamma / delta), 2 R_k tokens -- a side of rule i names a
// rule below i, in bits_for(i) bits under bit --, then start symbols -- each names a rule below R_k, in bits_for(R_k) bits -- until the
// stream ends.  WRITE = false: rule_off[k] = R_k, start_off[k] = m_k and the verdict of every stream the bits kernel left open; a refused
// stream has no tokens.  WRITE = true (rule_off, start_off scanned; R = rule_off[count]): the symbols of the accepted streams, rebased.
template <int KIND, bool WRITE>
__global__ __launch_bounds__(64) void rbd_walk_kernel(const u8* __restrict__ blob, u64 sub, const u64* __restrict__ s_off, const u64* __restrict__ s_len,
                                                       const u64* __restrict__ bits, u32 count, int* status, u64* rule_off, u64* start_off, u64 R,
                                                       u32* __restrict__ sym) {
    constexpr u32 REACH = RpdTok<KIND>::REACH;
    static_assert(31 + REACH + 32 * BitWin::PEEK_WORDS <= 16 * RBD_WIN, "a refilled window must hold a token and leave half of itself for progress");
    __shared__ u32 win[RBD_WIN];
    const u32 lane = threadIdx.x;
    for (u32 sidx = blockIdx.x; sidx < count; sidx += gridDim.x) {
        if (status[sidx] != 0) continue;                              // (set in an earlier launch; this one writes it behind the walk)
        const u64 total = bits[sidx];
        const u64 ro = WRITE ? rule_off[sidx] : 0ull, so = WRITE ? start_off[sidx] : 0ull;
        const u64 zk = WRITE ? 2 * (rule_off[sidx + 1] - ro) + (start_off[sidx + 1] - so) : 0ull;
        if (WRITE && zk == 0) continue;
        // the stream's words start at the 4-byte border in front of it: its bits are [skew, T) of them
        const u64 b = s_off[sidx] - sub, len = s_len[sidx];
        const u32* s32 = (const u32*)(blob + (b & ~3ull));
        const u64 skew = 8ull * (b & 3ull), T = skew + total;
        const u64 wmax = (T + 31) / 32 + 3;                           // words that exist (the pad behind the blob)
        u64 x = skew, kb = 0, t = 0, rk = 0;
        bool loaded = false, head = true;
        int verdict = 0;
        while (head || t < 2 * rk || x < T) {                         // every turn takes at least one bit, or ends the walk
            if (!loaded || x + REACH + 32 * BitWin::PEEK_WORDS > (kb + RBD_WIN) * 32) {
                __syncthreads();
                kb = x >> 5;
                for (u32 q = lane; q < RBD_WIN; q += 64) win[q] = kb + q < wmax ? __builtin_bswap32(s32[kb + q]) : 0u;
                __syncthreads();
                loaded = true;
            }
            const BitWin bw{win, kb, T};
            if (head) {                                               // the number of rules
                if (KIND == DEC_BIT) {
                    if (x + 32 > T) { verdict = TDC_GPU_ERR_ARG; break; }
                    rk = bw.peek(x) >> 32;
                    x += 32;
                } else {
                    u32 used, v;
                    if (read_field<KIND>(bw, x, RPD_INDEX_BITS, RPD_WBITS, used, v) != FIELD_READ || x + used > T) { verdict = TDC_GPU_ERR_ARG; break; }
                    rk = v;
                    x += used;
                }
                if (rk > 2 * len) { verdict = TDC_GPU_ERR_ARG; break; }              // (a rule takes two symbols of at least two bits each)
                head = false;
                continue;
            }
            const bool side = t < 2 * rk;
            const u64 limit = side ? t >> 1 : rk;
            const u32 w = KIND == DEC_BIT ? uni_bits_for((u32)limit) : 0u;
            u64 end; u32 rule, val;
            if (rpd_token<KIND>(bw, x, T, w, end, rule, val) != RPD_OK || (rule && (u64)val >= limit)) { verdict = TDC_GPU_ERR_ARG; break; }
            if (WRITE) {
                if (t >= zk) break;                                   // (never: the first walk counted the same tokens)
                if (lane == (u32)(t & 63u)) {
                    const u64 slot = side ? 2 * ro + t : 2 * R + so + (t - 2 * rk);
                    sym[slot] = rule ? 256u + (u32)ro + val : val;    // (ro + val < R, and 256 + R < 2^32: the call's token limit)
                }
            }
            ++t;
            x = end;
        }
        if (!WRITE && lane == 0) {
            if (verdict) status[sidx] = verdict;
            rule_off[sidx] = verdict ? 0ull : rk;
            start_off[sidx] = verdict ? 0ull : t - 2 * rk;
        }
    }
}

// One round of the lengths in the strict schedule: cur[k] = prev[k] where that is known, else len(l) + len(r) from prev where both are
// (0 = not known yet, saturating at 2^32 - 1).  prev was written by the launch before.
__global__ __launch_bounds__(256) void rbd_len_kernel(const u32* __restrict__ sym, u32 R, const u32* __restrict__ prev, u32* __restrict__ cur,
                                                       u32* __restrict__ changed) {
    bool any = false;
    for (u32 k = blockIdx.x * 256 + threadIdx.x; k < R; k += gridDim.x * 256) {
        u32 v = prev[k];
        if (!v) {
            const u32 l = sym[2 * (size_t)k], r = sym[2 * (size_t)k + 1];
            const u32 a = l < 256u ? 1u : prev[l - 256u], b = r < 256u ? 1u : prev[r - 256u];
            if (a && b) {
                const u32 s = a + b;
                v = s < a ? 0xFFFFFFFFu : s;
                any = true;
            }
        }
        cur[k] = v;
    }
    if (any) *changed = 1u;
}

// a rule whose length the rounds did not reach is higher than the cap: its stream is refused, whether anything names the rule or not
__global__ __launch_bounds__(256) void rbd_height_kernel(const u32* __restrict__ len, u32 R, const u64* __restrict__ rule_off, u32 count,
                                                          int* __restrict__ status) {
    for (u32 k = blockIdx.x * 256 + threadIdx.x; k < R; k += gridDim.x * 256)
        if (!len[k]) status[rbd_stream_of(rule_off, count, k)] = TDC_GPU_ERR_UNSUPPORTED;       // (every writer stores the same value)
}

// One workgroup per stream.  The start symbols of a refused stream become `nothing` (256 + R: the rule behind the last one, of length
// 0).  PLACE (behind the scans): they go to position 0, and the start symbols of an accepted stream move by ooff[k] - base[k], from the
// scan over all start symbols to their text's slot -- a move by 0 unless a stream in front claimed too much.
template <bool PLACE>
__global__ __launch_bounds__(256) void rbd_nothing_kernel(const u64* __restrict__ start_off, const int* __restrict__ status, u32 count, u32 nothing,
                                                           u32* __restrict__ start, u64* __restrict__ pos, const u64* __restrict__ ooff,
                                                           const u64* __restrict__ base) {
    for (u32 k = blockIdx.x; k < count; k += gridDim.x) {
        const u64 a = start_off[k], b = start_off[k + 1];
        if (a == b) continue;
        if (status[k]) {
            for (u64 j = a + threadIdx.x; j < b; j += 256) { start[j] = nothing; if (PLACE) pos[j] = 0ull; }
        } else if (PLACE) {
            const u64 delta = ooff[k] - base[k];
            if (delta) for (u64 j = a + threadIdx.x; j < b; j += 256) pos[j] += delta;
        }
    }
}

// per stream: its text length is the difference of the scan S (m + 1 entries) at its borders; above 2^32 - 2: refused.  ooff[k] = the
// accepted length (scanned next), base[k] = S at its first start symbol; the rules of the accepted streams are counted.
__global__ __launch_bounds__(256) void rbd_sizes_kernel(const u64* __restrict__ S, const u64* __restrict__ start_off, const u64* __restrict__ rule_off,
                                                         u32 count, int* __restrict__ status, u64* __restrict__ ooff, u64* __restrict__ base,
                                                         unsigned long long* __restrict__ rules) {
    const u32 rounds = (count + gridDim.x * 256 - 1) / (gridDim.x * 256);
    for (u32 r = 0; r < rounds; ++r) {                                // (whole waves stay together for the reduction)
        const u32 k = (r * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        unsigned long long nr = 0;
        if (k < count) {
            const u64 a = start_off[k], b = start_off[k + 1];
            u64 tl = S[b] - S[a];
            if (status[k]) tl = 0;
            else if (tl > RPD_TEXT_MAX) { status[k] = TDC_GPU_ERR_TOO_LARGE; tl = 0; }
            else nr = rule_off[k + 1] - rule_off[k];
            ooff[k] = tl; base[k] = S[a];
        }
        nr = wave_reduce_sum(nr);
        if (lane_id() == 0 && nr) atomicAdd(rules, nr);
    }
}

// workgroups of one wave (the walks) or one per stream: as many as there are streams, up to what keeps every CU busy several times over
unsigned rbd_stream_grid(size_t count) { return (unsigned)std::min<size_t>(count, (size_t)1 << 16); }

template <bool WRITE>
void rbd_walk(Ctx& c, int kind, size_t count, const RepairBatchDec& D, u64 R, u32* sym) {
    const unsigned g = rbd_stream_grid(count);
    with_dec_kind(kind, [&](auto K) {
        rbd_walk_kernel<decltype(K)::value, WRITE><<<g, 64, 0, c.stream>>>(D.blob, D.sub, D.s_off, D.s_len, D.bits, (u32)count, D.status, D.rule_off,
                                                                          D.start_off, R, sym);
    });
    LAUNCH_CHECK();
}

}  // namespace

void repair_batch_decode_count(Ctx& c, int kind, size_t count, RepairBatchDec& D) {
    if (count == 0 || count > 0xFFFFFFFEull) throw HipError{hipErrorInvalidValue, "repair batch decode: count out of range", (int)__LINE__};
    rbd_bits_kernel<<<dec_grid(count), 256, 0, c.stream>>>(D.blob, D.sub, D.s_off, D.s_len, (u32)count, D.bits, D.status, D.rule_off, D.start_off);
    LAUNCH_CHECK();
    rbd_walk<false>(c, kind, count, D, 0, nullptr);
    exclusive_sum_u64(c, D.rule_off, D.rule_off, count, D.rule_off + count);
    exclusive_sum_u64(c, D.start_off, D.start_off, count, D.start_off + count);
}

u32 repair_batch_decode_sizes(Ctx& c, int kind, size_t count, RepairBatchDec& D, RepairBatchGrammar& G, u32 cap, u32* d_flags) {
    hipStream_t s = c.stream;
    const size_t items = 2 * G.R + G.M;
    if (items == 0 || items >= 0xFFFFFFFEull - 256) throw HipError{hipErrorInvalidValue, "repair batch decode: token count out of range", (int)__LINE__};
    const u32 nr = (u32)G.R, m = (u32)G.M, nothing = 256u + nr;
    u32* start = G.sym + 2 * G.R;
    rbd_walk<true>(c, kind, count, D, (u64)G.R, G.sym);
    // lengths: at most `cap` rounds, each from the buffer of the round before; the read-back of the flags only ends the loop early
    HIP_TRY(hipMemsetAsync(G.len, 0, (G.R + 1) * 4, s));
    HIP_TRY(hipMemsetAsync(G.len2, 0, (G.R + 1) * 4, s));
    u32* prev = G.len, *cur = G.len2;
    u32 rounds = 0;
    for (bool quiet = nr == 0; !quiet && rounds < cap; ) {
        const u32 b = std::min(RPD_BATCH, cap - rounds);
        HIP_TRY(hipMemsetAsync(d_flags, 0, RPD_BATCH * sizeof(u32), s));
        for (u32 i = 0; i < b; ++i) {
            rbd_len_kernel<<<dec_grid(nr), 256, 0, s>>>(G.sym, nr, prev, cur, d_flags + i);
            LAUNCH_CHECK();
            std::swap(prev, cur);
        }
        u32 h[RPD_BATCH];
        c.read_n(d_flags, h, (size_t)RPD_BATCH);
        for (u32 i = 0; i < b && !quiet; ++i) { ++rounds; quiet = !h[i]; }
    }
    if (prev != G.len) HIP_TRY(hipMemcpyAsync(G.len, prev, (G.R + 1) * 4, hipMemcpyDeviceToDevice, s));   // (the rounds behind a quiet one copy)
    if (nr) {
        rbd_height_kernel<<<dec_grid(nr), 256, 0, s>>>(G.len, nr, D.rule_off, (u32)count, D.status);
        LAUNCH_CHECK();
    }
    // sizes: D.bits has served the walks and holds `base` from here on
    HIP_TRY(hipMemsetAsync(G.pos, 0, (G.M + 1) * 8, s));
    if (m) {
        rbd_nothing_kernel<false><<<rbd_stream_grid(count), 256, 0, s>>>(D.start_off, D.status, (u32)count, nothing, start, G.pos, D.ooff, D.bits);
        LAUNCH_CHECK();
        rpd_adv_kernel<<<dec_grid(m), 256, 0, s>>>(start, m, G.len, G.pos);
        LAUNCH_CHECK();
        exclusive_sum_u64(c, G.pos, G.pos, m, G.pos + m);
    }
    HIP_TRY(hipMemsetAsync(D.rules, 0, sizeof(u64), s));
    rbd_sizes_kernel<<<dec_grid(count), 256, 0, s>>>(G.pos, D.start_off, D.rule_off, (u32)count, D.status, D.ooff, D.bits, (unsigned long long*)D.rules);
    LAUNCH_CHECK();
    exclusive_sum_u64(c, D.ooff, D.ooff, count, D.ooff + count);
    if (m) {
        rbd_nothing_kernel<true><<<rbd_stream_grid(count), 256, 0, s>>>(D.start_off, D.status, (u32)count, nothing, start, G.pos, D.ooff, D.bits);
        LAUNCH_CHECK();
    }
    return rounds;
}

u32 repair_batch_decode_first(Ctx& c, const RepairBatchGrammar& G, u32 cap, u32* d_flags) {
    hipStream_t s = c.stream;
    const u32 nr = (u32)G.R, m = (u32)G.M;
    HIP_TRY(hipMemsetAsync(G.first, 0xFF, (G.R + 1) * 4, s));
    if (!m) return 1;
    rpd_first_start_kernel<<<dec_grid(m), 256, 0, s>>>(G.sym + 2 * G.R, m, G.pos, G.first);
    LAUNCH_CHECK();
    if (!nr) return 1;
    return rpd_rounds(c, d_flags, cap, [&](u32* flag) { rpd_first_kernel<<<dec_grid(nr), 256, 0, s>>>(G.sym, nr, G.len, G.first, flag); });
}

size_t repair_batch_decode_items(Ctx& c, const RepairBatchGrammar& G, size_t n, u8* d_text, u8* cls, u32* fidx, u32* d_cnt) {
    const size_t items = 2 * G.R + G.M;
    rpd_item_kernel<<<dec_grid(items), 256, 0, c.stream>>>(G.sym, G.pos, G.len, G.first, (u32)G.R, (u32)G.M, n, d_text, cls);
    LAUNCH_CHECK();
    select_by_class(c, cls, 1, items, nullptr, fidx, nullptr, nullptr, d_cnt);
    return c.read(d_cnt);
}

void repair_batch_decode_factors(Ctx& c, const RepairBatchGrammar& G, const u32* fidx, size_t zf, u32* fpos, u32* fsrc, u32* flen) {
    if (!zf) return;
    rpd_factor_kernel<<<dec_grid(zf), 256, 0, c.stream>>>(fidx, zf, G.sym, G.pos, G.len, G.first, (u32)G.R, (u32)G.M, fpos, fsrc, flen);
    LAUNCH_CHECK();
}

}  // namespace tdc
