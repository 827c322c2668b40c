// repair_decode.hip -- RePairCompressor::decompress (compressors/RePairCompressor.hpp:287-336) for the coders BitCoder, EliasGammaCoder and
// EliasDeltaCoder, on the device ("Device decoder").  The host loop that specifies it: repair_host.cpp
// (tdc_repair_decode); it also keeps the ascii streams, the streams below the threshold of option dec_parse, the grammars deeper than
// option repair_dec_rounds, and every stream that crosses one of the caps below -- there is no stream the device refuses and the host
// decodes.
//
// The stream: the number of rules R, both sides of rule 0 .. R - 1, the start sequence until the stream ends.  A side or start symbol is a
// token: a flag, then a byte or a rule index.  The host reads R.  Under gamma / delta every field is self-delimiting: next() for every bit
// position, the orbit of the first token's bit, the tokens decoded side by side, segment by segment (stream_parse.hpp); token
// ordinal 2 R is where the start sequence begins.  Under bit the index of a side of rule i takes bits_for(i) bits, constant over
// [2^(w-1), 2^w), and bits_for(R) in the start sequence: a segment reads with ONE width and takes from its token list exactly the tokens
// the stretch still holds (their number is known: twice its rules) -- everything behind was read with the wrong width, the next segment
// starts at the bit where the last taken token ends.  The rules below RPD_HOST_RULES, whose twelve stretches would cost a chain marking
// each for a few thousand tokens, are read by the host and uploaded.
//
// The grammar becomes a factor list: lengths bottom-up (rounds until nothing changes), one 64-bit scan over the start symbols' lengths
// -> their text positions and n, first occurrences top-down (atomicMin, rounds until nothing changes), then every start symbol and
// every side of a rule that occurs is an item -- a literal, nothing (a rule AT its first occurrence: its own sides write it) or the
// factor (q, first[c], len[c]) -- and resolve_and_download finishes.  Work: (rules + start symbols) * depth + n.
//
// Device caps (gamma / delta): an index field of at most 32 value bits, a literal code of at most 8 (the host keeps the low byte of a wider
// one).  A token that crosses one is classed RPD_WIDE and the whole stream goes to the host loop.
#include "repair_passes.hpp"

#include <chrono>
#include <stdio.h>
#include <vector>

namespace tdc {

namespace {

constexpr u32 RPD_HOST_RULES = 4096;                              // bit: the host reads the rules below this index

struct RpdToHost {};                                              // the host loop has the verdict on this stream

// first_bad: (index << 2 | class) of the first token of the segment's list that is not RPD_OK (all ones: none); exit_bit: where the
// last taken token ends
struct RpdScalars { u64 exit_bit; u64 first_bad; };

// The first `keep` tokens of a segment (offsets idx[0 .. keep)) -> sym[j]: the byte, or 256 + the rule.  Token j has ordinal t0 + j;
// below 2 R it is a side of rule (t0 + j) / 2 and names a rule in front of that one, else a start symbol and names a rule below R.
template <int KIND>
__global__ __launch_bounds__(256) void rpd_tokens_kernel(const u32* __restrict__ s32, u64 x_in, const u32* __restrict__ idx, u32 keep, u64 total,
                                                          u32 w, u64 t0, u64 R, u32* __restrict__ sym, RpdScalars* __restrict__ sc) {
    const BitWinG bw{s32, total};
    for (u32 j = blockIdx.x * 256 + threadIdx.x; j < keep; j += gridDim.x * 256) {
        u64 end; u32 rule, val;
        int st = rpd_token<KIND>(bw, x_in + idx[j], total, w, end, rule, val);
        const u64 t = t0 + j, limit = t < 2 * R ? t >> 1 : R;
        if (st == RPD_OK && rule && (u64)val >= limit) st = RPD_BAD;
        sym[j] = st != RPD_OK ? 0u : rule ? 256u + val : val;
        if (st != RPD_OK) atomicMin((unsigned long long*)&sc->first_bad, (unsigned long long)j << 2 | (unsigned)st);
        if (j == keep - 1) sc->exit_bit = end;
    }
}

// ---- the grammar's passes (the others: repair_passes.hpp).  sym[2 k], sym[2 k + 1]: the sides of rule k; sym[2 R + j]: start symbol j
// len[k] = len(l) + len(r), 0 = not known yet, saturating at 2^32 - 1.  The store is one aligned word: a neighbour's value of this round
// or the last one is equally right.
__global__ __launch_bounds__(256) void rpd_len_kernel(const u32* __restrict__ sym, u32 R, u32* len, u32* __restrict__ changed) {
    bool any = false;
    for (u32 k = blockIdx.x * 256 + threadIdx.x; k < R; k += gridDim.x * 256) {
        if (len[k]) continue;
        const u32 l = sym[2 * (size_t)k], r = sym[2 * (size_t)k + 1];
        const u32 a = l < 256u ? 1u : len[l - 256u], b = r < 256u ? 1u : len[r - 256u];
        if (!a || !b) continue;
        const u32 s = a + b;
        len[k] = s < a ? 0xFFFFFFFFu : s;
        any = true;
    }
    if (any) *changed = 1u;
}

// nb <= 32 bits from bit `pos` on; the caller has checked pos + nb <= total
u32 rpd_host_bits(const u8* in, u64 pos, u32 nb) {
    u32 v = 0;
    for (u32 i = 0; i < nb; ++i, ++pos) v = v << 1 | ((in[pos >> 3] >> (7 - (pos & 7))) & 1u);
    return v;
}

// one gamma / delta code of at most 32 value bits; false: not read (the host loop has the verdict)
bool rpd_host_code(const u8* in, u64 total, int kind, u64& pos, u32& val) {
    auto gamma = [&](u32 cap, u32& v) {
        u32 b = 0;
        for (;; ++b) {
            if (pos >= total || b > cap) return false;
            if (rpd_host_bits(in, pos++, 1)) break;
        }
        if (pos + b > total) return false;
        v = rpd_host_bits(in, pos, b);
        pos += b;
        return true;
    };
    if (kind == DEC_GAMMA) return gamma(32, val);
    u32 width;
    if (!gamma(6, width) || width > 32 || pos + width > total) return false;
    val = rpd_host_bits(in, pos, width);
    pos += width;
    return true;
}

struct RpdParse { size_t z = 0; SegCount seg; };

// The segments from bit x0 and token ordinal t_in on (stream_parse.hpp).  sym: zcap entries, the first t_in are filled.  More tokens
// than zcap: DecodeItemOverflow, before anything is written behind zcap.
template <int KIND>
RpdParse rpd_parse(Ctx& c, const u32* s32, u64 total, u64 R, u64 x0, u64 t_in, size_t zcap, u32* sym, const DecTick& tick) {
    hipStream_t s = c.stream;
    RpdScalars* d_sc = (RpdScalars*)c.arena.alloc(sizeof(RpdScalars));
    RpdParse r;
    r.z = (size_t)t_in;
    double rate = 0;                                              // bits per token, as the segment before had them
    u32 w = 0;
    u64 left = ~0ull;                                             // tokens the stretch still holds
    r.seg = parse_segments(c, s32, total, x0, "token list", "corrupt stream: token chain", tick,
        [&](u64, u64& mm) {
            w = 0; left = ~0ull;
            if (KIND == DEC_BIT) {
                const u64 t = r.z;
                if (t >= 2 * R) w = bits_for(R);
                else {
                    const u64 i = t >> 1;
                    w = bits_for(i);
                    const u64 stop = std::min<u64>(i < 2 ? 2 : 1ull << w, R);        // the first rule of the next stretch
                    left = 2 * stop - t;
                    if (rate == 0) rate = 1.0 + std::max(8u, w);
                    const double est = (double)left * rate * (1.0 + 1.0 / 64) + 4096.0;
                    if (est < (double)mm) mm = (u64)est;
                }
            }
            return RpdTok<KIND>{w};
        },
        [&](u64 x_in, const u32* idx, u32 cnt, u32*) {
            const u32 keep = (u32)std::min<u64>(cnt, left);
            if (r.z + keep > zcap) throw DecodeItemOverflow{r.z + keep};
            HIP_TRY(hipMemsetAsync(d_sc, 0xFF, sizeof(RpdScalars), s));
            rpd_tokens_kernel<KIND><<<dec_grid(keep), 256, 0, s>>>(s32, x_in, idx, keep, total, w, r.z, R, sym + r.z, d_sc);
            LAUNCH_CHECK();
            const RpdScalars h = c.read(d_sc);
            tick("token decode");
            if (h.first_bad != ~0ull) {
                if ((h.first_bad & 3) == (u64)RPD_WIDE) throw RpdToHost{};
                throw StreamFormatError{"corrupt stream: malformed or cut-off token, or a rule index out of range"};
            }
            rate = (double)(h.exit_bit - x_in) / (double)keep;
            r.z += keep;
            return h.exit_bit;
        });
    return r;
}


}  // namespace

bool decode_repair(Ctx& c, const u8* stream, size_t len, int kind, Sink& out, size_t* need, RepairDecodeStats* st, size_t* n_out) {
    RepairDecodeStats local;
    if (!st) st = &local;
    *st = RepairDecodeStats();
    *n_out = 0;
    // option dec_parse: 1 = the device for streams of 1 MiB and more, 2 = every stream, 0 = the host loop
    if (!c.dec_parse || (c.dec_parse < 2 && len < ((size_t)1 << 20))) return false;
    const u64 total = payload_bits(stream, len);

    // ---- the host's part: the count field and, under bit, the rules below RPD_HOST_RULES
    u64 x0 = 0, R = 0;
    if (kind == DEC_BIT) {
        if (total < 32) throw StreamFormatError{"corrupt stream: cut-off field"};
        R = rpd_host_bits(stream, 0, 32);
        x0 = 32;
    } else {
        u32 v;
        if (!rpd_host_code(stream, total, kind, x0, v)) return false;
        R = v;
    }
    if (R > 2 * (u64)len) throw StreamFormatError{"corrupt stream: more rules than the stream can hold"};
    std::vector<u32> head;
    if (kind == DEC_BIT) {
        const u32 H = (u32)std::min<u64>(R, RPD_HOST_RULES);
        head.resize(2 * (size_t)H);
        for (u32 t = 0; t < 2 * H; ++t) {
            const u32 i = t >> 1, w = bits_for(i);
            if (x0 >= total) throw StreamFormatError{"corrupt stream: cut-off field"};
            const bool rule = rpd_host_bits(stream, x0, 1) != 0;
            const u32 nb = rule ? w : 8u;
            if (x0 + 1 + nb > total) throw StreamFormatError{"corrupt stream: cut-off field"};
            const u32 v = rpd_host_bits(stream, x0 + 1, nb);
            if (!rule) head[t] = v;
            else {
                if (v >= i) throw StreamFormatError{"corrupt stream: rule index out of range"};
                head[t] = 256u + v;
            }
            x0 += 1 + nb;
        }
    }

    hipStream_t s = c.stream;
    const DecTick tick = dec_ticker(c, "repair decode");
    using Clock = std::chrono::steady_clock;
    auto lap = [&](Clock::time_point& t) {                        // (synchronises) ms since t, which moves on
        HIP_TRY(hipStreamSynchronize(s));
        const Clock::time_point now = Clock::now();
        const float ms = std::chrono::duration<float, std::milli>(now - t).count();
        t = now;
        return ms;
    };
    Clock::time_point t_lap = Clock::now();
    const u64 seg_bits = c.dec_seg ? (u64)c.dec_seg : (u64)DEC_SEG;
    const size_t seg = (size_t)std::min<u64>(seg_bits, total);
    const size_t slack = (size_t)16 << 20;
    // Tokens per stream bit behind the host's part.  bit: a literal takes 9 bits, a side of a rule from RPD_HOST_RULES on 14 and more, a
    // start symbol 1 + bits_for(R) >= 2.  gamma / delta: an encoder's shortest token is a literal below 2 in 4 bits, the shortest the
    // decoder reads is "1" "1", the rule 0, in 2.  The array is sized for the first figure and the parse starts over with room for the
    // second where a stream needs it.
    const u64 rem = total - x0;
    u64 zcap = head.size() + (kind == DEC_BIT ? rem / 8 + 4096 : rem / 4 + 2);
    const u64 zmax = head.size() + rem / 2 + 2;
    RpdParse P;
    u32* sym = nullptr;
    try {
        for (;;) {
            if (zcap > 0xFFFFFFFEull) return false;               // (item indices are 32-bit: the host loop has the verdict)
            // + 24 bytes per stream byte: room for the grammar's passes and the text pass of a stream that does not expand much -- with the
            // segment's scratch, free again by then; where it does not fit, the grammar moves (regrow_arena)
            c.ensure_arena(len + 64 + (size_t)zcap * 4 + 1024 + seg * 13 + 64 + len * 24 + 2 * slack);
            void* d_stream = c.arena.get<u8>(len + 64);
            t_lap = Clock::now();
            if (len) HIP_TRY(hipMemcpyAsync(d_stream, stream, len, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemsetAsync((u8*)d_stream + len, 0, 64, s));
            sym = c.arena.get<u32>(zcap);
            if (!head.empty()) HIP_TRY(hipMemcpyAsync(sym, head.data(), head.size() * 4, hipMemcpyHostToDevice, s));
            st->ms_h2d = lap(t_lap);
            tick("upload");
            try {
                P = with_dec_kind(kind, [&](auto K) { return rpd_parse<decltype(K)::value>(c, (const u32*)d_stream, total, R, x0, head.size(), (size_t)zcap, sym, tick); });
                break;
            }
            catch (const DecodeItemOverflow&) {
                if (zcap >= zmax) throw HipError{hipErrorUnknown, "repair decode: more tokens than the stream can hold", (int)__LINE__};
                zcap = zmax;
            }
        }
    } catch (const RpdToHost&) { return false; }
    if (P.z < 2 * R) throw StreamFormatError{"corrupt stream: cut-off field"};         // the stream ends inside the rules
    const u32 nr = (u32)R, m = (u32)(P.z - 2 * R);
    const size_t items = P.z;

    // ---- lengths, text positions and n, first occurrences
    const u32 cap = (u32)std::min<long>(std::max<long>(c.repair_dec_rounds, 1), 1l << 24);
    {
        const size_t pass = items * 8 + 8192 + slack;             // lengths, first occurrences, positions, and the scan's scratch
        if (c.arena.size < c.arena.mark() + pass) {               // (a stream of two-bit tokens)
            void* a = sym;
            regrow_arena(c, items * 4 + 1024 + pass + items * 17 + slack, {{&a, items * 4}});
            sym = (u32*)a;
        }
    }
    u32* d_flags = c.arena.get<u32>(RPD_BATCH);
    u64* d_n = c.arena.get<u64>(1);
    u32* rlen = c.arena.get<u32>((size_t)nr + 1), *first = c.arena.get<u32>((size_t)nr + 1);
    u64* pos = c.arena.get<u64>((size_t)m + 1);
    HIP_TRY(hipMemsetAsync(rlen, 0, ((size_t)nr + 1) * 4, s));
    HIP_TRY(hipMemsetAsync(first, 0xFF, ((size_t)nr + 1) * 4, s));
    if (nr) {
        st->len_rounds = rpd_rounds(c, d_flags, cap, [&](u32* flag) { rpd_len_kernel<<<dec_grid(nr), 256, 0, s>>>(sym, nr, rlen, flag); });
        if (!st->len_rounds) return false;                         // deeper than option repair_dec_rounds: the host loop
    }
    tick("lengths");
    u64 n64 = 0;
    if (m) {
        rpd_adv_kernel<<<dec_grid(m), 256, 0, s>>>(sym + 2 * (size_t)nr, m, rlen, pos);
        LAUNCH_CHECK();
        exclusive_sum_u64(c, pos, pos, m, d_n);
        n64 = c.read(d_n);
    }
    tick("text positions");
    if (n64 > RPD_TEXT_MAX) throw DecodeTooLarge{n64};
    const size_t n = (size_t)n64;
    if (need) *need = n;
    *n_out = n;
    if (out.into && n > out.cap) throw HipError{hipErrorOutOfMemory, "repair decode: the caller's buffer is too small for the text", (int)__LINE__};
    st->rules = R; st->nstart = m; st->segments = P.seg.segments;
    if (c.dec_log)
        fprintf(stderr, "repair decode: %u segments, next() evaluated for %llu bit positions (%.4f of the stream's %llu), %llu rules, %u start symbols\n",
                P.seg.segments, (unsigned long long)P.seg.evaluated, (double)P.seg.evaluated / (double)std::max<u64>(total, 1), (unsigned long long)total,
                (unsigned long long)R, m);
    if (n == 0) { st->dec.device_parse = 1; decode_dest(out, 0); return true; }
    if (nr) {
        rpd_first_start_kernel<<<dec_grid(m), 256, 0, s>>>(sym + 2 * (size_t)nr, m, pos, first);
        LAUNCH_CHECK();
        st->first_rounds = rpd_rounds(c, d_flags, cap, [&](u32* flag) { rpd_first_kernel<<<dec_grid(nr), 256, 0, s>>>(sym, nr, rlen, first, flag); });
        if (!st->first_rounds) return false;
    }
    tick("first occurrences");
    st->ms_grammar = lap(t_lap);

    // ---- the items: literals to the text, the factor list to the shared reference resolver
    u32* d_cnt = c.arena.get<u32>(2);
    {
        const size_t text_pass = items * 17 + n * 5 + n / 8 + 2 * slack;     // class byte, index and 12 bytes per factor, then the resolver's
        if (c.arena.size < c.arena.mark() + text_pass) {
            void* a = sym; void* b = rlen; void* f = first; void* p = pos;
            const size_t live = items * 4 + ((size_t)nr + 1) * 8 + ((size_t)m + 1) * 8 + 4 * 320;
            regrow_arena(c, live + text_pass, {{&a, items * 4}, {&b, ((size_t)nr + 1) * 4}, {&f, ((size_t)nr + 1) * 4}, {&p, ((size_t)m + 1) * 8}});
            sym = (u32*)a; rlen = (u32*)b; first = (u32*)f; pos = (u64*)p;
            d_cnt = c.arena.get<u32>(2);
        }
    }
    u8* cls = c.arena.get<u8>(items);
    u32* fidx = c.arena.get<u32>(items);
    u8* d_text = c.arena.get<u8>(n + 64);
    rpd_item_kernel<<<dec_grid(items), 256, 0, s>>>(sym, pos, rlen, first, nr, m, n, d_text, cls);
    LAUNCH_CHECK();
    select_by_class(c, cls, 1, items, nullptr, fidx, nullptr, nullptr, d_cnt);
    const size_t zf = c.read(d_cnt);
    st->dec.factors = zf;
    tick("items + literals");
    u32* fpos = c.arena.get<u32>(zf + 1), *fsrc = c.arena.get<u32>(zf + 1), *flen = c.arena.get<u32>(zf + 1);
    if (zf) {
        rpd_factor_kernel<<<dec_grid(zf), 256, 0, s>>>(fidx, zf, sym, pos, rlen, first, nr, m, fpos, fsrc, flen);
        LAUNCH_CHECK();
    }
    tick("factor list");
    u32* d_ref = c.arena.get<u32>(n);
    st->dec.device_parse = 1;
    if (zf == 0) {                                                 // literals only: the text is complete
        HIP_TRY(hipMemcpyAsync(decode_dest(out, n), d_text, n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    } else resolve_and_download(c, n, d_text, d_ref, fpos, fsrc, flen, zf, d_cnt, out, &st->dec);
    st->dec.device_parse = 1;
    st->ms_text = lap(t_lap);
    tick("references + download");
    if (c.dec_log)
        fprintf(stderr, "repair decode: %u length rounds, %u placement rounds, %zu factors, %u resolver rounds\n", st->len_rounds, st->first_rounds,
                zf, st->dec.rounds);
    return true;
}

}  // namespace tdc
