// api_chain.hip -- C ABI (include/tdc_gpu.h): bwt (BWTCompressor.hpp, ds/bwt.hpp; bwt.hip), the byte stages rle, mtf, encode(huff) and
// encode(sle) (bytestages.hip, encode.hip, bytestages_decode.hip) and chains of them (DESIGN.md sections 5.3 and 5.6), with the host
// decoders of the byte stages.
#include "api.hpp"
#include "bytestages.hpp"
#include "bytestages_batch.hpp"
#include "../host/tdc_coders.hpp"

#include <vector>
#include <chrono>
#include <functional>

using namespace tdc;

namespace {
// Upload + suffix array + gather: the transform of text[0..n) in a device buffer -- d_out (n + 64 bytes) if given, else the place of the
// ranks in the arena the caller reserved.  host_dst (nullable) is where bwt_finish() will download it: bwt_gather may send it there
// chunk by chunk already (`sent`).
struct BwtRun { u8* d_out; bool sent; int e0, e4; };
BwtRun bwt_device(Ctx& c, const uint8_t* text, size_t n, u8* d_out, u8* host_dst, tdc_gpu_stats* stats, Events& ev) {
    const int e0 = ev.tick();
    TextUpload up(c);
    const u8* d_text = up.send(text, n);
    const int e1 = ev.tick();
    validate_device_text(c, d_text, n);
    // the suffix array as tdc_gpu_suffix_array builds it; with the sink of the wide path the inverse suffix array is not materialised
    u32* d_sa = c.arena.get<u32>(n);
    u32* d_isa = c.arena.get<u32>(n);
    SAStats ss;
    SAExtra ex;
    ex.lcp8 = c.arena.get<u8>(n + 64);
    const int e2 = ev.tick();
    build_suffix_array(c, d_text, n, d_sa, d_isa, &ss, &ex);
    const int e3 = ev.tick();
    if (!d_out) d_out = (u8*)d_isa;                          // (the ranks are not needed: the transform takes their place)
    const bool sent = bwt_gather(c, d_text, d_sa, n, d_out, host_dst);
    const int e4 = ev.tick();
    if (stats) {
        stats->n = n; stats->out_len = n;
        sa_stats(stats, ss, &ex);
        stats->arena_bytes = c.arena.high;
        // ms_encode: the gather (with a page-locked destination the downloads of its chunks run inside it, and ms_d2h is what is left: nothing)
        ev.span(&stats->ms_h2d, e0, e1); ev.span(&stats->ms_sa, e2, e3); ev.span(&stats->ms_encode, e3, e4);
    }
    return BwtRun{d_out, sent, e0, e4};
}
// the download of what bwt_gather has not sent, and the end of the call's event frame
void bwt_finish(Ctx& c, const BwtRun& r, size_t n, u8* host_dst, tdc_gpu_stats* stats, Events& ev) {
    if (!r.sent && host_dst) HIP_TRY(hipMemcpyAsync(host_dst, r.d_out, n, hipMemcpyDeviceToHost, c.stream));
    const int e5 = ev.tick();
    if (stats) { ev.span(&stats->ms_d2h, r.e4, e5); ev.span(&stats->ms_total, r.e0, e5); }
    ev.finish();
}

void bwt_compress_host(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, Sink s, tdc_gpu_stats* stats) {
    sink_check(s, "out/out_len is NULL");
    check_host_text(text, n);
    *s.out_len = n;
    sink_fit(s, n);
    Ctx& c = ctx->c;
    if (stats) memset(stats, 0, sizeof(*stats));
    reserve_arena(c, arena_need(c, n));
    Events ev(c);
    u8* dst = sink_host(s, n);
    bwt_finish(c, bwt_device(c, text, n, nullptr, dst, stats, ev), n, dst, stats, ev);
    sink_commit(s, n);
}

void bwt_decompress_common(tdc_gpu_ctx* ctx, const uint8_t* bwt, size_t len, uint32_t sample, uint32_t max_steps, Sink& s, uint32_t* host_lf,
                           BwtInvStats* bs) {
    if (!bwt && len) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
    sink_check(s, "NULL argument");
    if (len >= 0x7FFFFFFFull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "bwt: the buffer must be shorter than 2^31 - 1 bytes (32-bit len_t)"};
    if (len > 1) sink_fit(s, len);
    const size_t n = run_decoder(s, "bwt: buffer too large", nullptr, [&] { return bwt_inverse(ctx->c, bwt, len, sample, max_steps, s, host_lf, bs); });
    sink_commit(s, n);
}

void bwt_decompress_entry(tdc_gpu_ctx* ctx, const uint8_t* bwt, size_t len, Sink s, uint32_t* rounds) {
    BwtInvStats bs;
    bwt_decompress_common(ctx, bwt, len, 0, 0, s, nullptr, rounds ? &bs : nullptr);
    if (rounds) *rounds = bs.rounds;
}
}  // namespace

extern "C" {

int tdc_gpu_bwt_compress(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint8_t** out, size_t* out_len, tdc_gpu_stats* stats) {
    return guarded(ctx, [&] { bwt_compress_host(ctx, text, n, sink_malloc(out, out_len), stats); });
}

int tdc_gpu_bwt_compress_into(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint8_t* out, size_t out_cap, size_t* out_len,
                              tdc_gpu_stats* stats) {
    return guarded(ctx, [&] { bwt_compress_host(ctx, text, n, sink_into(out, out_cap, out_len), stats); });
}

int tdc_gpu_bwt_decompress(tdc_gpu_ctx* ctx, const uint8_t* bwt, size_t len, uint8_t** out, size_t* out_len, uint32_t* rounds) {
    return guarded(ctx, [&] { bwt_decompress_entry(ctx, bwt, len, sink_malloc(out, out_len, "NULL argument"), rounds); });
}

int tdc_gpu_bwt_decompress_into(tdc_gpu_ctx* ctx, const uint8_t* bwt, size_t len, uint8_t* out, size_t out_cap, size_t* out_len,
                                uint32_t* rounds) {
    return guarded(ctx, [&] { bwt_decompress_entry(ctx, bwt, len, sink_into(out, out_cap, out_len), rounds); });
}

int tdc_gpu_bwt_inverse_stage(tdc_gpu_ctx* ctx, const uint8_t* bwt, size_t len, uint32_t sample, uint32_t max_steps, uint8_t* out,
                              uint32_t* lf, uint64_t* heads, uint32_t* launches) {
    return guarded(ctx, [&] {
        if (!out && len > 1) throw ArgError{TDC_GPU_ERR_ARG, "out is NULL"};
        size_t n = 0;
        uint8_t nothing;                                      // (`out` may be NULL for inputs that decode to nothing)
        Sink s = sink_into(out ? out : &nothing, len, &n);
        BwtInvStats bs;
        bwt_decompress_common(ctx, bwt, len, sample, max_steps, s, lf, &bs);
        if (heads) *heads = bs.heads;
        if (launches) *launches = bs.launches;
    });
}

}  // extern "C"

// ---- rle, mtf, encode(huff) and chains -------------------------------------------------------------------------------------------------
namespace {
bool pipeline_valid(const tdc_gpu_stage* st, int k) {
    if (!st || k < 1 || k > TDC_GPU_PIPELINE_MAX_STAGES) return false;
    for (int i = 0; i < k; ++i) {
        if (st[i].kind < TDC_GPU_STAGE_BWT || st[i].kind > TDC_GPU_STAGE_SLE) return false;
        if (st[i].kind == TDC_GPU_STAGE_BWT && i) return false;
        if (st[i].kind == TDC_GPU_STAGE_RLE && st[i].param > ((u64)1 << 62)) return false;
        if (st[i].kind == TDC_GPU_STAGE_SLE && st[i].param > 7) return false;               // kmer: 0 = 3 (SLECoder.hpp:12,38)
    }
    return true;
}
// worst-case output of one stage on n bytes
u64 stage_worst(const tdc_gpu_stage& st, u64 n) {
    return st.kind == TDC_GPU_STAGE_RLE ? rle_bound(n, st.param) : st.kind == TDC_GPU_STAGE_HUFF ? huff_literals_bound(n) :
           st.kind == TDC_GPU_STAGE_SLE ? sle_literals_bound(n) : n;
}
// the scratch it takes besides
u64 stage_scratch(const tdc_gpu_stage& st, u64 n) {
    return st.kind == TDC_GPU_STAGE_SLE ? sle_literals_scratch_bound(n, st.param ? (u32)st.param : 3u) : stage_scratch_bound(n);
}
// what the arena holds for it (a stage that would write more than STAGE_MAX_BYTES fails before it writes)
u64 stage_bound(const tdc_gpu_stage& st, u64 n) { return std::min<u64>(stage_worst(st, n), STAGE_MAX_BYTES); }
const char* stage_name(int kind) {
    return kind == TDC_GPU_STAGE_BWT ? "bwt" : kind == TDC_GPU_STAGE_RLE ? "rle" : kind == TDC_GPU_STAGE_MTF ? "mtf" : kind == TDC_GPU_STAGE_SLE ? "encode(sle)" : "encode(huff)";
}


void pipeline_compress_host(tdc_gpu_ctx* ctx, const tdc_gpu_stage* stages, int k, const uint8_t* in, size_t n, Sink s, tdc_gpu_stats* stats) {
    sink_check(s, "out/out_len is NULL");
    if (!in && n) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
    if (stages && k >= 1 && k <= TDC_GPU_PIPELINE_MAX_STAGES)
        for (int i = 1; i < k; ++i) if (stages[i].kind == TDC_GPU_STAGE_BWT) throw ArgError{TDC_GPU_ERR_NO_SENTINEL, "pipeline: bwt must be the first stage (its input is the escaped, 0-terminated view)"};
    if (!pipeline_valid(stages, k)) throw ArgError{TDC_GPU_ERR_ARG, "pipeline: 1 .. 8 stages of kind bwt (first only), rle (offset <= 2^62), mtf, encode(huff) or encode(sle) (kmer 1 .. 7)"};
    if (n > STAGE_MAX_BYTES) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "pipeline: the input must not be longer than 2^32 - 2 bytes"};
    const bool lead_bwt = stages[0].kind == TDC_GPU_STAGE_BWT;
    Ctx& c = ctx->c;
    const bool plog = c.pipe_log != 0;
    const auto t_start = std::chrono::steady_clock::now();
    auto t_last = t_start;
    float ms[TDC_GPU_PIPELINE_MAX_STAGES] = {0};
    auto tick = [&](int i) {                                  // (synchronises: only with the diagnostic option)
        if (!plog) return;
        HIP_TRY(hipStreamSynchronize(c.stream));
        const auto now = std::chrono::steady_clock::now();
        ms[i] = std::chrono::duration<float, std::milli>(now - t_last).count();
        t_last = now;
    };
    // the arena for the whole call: what the suffix array needs, or every intermediate at its worst case with the stages' scratch
    u64 need = 0, len = n;
    for (int i = lead_bwt ? 1 : 0; i < k; ++i) { need += stage_scratch(stages[i], len) + stage_bound(stages[i], len) + 4096; len = stage_bound(stages[i], len); }
    need += n + 4096;
    if (lead_bwt) {
        check_text_args(in, n);                               // (before the arena is sized from n)
        need = std::max<u64>(need, arena_need(c, n) + n + 4096);
    }
    if (stats) memset(stats, 0, sizeof(*stats));
    tdc_gpu_stats local = {};
    tdc_gpu_stats* st = stats ? stats : &local;
    reserve_arena(c, need);
    StageOut cur;
    cur.d = c.arena.get<u8>(n + 64);
    cur.len = n;
    const size_t base_mark = c.arena.mark();
    u64 lens[TDC_GPU_PIPELINE_MAX_STAGES] = {0};
    if (!lead_bwt && n) HIP_TRY(hipMemcpyAsync(cur.d, in, n, hipMemcpyHostToDevice, c.stream));
    for (int i = 0; i < k; ++i) {
        try {
            switch (stages[i].kind) {
                case TDC_GPU_STAGE_BWT: {
                    check_host_text(in, n);
                    Events ev(c);
                    bwt_device(c, in, n, cur.d, nullptr, st, ev);
                    ev.finish();
                    c.arena.release(base_mark);               // the suffix array's scratch goes back before the byte stages take theirs
                    break;
                }
                case TDC_GPU_STAGE_RLE: cur = rle_encode_device(c, cur.d, cur.len, stages[i].param); break;
                case TDC_GPU_STAGE_MTF: cur = mtf_encode_device(c, cur.d, cur.len); break;
                case TDC_GPU_STAGE_SLE: cur = sle_literals_device(c, cur.d, cur.len, (u32)stages[i].param); break;
                default: cur = huff_literals_device(c, cur.d, cur.len); break;
            }
        } catch (const StageTooLarge&) {
            throw ArgError{TDC_GPU_ERR_TOO_LARGE, "pipeline: a stage's output would pass 2^32 - 2 bytes"};
        }
        lens[i] = cur.len;
        tick(i);
    }
    const size_t out_len = (size_t)cur.len;
    *s.out_len = out_len;
    sink_fit(s, out_len);
    u8* dst = sink_host(s, out_len);
    if (out_len) {
        c.wait_for(c.copy_stream, c.stream);
        HIP_TRY(hipMemcpyAsync(dst, cur.d, out_len, hipMemcpyDeviceToHost, c.copy_stream));
        HIP_TRY(hipStreamSynchronize(c.copy_stream));
    }
    HIP_TRY(hipStreamSynchronize(c.stream));
    st->n = n; st->out_len = out_len; st->pipe_stages = (uint32_t)k;
    for (int i = 0; i < k; ++i) { st->pipe_len[i] = lens[i]; st->pipe_ms[i] = ms[i]; }
    st->arena_bytes = c.arena.high;
    st->ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    if (plog) {
        u64 prev = n;
        for (int i = 0; i < k; ++i) {
            fprintf(stderr, "pipe:     %-14s %12llu -> %12llu bytes %9.2f ms\n", stage_name(stages[i].kind), (unsigned long long)prev, (unsigned long long)lens[i], ms[i]);
            prev = lens[i];
        }
        fprintf(stderr, "pipe:     total incl. download %9.2f ms\n", st->ms_total);
    }
    sink_commit(s, out_len);
}


// ---- chains over a batch of texts (bytestages_batch.hip, bwt_batch.hip; DESIGN.md section 5.3 "Batches") ---------------------------------
// the refusals decided from the arguments alone, in the order include/tdc_gpu.h documents
void pipeline_batch_check(const tdc_gpu_stage* stages, int k, const uint8_t* in, const uint64_t* in_off, size_t count, const uint64_t* out_off,
                          const uint64_t* out_len, const int32_t* status) {
    if (!in_off || !out_off || !out_len || !status) throw ArgError{TDC_GPU_ERR_ARG, "pipeline batch: NULL argument"};
    if (in_off[0] != 0) throw ArgError{TDC_GPU_ERR_ARG, "pipeline batch: in_off[0] must be 0"};
    for (size_t t = 0; t < count; ++t)
        if (in_off[t + 1] < in_off[t]) throw ArgError{TDC_GPU_ERR_ARG, "pipeline batch: in_off must not decrease"};
    if (!in && in_off[count]) throw ArgError{TDC_GPU_ERR_ARG, "pipeline batch: NULL argument"};
    if (stages && k >= 1 && k <= TDC_GPU_PIPELINE_MAX_STAGES)
        for (int i = 1; i < k; ++i) if (stages[i].kind == TDC_GPU_STAGE_BWT) throw ArgError{TDC_GPU_ERR_NO_SENTINEL, "pipeline: bwt must be the first stage (its input is the escaped, 0-terminated view)"};
    if (!pipeline_valid(stages, k)) throw ArgError{TDC_GPU_ERR_ARG, "pipeline: 1 .. 8 stages of kind bwt (first only), rle (offset <= 2^62), mtf, encode(huff) or encode(sle) (kmer 1 .. 7)"};
    for (int i = 0; i < k; ++i) if (stages[i].kind == TDC_GPU_STAGE_SLE) throw ArgError{TDC_GPU_ERR_UNSUPPORTED, "pipeline batch: encode(sle) has no batch form"};
    if (in_off[count] > STAGE_MAX_BYTES || count > 0x7FFFFFFFull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "pipeline batch: too many bytes or texts in one call"};
}

void pipeline_compress_batch_host(tdc_gpu_ctx* ctx, const tdc_gpu_stage* stages, int k, const uint8_t* in, const uint64_t* in_off, size_t count,
                                  uint8_t* out, size_t out_cap, uint64_t* out_off, uint64_t* out_len, int32_t* status, tdc_gpu_stats* stats) {
    Ctx& c = ctx->c;
    if (stats) memset(stats, 0, sizeof(*stats));
    out_off[0] = 0;
    if (count == 0) return;
    const size_t n = (size_t)in_off[count];
    const bool lead_bwt = stages[0].kind == TDC_GPU_STAGE_BWT;
    const int first = lead_bwt ? 1 : 0;
    const bool plog = c.pipe_log != 0;
    // the arena for the whole call, reserved before any work: the padded input, the offsets and verdicts, then the larger of what the
    // bwt batch takes and of every intermediate at its worst case with its stage's scratch, and the output image
    u64 need = n + 16 * (u64)count + 64 * (u64)count + 8192, byte_stages = 0, len = std::min<u64>(n, (u64)count * BATCH_TEXT_CAP);
    for (int i = first; i < k; ++i) {
        const u64 o = stage_bound(stages[i], len) + (stages[i].kind == TDC_GPU_STAGE_HUFF ? 1024 * (u64)count : 0);    // (a header per text)
        byte_stages += batch_stage_scratch(len, count) + o + 16 * (u64)count + 4096;
        len = std::min<u64>(o, STAGE_MAX_BYTES);
    }
    byte_stages += len + 48 * (u64)count + (n + 4096) + batch_stage_scratch(0, count);    // the output image, its offsets; the plain input on its way in
    need += std::max<u64>(byte_stages, lead_bwt ? bwtb_forward_arena(n, count) + 4096 : 0);
    reserve_arena(c, need);
    const auto t_start = std::chrono::steady_clock::now();
    auto t_last = t_start;
    auto since = [&](std::chrono::steady_clock::time_point a) { return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - a).count(); };
    float ms[TDC_GPU_PIPELINE_MAX_STAGES] = {0};
    auto tick = [&](int i) {                                  // (synchronises: only with the diagnostic option)
        if (!plog) return;
        HIP_TRY(hipStreamSynchronize(c.stream));
        ms[i] = since(t_last);
        t_last = std::chrono::steady_clock::now();
    };
    hipStream_t s = c.stream;
    tdc_gpu_stats local = {};
    tdc_gpu_stats* st = stats ? stats : &local;
    // layout 0: the accepted texts at multiples of 16, a refused text with length 0
    BatchLay cur;
    cur.off = c.arena.get<u64>(count + 1);
    cur.len = c.arena.get<u64>(count);
    u64* d_inoff = c.arena.get<u64>(count + 1);
    int* d_status = c.arena.get<int>(count);
    std::vector<u64> h_off(count + 1), h_len(count);
    BwtbKeep keep;
    if (lead_bwt) {
        // (the padded buffer is taken first: the bwt batch's scratch goes back before the byte stages take theirs)
        u64 pad = 0;
        for (size_t t = 0; t < count; ++t) pad += align_up((size_t)std::min<u64>(in_off[t + 1] - in_off[t], BATCH_TEXT_CAP), 16);
        cur.d = c.arena.get<u8>(pad + 64);
    } else {
        for (size_t t = 0; t < count; ++t) status[t] = in_off[t + 1] - in_off[t] > BATCH_TEXT_CAP ? TDC_GPU_ERR_TOO_LARGE : TDC_GPU_OK;
    }
    const size_t mark = lead_bwt ? c.arena.mark() : 0;
    if (lead_bwt) bwtb_forward(ctx, in, in_off, count, nullptr, 0, false, nullptr, status, st, &keep);
    for (size_t t = 0; t < count; ++t) {
        h_len[t] = status[t] == 0 ? in_off[t + 1] - in_off[t] : 0;
        h_off[t] = cur.padded;
        cur.padded += align_up((size_t)h_len[t], 16);
        cur.total += h_len[t];
    }
    h_off[count] = cur.padded;
    if (!lead_bwt) cur.d = c.arena.get<u8>(cur.padded + 64);
    const size_t mark2 = lead_bwt ? mark : c.arena.mark();
    HIP_TRY(hipMemcpyAsync(cur.off, h_off.data(), (count + 1) * sizeof(u64), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(cur.len, h_len.data(), count * sizeof(u64), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_inoff, in_off, (count + 1) * sizeof(u64), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_status, status, count * sizeof(int), hipMemcpyHostToDevice, s));
    const u8* d_plain = lead_bwt ? keep.d_out : upload_plain(c, in, n);
    if (cur.total) batch_relayout(c, d_plain, d_inoff, cur.d, cur.off, cur.len, count);
    HIP_TRY(hipStreamSynchronize(s));                         // (the host arrays above; the plain input goes back to the arena)
    c.arena.release(mark2);
    if (!lead_bwt) st->ms_h2d = since(t_start);
    u64 lens[TDC_GPU_PIPELINE_MAX_STAGES] = {0};
    if (lead_bwt) { lens[0] = cur.total; tick(0); }
    // the sizes, as soon as the last stage knows them: the caller's arrays are complete before its buffer is looked at
    u64 used = 0;
    const BatchSizesHook sizes = [&](const u64* d_len) {
        std::vector<u64> hl(count);
        c.read_n(d_len, hl.data(), count);
        for (size_t t = 0; t < count; ++t) {
            out_off[t] = used;
            out_len[t] = status[t] == 0 ? hl[t] : 0;
            used += align_up((size_t)out_len[t], 8);
        }
        out_off[count] = used;
        if (!out || out_cap < used) throw ArgError{TDC_GPU_ERR_OOM, "pipeline batch: output buffer too small (out_off[count] holds the required size)"};
    };
    const BatchSizesHook none;
    BatchHuffInfo hinfo;
    int huff_stage = -1;
    if (first == k) sizes(cur.len);
    for (int i = first; i < k; ++i) {
        const BatchSizesHook& hook = i + 1 == k ? sizes : none;
        try {
            switch (stages[i].kind) {
                case TDC_GPU_STAGE_RLE: cur = rle_encode_batch(c, cur, count, stages[i].param, hook); break;
                case TDC_GPU_STAGE_MTF: cur = mtf_encode_batch(c, cur, count, hook); break;
                default: cur = huff_literals_batch(c, cur, count, d_status, status, (u32)c.pipe_batch_threads, &hinfo, hook); huff_stage = i; break;
            }
        } catch (const StageTooLarge&) {
            throw ArgError{TDC_GPU_ERR_TOO_LARGE, "pipeline batch: a stage's output would pass 2^32 - 2 bytes over the batch"};
        }
        lens[i] = cur.total;
        tick(i);
    }
    // the streams back to back at multiples of 8, one download
    const auto t_down = std::chrono::steady_clock::now();
    if (used) {
        std::vector<u64> h_ooff(out_off, out_off + count + 1);
        u64* d_ooff = c.arena.get<u64>(count + 1);
        u8* d_img = c.arena.get<u8>(used + 64);
        HIP_TRY(hipMemcpyAsync(d_ooff, h_ooff.data(), (count + 1) * sizeof(u64), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(d_img, 0, used, s));
        batch_relayout(c, cur.d, cur.off, d_img, d_ooff, cur.len, count);
        HIP_TRY(hipMemcpyAsync(out, d_img, used, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    st->ms_d2h = since(t_down);
    st->n = n; st->out_len = used; st->pipe_stages = (uint32_t)k;
    for (int i = 0; i < k; ++i) { st->pipe_len[i] = lens[i]; st->pipe_ms[i] = ms[i]; }
    st->arena_bytes = c.arena.high;
    st->ms_total = since(t_start);
    if (plog) {
        u64 prev = n;
        for (int i = 0; i < k; ++i) {
            fprintf(stderr, "pipe:     %-14s %12llu -> %12llu bytes %9.2f ms\n", stage_name(stages[i].kind), (unsigned long long)prev, (unsigned long long)lens[i], ms[i]);
            if (i == huff_stage) fprintf(stderr, "pipe:     huff tables    %12llu tables on %u host threads %9.2f ms (inside encode(huff))\n", (unsigned long long)count, hinfo.threads, hinfo.ms_tables);
            prev = lens[i];
        }
        fprintf(stderr, "pipe:     batch of %llu texts, total incl. download %9.2f ms\n", (unsigned long long)count, st->ms_total);
    }
}


// host decoder of one stage: `in` -> `out` (at most STAGE_MAX_BYTES)
void host_stage_decode(const tdc_gpu_stage& st, const std::vector<uint8_t>& in, std::vector<uint8_t>& out) {
    auto run = [&](uint8_t* o, size_t cap) {
        tdc_amd::ByteSink sink(o, cap);
        if (st.kind == TDC_GPU_STAGE_RLE) tdc_amd::rle_decode(in.data(), in.size(), st.param, sink);
        else if (st.kind == TDC_GPU_STAGE_MTF) tdc_amd::mtf_decode(in.data(), in.size(), sink);
        else if (st.kind == TDC_GPU_STAGE_SLE) tdc_amd::sle_decode_literals(in.data(), in.size(), st.param ? (unsigned)st.param : 3u, sink);
        else tdc_amd::huff_decode_literals(in.data(), in.size(), sink);
        return sink.n;
    };
    try {
        if (st.kind == TDC_GPU_STAGE_MTF) out.resize(in.size());
        else {
            const u64 need = run(nullptr, 0);
            if (need > STAGE_MAX_BYTES) throw ArgError{TDC_GPU_ERR_ARG, "pipeline: a stage decodes to more than 2^32 - 2 bytes"};
            out.resize((size_t)need);
        }
        run(out.data(), out.size());
    } catch (const std::runtime_error&) {
        throw ArgError{TDC_GPU_ERR_ARG, "pipeline: malformed stream"};
    } catch (const std::length_error&) {                          // (sle_decode_literals)
        throw ArgError{TDC_GPU_ERR_ARG, "pipeline: a stage decodes to more than 2^32 - 2 bytes"};
    }
}


// what a call reports (tdc_gpu_pipeline_decompress_stats): lens[i] = the length behind stage i's encoder = in front of its decoder, as in
// the stats of the compress call; dev: bit i = stage i ran on the device
struct PipeReport { u64 lens[TDC_GPU_PIPELINE_MAX_STAGES] = {0}; float ms[TDC_GPU_PIPELINE_MAX_STAGES] = {0}; uint32_t dev = 0; };

void pipe_line(bool plog, int kind, u64 out, u64 in, double ms, bool dev) {
    if (plog) fprintf(stderr, "pipe:     %-14s %12llu <- %12llu bytes %9.2f ms (%s)\n", stage_name(kind), (unsigned long long)out, (unsigned long long)in, ms, dev ? "device" : "host");
}

// the inverse of a leading bwt from a host buffer or (on_device) from the arena
void bwt_invert_into(tdc_gpu_ctx* ctx, const uint8_t* bwt, size_t len, Sink& s, bool on_device) {
    if (len >= 0x7FFFFFFFull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "bwt: the buffer must be shorter than 2^31 - 1 bytes (32-bit len_t)"};
    if (len > 1) sink_fit(s, len);
    const size_t n = run_decoder(s, "bwt: buffer too large", nullptr, [&] { return bwt_inverse(ctx->c, bwt, len, 0, 0, s, nullptr, nullptr, on_device); });
    sink_commit(s, n);
}

// the host loops: the fall-back (option dec_parse = 0, small streams, a device that cannot hold the arena) and the specification
void pipeline_decompress_loops(tdc_gpu_ctx* ctx, const tdc_gpu_stage* stages, int k, const uint8_t* in, size_t len, Sink& s, PipeReport& rep) {
    const bool plog = ctx->c.pipe_log != 0;
    std::vector<uint8_t> a(in, in + len), b;
    for (int i = k - 1; i >= (stages[0].kind == TDC_GPU_STAGE_BWT ? 1 : 0); --i) {
        const auto t0 = std::chrono::steady_clock::now();
        rep.lens[i] = a.size();
        host_stage_decode(stages[i], a, b);
        rep.ms[i] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        pipe_line(plog, stages[i].kind, b.size(), a.size(), rep.ms[i], false);
        a.swap(b);
    }
    if (stages[0].kind == TDC_GPU_STAGE_BWT) {
        const auto t0 = std::chrono::steady_clock::now();
        rep.lens[0] = a.size();
        bwt_invert_into(ctx, a.data(), a.size(), s, false);
        rep.dev |= 1u;
        rep.ms[0] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        pipe_line(plog, TDC_GPU_STAGE_BWT, *s.out_len, a.size(), rep.ms[0], true);
        return;
    }
    *s.out_len = a.size();
    sink_fit(s, a.size());
    u8* dst = sink_host(s, a.size());
    if (!a.empty()) memcpy(dst, a.data(), a.size());
    sink_commit(s, a.size());
}

// The stages backwards on the device: one upload, every intermediate in the arena, one download.  False: the device cannot hold the
// arena (nothing has been written, the host loops take the call).  An arena that turns out too small for a stage's output -- the
// lengths are only known once the stage in front has been decoded -- is reserved again with what is known by then, the output's length
// and the scratch the stage held beside it, and the call starts over: at most once per stage, and never with the same figures twice.
bool pipeline_decompress_device(tdc_gpu_ctx* ctx, const tdc_gpu_stage* stages, int k, const uint8_t* in, size_t len, Sink& s, PipeReport& rep) {
    Ctx& c = ctx->c;
    const bool plog = c.pipe_log != 0;
    const bool lead_bwt = stages[0].kind == TDC_GPU_STAGE_BWT;
    const int first = lead_bwt ? 1 : 0;
    u64 known[TDC_GPU_PIPELINE_MAX_STAGES] = {0};              // decoded length of stage i, once an attempt has seen it
    bool have[TDC_GPU_PIPELINE_MAX_STAGES] = {false};
    u64 held[TDC_GPU_PIPELINE_MAX_STAGES] = {0};               // scratch stage i held when its output did not fit
    u64 extra = 0;
    for (int attempt = 0; attempt < 2 * TDC_GPU_PIPELINE_MAX_STAGES + 4; ++attempt) {
        u64 need = len + 4096 + extra, L = len;
        for (int i = k - 1; i >= first; --i) {
            const u64 out = have[i] ? known[i] : stages[i].kind == TDC_GPU_STAGE_MTF ? L : std::min<u64>(3 * L + 4096, STAGE_MAX_BYTES);
            need += out + 4096 + std::max<u64>(stage_decode_scratch_bound(L, out), held[i] + 4096);
            L = out;
        }
        if (lead_bwt) need += bwt_inverse_arena((size_t)std::min<u64>(L, 0x7FFFFFFFull)) + 4096;
        try { reserve_arena(c, need); }
        catch (const ArgError& e) { if (e.code == TDC_GPU_ERR_OOM) return false; throw; }
        catch (const HipError& e) { if (e.e == hipErrorOutOfMemory) { (void)hipGetLastError(); return false; } throw; }
        rep = PipeReport();
        auto t_last = std::chrono::steady_clock::now();
        auto tick = [&]() -> float {                                // (synchronises: only with the diagnostic option)
            if (!plog) return 0.f;
            HIP_TRY(hipStreamSynchronize(c.stream));
            const auto now = std::chrono::steady_clock::now();
            const float ms = std::chrono::duration<float, std::milli>(now - t_last).count();
            t_last = now;
            return ms;
        };
        StageOut cur;
        cur.d = c.arena.get<u8>(len + 64);
        cur.len = len;
        if (len) HIP_TRY(hipMemcpyAsync(cur.d, in, len, hipMemcpyHostToDevice, c.stream));
        HIP_TRY(hipMemsetAsync(cur.d + len, 0, 64, c.stream));
        bool again = false;
        for (int i = k - 1; i >= first && !again; --i) {
            rep.lens[i] = cur.len;
            bool dev = true;
            try {
                try {
                    switch (stages[i].kind) {
                        case TDC_GPU_STAGE_RLE: cur = rle_decode_device(c, cur.d, (size_t)cur.len, stages[i].param); break;
                        case TDC_GPU_STAGE_MTF: cur = mtf_decode_device(c, cur.d, (size_t)cur.len); break;
                        case TDC_GPU_STAGE_SLE: cur = sle_decode_device(c, cur.d, (size_t)cur.len, (u32)stages[i].param); break;
                        default: cur = huff_decode_device(c, cur.d, (size_t)cur.len); break;
                    }
                } catch (const StageHostOnly&) {                 // this one stage through its host loop
                    dev = false;
                    c.arena.release_top();
                    std::vector<uint8_t> a((size_t)cur.len), b;
                    if (cur.len) HIP_TRY(hipMemcpy(a.data(), cur.d, (size_t)cur.len, hipMemcpyDeviceToHost));
                    host_stage_decode(stages[i], a, b);
                    const size_t off = align_up(c.arena.top, 256);
                    if (off + b.size() + 64 > c.arena.size) throw StageArenaShort{b.size(), 0};
                    StageOut o;
                    o.d = c.arena.get<u8>(b.size() + 64); o.len = b.size();
                    if (o.len) HIP_TRY(hipMemcpy(o.d, b.data(), b.size(), hipMemcpyHostToDevice));
                    cur = o;
                }
            } catch (const StageArenaShort& a) {
                // The same figures a second time: the reservation already counts them and was still short -- a stage behind
                // StageHostOnly, whose output is measured against the whole arena, or an arena that could not grow.  Not the
                // same attempt again: grow as the out-of-memory path below does.
                if (have[i] && known[i] == a.out_bytes && held[i] >= a.scratch_bytes) extra = extra ? 2 * extra : need;
                known[i] = a.out_bytes; have[i] = true; held[i] = std::max(held[i], a.scratch_bytes); again = true;
            } catch (const HipError& e) {
                if (e.e != hipErrorOutOfMemory) throw;             // the stage's scratch did not fit
                (void)hipGetLastError();
                extra = extra ? 2 * extra : need; again = true;
            } catch (const StageTooLarge&) {
                throw ArgError{TDC_GPU_ERR_ARG, "pipeline: a stage decodes to more than 2^32 - 2 bytes"};
            } catch (const StreamFormatError&) {
                throw ArgError{TDC_GPU_ERR_ARG, "pipeline: malformed stream"};
            }
            c.arena.release_top();                                // the stage's scratch goes back once its output exists
            if (again) break;
            known[i] = cur.len; have[i] = true;
            if (dev) rep.dev |= 1u << i;
            rep.ms[i] = tick();
            pipe_line(plog, stages[i].kind, cur.len, rep.lens[i], rep.ms[i], dev);
        }
        if (again) { HIP_TRY(hipStreamSynchronize(c.stream)); continue; }
        if (lead_bwt) {
            if (cur.len < 0x7FFFFFFFull && align_up(c.arena.top, 256) + bwt_inverse_arena((size_t)cur.len) > c.arena.size) { HIP_TRY(hipStreamSynchronize(c.stream)); continue; }
            rep.lens[0] = cur.len;
            bwt_invert_into(ctx, cur.d, (size_t)cur.len, s, true);
            rep.dev |= 1u;
            rep.ms[0] = tick();
            pipe_line(plog, TDC_GPU_STAGE_BWT, *s.out_len, cur.len, rep.ms[0], true);
            return true;
        }
        const size_t out_len = (size_t)cur.len;
        *s.out_len = out_len;
        sink_fit(s, out_len);
        u8* dst = sink_host(s, out_len);
        if (out_len) {
            c.wait_for(c.copy_stream, c.stream);
            HIP_TRY(hipMemcpyAsync(dst, cur.d, out_len, hipMemcpyDeviceToHost, c.copy_stream));
            HIP_TRY(hipStreamSynchronize(c.copy_stream));
        }
        HIP_TRY(hipStreamSynchronize(c.stream));
        sink_commit(s, out_len);
        return true;
    }
    return false;
}

void pipeline_decompress_host(tdc_gpu_ctx* ctx, const tdc_gpu_stage* stages, int k, const uint8_t* in, size_t len, Sink s, tdc_gpu_stats* stats = nullptr) {
    if (!in && len) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
    sink_check(s, "NULL argument");
    if (stages && k >= 1 && k <= TDC_GPU_PIPELINE_MAX_STAGES)
        for (int i = 1; i < k; ++i) if (stages[i].kind == TDC_GPU_STAGE_BWT) throw ArgError{TDC_GPU_ERR_NO_SENTINEL, "pipeline: bwt must be the first stage"};
    if (!pipeline_valid(stages, k)) throw ArgError{TDC_GPU_ERR_ARG, "pipeline: 1 .. 8 stages of kind bwt (first only), rle, mtf, encode(huff) or encode(sle) (kmer 1 .. 7)"};
    if (len > STAGE_MAX_BYTES) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "pipeline: the stream must not be longer than 2^32 - 2 bytes"};
    Ctx& c = ctx->c;
    if (stats) memset(stats, 0, sizeof(*stats));
    const auto t_start = std::chrono::steady_clock::now();
    PipeReport rep;
    // option dec_parse, decided once per call from the stream's length: 1 = the device for streams of 1 MiB and more, 2 = always, 0 = never
    // (a pipeline of bwt alone has no byte stage: the path it always took)
    const bool byte_stages = k > (stages[0].kind == TDC_GPU_STAGE_BWT ? 1 : 0);
    const bool device = byte_stages && c.dec_parse && (c.dec_parse >= 2 || len >= ((size_t)1 << 20));
    if (!device || !pipeline_decompress_device(ctx, stages, k, in, len, s, rep)) {
        rep = PipeReport();
        pipeline_decompress_loops(ctx, stages, k, in, len, s, rep);
    }
    if (c.dec_log) fprintf(stderr, "pipe:     decompress %zu <- %zu bytes, stages on the device 0x%x\n", *s.out_len, len, rep.dev);
    if (stats) {
        stats->n = len; stats->out_len = *s.out_len; stats->pipe_stages = (uint32_t)k; stats->pipe_dev = rep.dev;
        for (int i = 0; i < k; ++i) { stats->pipe_len[i] = rep.lens[i]; stats->pipe_ms[i] = c.pipe_log ? rep.ms[i] : 0.f; }
        stats->arena_bytes = c.arena.high;
        stats->ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    }
}

int host_decode_entry(const uint8_t* in, size_t len, uint8_t* out, size_t out_cap, size_t* out_len, const std::function<void(tdc_amd::ByteSink&)>& f) {
    if ((!in && len) || !out_len) return TDC_GPU_ERR_ARG;
    try {
        tdc_amd::ByteSink sink(out, out_cap);
        f(sink);
        *out_len = sink.n > (u64)SIZE_MAX ? SIZE_MAX : (size_t)sink.n;
        return out && sink.n > out_cap ? TDC_GPU_ERR_ARG : TDC_GPU_OK;
    } catch (const std::runtime_error&) { return TDC_GPU_ERR_ARG;
    } catch (const std::length_error&) { return TDC_GPU_ERR_TOO_LARGE;       // (lzw_decode: more than 2^32 - 2 bytes)
    } catch (...) { return TDC_GPU_ERR_INTERNAL; }
}
}  // namespace

extern "C" {

size_t tdc_gpu_pipeline_bound(const tdc_gpu_stage* stages, int nstages, size_t n) {
    if (!pipeline_valid(stages, nstages) || n > STAGE_MAX_BYTES) return 0;
    u64 len = n;
    for (int i = 0; i < nstages; ++i) {
        len = stage_worst(stages[i], len);
        if (len > STAGE_MAX_BYTES) return 0;                  // (where the arena's stage_bound() clamps, the public bound says "no bound")
    }
    return (size_t)len;
}

int tdc_gpu_pipeline_compress(tdc_gpu_ctx* ctx, const tdc_gpu_stage* stages, int nstages, const uint8_t* in, size_t n, uint8_t** out,
                              size_t* out_len, tdc_gpu_stats* stats) {
    return guarded(ctx, [&] { pipeline_compress_host(ctx, stages, nstages, in, n, sink_malloc(out, out_len), stats); });
}

int tdc_gpu_pipeline_compress_into(tdc_gpu_ctx* ctx, const tdc_gpu_stage* stages, int nstages, const uint8_t* in, size_t n, uint8_t* out,
                                   size_t out_cap, size_t* out_len, tdc_gpu_stats* stats) {
    return guarded(ctx, [&] { pipeline_compress_host(ctx, stages, nstages, in, n, sink_into(out, out_cap, out_len), stats); });
}

size_t tdc_gpu_pipeline_batch_bound(const tdc_gpu_stage* stages, int nstages, const uint64_t* in_off, size_t count) {
    if (!in_off || in_off[0] != 0 || !pipeline_valid(stages, nstages) || count > 0x7FFFFFFFull) return 0;
    for (int i = 0; i < nstages; ++i) if (stages[i].kind == TDC_GPU_STAGE_SLE) return 0;
    size_t sum = 0;
    for (size_t t = 0; t < count; ++t) {
        if (in_off[t + 1] < in_off[t]) return 0;
        const u64 nk = in_off[t + 1] - in_off[t];
        if (nk <= BATCH_TEXT_CAP) sum += align_up(tdc_gpu_pipeline_bound(stages, nstages, (size_t)nk), 8);
    }
    return in_off[count] > STAGE_MAX_BYTES ? 0 : sum;
}

int tdc_gpu_pipeline_compress_batch(tdc_gpu_ctx* ctx, const tdc_gpu_stage* stages, int nstages, const uint8_t* in, const uint64_t* in_off, size_t count,
                                    uint8_t* out, size_t out_cap, uint64_t* out_off, uint64_t* out_len, int32_t* status, tdc_gpu_stats* stats) {
    try { pipeline_batch_check(stages, nstages, in, in_off, count, out_off, out_len, status); }       // (before the context: no device needed)
    catch (const ArgError& e) { if (ctx) ctx->last_error = e.msg; return e.code; }
    return guarded(ctx, [&] { pipeline_compress_batch_host(ctx, stages, nstages, in, in_off, count, out, out_cap, out_off, out_len, status, stats); });
}

int tdc_gpu_pipeline_decompress(tdc_gpu_ctx* ctx, const tdc_gpu_stage* stages, int nstages, const uint8_t* in, size_t len, uint8_t** out,
                                size_t* out_len) {
    return guarded(ctx, [&] { pipeline_decompress_host(ctx, stages, nstages, in, len, sink_malloc(out, out_len, "NULL argument")); });
}

int tdc_gpu_pipeline_decompress_into(tdc_gpu_ctx* ctx, const tdc_gpu_stage* stages, int nstages, const uint8_t* in, size_t len,
                                     uint8_t* out, size_t out_cap, size_t* out_len) {
    return guarded(ctx, [&] { pipeline_decompress_host(ctx, stages, nstages, in, len, sink_into(out, out_cap, out_len)); });
}

int tdc_gpu_pipeline_decompress_stats(tdc_gpu_ctx* ctx, const tdc_gpu_stage* stages, int nstages, const uint8_t* in, size_t len,
                                      uint8_t* out, size_t out_cap, size_t* out_len, tdc_gpu_stats* stats) {
    return guarded(ctx, [&] { pipeline_decompress_host(ctx, stages, nstages, in, len, sink_into(out, out_cap, out_len), stats); });
}

int tdc_rle_decode(const uint8_t* in, size_t len, uint64_t offset, uint8_t* out, size_t out_cap, size_t* out_len) {
    return host_decode_entry(in, len, out, out_cap, out_len, [&](tdc_amd::ByteSink& s) { tdc_amd::rle_decode(in, len, offset, s); });
}
int tdc_mtf_decode(const uint8_t* in, size_t len, uint8_t* out, size_t out_cap, size_t* out_len) {
    return host_decode_entry(in, len, out, out_cap, out_len, [&](tdc_amd::ByteSink& s) { tdc_amd::mtf_decode(in, len, s); });
}
int tdc_huff_decode_literals(const uint8_t* in, size_t len, uint8_t* out, size_t out_cap, size_t* out_len) {
    return host_decode_entry(in, len, out, out_cap, out_len, [&](tdc_amd::ByteSink& s) { tdc_amd::huff_decode_literals(in, len, s); });
}
int tdc_sle_decode(const uint8_t* in, size_t len, uint32_t kmer, uint8_t* out, size_t out_cap, size_t* out_len) {
    if (kmer > 7) return TDC_GPU_ERR_ARG;
    return host_decode_entry(in, len, out, out_cap, out_len, [&](tdc_amd::ByteSink& s) { tdc_amd::sle_decode_literals(in, len, kmer ? kmer : 3u, s); });
}
int tdc_lzw_decode(const uint8_t* in, size_t len, int coder, uint8_t* out, size_t out_cap, size_t* out_len) {
    if (coder != TDC_GPU_CODER_BIT && coder != TDC_GPU_CODER_GAMMA) return TDC_GPU_ERR_UNSUPPORTED;
    return host_decode_entry(in, len, out, out_cap, out_len, [&](tdc_amd::ByteSink& s) { tdc_amd::lzw_decode(in, len, coder == TDC_GPU_CODER_BIT, s); });
}
int tdc_lzss_decode(const uint8_t* in, size_t len, int coder, uint8_t* out, size_t out_cap, size_t* out_len) {
    if (coder != TDC_GPU_CODER_HUFF && coder != TDC_GPU_CODER_BIT && coder != TDC_GPU_CODER_GAMMA && coder != TDC_GPU_CODER_DELTA &&
        coder != TDC_GPU_CODER_ASCII) return TDC_GPU_ERR_UNSUPPORTED;
    return host_decode_entry(in, len, out, out_cap, out_len, [&](tdc_amd::ByteSink& s) {
        std::vector<uint8_t> text;
        tdc_amd::lzss_decode_coder(in, len, coder, text);
        for (uint8_t b : text) s.put(b);
    });
}

}  // extern "C"
