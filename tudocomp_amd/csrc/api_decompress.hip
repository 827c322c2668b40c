// api_decompress.hip -- C ABI (include/tdc_gpu.h): lcpcomp, lzss_lcp, lz78, lzw, lzss and repair decompression.
#include "api.hpp"
#include "stream_parse.hpp"
#include "../host/tdc_coders.hpp"

#include <chrono>
#include <stdexcept>
#include <vector>

using namespace tdc;

namespace {
void lcpcomp_decompress(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, Sink s, uint64_t* factors, uint32_t* rounds) {
    ctx->last_decode_device = 0;                             // (a failed call must not report the previous call's value)
    if (!stream) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
    sink_check(s, "NULL argument");
    const int enc = lcpcomp_enc_coder(coder);
    if (enc == 1) throw ArgError{TDC_GPU_ERR_UNSUPPORTED, "lcpcomp(coder=arithmetic) streams cannot be decoded (neither can the reference)"};
    DecodeStats ds;
    // (no `need`: a caller's buffer that is too small is reported as the decoder's allocation failure, without the required size)
    const size_t n = run_decoder(s, "lcpcomp: the stream decodes to too large a text", nullptr, [&] { return decode_lzss(ctx->c, stream, len, enc, s, &ds); });
    if (factors) *factors = ds.factors;
    if (rounds) *rounds = ds.rounds;
    ctx->last_decode_device = (int)ds.device_parse;
    sink_commit(s, n);
}

// LZSSLCPCompressor::decompress for its five coders.  huff and ascii are lcpcomp's streams.  bit, gamma, delta: the device parse where
// decode_lzss_uni takes the stream, else the host loop that is its specification (tdc_lzss_decode).
void lzss_lcp_decompress(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, Sink s, uint64_t* factors, uint32_t* rounds) {
    ctx->last_decode_device = 0;
    if (coder == TDC_GPU_CODER_HUFF || coder == TDC_GPU_CODER_ASCII) { lcpcomp_decompress(ctx, stream, len, coder, std::move(s), factors, rounds); return; }
    if (coder != TDC_GPU_CODER_BIT && coder != TDC_GPU_CODER_GAMMA && coder != TDC_GPU_CODER_DELTA)
        throw ArgError{TDC_GPU_ERR_UNSUPPORTED, "lzss_lcp: coder must be huff, bit, gamma, delta or ascii"};
    if (!stream) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
    sink_check(s, "NULL argument");
    DecodeStats ds;
    size_t n = 0;
    const int kind = coder == TDC_GPU_CODER_BIT ? 0 : coder == TDC_GPU_CODER_GAMMA ? 1 : 2;
    const bool dev = run_decoder(s, "lzss_lcp: the stream decodes to too large a text", nullptr,
                                 [&] { return (size_t)decode_lzss_uni(ctx->c, stream, len, kind, s, &ds, &n); }) != 0;
    if (!dev) {
        std::vector<uint8_t> text;
        try { tdc_amd::lzss_decode_coder(stream, len, coder, text); }
        catch (const std::runtime_error&) { throw ArgError{TDC_GPU_ERR_ARG, "lzss_lcp: corrupt stream"}; }
        n = text.size();
        sink_fit(s, n);
        u8* dst = decode_dest(s, n);
        if (n) memcpy(dst, text.data(), n);
        ds = DecodeStats();
    }
    if (factors) *factors = ds.factors;
    if (rounds) *rounds = ds.rounds;
    ctx->last_decode_device = (int)ds.device_parse;
    sink_commit(s, n);
}

void lz78_decompress(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, Sink s, uint64_t* phrases, uint32_t* rounds) {
    if (coder != TDC_GPU_CODER_GAMMA) throw ArgError{TDC_GPU_ERR_UNSUPPORTED, "lz78: only coder=gamma is built"};
    if (!stream && len) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
    sink_check(s, "NULL argument");
    DecodeStats ds;
    size_t need = 0;
    const size_t n = run_decoder(s, "lz78: the stream decodes to more than 2^32 - 2 bytes", &need, [&] { return decode_lz78_gamma(ctx->c, stream, len, s, &need, &ds); });
    if (phrases) *phrases = ds.factors;
    if (rounds) *rounds = ds.rounds;
    sink_commit(s, n);
}

void lzw_decompress(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, Sink s, uint64_t* codes, uint32_t* rounds) {
    ctx->last_decode_device = 0;
    if (coder != TDC_GPU_CODER_BIT && coder != TDC_GPU_CODER_GAMMA) throw ArgError{TDC_GPU_ERR_UNSUPPORTED, "lzw: only coder=bit and coder=gamma are built"};
    if (!stream && len) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
    sink_check(s, "NULL argument");
    DecodeStats ds;
    size_t need = 0;
    const size_t n = run_decoder(s, "lzw: the stream decodes to more than 2^32 - 2 bytes", &need,
                                 [&] { return decode_lzw(ctx->c, stream, len, coder == TDC_GPU_CODER_BIT, s, &need, &ds); });
    if (codes) *codes = ds.factors;
    if (rounds) *rounds = ds.rounds;
    ctx->last_decode_device = (int)ds.device_parse;
    sink_commit(s, n);
}

// LZSSSlidingWindowCompressor::decompress.  bit, gamma, delta: the device where decode_lzss_sw takes the stream, else -- and for ascii --
// the host loop that is its specification (tdc_lzss_sw_decode).
void lzss_sw_decompress(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint32_t window, Sink s, uint64_t* factors, uint32_t* rounds) {
    ctx->last_decode_device = 0;
    if (coder != TDC_GPU_CODER_BIT && coder != TDC_GPU_CODER_GAMMA && coder != TDC_GPU_CODER_DELTA && coder != TDC_GPU_CODER_ASCII)
        throw ArgError{TDC_GPU_ERR_UNSUPPORTED, "lzss: coder must be bit, gamma, delta or ascii"};
    if (coder == TDC_GPU_CODER_BIT && window == 0) throw ArgError{TDC_GPU_ERR_ARG, "lzss: coder=bit needs the window (the width of the length field)"};
    if (!stream && len) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
    sink_check(s, "NULL argument");
    DecodeStats ds;
    size_t n = 0, need = 0;
    bool dev = false;
    if (coder != TDC_GPU_CODER_ASCII) {
        const int kind = dec_kind(coder);
        dev = run_decoder(s, "lzss: the stream decodes to more than 2^32 - 2 bytes", &need,
                          [&] { return (size_t)decode_lzss_sw(ctx->c, stream, len, kind, window, s, &need, &ds, &n); }) != 0;
    }
    if (!dev) {
        std::vector<uint8_t> text;
        const int rc = lzss_sw_decode_host(stream, len, coder, window, text);
        if (rc == TDC_GPU_ERR_TOO_LARGE) throw ArgError{rc, "lzss: the stream decodes to more than 2^32 - 2 bytes"};
        if (rc == TDC_GPU_ERR_OOM) throw std::bad_alloc();
        if (rc) throw ArgError{rc, "lzss: corrupt stream"};
        n = text.size();
        sink_fit(s, n);
        u8* dst = decode_dest(s, n);
        if (n) memcpy(dst, text.data(), n);
        ds = DecodeStats();
    }
    if (factors) *factors = ds.factors;
    if (rounds) *rounds = ds.rounds;
    ctx->last_decode_device = (int)ds.device_parse;
    sink_commit(s, n);
}

// ---- lzss streams in a batch (lzss_sw_batch.hip): one wave per stream, never the host loop ----------------------------------------
void lzss_sw_batch_dec_check(const uint8_t* streams, const uint64_t* s_off, const uint64_t* s_len, size_t count, int coder, uint32_t window,
                             const uint64_t* out_off, const int32_t* status) {
    if (!out_off || (count && (!s_off || !s_len || !status))) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
    if (coder != TDC_GPU_CODER_BIT && coder != TDC_GPU_CODER_GAMMA && coder != TDC_GPU_CODER_DELTA)
        throw ArgError{TDC_GPU_ERR_UNSUPPORTED, "lzss batch: coder must be bit, gamma or delta (ascii streams: tdc_lzss_sw_decode)"};
    if (coder == TDC_GPU_CODER_BIT && window == 0) throw ArgError{TDC_GPU_ERR_ARG, "lzss: coder=bit needs the window (the width of the length field)"};
    if (count > 0xFFFFFFFEull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "lzss batch: too many streams"};
    for (size_t k = 0; k < count; ++k) {
        if (s_off[k] + s_len[k] < s_off[k]) throw ArgError{TDC_GPU_ERR_ARG, "lzss batch: a stream's end overflows"};
        if (s_len[k] && !streams) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
    }
}

void lzss_sw_decompress_batch(tdc_gpu_ctx* ctx, const uint8_t* streams, const uint64_t* s_off, const uint64_t* s_len, size_t count, int coder,
                              uint32_t window, uint8_t* out, size_t out_cap, uint64_t* out_off, int32_t* status, tdc_gpu_stats* stats) {
    Ctx& c = ctx->c;
    ctx->last_decode_device = 0;
    if (stats) memset(stats, 0, sizeof(*stats));
    out_off[0] = 0;
    if (count == 0) return;
    // the part of `streams` the batch lies in, from the 4-byte border in front of its first byte on
    u64 lo = ~0ull, hi = 0, bytes_in = 0;
    for (size_t k = 0; k < count; ++k) {
        if (!s_len[k]) continue;
        lo = std::min<u64>(lo, s_off[k]); hi = std::max<u64>(hi, s_off[k] + s_len[k]);
        bytes_in += s_len[k];
    }
    if (hi == 0) lo = 0;
    const u64 sub = lo & ~3ull;
    const size_t extent = (size_t)(hi - sub);
    if (extent > 0xFFFFFFFEull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "lzss batch: the streams must lie within 2^32 - 2 bytes"};
    const size_t slack = (size_t)16 << 20;
    const size_t fixed = extent + 64 + 40 * (count + 1) + 8 * 256 + slack;
    reserve_arena(c, fixed + 4 * extent);                         // (room for texts of four times the streams; more: the arena moves below)
    Events ev(c);
    const int e0 = ev.tick();
    hipStream_t s = c.stream;
    u8* d_blob = c.arena.get<u8>(extent + 64);
    if (extent) HIP_TRY(hipMemcpyAsync(d_blob, streams + sub, extent, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_blob + extent, 0, 64, s));
    u64* d_soff = c.arena.get<u64>(count), *d_slen = c.arena.get<u64>(count), *d_ooff = c.arena.get<u64>(count + 1);
    u32* d_tlen = c.arena.get<u32>(count);
    int* d_status = c.arena.get<int>(count);
    u64* d_fac = c.arena.get<u64>(1);
    HIP_TRY(hipMemcpyAsync(d_soff, s_off, count * sizeof(u64), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_slen, s_len, count * sizeof(u64), hipMemcpyHostToDevice, s));
    const int e1 = ev.tick();
    const int kind = dec_kind(coder);
    LzssSwBatchDec D;
    D.blob = d_blob; D.sub = sub; D.s_off = d_soff; D.s_len = d_slen; D.tlen = d_tlen; D.status = d_status; D.ooff = d_ooff; D.factors = d_fac;
    lzss_sw_batch_decode_sizes(c, kind, window, count, D);
    c.read_n(d_ooff, (u64*)out_off, count + 1);
    c.read_n(d_status, (int*)status, count);
    const u64 factors = c.read(d_fac);
    const int e2 = ev.tick();
    const u64 total = out_off[count];
    if (total > 0xFFFFFFFEull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "lzss batch: the streams decode to more than 2^32 - 2 bytes in all"};
    if (!out || total > out_cap) throw ArgError{TDC_GPU_ERR_OOM, "lzss batch: output buffer too small (out_off[count] holds the required size)"};
    if (c.arena.size < c.arena.mark() + (size_t)total + 64 + 512 + slack) {
        void* a = d_blob; void* b = d_soff; void* l = d_slen; void* o = d_ooff; void* t = d_tlen; void* v = d_status;
        regrow_arena(c, fixed + (size_t)total + 1024, {{&a, extent + 64}, {&b, count * 8}, {&l, count * 8}, {&o, (count + 1) * 8}, {&t, count * 4}, {&v, count * 4}});
        D.blob = (const u8*)a; D.s_off = (const u64*)b; D.s_len = (const u64*)l; D.ooff = (u64*)o; D.tlen = (u32*)t; D.status = (int*)v;
    }
    u8* d_text = c.arena.get<u8>((size_t)total + 64);
    lzss_sw_batch_decode_write(c, kind, window, count, D, d_text);
    const int e3 = ev.tick();
    if (total) HIP_TRY(hipMemcpyAsync(out, d_text, (size_t)total, hipMemcpyDeviceToHost, s));
    const int e4 = ev.tick();
    if (stats) {
        stats->n = bytes_in; stats->out_len = total; stats->factors = factors; stats->arena_bytes = c.arena.high;
        ev.span(&stats->ms_h2d, e0, e1); ev.span(&stats->ms_factorize, e1, e2); ev.span(&stats->ms_encode, e2, e3);
        ev.span(&stats->ms_d2h, e3, e4); ev.span(&stats->ms_total, e0, e4);
    }
    ev.finish();
    ctx->last_decode_device = 1;
}

// ---- lzw / lz78 streams in a batch (lz_batch_decode.hip): one forest of items, one pass, never the host loop -------------------------
void lz_batch_dec_check(bool lzw, const uint8_t* streams, const uint64_t* s_off, const uint64_t* s_len, size_t count, int coder,
                        const uint64_t* out_off, const int32_t* status) {
    if (!out_off || (count && (!s_off || !s_len || !status))) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
    if (lzw ? (coder != TDC_GPU_CODER_BIT && coder != TDC_GPU_CODER_GAMMA) : coder != TDC_GPU_CODER_GAMMA)
        throw ArgError{TDC_GPU_ERR_UNSUPPORTED, lzw ? "lzw batch: only coder=bit and coder=gamma are built" : "lz78 batch: only coder=gamma is built"};
    if (count > 0xFFFFFFFEull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "lz batch: too many streams"};
    for (size_t k = 0; k < count; ++k) {
        if (s_off[k] + s_len[k] < s_off[k]) throw ArgError{TDC_GPU_ERR_ARG, "lz batch: a stream's end overflows"};
        if (s_len[k] && !streams) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
    }
}

void lz_decompress_batch(tdc_gpu_ctx* ctx, bool lzw, const uint8_t* streams, const uint64_t* s_off, const uint64_t* s_len, size_t count, int coder,
                         uint8_t* out, size_t out_cap, uint64_t* out_off, int32_t* status, tdc_gpu_stats* stats) {
    Ctx& c = ctx->c;
    ctx->last_decode_device = 0;
    if (stats) memset(stats, 0, sizeof(*stats));
    out_off[0] = 0;
    if (count == 0) return;
    const bool bit = coder == TDC_GPU_CODER_BIT;
    // the part of `streams` the batch lies in, from the 4-byte border in front of its first byte on
    u64 lo = ~0ull, hi = 0, bytes_in = 0;
    for (size_t k = 0; k < count; ++k) {
        if (!s_len[k]) continue;
        lo = std::min<u64>(lo, s_off[k]); hi = std::max<u64>(hi, s_off[k] + s_len[k]);
        bytes_in += s_len[k];
    }
    if (hi == 0) lo = 0;
    const u64 sub = lo & ~3ull;
    const size_t extent = (size_t)(hi - sub);
    if (extent > 0xFFFFFFFEull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "lz batch: the streams must lie within 2^32 - 2 bytes"};
    const size_t slack = (size_t)16 << 20;
    const size_t fixed = extent + 64 + 48 * (count + 1) + 12 * 256 + slack;
    const size_t per_item = 38, per_byte = 5;                     // ids, chars, owner, J, S, the factor list, lit | text, d_ref, the done bits
    reserve_arena(c, fixed + 40 * extent);                        // (room for the items and the texts of most batches; more: the arena moves below)
    Events ev(c);
    const int e0 = ev.tick();
    hipStream_t s = c.stream;
    u8* d_blob = c.arena.get<u8>(extent + 64);
    if (extent) HIP_TRY(hipMemcpyAsync(d_blob, streams + sub, extent, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_blob + extent, 0, 64, s));
    u64* d_soff = c.arena.get<u64>(count), *d_slen = c.arena.get<u64>(count), *d_bits = c.arena.get<u64>(count);
    u64* d_ioff = c.arena.get<u64>(count + 1), *d_ooff = c.arena.get<u64>(count + 1);
    int* d_status = c.arena.get<int>(count);
    u64* d_fac = c.arena.get<u64>(1);
    HIP_TRY(hipMemcpyAsync(d_soff, s_off, count * sizeof(u64), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_slen, s_len, count * sizeof(u64), hipMemcpyHostToDevice, s));
    const int e1 = ev.tick();
    LzBatchDec D;
    D.blob = d_blob; D.sub = sub; D.s_off = d_soff; D.s_len = d_slen; D.bits = d_bits; D.status = d_status; D.item_off = d_ioff; D.ooff = d_ooff;
    D.factors = d_fac;
    lz_batch_decode_count(c, lzw, bit, count, D);
    // the one number the arena's size depends on (gamma: no array may hold an entry per stream bit, so the items are counted first)
    const u64 z = c.read(d_ioff + count);
    if (z >= 0xFFFFFFFEull - 256) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "lz batch: the streams hold 2^32 - 258 items or more in all"};
    u64 factors = 0;
    u32 len_rounds = 0, ref_rounds = 0;
    LzBatchItems I;
    I.z = (size_t)z;
    size_t mk_items = 0;
    if (z == 0) {                                                 // no item anywhere: every text is empty, the verdicts are the bits kernel's
        HIP_TRY(hipMemsetAsync(d_ooff, 0, (count + 1) * sizeof(u64), s));
    } else {
        if (c.arena.size < c.arena.mark() + per_item * (size_t)z + per_byte * extent + slack) {
            void* a = d_blob; void* b = d_soff; void* l = d_slen; void* t = d_bits; void* i = d_ioff; void* o = d_ooff; void* v = d_status; void* f = d_fac;
            regrow_arena(c, fixed + per_item * (size_t)z + 4 * per_byte * extent + 4096,
                         {{&a, extent + 64}, {&b, count * 8}, {&l, count * 8}, {&t, count * 8}, {&i, (count + 1) * 8}, {&o, (count + 1) * 8}, {&v, count * 4}, {&f, 8}});
            D.blob = (const u8*)a; D.s_off = (const u64*)b; D.s_len = (const u64*)l; D.bits = (u64*)t; D.item_off = (u64*)i; D.ooff = (u64*)o;
            D.status = (int*)v; D.factors = (u64*)f;
        }
        I.fpos = c.arena.get<u32>(I.z); I.fsrc = c.arena.get<u32>(I.z); I.flen = c.arena.get<u32>(I.z); I.lit = c.arena.get<u8>(I.z + 64);
        mk_items = c.arena.mark();                                // (what lies above lives until the factor list is made)
        I.ids = c.arena.get<u32>(I.z); I.owner = c.arena.get<u32>(I.z); I.J = c.arena.get<u64>(I.z); I.S = c.arena.get<u64>(I.z + 1);
        I.chars = lzw ? nullptr : c.arena.get<u8>(I.z + 64);
        u32* d_cnt = c.arena.get<u32>(2);
        len_rounds = lz_batch_decode_sizes(c, lzw, bit, count, D, I, d_cnt);
    }
    // the one round of read-backs every decision below rests on
    c.read_n(D.ooff, (u64*)out_off, count + 1);
    c.read_n(D.status, (int*)status, count);
    if (z) factors = c.read(D.factors);
    const int e2 = ev.tick();
    const u64 total = out_off[count];
    if (total > 0xFFFFFFFEull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "lz batch: the streams decode to more than 2^32 - 2 bytes in all"};
    if (!out || total > out_cap) throw ArgError{TDC_GPU_ERR_OOM, "lz batch: output buffer too small (out_off[count] holds the required size)"};
    int e3 = e2;
    if (total) {
        c.arena.release(mk_items);
        const size_t text_need = (size_t)total * per_byte + (size_t)total / 8 + 4096 + slack;
        if (c.arena.size < c.arena.mark() + text_need) {
            void* p = I.fpos; void* q = I.fsrc; void* l = I.flen; void* t = I.lit;
            regrow_arena(c, fixed + 13 * I.z + text_need, {{&p, I.z * 4}, {&q, I.z * 4}, {&l, I.z * 4}, {&t, I.z}});
            I.fpos = (u32*)p; I.fsrc = (u32*)q; I.flen = (u32*)l; I.lit = (u8*)t;
        }
        u32* d_cnt = c.arena.get<u32>(2);
        u8* d_text = c.arena.get<u8>((size_t)total + 64);
        u32* d_ref = c.arena.get<u32>((size_t)total);
        lz_batch_decode_literals(c, lzw, I, d_text);
        Sink sink;
        size_t written = 0;
        sink.into = out; sink.cap = out_cap; sink.out_len = &written;
        DecodeStats ds;
        resolve_and_download(c, (size_t)total, d_text, d_ref, I.fpos, I.fsrc, I.flen, I.z, d_cnt, sink, &ds);
        ref_rounds = ds.rounds;
        e3 = ev.tick();
    }
    if (stats) {
        stats->n = bytes_in; stats->out_len = total; stats->factors = factors; stats->arena_bytes = c.arena.high;
        stats->len_rounds = len_rounds; stats->flatten_rounds = ref_rounds;
        ev.span(&stats->ms_h2d, e0, e1); ev.span(&stats->ms_factorize, e1, e2); ev.span(&stats->ms_encode, e2, e3);
        ev.span(&stats->ms_total, e0, e3);
    }
    ev.finish();
    ctx->last_decode_device = 1;
}

// RePairCompressor::decompress.  bit, gamma, delta: the device where decode_repair takes the stream, else -- and for ascii -- the host
// loop that is its specification (tdc_repair_decode), whose status codes the call returns.
void repair_decompress(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, Sink s, tdc_gpu_stats* stats) {
    ctx->last_decode_device = 0;
    if (!stream && len) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
    sink_check(s, "NULL argument");
    if (stats) memset(stats, 0, sizeof(*stats));
    const auto t_start = std::chrono::steady_clock::now();
    RepairDecodeStats rs;
    size_t n = 0, need = 0;
    bool dev = false;
    if (coder == TDC_GPU_CODER_BIT || coder == TDC_GPU_CODER_GAMMA || coder == TDC_GPU_CODER_DELTA) {
        const int kind = dec_kind(coder);
        dev = run_decoder(s, "repair: the stream decodes to more than 2^32 - 2 bytes", &need,
                          [&] { return (size_t)decode_repair(ctx->c, stream, len, kind, s, &need, &rs, &n); }) != 0;
    }
    if (!dev) {
        int rc = tdc_repair_decode(stream, len, coder, nullptr, 0, &n);          // the verdict and the length, before any text is made
        if (rc == TDC_GPU_OK) {
            sink_fit(s, n);
            rc = tdc_repair_decode(stream, len, coder, decode_dest(s, n), n, &n);
        }
        if (rc) throw ArgError{rc, "repair: the stream is refused (tdc_repair_decode)"};
        rs = RepairDecodeStats();
    }
    if (stats) {
        stats->n = n; stats->out_len = n; stats->rules = rs.rules; stats->factors = rs.dec.factors; stats->arena_bytes = dev ? ctx->c.arena.high : 0;
        stats->flatten_rounds = rs.dec.rounds; stats->len_rounds = rs.len_rounds; stats->levels = rs.first_rounds; stats->small_levels = rs.segments;
        stats->ms_h2d = rs.ms_h2d; stats->ms_factorize = rs.ms_grammar; stats->ms_d2h = rs.ms_text;
        stats->ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    }
    ctx->last_decode_device = (int)rs.dec.device_parse;
    sink_commit(s, n);
}

// ---- repair streams in a batch (repair_batch_decode.hip): one forest of rules, one pass, never the host loop ----------------------------
// the refusals decided from the arguments alone, in the order of tdc_gpu_repair_compress_batch: the coder first
void repair_batch_dec_check(const uint8_t* streams, const uint64_t* s_off, const uint64_t* s_len, size_t count, int coder, const uint64_t* out_off,
                            const int32_t* status) {
    if (coder != TDC_GPU_CODER_BIT && coder != TDC_GPU_CODER_GAMMA && coder != TDC_GPU_CODER_DELTA)
        throw ArgError{TDC_GPU_ERR_UNSUPPORTED, "repair batch: coder must be bit, gamma or delta (ascii streams: tdc_repair_decode)"};
    if (!out_off || (count && (!s_off || !s_len || !status))) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
    for (size_t k = 0; k < count; ++k)
        if (s_off[k] + s_len[k] < s_off[k]) throw ArgError{TDC_GPU_ERR_ARG, "repair batch: a stream's end overflows"};
    for (size_t k = 0; k < count; ++k)
        if (s_len[k] && !streams) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
    if (count > 0xFFFFFFFEull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "repair batch: too many streams"};
}

void repair_decompress_batch(tdc_gpu_ctx* ctx, const uint8_t* streams, const uint64_t* s_off, const uint64_t* s_len, size_t count, int coder,
                             uint8_t* out, size_t out_cap, uint64_t* out_off, int32_t* status, tdc_gpu_stats* stats) {
    Ctx& c = ctx->c;
    ctx->last_decode_device = 0;
    if (stats) memset(stats, 0, sizeof(*stats));
    out_off[0] = 0;
    if (count == 0) return;
    const int kind = dec_kind(coder);
    // the part of `streams` the batch lies in, from the 4-byte border in front of its first byte on
    u64 lo = ~0ull, hi = 0, bytes_in = 0;
    for (size_t k = 0; k < count; ++k) {
        if (!s_len[k]) continue;
        lo = std::min<u64>(lo, s_off[k]); hi = std::max<u64>(hi, s_off[k] + s_len[k]);
        bytes_in += s_len[k];
    }
    if (hi == 0) lo = 0;
    const u64 sub = lo & ~3ull;
    const size_t extent = (size_t)(hi - sub);
    if (extent > 0xFFFFFFFEull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "repair batch: the streams must lie within 2^32 - 2 bytes"};
    const size_t slack = (size_t)16 << 20;
    // (with the slack of the grammar and the two of the text pass: the batches a compressor writes do not move the arena)
    const size_t fixed = extent + 64 + 56 * (count + 1) + 16 * 256 + 16384 + 3 * slack;
    // per token: its symbol, and what a rule (two tokens: two lengths, a first occurrence) or a start symbol (a position) adds at most |
    // per token: class byte, index and 12 bytes per factor | per text byte: text, d_ref, the done bits
    const size_t per_token = 12, per_item = 17, per_byte = 5;
    reserve_arena(c, fixed + 40 * extent);                        // (room for the grammars and the texts of most batches; more: the arena moves below)
    Events ev(c);
    const int e0 = ev.tick();
    hipStream_t s = c.stream;
    u8* d_blob = c.arena.get<u8>(extent + 64);
    if (extent) HIP_TRY(hipMemcpyAsync(d_blob, streams + sub, extent, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_blob + extent, 0, 64, s));
    u64* d_soff = c.arena.get<u64>(count), *d_slen = c.arena.get<u64>(count), *d_bits = c.arena.get<u64>(count);
    u64* d_roff = c.arena.get<u64>(count + 1), *d_toff = c.arena.get<u64>(count + 1), *d_ooff = c.arena.get<u64>(count + 1);
    int* d_status = c.arena.get<int>(count);
    u64* d_rules = c.arena.get<u64>(1);
    HIP_TRY(hipMemcpyAsync(d_soff, s_off, count * sizeof(u64), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_slen, s_len, count * sizeof(u64), hipMemcpyHostToDevice, s));
    const int e1 = ev.tick();
    RepairBatchDec D;
    D.blob = d_blob; D.sub = sub; D.s_off = d_soff; D.s_len = d_slen; D.bits = d_bits; D.status = d_status; D.rule_off = d_roff; D.start_off = d_toff;
    D.ooff = d_ooff; D.rules = d_rules;
    repair_batch_decode_count(c, kind, count, D);
    // the two numbers the arena's size depends on (no array may hold an entry per stream bit, so the tokens are counted first)
    RepairBatchGrammar G;
    G.R = (size_t)c.read(d_roff + count); G.M = (size_t)c.read(d_toff + count);
    const u64 items = 2 * (u64)G.R + G.M;
    if (items >= 0xFFFFFFFEull - 256) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "repair batch: the streams hold 2^32 - 258 tokens or more in all"};
    const u32 cap = (u32)std::min<long>(std::max<long>(c.repair_dec_rounds, 1), 1l << 24);
    u64 rules = 0;
    u32 len_rounds = 0, first_rounds = 0, ref_rounds = 0;
    size_t zf = 0, mk_len2 = 0;
    if (items == 0) {                                             // no token anywhere: every text is empty, the verdicts are the first walk's
        HIP_TRY(hipMemsetAsync(d_ooff, 0, (count + 1) * sizeof(u64), s));
    } else {
        if (c.arena.size < c.arena.mark() + per_token * (size_t)items + 8192 + 3 * slack) {              // (the text pass keeps its slack)
            void* a = d_blob; void* b = d_soff; void* l = d_slen; void* t = d_bits; void* r = d_roff; void* m = d_toff; void* o = d_ooff; void* v = d_status;
            void* f = d_rules;
            regrow_arena(c, fixed + (per_token + per_item) * (size_t)items + 4 * per_byte * extent + 8192 + slack,
                         {{&a, extent + 64}, {&b, count * 8}, {&l, count * 8}, {&t, count * 8}, {&r, (count + 1) * 8}, {&m, (count + 1) * 8},
                          {&o, (count + 1) * 8}, {&v, count * 4}, {&f, 8}});
            D.blob = (const u8*)a; D.s_off = (const u64*)b; D.s_len = (const u64*)l; D.bits = (u64*)t; D.rule_off = (u64*)r; D.start_off = (u64*)m;
            D.ooff = (u64*)o; D.status = (int*)v; D.rules = (u64*)f;
        }
        G.sym = c.arena.get<u32>((size_t)items); G.len = c.arena.get<u32>(G.R + 1); G.first = c.arena.get<u32>(G.R + 1); G.pos = c.arena.get<u64>(G.M + 1);
        mk_len2 = c.arena.mark();                                 // (what lies above is dead behind the sizes)
        G.len2 = c.arena.get<u32>(G.R + 1);
        u32* d_flags = c.arena.get<u32>(8);
        len_rounds = repair_batch_decode_sizes(c, kind, count, D, G, cap, d_flags);
    }
    // the one round of read-backs every decision below rests on
    c.read_n(D.ooff, (u64*)out_off, count + 1);
    c.read_n(D.status, (int*)status, count);
    if (items) rules = c.read(D.rules);
    const int e2 = ev.tick();
    const u64 total = out_off[count];
    if (total > 0xFFFFFFFEull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "repair batch: the streams decode to more than 2^32 - 2 bytes in all"};
    if (!out || total > out_cap) throw ArgError{TDC_GPU_ERR_OOM, "repair batch: output buffer too small (out_off[count] holds the required size)"};
    int e3 = e2;
    if (total) {
        const size_t n = (size_t)total, nit = (size_t)items;
        c.arena.release(mk_len2);
        u32* d_flags = c.arena.get<u32>(8);
        // every accepted grammar is at most `cap` high: its first occurrences rest after cap rounds and are seen to in the one behind
        first_rounds = repair_batch_decode_first(c, G, cap + 1, d_flags);
        if (!first_rounds) throw HipError{hipErrorUnknown, "repair batch decode: the first occurrences did not come to rest", (int)__LINE__};
        const size_t text_need = per_item * nit + per_byte * n + n / 8 + 8192 + 2 * slack;
        if (c.arena.size < c.arena.mark() + text_need) {
            void* a = G.sym; void* b = G.len; void* f = G.first; void* p = G.pos;
            const size_t live = nit * 4 + (G.R + 1) * 8 + (G.M + 1) * 8 + 4 * 320;
            regrow_arena(c, live + text_need, {{&a, nit * 4}, {&b, (G.R + 1) * 4}, {&f, (G.R + 1) * 4}, {&p, (G.M + 1) * 8}});
            G.sym = (u32*)a; G.len = (u32*)b; G.first = (u32*)f; G.pos = (u64*)p;
        }
        u32* d_cnt = c.arena.get<u32>(2);
        u8* cls = c.arena.get<u8>(nit);
        u32* fidx = c.arena.get<u32>(nit);
        u8* d_text = c.arena.get<u8>(n + 64);
        zf = repair_batch_decode_items(c, G, n, d_text, cls, fidx, d_cnt);
        u32* fpos = c.arena.get<u32>(zf + 1), *fsrc = c.arena.get<u32>(zf + 1), *flen = c.arena.get<u32>(zf + 1);
        repair_batch_decode_factors(c, G, fidx, zf, fpos, fsrc, flen);
        u32* d_ref = c.arena.get<u32>(n);
        if (zf == 0) {                                            // literals only: the text is complete
            HIP_TRY(hipMemcpyAsync(out, d_text, n, hipMemcpyDeviceToHost, s));
        } else {
            Sink sink;
            size_t written = 0;
            sink.into = out; sink.cap = out_cap; sink.out_len = &written;
            DecodeStats ds;
            resolve_and_download(c, n, d_text, d_ref, fpos, fsrc, flen, zf, d_cnt, sink, &ds);
            ref_rounds = ds.rounds;
        }
        e3 = ev.tick();
    }
    if (stats) {
        stats->n = bytes_in; stats->out_len = total; stats->rules = rules; stats->factors = zf; stats->arena_bytes = c.arena.high;
        stats->len_rounds = len_rounds; stats->levels = first_rounds; stats->flatten_rounds = ref_rounds;
        ev.span(&stats->ms_h2d, e0, e1); ev.span(&stats->ms_factorize, e1, e2); ev.span(&stats->ms_encode, e2, e3);
        ev.span(&stats->ms_total, e0, e3);
    }
    ev.finish();
    ctx->last_decode_device = 1;
}
}  // namespace

extern "C" {

int tdc_gpu_lcpcomp_decompress(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, uint8_t** out, size_t* out_len,
                               uint64_t* factors, uint32_t* rounds) {
    return tdc_gpu_lcpcomp_decompress_coder(ctx, stream, len, TDC_GPU_CODER_HUFF, out, out_len, factors, rounds);
}

int tdc_gpu_lcpcomp_decompress_coder(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint8_t** out, size_t* out_len,
                                     uint64_t* factors, uint32_t* rounds) {
    return guarded(ctx, [&] { lcpcomp_decompress(ctx, stream, len, coder, sink_malloc(out, out_len, "NULL argument"), factors, rounds); });
}

int tdc_gpu_lcpcomp_decompress_into(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint8_t* out, size_t out_cap,
                                    size_t* out_len, uint64_t* factors, uint32_t* rounds) {
    return guarded(ctx, [&] { lcpcomp_decompress(ctx, stream, len, coder, sink_into(out, out_cap, out_len), factors, rounds); });
}

int tdc_gpu_lzss_lcp_decompress(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint8_t** out, size_t* out_len,
                                uint64_t* factors, uint32_t* rounds) {
    return guarded(ctx, [&] { lzss_lcp_decompress(ctx, stream, len, coder, sink_malloc(out, out_len, "NULL argument"), factors, rounds); });
}

int tdc_gpu_lzss_lcp_decompress_into(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint8_t* out, size_t out_cap,
                                     size_t* out_len, uint64_t* factors, uint32_t* rounds) {
    return guarded(ctx, [&] { lzss_lcp_decompress(ctx, stream, len, coder, sink_into(out, out_cap, out_len), factors, rounds); });
}

int tdc_gpu_ctx_last_decode_on_device(const tdc_gpu_ctx* ctx) { return ctx ? ctx->last_decode_device : 0; }

int tdc_gpu_lz78_decompress(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint8_t** out, size_t* out_len,
                            uint64_t* phrases, uint32_t* rounds) {
    return guarded(ctx, [&] { lz78_decompress(ctx, stream, len, coder, sink_malloc(out, out_len, "NULL argument"), phrases, rounds); });
}

int tdc_gpu_lz78_decompress_into(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint8_t* out, size_t out_cap,
                                 size_t* out_len, uint64_t* phrases, uint32_t* rounds) {
    return guarded(ctx, [&] { lz78_decompress(ctx, stream, len, coder, sink_into(out, out_cap, out_len), phrases, rounds); });
}

int tdc_gpu_lzw_decompress(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint8_t** out, size_t* out_len,
                           uint64_t* codes, uint32_t* rounds) {
    return guarded(ctx, [&] { lzw_decompress(ctx, stream, len, coder, sink_malloc(out, out_len, "NULL argument"), codes, rounds); });
}

int tdc_gpu_lzw_decompress_into(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint8_t* out, size_t out_cap,
                                size_t* out_len, uint64_t* codes, uint32_t* rounds) {
    return guarded(ctx, [&] { lzw_decompress(ctx, stream, len, coder, sink_into(out, out_cap, out_len), codes, rounds); });
}

int tdc_gpu_lzss_sw_decompress(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint32_t window, uint8_t** out, size_t* out_len,
                               uint64_t* factors, uint32_t* rounds) {
    return guarded(ctx, [&] { lzss_sw_decompress(ctx, stream, len, coder, window, sink_malloc(out, out_len, "NULL argument"), factors, rounds); });
}

int tdc_gpu_lzss_sw_decompress_batch(tdc_gpu_ctx* ctx, const uint8_t* streams, const uint64_t* s_off, const uint64_t* s_len, size_t count, int coder,
                                     uint32_t window, uint8_t* out, size_t out_cap, uint64_t* out_off, int32_t* status, tdc_gpu_stats* stats) {
    try { lzss_sw_batch_dec_check(streams, s_off, s_len, count, coder, window, out_off, status); }      // (before the context: no device needed)
    catch (const ArgError& e) { if (ctx) ctx->last_error = e.msg; return e.code; }
    return guarded(ctx, [&] { lzss_sw_decompress_batch(ctx, streams, s_off, s_len, count, coder, window, out, out_cap, out_off, status, stats); });
}

int tdc_gpu_lzw_decompress_batch(tdc_gpu_ctx* ctx, const uint8_t* streams, const uint64_t* s_off, const uint64_t* s_len, size_t count, int coder,
                                 uint8_t* out, size_t out_cap, uint64_t* out_off, int32_t* status, tdc_gpu_stats* stats) {
    try { lz_batch_dec_check(true, streams, s_off, s_len, count, coder, out_off, status); }             // (before the context: no device needed)
    catch (const ArgError& e) { if (ctx) ctx->last_error = e.msg; return e.code; }
    return guarded(ctx, [&] { lz_decompress_batch(ctx, true, streams, s_off, s_len, count, coder, out, out_cap, out_off, status, stats); });
}

int tdc_gpu_lz78_decompress_batch(tdc_gpu_ctx* ctx, const uint8_t* streams, const uint64_t* s_off, const uint64_t* s_len, size_t count, int coder,
                                  uint8_t* out, size_t out_cap, uint64_t* out_off, int32_t* status, tdc_gpu_stats* stats) {
    try { lz_batch_dec_check(false, streams, s_off, s_len, count, coder, out_off, status); }
    catch (const ArgError& e) { if (ctx) ctx->last_error = e.msg; return e.code; }
    return guarded(ctx, [&] { lz_decompress_batch(ctx, false, streams, s_off, s_len, count, coder, out, out_cap, out_off, status, stats); });
}

int tdc_gpu_lzss_sw_decompress_into(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint32_t window, uint8_t* out, size_t out_cap,
                                    size_t* out_len, uint64_t* factors, uint32_t* rounds) {
    return guarded(ctx, [&] { lzss_sw_decompress(ctx, stream, len, coder, window, sink_into(out, out_cap, out_len), factors, rounds); });
}

int tdc_gpu_repair_decompress(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint8_t** out, size_t* out_len) {
    return guarded(ctx, [&] { repair_decompress(ctx, stream, len, coder, sink_malloc(out, out_len, "NULL argument"), nullptr); });
}

int tdc_gpu_repair_decompress_into(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint8_t* out, size_t out_cap, size_t* out_len) {
    return guarded(ctx, [&] { repair_decompress(ctx, stream, len, coder, sink_into(out, out_cap, out_len), nullptr); });
}

int tdc_gpu_repair_decompress_stats(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint8_t* out, size_t out_cap, size_t* out_len,
                                    tdc_gpu_stats* stats) {
    return guarded(ctx, [&] { repair_decompress(ctx, stream, len, coder, sink_into(out, out_cap, out_len), stats); });
}

int tdc_gpu_repair_decompress_batch(tdc_gpu_ctx* ctx, const uint8_t* streams, const uint64_t* s_off, const uint64_t* s_len, size_t count, int coder,
                                    uint8_t* out, size_t out_cap, uint64_t* out_off, int32_t* status, tdc_gpu_stats* stats) {
    try { repair_batch_dec_check(streams, s_off, s_len, count, coder, out_off, status); }                 // (before the context: no device needed)
    catch (const ArgError& e) { if (ctx) ctx->last_error = e.msg; return e.code; }
    return guarded(ctx, [&] { repair_decompress_batch(ctx, streams, s_off, s_len, count, coder, out, out_cap, out_off, status, stats); });
}

}  // extern "C"

// ---- bwt buffers in a batch (bwt_batch.hip, DESIGN.md section 5.2 "Batch decoder"): the LF cycles of all buffers as one forest --------------
extern "C" {

int tdc_gpu_bwt_decompress_batch(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* off, size_t count, uint8_t* out, size_t out_cap,
                                 int32_t* status, tdc_gpu_stats* stats) {
    try { bwtb_check(in, off, count, out, out_cap, 1, status, 0x7FFFFFFEull); }                       // (the top bit of an LF word stays free)
    catch (const ArgError& e) { if (ctx) ctx->last_error = e.msg; return e.code; }
    return guarded(ctx, [&] { bwtb_inverse(ctx, in, off, count, out, out_cap, status, stats); });
}

}  // extern "C"
