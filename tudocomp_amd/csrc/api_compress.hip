// api_compress.hip -- C ABI (include/tdc_gpu.h): lcpcomp, lzss_lcp, lz78, lzw, lzss and repair compression -- the upload, the text's arrays, the factors,
// the whole pipeline on host and device buffers.
#include "api.hpp"
#include "bitsink.hpp"

#include <vector>

using namespace tdc;

namespace tdc {

void validate_device_text(Ctx& c, const u8* d_text, size_t n) {
    if (!(c.hist_ptr == d_text && c.hist_n == n)) {
        const size_t mark = c.arena.mark();
        u32* d_hist = c.arena.get<u32>(256);
        HIP_TRY(hipMemsetAsync(d_hist, 0, 256 * sizeof(u32), c.stream));
        text_histogram_add(c, d_text, n, d_hist);
        text_histogram_finish(c, d_text, n, d_hist);
        c.arena.release(mark);
    }
    u8 last = 1;
    HIP_TRY(hipMemcpyAsync(&last, d_text + n - 1, 1, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    const u32 zeros = c.hist_cache[0];
    if (last != 0) throw ArgError{TDC_GPU_ERR_NO_SENTINEL, "text does not end with a 0 sentinel"};
    if (zeros != 1) throw ArgError{TDC_GPU_ERR_ARG, "text contains 0 bytes besides the sentinel (escape the input first)"};
}

// the metric's path (lcpcomp(comp=arrays, coder=huff) with the encoder's first half inside the flatten stage: nothing reads the dense
// flen[] array behind build_owner): the factor lengths travel as bytes until then
static bool early_is_planned(const Ctx& c, size_t n, u32 threshold, int flatten, int strategy, int enc_coder, const u8* d_text) {
    return strategy == TDC_GPU_COMP_ARRAYS && flatten && enc_coder == 0 && d_text && c.enc_early && c.enc_rec && c.huff_ok &&
           n >= (c.enc_early >= 2 ? (size_t)1 : ((size_t)1 << 20)) && threshold >= 2;
}

void run_textds(Ctx& c, const u8* d_text, size_t n, DevArrays& A, tdc_gpu_stats* st, Events* ev, bool want_phi, const CandWant* cw) {
    A.sa = c.arena.get<u32>(n);
    A.isa = c.arena.get<u32>(n);
    A.phi = nullptr;                                          // (taken behind the suffix array, and only where a Phi array is built)
    A.plcp = c.arena.get<u32>(n);
    u32* d_max = c.arena.get<u32>(1);
    SAStats ss;
    SAExtra ex;
    ex.lcp8 = c.arena.get<u8>(n + 64);                        // neighbour LCPs of the wide path (suffix_array.hip)
    const int e0 = ev ? ev->tick() : 0;
    build_suffix_array(c, d_text, n, A.sa, A.isa, &ss, &ex);
    const int e1 = ev ? ev->tick() : 0;
    int e2;
    if (!(ex.mode == 1 && !want_phi && c.phi_lazy)) A.phi = c.arena.get<u32>(n);
    if (ex.mode == 1) {                                       // ISA + Phi + PLCP in one scatter of the final suffix array
        // comp=arrays without Phi: the scatter's image kernel classifies the factorizer's candidates while it holds the PLCP values
        // (CandFused).  What it fills is taken here, below the scatter's scratch; run_factorize finds the length array in place.
        CandFused* cf = nullptr;
        if (cw && c.fused_cand && !A.phi && fused_scatter_has_image(c, n)) {
            cf = &A.cand;
            cf->threshold = cw->threshold;
            cf->lcut = factorize_arrays_lcut0(c, n, cw->threshold);
            cf->cls = c.arena.get<u8>(n);
            if (cf->lcut) cf->res8 = c.arena.get<u8>(n);
            if (cw->flen8) cf->flen8 = A.fs.flen8 = c.arena.get<u8>(n + 64); else cf->flen = A.fs.flen = c.arena.get<u32>(n);
            if (c.sel_tile_counts) cf->tilecnt = c.arena.get<u32>(cdiv(n, SEL_TILE_CLASSES));
            cf->acc = c.arena.get<u32>((size_t)CF_COPIES * CF_ACC);
            cf->lvlhist = c.arena.get<u32>(128);
            cf->entries = cf->lvlhist + 64;
        }
        build_isa_phi_plcp_fused(c, A.sa, ex.lcp8, n, A.isa, A.phi, A.plcp, d_max, cf);
        e2 = ev ? ev->tick() : 0;
    } else {
        build_phi(c, A.sa, n, A.phi);
        e2 = ev ? ev->tick() : 0;
        build_plcp(c, d_text, n, A.phi, A.plcp, d_max);
    }
    const int e3 = ev ? ev->tick() : 0;
    A.maxlcp = c.read(d_max);
    if (st) {
        st->maxlcp = A.maxlcp;
        sa_stats(st, ss, &ex);
        if (ev) { ev->span(&st->ms_sa, e0, e1); ev->span(&st->ms_phi, e1, e2); ev->span(&st->ms_plcp, e2, e3); }
    }
}

// flatten in rank ranges on the path that overlaps pack and download (option flatten_chunks = 0): factors per range at least, ranges at most
// (2e9 B of English, 150 M factors, gains with 8 ranges; 256 MiB, 20 M factors, gains nothing with 2 or 4)
constexpr size_t FLAT_CHUNK_MIN = (size_t)16 << 20;
constexpr size_t FLAT_CHUNK_MAX = 8;

void run_factorize(Ctx& c, size_t n, DevArrays& A, u32 threshold, int flatten, tdc_gpu_stats* st, Events* ev, int strategy,
                   int enc_coder, const u8* d_text) {
    if (!A.fs.flen) A.fs.flen = c.arena.get<u32>(n);          // (either length array may be in place already: run_textds, CandFused)
    A.fs.owner = c.arena.get<u32>(n);
    A.fs.fsrc = c.arena.get<u32>(n);
    A.fs.fpos = c.arena.get<u32>(n);
    A.fs.flenl = threshold >= 2 ? A.fs.fpos + (n + 1) / 2 : nullptr;    // (a factor covers >= threshold positions: at most n / 2 of them, the list of
                                                                         //  their lengths fits the upper half of the position list)
    A.fs.cls = c.arena.get<u8>(n + 64);                  // class bytes for the encoder (filled by build_owner)
    const bool early_planned = early_is_planned(c, n, threshold, flatten, strategy, enc_coder, d_text);
    if (early_planned && c.flen_bytes && !A.fs.flen8) A.fs.flen8 = c.arena.get<u8>(n + 64);
    A.fs.want_owner_rem = early_planned ? (u32)c.owner_rem : 0u;   // (behind build_owner only the flatten rounds read owner[] on this path: the encoder reads cls[] and the records)
    FactorizeStats fz;
    FlattenStats fl;
    const int e0 = ev ? ev->tick() : 0;
    if (strategy == TDC_GPU_COMP_PLCPPEAKS) plcp_peaks_factorize(c, n, A.phi, A.plcp, threshold, A.fs, &fz.factors);
    else if (strategy == TDC_GPU_COMP_MAXLCP) factorize_max_lcp(c, n, A.isa, A.phi, A.plcp, A.maxlcp, threshold, A.fs, &fz);
    else if (strategy == TDC_GPU_COMP_HEAP) factorize_max_heap(c, n, A.sa, A.isa, A.plcp, A.maxlcp, threshold, A.fs, &fz);
    else factorize_arrays(c, n, A.sa, A.isa, A.phi, A.plcp, A.maxlcp, threshold, A.fs, &fz, A.cand.filled ? &A.cand : nullptr);
    const int e1 = ev ? ev->tick() : 0;
    // The first half of the Huffman encoder (gaps, literal histogram, code table, bits per tile and their scan: 4-5 ms of streaming
    // kernels and three host round trips at 2e9 B) reads positions, lengths and class bytes but no source, and the flatten rounds are
    // bound by the latency of their chains, not by bandwidth: it runs on the copy stream next to the first round.
    const bool early = flatten && enc_coder == 0 && d_text && c.enc_early && c.huff_ok && n >= (c.enc_early >= 2 ? (size_t)1 : ((size_t)1 << 20)) &&
                       A.fs.have_list && A.fs.have_cls && A.fs.flenl && A.fs.nfact > 0;
    if (!early) expand_flen8(c, n, A.fs);                  // (planned, but there is no factor list to run it on: everybody else reads the dense array)
    if (early) {
        A.early = encode_early_reserve(c, n, c.enc_rec ? A.fs.nfact : 0);
        // Where pack and download overlap (a host buffer of the caller's, records kept), the rounds run on rank ranges and each range's
        // tiles are packed and sent while the next range is flattened.  Auto: a range holds at least FLAT_CHUNK_MIN
        // factors, below that its later rounds no longer fill the device.
        u32 K = c.flatten_chunks ? (u32)c.flatten_chunks : (u32)std::min<size_t>(A.fs.nfact / FLAT_CHUNK_MIN, FLAT_CHUNK_MAX);
        K = flatten_chunk_count(K, A.fs.nfact);
        const bool packed = K >= 2 && encode_early_chunks(c, n, A.fs, A.early, K, align_up(encode_bound_coder(n, enc_coder) + 16, 8));
        if (!packed && c.flatten_chunks < 2) K = 1;                        // (forced ranges run without a consumer)
        c.wait_for(c.copy_stream, c.stream);                               // the factors are in place
        // one step per round (the host never waits for the copy stream while a round needs it), the rest when the rounds are over
        flatten_factors(c, n, A.fs, &fl, [&](int round) {
            StreamSwap sw(c, c.copy_stream);
            if (round == 1 || round == 2) encode_early_run(c, d_text, n, A.fs, enc_coder, A.early, false);
            else if (round == 0) encode_early_run(c, d_text, n, A.fs, enc_coder, A.early, true);
        }, c.enc_rec ? encode_early_rec(A.early) : nullptr, K,
        packed ? std::function<void(u32, size_t)>([&](u32 k, size_t) { encode_early_chunk_done(c, d_text, n, A.fs, A.early, k); }) : std::function<void(u32, size_t)>());
    } else if (flatten) {
        flatten_factors(c, n, A.fs, &fl);
    } else {
        materialize_sources(c, n, A.fs);                   // (no Phi array: the encoder reads fsrc[] at every factor start)
    }
    const int e2 = ev ? ev->tick() : 0;
    if (st) {
        st->factors = fz.factors; st->entries = fz.entries; st->pushes = fz.pushes;
        st->levels = fz.levels; st->mis_rounds = fz.rounds; st->small_levels = fz.small_levels; st->purges = fz.purges; st->window_pass = fz.window_pass; st->window_lcut = fz.window_lcut; st->eager_levels = fz.eager_levels; st->eager_phases = fz.eager_phases;
        st->probes = fz.probes; st->max_push_targets = fz.max_push_targets;
        st->num_flattened = fl.num_flattened; st->max_depth_lb = fl.max_depth_lb; st->flatten_rounds = fl.rounds;
        st->ranges_early = A.early ? encode_early_packed(A.early) : 0u;
        if (ev) { ev->span(&st->ms_factorize, e0, e1); ev->span(&st->ms_flatten, e1, e2); }
    }
}

// (api.hpp: what the object undoes when it goes)
u8* TextUpload::send(const uint8_t* text, size_t n) {
    if (n < ((size_t)1 << 26)) return upload_plain(c, text, n);
    u8* d_text = c.arena.get<u8>(n + 64);
    // The upload in chunks on the copy stream.  Behind every chunk, on the compute stream: its byte histogram (sentinel check,
    // symbol codes) and -- texts that take the wide suffix sort -- level 1 of that sort for the chunk in front of it (a key reads
    // up to 64 bytes ahead), with the code map and the splitters taken from chunk 0 (prim.hpp WPre).  All copies are queued
    // first: the one host wait in between (the histogram of chunk 0) does not stall them.
    u32* d_hist = c.arena.get<u32>(256);
    HIP_TRY(hipMemsetAsync(d_hist, 0, 256 * sizeof(u32), c.stream));
    c.wait_for(c.copy_stream, c.stream);                                // (the copy stream starts behind whatever the compute stream did before)
    const bool try_pre = c.wsort_overlap && c.wpre && wsort_applicable(c, n);
    const size_t CH = try_pre ? (size_t)c.upload_chunks : 8;
    // Chunk boundaries (multiples of 4096).  With level 1 behind the copies the last three chunks shrink geometrically (0.6, 0.36,
    // 0.22 of the others): level 1 of a chunk runs 1.7 x as fast as its copy, so each of them is done before the next, shorter copy
    // ends, and what is left behind the last copy is the level 1 of a fifth of a chunk.
    std::vector<size_t> coff;
    {
        std::vector<double> w(CH, 1.0);
        if (try_pre) {                                   // (the last chunks shrink geometrically: options upload_tail_n / upload_tail_pct)
            const size_t T = std::min<size_t>((size_t)c.upload_tail_n, CH - 1);
            double f = 1.0;
            for (size_t k = 0; k < T; ++k) { f *= (double)c.upload_tail_pct / 100.0; w[CH - T + k] = f; }
        }
        double tot = 0; for (double x : w) tot += x;
        coff.push_back(0);
        double acc = 0;
        for (size_t k = 0; k + 1 < CH; ++k) {
            acc += w[k];
            size_t o = ((size_t)((double)n * (acc / tot)) + 4095) & ~(size_t)4095;
            if (o <= coff.back()) o = coff.back() + 4096;
            if (o >= n) break;
            coff.push_back(o);
        }
        coff.push_back(n);
    }
    const size_t nch = coff.size() - 1;
    if (nch > Ctx::CHUNK_EVENTS) throw HipError{hipErrorUnknown, "upload: more chunks than chunk events", (int)__LINE__};
    size_t queued = 0;                                                  // copies handed to the copy stream so far
    auto queue_copies = [&](size_t upto) {                              // (a few chunks ahead of the compute stream's work, not all at once:
        for (; queued < nch && queued < upto; ++queued) {               //  the runtime batches what it is given in one go)
            // (a copy takes the first 64 bytes of the next chunk along -- a key reads that far ahead --, so level 1 of a chunk
            //  can start as soon as the chunk itself is there: behind the last copy one chunk's level 1 is left, not two)
            //  -- and a copy starts behind the 64 bytes its predecessor delivered: no byte is written twice while level 1 reads it)
            const size_t off = coff[queued] + (queued ? 64 : 0), end = std::min(coff[queued + 1] + 64, n);
            if (end > off) HIP_TRY(hipMemcpyAsync(d_text + off, text + off, end - off, hipMemcpyHostToDevice, c.copy_stream));
            HIP_TRY(hipEventRecord(c.ev_chunk[queued], c.copy_stream));
            (void)hipStreamQuery(c.copy_stream);                        // (submit now)
        }
    };
    bool pre_on = false;
    for (size_t q = 0; q < nch; ++q) {
        const size_t off = coff[q], len = coff[q + 1] - off;
        queue_copies(q + 4);
        HIP_TRY(hipStreamWaitEvent(c.stream, c.ev_chunk[q], 0));
        text_histogram_add(c, d_text + off, len, d_hist);
        if (q == 0 && try_pre) {
            u32 h0[256];
            c.read_n(d_hist, h0, 256);                                 // (waits for chunk 0 only; chunks 1 .. 3 are on their way)
            pre_on = wsort_pre_begin(c, *c.wpre, d_text, n, coff.data(), (u32)nch, h0);
            if (!pre_on) c.arena.release_top();
        }
        if (pre_on) wsort_pre_chunk(c, *c.wpre, (u32)q);
    }
    text_histogram_finish(c, d_text, n, d_hist);
    if (pre_on) {
        wsort_pre_finish(c, *c.wpre, c.hist_cache);
        if (!c.wpre->active) c.arena.release_top();                      // chunk 0 did not show every byte value: the classic order of things
    }
    return d_text;
}

// malloc'd host buffer that is freed unless release()d: the factor arrays handed to the caller are allocated before the last
// synchronisation, and an error surfacing there must not leak them
struct HostBuf {
    void* p = nullptr;
    explicit HostBuf(size_t bytes) : p(malloc(bytes ? bytes : 1)) { if (!p) throw std::bad_alloc(); }
    ~HostBuf() { free(p); }
    template <typename T> T* release() { T* r = (T*)p; p = nullptr; return r; }
    HostBuf(const HostBuf&) = delete;
    HostBuf& operator=(const HostBuf&) = delete;
};

void download_factors(Ctx& c, size_t n, const FactorSpace& fs, Events& ev, uint32_t** pos, uint32_t** src, uint32_t** len, size_t* z) {
    u32* d_pos = c.arena.get<u32>(n), *d_src = c.arena.get<u32>(n), *d_len = c.arena.get<u32>(n);
    const size_t cnt = extract_factors(c, n, fs, d_pos, d_src, d_len, n);
    HostBuf hp(cnt * 4), hs(cnt * 4), hl(cnt * 4);
    if (cnt) {
        HIP_TRY(hipMemcpyAsync(hp.p, d_pos, cnt * 4, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipMemcpyAsync(hs.p, d_src, cnt * 4, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipMemcpyAsync(hl.p, d_len, cnt * 4, hipMemcpyDeviceToHost, c.stream));
    }
    ev.finish();
    *pos = hp.release<uint32_t>(); *src = hs.release<uint32_t>(); *len = hl.release<uint32_t>(); *z = cnt;
}

}  // namespace tdc

namespace {
// whole pipeline on a device-resident text; output written to *d_out (8-byte aligned, capacity out_cap); if *d_out is
// NULL the buffer is taken from the arena once the factorization scratch has been released
size_t run_pipeline(Ctx& c, const u8* d_text, size_t n, u32 threshold, int flatten, int coder, u8** d_out_io, size_t out_cap,
                    tdc_gpu_stats* st, Events& ev, int strategy = 0) {
    if (threshold == 0) throw ArgError{TDC_GPU_ERR_ARG, "threshold must be >= 1"};
    validate_device_text(c, d_text, n);
    DevArrays A;
    const int enc_coder = lcpcomp_enc_coder(coder);
    const CandWant cw{threshold, early_is_planned(c, n, threshold, flatten, strategy, enc_coder, d_text) && c.flen_bytes};
    run_textds(c, d_text, n, A, st, &ev, strategy != TDC_GPU_COMP_ARRAYS, strategy == TDC_GPU_COMP_ARRAYS ? &cw : nullptr);
    run_factorize(c, n, A, threshold, flatten, st, &ev, strategy, enc_coder, d_text);
    EncodeStats es;
    if (!*d_out_io && A.early) *d_out_io = encode_early_out(A.early, &out_cap);       // (reserved in front of the flatten ranges, whose packs wrote it)
    if (!*d_out_io) { out_cap = align_up(encode_bound_coder(n, enc_coder) + 16, 8); *d_out_io = c.arena.get<u8>(out_cap); }
    u8* d_out = *d_out_io;
    const int e0 = ev.tick();
    const size_t out_len = encode_stream(c, d_text, n, A.fs, enc_coder, d_out, out_cap, &es, A.early);
    const int e1 = ev.tick();
    HIP_TRY(hipStreamSynchronize(c.stream));
    if (st) {
        st->n = n; st->out_len = out_len;
        st->flen_min = es.flen_min; st->flen_max = es.flen_max; st->fdist_max = es.fdist_max; st->sigma = es.sigma;
        ev.span(&st->ms_encode, e0, e1);
        st->arena_bytes = c.arena.high;
    }
    return out_len;
}

// Host buffers in, host buffer out: H2D, (escape,) the whole pipeline, D2H.  The output goes where the sink says; copies from / to
// pinned memory (tdc_gpu_host_alloc) run at PCIe speed, pageable memory is staged by the runtime.
void compress_host(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, bool raw, uint32_t threshold, int flatten, int coder, int comp,
                   Sink s, tdc_gpu_stats* stats) {
    (void)lcpcomp_enc_coder(coder);
    if (comp != TDC_GPU_COMP_ARRAYS && comp != TDC_GPU_COMP_PLCPPEAKS && comp != TDC_GPU_COMP_MAXLCP && comp != TDC_GPU_COMP_HEAP)
        throw ArgError{TDC_GPU_ERR_UNSUPPORTED, "lcpcomp: comp must be arrays, plcppeaks, max_lcp or heap"};
    sink_check(s, "out/out_len is NULL");
    if (raw) {
        if (!text && n) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
        if (n >= 0x7FFFFFFEull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "raw input too large: the escaped text must stay < 2^31 - 1 bytes"};
    } else {
        check_host_text(text, n);
    }
    Ctx& c = ctx->c;
    if (stats) memset(stats, 0, sizeof(*stats));
    // raw input: sized for a text without escapes first; the 0x00 / 0xFF bytes are counted on the device after the upload
    reserve_arena(c, raw ? arena_need(c, n + 1) + n + 64 : arena_need(c, n));
    Events ev(c);
    const int e0 = ev.tick();
    TextUpload up(c);
    u8* d_text;
    size_t tn = n;
    if (raw) {
        u8* d_raw = upload_plain(c, text, n);
        tn = n + count_escapes_device(c, d_raw, n) + 1;
        if (tn >= 0x7FFFFFFFull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "raw input too large: the escaped text must stay < 2^31 - 1 bytes"};
        if (c.arena.size < arena_need(c, tn) + n + 64) {                        // many escapes: a larger arena, upload once more
            HIP_TRY(hipStreamSynchronize(c.stream));
            reserve_arena(c, arena_need(c, tn) + n + 64);
            d_raw = upload_plain(c, text, n);
        }
        d_text = c.arena.get<u8>(tn + 64);
        if (escape_device(c, d_raw, n, d_text) != tn) throw HipError{hipErrorUnknown, "escape: length mismatch", (int)__LINE__};
    } else {
        d_text = up.send(text, n);
    }
    const int e1 = ev.tick();
    u8* d_out = nullptr;
    struct SinkGuard {       // on every exit path the sink is forgotten (guarded() waits for a copy into it that is still in flight)
        Ctx& c;
        ~SinkGuard() { c.d2h_host = nullptr; c.d2h_cap = 0; c.d2h_done = 0; }
    } sink_guard{c};
    // the encoder may start the D2H while it still packs -- into the caller's buffer only (a malloc'd one is pageable and not there yet)
    c.d2h_host = s.into; c.d2h_cap = s.into ? s.cap : 0; c.d2h_done = 0;
    const size_t len = run_pipeline(c, d_text, tn, threshold, flatten, coder, &d_out, 0, stats, ev, comp);
    const int e2 = ev.tick();
    *s.out_len = len;
    sink_fit(s, len);
    if (stats) ev.span(&stats->ms_h2d, e0, e1);
    if (s.keep) {
        if (stats) ev.span(&stats->ms_total, e0, e2);
        ev.finish();
        ctx->kept = d_out; ctx->kept_len = len;
        return;
    }
    const size_t done = c.d2h_done <= len ? c.d2h_done : 0;                 // (0 unless the sink is the caller's buffer)
    if (stats) stats->d2h_early = done;
    HIP_TRY(hipMemcpyAsync(sink_host(s, len) + done, d_out + done, len - done, hipMemcpyDeviceToHost, c.stream));
    if (done) {                                                             // the front part travels on a side stream
        c.wait_for(c.stream, c.copy_stream);
        if (c.aux_stream) c.wait_for(c.stream, c.aux_stream);
    }
    const int e3 = ev.tick();
    if (stats) { ev.span(&stats->ms_d2h, e2, e3); ev.span(&stats->ms_total, e0, e3); }
    ev.finish();
    sink_commit(s, len);
}
}  // namespace

extern "C" {

size_t tdc_gpu_lcpcomp_bound(size_t n) { return align_up(encode_bound(n) + 16, 8); }
size_t tdc_gpu_lcpcomp_bound_coder(size_t n, int coder) {
    try { return align_up(encode_bound_coder(n, lcpcomp_enc_coder(coder)) + 16, 8); } catch (...) { return 0; }
}

int tdc_gpu_lcpcomp_compress_dev(tdc_gpu_ctx* ctx, const void* d_text, size_t n, uint32_t threshold, int flatten, int coder,
                                 void* d_out, size_t out_cap, size_t* out_len, tdc_gpu_stats* stats) {
    return guarded(ctx, [&] {
        (void)lcpcomp_enc_coder(coder);
        check_text_args(d_text, n);
        if (!d_out || !out_len || ((uintptr_t)d_out & 7)) throw ArgError{TDC_GPU_ERR_ARG, "d_out must be non-NULL and 8-byte aligned"};
        Ctx& c = ctx->c;
        if (stats) memset(stats, 0, sizeof(*stats));
        reserve_arena(c, arena_need(c, n));
        Events ev(c);
        const int e0 = ev.tick();
        u8* dst = (u8*)d_out;
        *out_len = run_pipeline(c, (const u8*)d_text, n, threshold, flatten, coder, &dst, out_cap, stats, ev);
        const int e1 = ev.tick();
        if (stats) ev.span(&stats->ms_total, e0, e1);
        ev.finish();
    });
}

int tdc_gpu_lcpcomp_compress(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint32_t threshold, int flatten, int coder,
                             uint8_t** out, size_t* out_len, tdc_gpu_stats* stats) {
    return guarded(ctx, [&] { compress_host(ctx, text, n, false, threshold, flatten, coder, TDC_GPU_COMP_ARRAYS, sink_malloc(out, out_len), stats); });
}

int tdc_gpu_lcpcomp_compress_comp(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint32_t threshold, int flatten, int coder,
                                  int comp, uint8_t** out, size_t* out_len, tdc_gpu_stats* stats) {
    return guarded(ctx, [&] { compress_host(ctx, text, n, false, threshold, flatten, coder, comp, sink_malloc(out, out_len), stats); });
}

int tdc_gpu_lcpcomp_compress_into(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint32_t threshold, int flatten, int coder,
                                  int comp, uint8_t* out, size_t out_cap, size_t* out_len, tdc_gpu_stats* stats) {
    return guarded(ctx, [&] { compress_host(ctx, text, n, false, threshold, flatten, coder, comp, sink_into(out, out_cap, out_len), stats); });
}

int tdc_gpu_lcpcomp_compress_keep(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint32_t threshold, int flatten, int coder,
                                  int comp, size_t* out_len, tdc_gpu_stats* stats) {
    return guarded(ctx, [&] { compress_host(ctx, text, n, false, threshold, flatten, coder, comp, sink_keep(out_len), stats); });
}

int tdc_gpu_lcpcomp_compress_raw(tdc_gpu_ctx* ctx, const uint8_t* data, size_t n, uint32_t threshold, int flatten, int coder,
                                 uint8_t** out, size_t* out_len, tdc_gpu_stats* stats) {
    return guarded(ctx, [&] { compress_host(ctx, data, n, true, threshold, flatten, coder, TDC_GPU_COMP_ARRAYS, sink_malloc(out, out_len), stats); });
}

// the stream kept by tdc_gpu_lcpcomp_compress_keep, to host or device memory; guarded() forgets it like every call, so it is put back
// afterwards (it may be fetched again)
static int stream_fetch(tdc_gpu_ctx* ctx, void* dst, size_t cap, size_t* len, hipMemcpyKind kind) {
    if (!ctx) return TDC_GPU_ERR_ARG;
    const u8* kept = ctx->kept;
    const size_t kept_len = ctx->kept_len;
    const int rc = guarded(ctx, [&] {
        if (!kept) throw ArgError{TDC_GPU_ERR_ARG, "no stream is kept on this context (tdc_gpu_lcpcomp_compress_keep, and no other call since)"};
        if (len) *len = kept_len;
        if (!dst || cap < kept_len) throw ArgError{TDC_GPU_ERR_OOM, "destination too small (*len holds the stream length)"};
        if (kept_len) HIP_TRY(hipMemcpyAsync(dst, kept, kept_len, kind, ctx->c.stream));
        HIP_TRY(hipStreamSynchronize(ctx->c.stream));
    });
    ctx->kept = kept; ctx->kept_len = kept_len;
    return rc;
}
int tdc_gpu_stream_fetch(tdc_gpu_ctx* ctx, uint8_t* dst, size_t cap, size_t* len) { return stream_fetch(ctx, dst, cap, len, hipMemcpyDeviceToHost); }
int tdc_gpu_stream_fetch_dev(tdc_gpu_ctx* ctx, void* d_dst, size_t cap, size_t* len) { return stream_fetch(ctx, d_dst, cap, len, hipMemcpyDeviceToDevice); }

}  // extern "C"

// ---- lzss_lcp, lz78, lzw ------------------------------------------------------------------------------------------------------------------
namespace {
// shared front end of the two lzss_lcp entry points: text to the device, SA + ISA, factorization into position space
u8* run_lzss_lcp(Ctx& c, const uint8_t* text, size_t n, uint32_t threshold, DevArrays& A, tdc_gpu_stats* st, Events& ev) {
    if (threshold == 0) throw ArgError{TDC_GPU_ERR_ARG, "threshold must be >= 1"};
    reserve_arena(c, arena_need(c, n));
    u8* d_text = upload_plain(c, text, n);
    validate_device_text(c, d_text, n);
    A.sa = c.arena.get<u32>(n);
    A.isa = c.arena.get<u32>(n);
    A.fs.flen = c.arena.get<u32>(n); A.fs.owner = c.arena.get<u32>(n); A.fs.fsrc = c.arena.get<u32>(n);
    SAStats ss;
    const int e0 = ev.tick();
    build_suffix_array(c, d_text, n, A.sa, A.isa, &ss);
    const int e1 = ev.tick();
    LzssStats ls;
    lzss_lcp_factorize(c, d_text, n, A.sa, A.isa, threshold, A.fs, &ls);
    const int e2 = ev.tick();
    if (st) {
        st->n = n; st->factors = ls.factors;
        sa_stats(st, ss, nullptr);
        ev.span(&st->ms_sa, e0, e1); ev.span(&st->ms_factorize, e1, e2);
    }
    return d_text;
}

// public coder id -> coder id of encode_stream for the coders LZSSLCPCompressor is registered with (etc/registry_config.py:33-34); -1: none
int lzss_lcp_enc_coder(int coder) {
    switch (coder) {
        case TDC_GPU_CODER_HUFF: return 0;
        case TDC_GPU_CODER_ASCII: return 2;
        case TDC_GPU_CODER_BIT: return 4;
        case TDC_GPU_CODER_GAMMA: return 5;
        case TDC_GPU_CODER_DELTA: return 6;
        default: return -1;
    }
}

void lzss_lcp_compress(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint32_t threshold, int coder, Sink s, tdc_gpu_stats* stats) {
    const int enc = lzss_lcp_enc_coder(coder);
    if (enc < 0) throw ArgError{TDC_GPU_ERR_UNSUPPORTED, "lzss_lcp: coder must be huff, bit, gamma, delta or ascii"};
    check_host_text(text, n);
    sink_check(s, "out/out_len is NULL");
    Ctx& c = ctx->c;
    if (stats) memset(stats, 0, sizeof(*stats));
    Events ev(c);
    DevArrays A;
    const int e0 = ev.tick();
    const u8* d_text = run_lzss_lcp(c, text, n, threshold, A, stats, ev);
    const size_t cap = tdc_gpu_lzss_lcp_bound(n, coder);                    // the stream's worst case is what the device buffer is sized by
    u8* d_out = c.arena.get<u8>(cap);
    EncodeStats es;
    const int e1 = ev.tick();
    const size_t len = encode_stream(c, d_text, n, A.fs, enc, d_out, cap, &es);
    const int e2 = ev.tick();
    *s.out_len = len;
    sink_fit(s, len);
    sink_download(c, s, d_out, len);
    const int e3 = ev.tick();
    if (stats) {
        stats->out_len = len; stats->flen_min = es.flen_min; stats->flen_max = es.flen_max; stats->fdist_max = es.fdist_max;
        stats->sigma = es.sigma; stats->arena_bytes = c.arena.high;
        ev.span(&stats->ms_encode, e1, e2); ev.span(&stats->ms_d2h, e2, e3); ev.span(&stats->ms_total, e0, e3);
    }
    ev.finish();
    sink_commit(s, len);
}
}  // namespace

extern "C" {

size_t tdc_gpu_lzss_lcp_bound(size_t n, int coder) {
    const int enc = lzss_lcp_enc_coder(coder);
    if (enc < 0) return 0;
    if (enc >= 4) return align_up(encode_bound_uni(n, enc) + 16, 8);       // (encode.hip: the worst case per coder; + 16: the pack's last word)
    return align_up(encode_bound_coder(n, enc) + 16, 8);
}

int tdc_gpu_lzss_lcp_compress(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint32_t threshold, int coder,
                              uint8_t** out, size_t* out_len, tdc_gpu_stats* stats) {
    return guarded(ctx, [&] { lzss_lcp_compress(ctx, text, n, threshold, coder, sink_malloc(out, out_len), stats); });
}

int tdc_gpu_lzss_lcp_compress_into(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint32_t threshold, int coder,
                                   uint8_t* out, size_t out_cap, size_t* out_len, tdc_gpu_stats* stats) {
    return guarded(ctx, [&] { lzss_lcp_compress(ctx, text, n, threshold, coder, sink_into(out, out_cap, out_len), stats); });
}

int tdc_gpu_lzss_lcp_factorize(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint32_t threshold,
                               uint32_t** pos, uint32_t** src, uint32_t** len, size_t* z) {
    return guarded(ctx, [&] {
        check_host_text(text, n);
        if (!pos || !src || !len || !z) throw ArgError{TDC_GPU_ERR_ARG, "output pointer is NULL"};
        Ctx& c = ctx->c;
        Events ev(c);
        DevArrays A;
        run_lzss_lcp(c, text, n, threshold, A, nullptr, ev);
        download_factors(c, n, A.fs, ev, pos, src, len, z);
    });
}

int tdc_gpu_lz78_compress(tdc_gpu_ctx* ctx, const uint8_t* in, size_t n, int coder, uint8_t** out, size_t* out_len,
                          tdc_gpu_stats* stats) {
    return guarded(ctx, [&] {
        if (coder != TDC_GPU_CODER_GAMMA) throw ArgError{TDC_GPU_ERR_UNSUPPORTED, "lz78: only coder=gamma is built"};
        Sink s = sink_malloc(out, out_len);
        if (!in && n) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
        sink_check(s, "NULL argument");
        if (n >= 0xFFFFFFFFull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "lz78: input must be < 2^32 bytes"};
        Ctx& c = ctx->c;
        if (stats) memset(stats, 0, sizeof(*stats));
        std::vector<u32> ids;
        std::vector<u8> chars;
        bool high = false;
        const size_t z = lz78_parse_host(in, n, ids, chars, &high);
        if (high) throw ArgError{TDC_GPU_ERR_UNSUPPORTED,
            "lz78: the left-over phrase ends in a byte >= 0x80; the reference encodes it as a signed char (undefined shifts) -- not reproduced"};
        // arena: pairs (5 B each) + tile sums + worst-case output (2*33+2*9 bits = 84 bits < 11 B per pair)
        const size_t cap = align_up(z * 11 + 64, 8);
        reserve_arena(c, z * 5 + cap + ((size_t)64 << 20));
        Events ev(c);
        const int e0 = ev.tick();
        u32* d_ids = c.arena.get<u32>(z + 1);
        u8* d_chars = c.arena.get<u8>(z + 8);
        u8* d_out = c.arena.get<u8>(cap);
        if (z) {
            HIP_TRY(hipMemcpyAsync(d_ids, ids.data(), z * 4, hipMemcpyHostToDevice, c.stream));
            HIP_TRY(hipMemcpyAsync(d_chars, chars.data(), z, hipMemcpyHostToDevice, c.stream));
        }
        const int e1 = ev.tick();
        const size_t len = lz78_gamma_encode(c, d_ids, d_chars, z, d_out, cap);
        const int e2 = ev.tick();
        sink_download(c, s, d_out, len);
        const int e3 = ev.tick();
        if (stats) {
            stats->n = n; stats->out_len = len; stats->factors = z; stats->arena_bytes = c.arena.high;
            ev.span(&stats->ms_h2d, e0, e1); ev.span(&stats->ms_encode, e1, e2); ev.span(&stats->ms_d2h, e2, e3); ev.span(&stats->ms_total, e0, e3);
        }
        ev.finish();
        sink_commit(s, len);
    });
}

int tdc_gpu_lzw_compress(tdc_gpu_ctx* ctx, const uint8_t* in, size_t n, int coder, uint8_t** out, size_t* out_len,
                         tdc_gpu_stats* stats) {
    return guarded(ctx, [&] {
        if (coder != TDC_GPU_CODER_BIT && coder != TDC_GPU_CODER_GAMMA) throw ArgError{TDC_GPU_ERR_UNSUPPORTED, "lzw: only coder=bit and coder=gamma are built"};
        Sink s = sink_malloc(out, out_len);
        if (!in && n) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
        sink_check(s, "NULL argument");
        if (n >= 0xFFFFFF00ull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "lzw: input must be < 2^32 - 256 bytes"};
        Ctx& c = ctx->c;
        if (stats) memset(stats, 0, sizeof(*stats));
        std::vector<u32> codes;
        const size_t z = lzw_parse_host(in, n, codes);
        // arena: codes (4 B each) + tile sums + worst-case output (bit: 33 bits, gamma: 2 * 32 + 1 bits: < 9 B per code)
        const size_t cap = align_up(z * 9 + 64, 8);
        reserve_arena(c, z * 4 + cap + ((size_t)64 << 20));
        Events ev(c);
        const int e0 = ev.tick();
        u32* d_codes = c.arena.get<u32>(z + 1);
        u8* d_out = c.arena.get<u8>(cap);
        if (z) HIP_TRY(hipMemcpyAsync(d_codes, codes.data(), z * 4, hipMemcpyHostToDevice, c.stream));
        const int e1 = ev.tick();
        const size_t len = lzw_encode(c, d_codes, z, coder == TDC_GPU_CODER_BIT, d_out, cap);
        const int e2 = ev.tick();
        sink_download(c, s, d_out, len);
        const int e3 = ev.tick();
        if (stats) {
            stats->n = n; stats->out_len = len; stats->factors = z; stats->arena_bytes = c.arena.high;
            ev.span(&stats->ms_h2d, e0, e1); ev.span(&stats->ms_encode, e1, e2); ev.span(&stats->ms_d2h, e2, e3); ev.span(&stats->ms_total, e0, e3);
        }
        ev.finish();
        sink_commit(s, len);
    });
}

}  // extern "C"

// ---- lzss (LZSSSlidingWindowCompressor; lzss_sw.hip) ------------------------------------------------------------
namespace {
// public coder id -> kind of lzss_sw_encode_tokens for the coders the reference registers lzss with (etc/registry_config.py:13-18,236); -1: none
int lzss_sw_kind(int coder) {
    switch (coder) {
        case TDC_GPU_CODER_BIT: return 0;
        case TDC_GPU_CODER_ASCII: return 1;
        case TDC_GPU_CODER_GAMMA: return 2;
        case TDC_GPU_CODER_DELTA: return 3;
        default: return -1;
    }
}
void lzss_sw_check(const uint8_t* in, size_t n, uint32_t window) {
    if (!in && n) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
    if (window == 0) throw ArgError{TDC_GPU_ERR_ARG, "lzss: window must be >= 1"};
    if (window > LZSS_SW_MAX_WINDOW) throw ArgError{TDC_GPU_ERR_UNSUPPORTED, "lzss: windows above 4096 are not built"};
    if (n > 0xFFFFFFFEull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "lzss: input must be at most 2^32 - 2 bytes"};
}
// text (n + 64), next / factor / two scratch words and the mark per position (17 n) and what comes behind them: the stream's worst case,
// or the factor lists (three words and a class byte per token, at most n tokens)
size_t lzss_sw_arena(size_t n, size_t behind) { return 18 * n + behind + ((size_t)64 << 20); }

void lzss_sw_compress(tdc_gpu_ctx* ctx, const uint8_t* in, size_t n, uint32_t window, uint32_t threshold, int coder, Sink s, tdc_gpu_stats* stats) {
    const int kind = lzss_sw_kind(coder);
    if (kind < 0) throw ArgError{TDC_GPU_ERR_UNSUPPORTED, "lzss: coder must be ascii, bit, gamma or delta"};
    lzss_sw_check(in, n, window);
    sink_check(s, "NULL argument");
    Ctx& c = ctx->c;
    if (stats) memset(stats, 0, sizeof(*stats));
    const size_t cap = align_up(lzss_sw_bound(n, window, kind) + 16, 8);       // (+ 16: the pack's last word)
    reserve_arena(c, lzss_sw_arena(n, cap));
    Events ev(c);
    const int e0 = ev.tick();
    const u8* d_text = upload_plain(c, in, n);
    const int e1 = ev.tick();
    u32* tokpos = nullptr, *fac = nullptr;
    const size_t ntok = lzss_sw_tokens(c, d_text, n, window, threshold, &tokpos, &fac);
    const int e2 = ev.tick();
    u8* d_out = c.arena.get<u8>(cap);
    LzssSwStats ls;
    const size_t len = lzss_sw_encode_tokens(c, d_text, tokpos, fac, ntok, window, kind, d_out, cap, &ls);
    if (ls.truncates) throw ArgError{TDC_GPU_ERR_UNSUPPORTED,
        "lzss(coder=bit): a factor is longer than bits_for(window) bits hold; the reference truncates it and decodes another text -- not reproduced"};
    const int e3 = ev.tick();
    *s.out_len = len;
    sink_fit(s, len);
    sink_download(c, s, d_out, len);
    const int e4 = ev.tick();
    if (stats) {
        stats->n = n; stats->out_len = len; stats->factors = ls.factors; stats->flen_max = ls.flen_max; stats->arena_bytes = c.arena.high;
        ev.span(&stats->ms_h2d, e0, e1); ev.span(&stats->ms_factorize, e1, e2); ev.span(&stats->ms_encode, e2, e3);
        ev.span(&stats->ms_d2h, e3, e4); ev.span(&stats->ms_total, e0, e4);
    }
    ev.finish();
    sink_commit(s, len);
}
}  // namespace

extern "C" {

size_t tdc_gpu_lzss_sw_bound(size_t n, uint32_t window, int coder) { return lzss_sw_bound(n, window, lzss_sw_kind(coder)); }

int tdc_gpu_lzss_sw_compress(tdc_gpu_ctx* ctx, const uint8_t* in, size_t n, uint32_t window, uint32_t threshold, int coder,
                             uint8_t** out, size_t* out_len, tdc_gpu_stats* stats) {
    return guarded(ctx, [&] { lzss_sw_compress(ctx, in, n, window, threshold, coder, sink_malloc(out, out_len), stats); });
}

int tdc_gpu_lzss_sw_compress_into(tdc_gpu_ctx* ctx, const uint8_t* in, size_t n, uint32_t window, uint32_t threshold, int coder,
                                  uint8_t* out, size_t out_cap, size_t* out_len, tdc_gpu_stats* stats) {
    return guarded(ctx, [&] { lzss_sw_compress(ctx, in, n, window, threshold, coder, sink_into(out, out_cap, out_len), stats); });
}

int tdc_gpu_lzss_sw_factorize(tdc_gpu_ctx* ctx, const uint8_t* in, size_t n, uint32_t window, uint32_t threshold,
                              uint32_t** pos, uint32_t** src, uint32_t** len, size_t* z) {
    return guarded(ctx, [&] {
        lzss_sw_check(in, n, window);
        if (!pos || !src || !len || !z) throw ArgError{TDC_GPU_ERR_ARG, "output pointer is NULL"};
        Ctx& c = ctx->c;
        reserve_arena(c, lzss_sw_arena(n, 13 * n));
        Events ev(c);
        const u8* d_text = upload_plain(c, in, n);
        u32* tokpos = nullptr, *fac = nullptr;
        const size_t ntok = lzss_sw_tokens(c, d_text, n, window, threshold, &tokpos, &fac);
        u32* d_pos = c.arena.get<u32>(ntok + 1), *d_src = c.arena.get<u32>(ntok + 1), *d_len = c.arena.get<u32>(ntok + 1);
        const size_t cnt = lzss_sw_factor_list(c, tokpos, fac, ntok, d_pos, d_src, d_len);
        HostBuf hp(cnt * 4), hs(cnt * 4), hl(cnt * 4);
        if (cnt) {
            HIP_TRY(hipMemcpyAsync(hp.p, d_pos, cnt * 4, hipMemcpyDeviceToHost, c.stream));
            HIP_TRY(hipMemcpyAsync(hs.p, d_src, cnt * 4, hipMemcpyDeviceToHost, c.stream));
            HIP_TRY(hipMemcpyAsync(hl.p, d_len, cnt * 4, hipMemcpyDeviceToHost, c.stream));
        }
        ev.finish();
        *pos = hp.release<uint32_t>(); *src = hs.release<uint32_t>(); *len = hl.release<uint32_t>(); *z = cnt;
    });
}

}  // extern "C"

// ---- lzss over a batch of texts (lzss_sw_batch.hip, DESIGN.md section 5.7 "Batches") ----------------------------------------------------
namespace {
// what can be said of the arguments without a device; throws ArgError
void lzss_sw_batch_check(const uint8_t* in, const uint64_t* in_off, size_t count, uint32_t window, int coder, const uint8_t* out,
                         const uint64_t* out_off, const uint64_t* out_len, const int32_t* status) {
    if (!in_off || !out_off || (count && (!out || !out_len || !status))) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
    if (lzss_sw_kind(coder) < 0) throw ArgError{TDC_GPU_ERR_UNSUPPORTED, "lzss: coder must be ascii, bit, gamma or delta"};
    if (window == 0) throw ArgError{TDC_GPU_ERR_ARG, "lzss: window must be >= 1"};
    if (window > LZSS_SW_MAX_WINDOW) throw ArgError{TDC_GPU_ERR_UNSUPPORTED, "lzss: windows above 4096 are not built"};
    if (in_off[0] != 0) throw ArgError{TDC_GPU_ERR_ARG, "lzss batch: in_off[0] must be 0"};
    for (size_t k = 0; k < count; ++k)
        if (in_off[k + 1] < in_off[k]) throw ArgError{TDC_GPU_ERR_ARG, "lzss batch: in_off must not decrease"};
    if (in_off[count] > 0xFFFFFFFEull || count > 0xFFFFFFFEull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "lzss batch: the texts must be at most 2^32 - 2 bytes in all"};
    if (!in && in_off[count]) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
}
// the single bounds, each rounded up to 8, summed; 0 where one of them is 0 (window and kind are valid here)
size_t lzss_sw_batch_bound_sum(const uint64_t* in_off, size_t count, uint32_t window, int kind) {
    size_t sum = 0;
    for (size_t k = 0; k < count; ++k) {
        const size_t b = in_off[k + 1] >= in_off[k] ? lzss_sw_bound((size_t)(in_off[k + 1] - in_off[k]), window, kind) : 0;
        if (!b) return 0;
        sum += align_up(b, 8);
    }
    return sum;
}

void lzss_sw_compress_batch(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* in_off, size_t count, uint32_t window, uint32_t threshold,
                            int coder, uint8_t* out, size_t out_cap, uint64_t* out_off, uint64_t* out_len, int32_t* status, tdc_gpu_stats* stats) {
    const int kind = lzss_sw_kind(coder);
    Ctx& c = ctx->c;
    if (stats) memset(stats, 0, sizeof(*stats));
    out_off[0] = 0;
    if (count == 0) return;
    const size_t n = (size_t)in_off[count];
    std::vector<u32> off32(count + 1);
    for (size_t k = 0; k <= count; ++k) off32[k] = (u32)in_off[k];
    // per byte as the single call (the worst case of the output behind the position arrays), 24 bytes per text
    reserve_arena(c, lzss_sw_arena(n, lzss_sw_batch_bound_sum(in_off, count, window, kind) + 16) + 24 * (count + 1) + 4096);
    Events ev(c);
    const int e0 = ev.tick();
    const u8* d_text = upload_plain(c, in, n);
    LzssSwBatch B;
    u32* d_off = c.arena.get<u32>(count + 1);
    B.off = d_off; B.gfirst = c.arena.get<u64>(count + 1); B.ooff = c.arena.get<u64>(count + 1); B.flag = c.arena.get<u32>(count);
    HIP_TRY(hipMemcpyAsync(d_off, off32.data(), (count + 1) * sizeof(u32), hipMemcpyHostToDevice, c.stream));
    const int e1 = ev.tick();
    lzss_sw_batch_sizes(c, d_text, n, count, window, threshold, kind, B);
    // the sizes: where every stream goes, its bits, and the texts BitCoder would truncate
    std::vector<u64> gfirst(count + 1);
    std::vector<u32> flag(count);
    c.read_n(B.ooff, (u64*)out_off, count + 1);
    c.read_n(B.gfirst, gfirst.data(), count + 1);
    c.read_n(B.flag, flag.data(), count);
    for (size_t k = 0; k < count; ++k) {
        status[k] = flag[k] ? TDC_GPU_ERR_UNSUPPORTED : TDC_GPU_OK;
        out_len[k] = flag[k] ? 0 : bit_stream_len(gfirst[k + 1] - gfirst[k]);
    }
    const int e2 = ev.tick();
    const size_t used = (size_t)out_off[count];
    if (used > out_cap) throw ArgError{TDC_GPU_ERR_OOM, "lzss batch: output buffer too small (out_off[count] holds the required size)"};
    u8* d_out = c.arena.get<u8>(used + 8);
    lzss_sw_batch_pack(c, d_text, count, window, kind, B, d_out, used);
    const int e3 = ev.tick();
    if (used) HIP_TRY(hipMemcpyAsync(out, d_out, used, hipMemcpyDeviceToHost, c.stream));
    const int e4 = ev.tick();
    if (stats) {
        stats->n = n; stats->out_len = used; stats->factors = B.factors; stats->arena_bytes = c.arena.high;
        ev.span(&stats->ms_h2d, e0, e1); ev.span(&stats->ms_factorize, e1, e2); ev.span(&stats->ms_encode, e2, e3);
        ev.span(&stats->ms_d2h, e3, e4); ev.span(&stats->ms_total, e0, e4);
    }
    ev.finish();
}
}  // namespace

extern "C" {

size_t tdc_gpu_lzss_sw_batch_bound(const uint64_t* in_off, size_t count, uint32_t window, int coder) {
    const int kind = lzss_sw_kind(coder);
    if (!in_off || in_off[0] != 0 || kind < 0 || window == 0 || window > LZSS_SW_MAX_WINDOW) return 0;
    const size_t sum = lzss_sw_batch_bound_sum(in_off, count, window, kind);
    return in_off[count] > 0xFFFFFFFEull ? 0 : sum;
}

int tdc_gpu_lzss_sw_compress_batch(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* in_off, size_t count, uint32_t window, uint32_t threshold,
                                   int coder, uint8_t* out, size_t out_cap, uint64_t* out_off, uint64_t* out_len, int32_t* status,
                                   tdc_gpu_stats* stats) {
    try { lzss_sw_batch_check(in, in_off, count, window, coder, out, out_off, out_len, status); }      // (before the context: no device needed)
    catch (const ArgError& e) { if (ctx) ctx->last_error = e.msg; return e.code; }
    return guarded(ctx, [&] { lzss_sw_compress_batch(ctx, in, in_off, count, window, threshold, coder, out, out_cap, out_off, out_len, status, stats); });
}

}  // extern "C"

// ---- repair (RePairCompressor; repair.hip) -----------------------------------------------------------------------
namespace {
// public coder id -> kind of repair_encode for the coders that need no literal iterator (etc/registry_config.py:13-18,240); -1: none
int repair_kind(int coder) {
    switch (coder) {
        case TDC_GPU_CODER_BIT: return 0;
        case TDC_GPU_CODER_ASCII: return 1;
        case TDC_GPU_CODER_GAMMA: return 2;
        case TDC_GPU_CODER_DELTA: return 3;
        default: return -1;
    }
}
void repair_check(const uint8_t* in, size_t n) {
    if (!in && n) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
    if (n > REPAIR_MAX_N) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "repair: input must be at most 2^30 bytes"};
}
void repair_fill_stats(tdc_gpu_stats* stats, const RepairStats& rs) {
    stats->rules = rs.rules; stats->replaced = rs.replaced; stats->tie_rounds = rs.tie_rounds; stats->rebuilds = rs.rebuilds;
    stats->ms_round_first = rs.ms_first; stats->ms_round_last = rs.ms_last; stats->ms_round_tie = rs.ms_tie;
}

void repair_compress(tdc_gpu_ctx* ctx, const uint8_t* in, size_t n, uint64_t max_rules, int coder, Sink s, tdc_gpu_stats* stats) {
    const int kind = repair_kind(coder);
    if (kind < 0) throw ArgError{TDC_GPU_ERR_UNSUPPORTED, "repair: coder must be bit, ascii, gamma or delta"};
    repair_check(in, n);
    sink_check(s, "NULL argument");
    Ctx& c = ctx->c;
    if (stats) memset(stats, 0, sizeof(*stats));
    const size_t cap = align_up(repair_bound(n, kind) + 16, 8);                 // (+ 16: the pack's last word)
    reserve_arena(c, n + 64 + repair_arena(c, n, max_rules) + cap);             // before anything is written
    Events ev(c);
    const int e0 = ev.tick();
    const u8* d_text = upload_plain(c, in, n);
    const int e1 = ev.tick();
    u64* d_rules = nullptr; u32* d_start = nullptr;
    RepairStats rs;
    repair_grammar(c, d_text, n, max_rules, &d_rules, &d_start, &rs);
    const int e2 = ev.tick();
    u8* d_out = c.arena.get<u8>(cap);
    const size_t len = repair_encode(c, d_rules, (size_t)rs.rules, d_start, rs.nstart, kind, d_out, cap);
    const int e3 = ev.tick();
    *s.out_len = len;
    sink_fit(s, len);
    sink_download(c, s, d_out, len);
    const int e4 = ev.tick();
    if (stats) {
        stats->n = n; stats->out_len = len; stats->arena_bytes = c.arena.high;
        repair_fill_stats(stats, rs);
        ev.span(&stats->ms_h2d, e0, e1); ev.span(&stats->ms_factorize, e1, e2); ev.span(&stats->ms_encode, e2, e3);
        ev.span(&stats->ms_d2h, e3, e4); ev.span(&stats->ms_total, e0, e4);
    }
    ev.finish();
    sink_commit(s, len);
}
}  // namespace

extern "C" {

size_t tdc_gpu_repair_bound(size_t n, int coder) { return repair_bound(n, repair_kind(coder)); }

int tdc_gpu_repair_compress(tdc_gpu_ctx* ctx, const uint8_t* in, size_t n, uint64_t max_rules, int coder, uint8_t** out, size_t* out_len,
                            tdc_gpu_stats* stats) {
    return guarded(ctx, [&] { repair_compress(ctx, in, n, max_rules, coder, sink_malloc(out, out_len), stats); });
}

int tdc_gpu_repair_compress_into(tdc_gpu_ctx* ctx, const uint8_t* in, size_t n, uint64_t max_rules, int coder, uint8_t* out, size_t out_cap,
                                 size_t* out_len, tdc_gpu_stats* stats) {
    return guarded(ctx, [&] { repair_compress(ctx, in, n, max_rules, coder, sink_into(out, out_cap, out_len), stats); });
}

int tdc_gpu_repair_grammar(tdc_gpu_ctx* ctx, const uint8_t* in, size_t n, uint64_t max_rules, uint64_t** rules, size_t* nrules,
                           uint32_t** start, size_t* nstart, tdc_gpu_stats* stats) {
    return guarded(ctx, [&] {
        repair_check(in, n);
        if (!rules || !nrules || !start || !nstart) throw ArgError{TDC_GPU_ERR_ARG, "output pointer is NULL"};
        Ctx& c = ctx->c;
        if (stats) memset(stats, 0, sizeof(*stats));
        reserve_arena(c, n + 64 + repair_arena(c, n, max_rules));
        Events ev(c);
        const int e0 = ev.tick();
        const u8* d_text = upload_plain(c, in, n);
        u64* d_rules = nullptr; u32* d_start = nullptr;
        RepairStats rs;
        repair_grammar(c, d_text, n, max_rules, &d_rules, &d_start, &rs);
        const int e1 = ev.tick();
        HostBuf hr((size_t)rs.rules * 8), hs(rs.nstart * 4);
        if (rs.rules) HIP_TRY(hipMemcpyAsync(hr.p, d_rules, (size_t)rs.rules * 8, hipMemcpyDeviceToHost, c.stream));
        if (rs.nstart) HIP_TRY(hipMemcpyAsync(hs.p, d_start, rs.nstart * 4, hipMemcpyDeviceToHost, c.stream));
        if (stats) {
            stats->n = n; stats->arena_bytes = c.arena.high;
            repair_fill_stats(stats, rs);
            ev.span(&stats->ms_factorize, e0, e1);
        }
        ev.finish();
        *rules = hr.release<uint64_t>(); *nrules = (size_t)rs.rules; *start = hs.release<uint32_t>(); *nstart = rs.nstart;
    });
}

}  // extern "C"

// ---- bwt over a batch of texts (bwt_batch.hip, DESIGN.md section 5.2 "Batches") ----------------------------------------------------------
extern "C" {

int tdc_gpu_bwt_compress_batch(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* off, size_t count, uint8_t* out, size_t out_cap,
                               int32_t* status, tdc_gpu_stats* stats) {
    try { bwtb_check(in, off, count, out, out_cap, 1, status, 0xFFFFFFFEull); }                       // (before the context: no device needed)
    catch (const ArgError& e) { if (ctx) ctx->last_error = e.msg; return e.code; }
    return guarded(ctx, [&] { bwtb_forward(ctx, in, off, count, out, out_cap, true, nullptr, status, stats); });
}

int tdc_gpu_suffix_array_batch(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* off, size_t count, uint32_t* sa, int32_t* status) {
    try { bwtb_check(in, off, count, sa, SIZE_MAX, 4, status, 0xFFFFFFFEull); }
    catch (const ArgError& e) { if (ctx) ctx->last_error = e.msg; return e.code; }
    return guarded(ctx, [&] { bwtb_forward(ctx, in, off, count, nullptr, 0, false, sa, status, nullptr); });
}

}  // extern "C"
