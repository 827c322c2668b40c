// api.hpp -- what the files of the C ABI layer (api_*.hip: include/tdc_gpu.h on top of the stage functions of stages.hpp) share:
// the context, the frame every entry point runs in (guarded), the output sink, the text on its way to the device.  Host code only.
#pragma once
#include "../../include/tdc_gpu.h"
#include "stages.hpp"
#include "prim.hpp"

#include <new>
#include <string>
#include <stdlib.h>
#include <string.h>

struct tdc_gpu_ctx {
    tdc::Ctx c;
    tdc::WPre pre;              // level 1 of the suffix sort behind the upload (TextUpload); c.wpre points here
    std::string last_error;
    int last_decode_device = 0; // the last decompression parsed its token stream on the device
    const tdc::u8* kept = nullptr;   // tdc_gpu_lcpcomp_compress_keep: the stream of the last call, in the arena (until the next call)
    size_t kept_len = 0;
};

namespace tdc {

struct ArgError { int code; const char* msg; };

// hipSetDevice is a per-thread setting of the embedding program: switch to the context's device for the duration of one
// API call only
struct DeviceGuard {
    int want, prev = -1;
    explicit DeviceGuard(int d) : want(d) {}
    hipError_t enter() {
        if (hipGetDevice(&prev) != hipSuccess) { prev = -1; (void)hipGetLastError(); }
        return prev == want ? hipSuccess : hipSetDevice(want);
    }
    ~DeviceGuard() { if (prev >= 0 && prev != want) (void)hipSetDevice(prev); }
};

// waits for every stream of the context; the first error, if any
inline hipError_t sync_streams(Ctx& c) {
    hipError_t first = hipSuccess;
    for (hipStream_t s : {c.stream, c.copy_stream, c.aux_stream}) {
        const hipError_t e = s ? hipStreamSynchronize(s) : hipSuccess;
        if (first == hipSuccess) first = e;
    }
    return first;
}

// Every call that enqueues device work goes through here, and returns with every stream of its context idle: nothing of it
// still reads the caller's buffers or writes into the arena the next call reuses, whichever way it ended.
template <typename F>
int guarded(tdc_gpu_ctx* ctx, F&& f) {
    if (!ctx) return TDC_GPU_ERR_ARG;
    ctx->last_error.clear();
    ctx->kept = nullptr; ctx->kept_len = 0;      // (every call may reuse the arena)
    ctx->c.hist_ptr = nullptr;                   // the cached byte histogram belongs to ONE call (same address, other text: stale)
    DeviceGuard dg(ctx->c.device);               // the caller's current device is restored on every exit path
    const hipStream_t compute = ctx->c.stream;
    auto drain = [&] { ctx->c.stream = compute; return sync_streams(ctx->c); };
    try {
        HIP_TRY(dg.enter());
        try { f(); } catch (...) { (void)drain(); throw; }
        HIP_TRY(drain());
        if (ctx->c.d_err) {                      // device-side error word (e.g. a look-back that timed out)
            u32 e = 0;
            HIP_TRY(hipMemcpy(&e, ctx->c.d_err, sizeof(u32), hipMemcpyDeviceToHost));
            if (e) {
                HIP_TRY(hipMemset(ctx->c.d_err, 0, sizeof(u32)));
                throw HipError{hipErrorUnknown, "device-side error flag set (radix look-back timeout)", (int)e};
            }
        }
        return TDC_GPU_OK;
    } catch (const HipError& e) {
        char buf[512];
        snprintf(buf, sizeof(buf), "%s (%s:%d)", hipGetErrorString(e.e), e.file, e.line);
        ctx->last_error = buf;
        (void)hipGetLastError();
        if (e.e == hipErrorOutOfMemory) return TDC_GPU_ERR_OOM;
        if (e.e == hipErrorUnknown) return TDC_GPU_ERR_INTERNAL;
        if (e.e == hipErrorInvalidValue && e.line < 0) return TDC_GPU_ERR_UNSUPPORTED;
        return TDC_GPU_ERR_HIP;
    } catch (const ArgError& e) {
        ctx->last_error = e.msg;
        return e.code;
    } catch (const std::bad_alloc&) {
        ctx->last_error = "host allocation failed";
        return TDC_GPU_ERR_OOM;
    } catch (...) {
        ctx->last_error = "unknown exception";
        return TDC_GPU_ERR_INTERNAL;
    }
}

// + 192 MiB: fixed-size scratch (the SLE coder's 2^24-entry k-mer table and its sort buffers are the largest)
inline size_t arena_need(size_t n) { return 112 * n + ((size_t)192 << 20); }
// (a context created with TDC_GPU_WSORT_SMALLRUN -- tests: every run of tying records is handed on -- needs ~48 B per byte more for the
//  hand-over lists; per context, not per process: other contexts of a test run keep the product's budget)
inline size_t arena_need(const Ctx& c, size_t n) { return arena_need(n) + (c.wsort_small ? 64 * n : 0) + (c.wsort_cmax < 16 ? 8 * n : 0); }
// the context's arena for a call; a device that cannot hold it is reported with both numbers instead of a bare allocation failure
void reserve_arena(Ctx& c, size_t bytes);

// public coder id (+ SLE's kmer option in bits 8..) -> coder id of encode_stream
int lcpcomp_enc_coder(int coder);

// ---- the call frame of "host text in" ---------------------------------------------------------------------------------------------
// a text of n bytes, on the host or on the device
inline void check_text_args(const void* text, size_t n) {
    if (!text) throw ArgError{TDC_GPU_ERR_ARG, "text is NULL"};
    if (n == 0) throw ArgError{TDC_GPU_ERR_NO_SENTINEL, "empty view: the text must end with a 0 sentinel"};
    if (n >= 0x7FFFFFFFull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "text length must be < 2^31 - 1 (32-bit len_t)"};
}
// the escaped, 0-terminated view of a host text (what Input::as_view() yields); the 0 bytes inside it are counted on the device
// (validate_device_text)
inline void check_host_text(const uint8_t* text, size_t n) {
    check_text_args(text, n);
    if (text[n - 1] != 0) throw ArgError{TDC_GPU_ERR_NO_SENTINEL, "text does not end with a 0 sentinel"};
}
// Checks that the 0 byte occurs exactly once, at n - 1 (ds/TextDS.hpp:132-138).  The count comes from the byte histogram of the text,
// which the suffix array needs anyway (one pass for both; a host-buffer call has accumulated it behind the upload already).
void validate_device_text(Ctx& c, const u8* d_text, size_t n);

// n bytes of host memory into n + 64 bytes of the arena, on the compute stream
inline u8* upload_plain(Ctx& c, const uint8_t* src, size_t n) {
    u8* d = c.arena.get<u8>(n + 64);
    if (n) HIP_TRY(hipMemcpyAsync(d, src, n, hipMemcpyHostToDevice, c.stream));
    return d;
}

// The text of a host-buffer call on its way to the device (n + 64 bytes from the arena).  Texts of 64 MiB and more travel in chunks on the
// copy stream with device work behind every chunk -- level 1 of the suffix sort among it, whose records sit at the top of the arena.
// Whatever send() started is forgotten again when the object goes, on every exit path of the call: the WPre state and the top of the arena.
struct TextUpload {
    Ctx& c;
    explicit TextUpload(Ctx& ctx) : c(ctx) {}
    u8* send(const uint8_t* text, size_t n);
    ~TextUpload() { if (c.wpre) { c.wpre->active = false; c.wpre->begun = false; } c.arena.release_top(); }
    TextUpload(const TextUpload&) = delete;
    TextUpload& operator=(const TextUpload&) = delete;
};

// Event marks are recorded while the pipeline is enqueued; the elapsed times are only read in finish(), after the
// stream has been synchronised (hipEventElapsedTime on a pending event returns hipErrorNotReady).
struct Events {
    Ctx& c;
    int used = 0;
    struct Span { float* dst; int a, b; };
    Span spans[16];
    int nspans = 0;
    explicit Events(Ctx& ctx) : c(ctx) {}
    int tick() { HIP_TRY(hipEventRecord(c.ev[used], c.stream)); return used++; }
    void span(float* dst, int a, int b) { if (dst) spans[nspans++] = Span{dst, a, b}; }
    void finish() {
        HIP_TRY(hipStreamSynchronize(c.stream));
        for (int i = 0; i < nspans; ++i) HIP_TRY(hipEventElapsedTime(spans[i].dst, c.ev[spans[i].a], c.ev[spans[i].b]));
        nspans = 0;
        c.prof_collect();
    }
};

// what the suffix array reports; ex == NULL (lzss_lcp: built without the wide path's extras): the three fields that path reports
inline void sa_stats(tdc_gpu_stats* st, const SAStats& ss, const SAExtra* ex) {
    st->sa_rounds = ss.rounds; st->sa_init_syms = ss.init_syms; st->sa_sorted_elems = ss.sorted_elems;
    if (!ex) return;
    st->sa_key_words = ss.wide_kw; st->sa_text_rounds = ss.text_rounds; st->sa_mode = (uint32_t)ex->mode; st->sa_overlapped = ss.overlapped;
    st->sa_star_chains = (uint32_t)std::min<u64>(ss.star_chains, 0xFFFFFFFFull);
}

// ---- the text's arrays and its factors (api_compress.hip; the stage-level entry points of api_stages.hip run them one by one) ------
struct DevArrays {
    u32 *sa = nullptr, *isa = nullptr, *phi = nullptr, *plcp = nullptr;
    FactorSpace fs;
    u32 maxlcp = 0;
    CandFused cand;                         // the factorizer's candidates, classified by the fused scatter (run_textds; filled: it did)
    EncodeEarly* early = nullptr;           // first half of the encoder, run inside the flatten stage (run_factorize)
    DevArrays() = default;
    DevArrays(const DevArrays&) = delete;
    DevArrays& operator=(const DevArrays&) = delete;
    ~DevArrays() { encode_early_free(early); }
};
// SA -> ISA -> Phi -> PLCP  (TextDS::require, ds/TextDS.hpp:247-292)
// want_phi = false (lcpcomp with comp=arrays): where the fused scatter runs, Phi is not materialised -- 8-byte instead of 12-byte records
// through its two partition levels; the factorizer takes a factor's source from SA[ISA[p] - 1] (A.phi stays NULL)
// cw (optional): factorize_arrays(threshold) comes next -- where the fused scatter runs without Phi, it classifies the candidates on the
// way (CandFused) and zero-fills the length array the factorizer will use: the byte array (flen8) or the dense one
struct CandWant { u32 threshold; bool flen8; };
void run_textds(Ctx& c, const u8* d_text, size_t n, DevArrays& A, tdc_gpu_stats* st, Events* ev, bool want_phi = true, const CandWant* cw = nullptr);
// enc_coder >= 0 (with d_text): the stream is encoded next with this coder of encode_stream -- the first half of the encoder may run
// inside the flatten stage
void run_factorize(Ctx& c, size_t n, DevArrays& A, u32 threshold, int flatten, tdc_gpu_stats* st, Events* ev, int strategy = 0,
                   int enc_coder = -1, const u8* d_text = nullptr);
// the factor list of fs, sorted by pos, in three malloc'd arrays for the caller (tdc_gpu_free); ends the call's event frame (ev.finish())
void download_factors(Ctx& c, size_t n, const FactorSpace& fs, Events& ev, uint32_t** pos, uint32_t** src, uint32_t** len, size_t* z);

// ---- bwt over a batch of texts (bwt_batch.hip, DESIGN.md section 5.2 "Batches" and "Batch decoder") ----------------------------------------
// the refusals decided from the arguments alone, before the context is looked at (throws ArgError); `out` holds out_cap elements of elem bytes
void bwtb_check(const uint8_t* in, const uint64_t* off, size_t count, const void* out, size_t out_cap, size_t elem, const int32_t* status, u64 total_max);
// the transforms into `out` (want_out) or the suffix arrays into sa_out; the inverse.
// keep != NULL (the batch pipeline, api_chain.hip): nothing is downloaded -- transform k stays in the arena at d_out + off[k] (the range
// of a refused text holds nothing), status[] is filled as ever, and the CALLER has reserved the arena (bwtb_forward_arena and its own)
struct BwtbKeep { u8* d_out = nullptr; };
size_t bwtb_forward_arena(size_t n, size_t count);
void bwtb_forward(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* off, size_t count, uint8_t* out, size_t out_cap, bool want_out, uint32_t* sa_out,
                  int32_t* status, tdc_gpu_stats* stats, BwtbKeep* keep = nullptr);
void bwtb_inverse(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* off, size_t count, uint8_t* out, size_t out_cap, int32_t* status,
                  tdc_gpu_stats* stats);

// ---- the output sink (stages.hpp Sink) ----------------------------------------------------------------------------------------------
// One of these three builds the sink of an entry point from its arguments.
// A malloc'd buffer handed to *out.  null_msg: the decompressing entry points refuse a NULL `out` before they look at anything else;
// the compressing ones check it among their other arguments (sink_check).
inline Sink sink_malloc(uint8_t** out, size_t* out_len, const char* null_msg = nullptr) {
    if (null_msg && !out) throw ArgError{TDC_GPU_ERR_ARG, null_msg};
    Sink s; s.out = out; s.out_len = out_len;
    return s;
}
// the caller's buffer `out` of `cap` bytes (the _into entry points)
inline Sink sink_into(uint8_t* out, size_t cap, size_t* out_len) {
    if (!out) throw ArgError{TDC_GPU_ERR_ARG, "out is NULL"};
    Sink s; s.into = out; s.cap = cap; s.out_len = out_len;
    return s;
}
// nowhere: the stream stays on the device (tdc_gpu_lcpcomp_compress_keep)
inline Sink sink_keep(size_t* out_len) { Sink s; s.keep = true; s.out_len = out_len; return s; }

inline void sink_check(const Sink& s, const char* msg) {
    if (!s.out_len || (!s.out && !s.into && !s.keep)) throw ArgError{TDC_GPU_ERR_ARG, msg};
}
// the "too small" rule: the required size goes to *out_len, the call fails with TDC_GPU_ERR_OOM
[[noreturn]] inline void sink_too_small(Sink& s, size_t need) {
    *s.out_len = need;
    throw ArgError{TDC_GPU_ERR_OOM, "output buffer too small (*out_len holds the required size)"};
}
inline void sink_fit(Sink& s, size_t need) { if (s.into && s.cap < need) sink_too_small(s, need); }
// host memory for `bytes` bytes of output: the caller's buffer, or one the sink owns until it is committed
inline u8* sink_host(Sink& s, size_t bytes) {
    if (s.into) return s.into;
    s.owned = (u8*)malloc(bytes ? bytes : 1);
    if (!s.owned) throw std::bad_alloc();
    return s.owned;
}
// the download of `len` bytes at d_src, enqueued on the compute stream
inline void sink_download(Ctx& c, Sink& s, const u8* d_src, size_t len) {
    HIP_TRY(hipMemcpyAsync(sink_host(s, len), d_src, len, hipMemcpyDeviceToHost, c.stream));
}
// the call has succeeded: the length and (malloc'd destination) the buffer go to the caller
inline void sink_commit(Sink& s, size_t len) {
    *s.out_len = len;
    if (s.out) *s.out = s.release();
}

// Runs a stage's decoder and translates what it throws: malformed input -> TDC_GPU_ERR_ARG with its text, a text beyond the format's
// limit -> TDC_GPU_ERR_TOO_LARGE with too_large, and -- need != NULL: the decoder reports the text length there as soon as it knows
// it -- a caller's buffer shorter than that -> the "too small" rule.
template <typename F>
size_t run_decoder(Sink& s, const char* too_large, const size_t* need, F&& decode) {
    try { return decode(); }
    catch (const StreamFormatError& e) { throw ArgError{TDC_GPU_ERR_ARG, e.what}; }
    catch (const DecodeTooLarge&) { throw ArgError{TDC_GPU_ERR_TOO_LARGE, too_large}; }
    catch (const HipError& e) {
        if (e.e == hipErrorOutOfMemory && need && s.into && *need > s.cap) sink_too_small(s, *need);
        throw;
    }
}

}  // namespace tdc
