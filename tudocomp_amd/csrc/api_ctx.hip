// api_ctx.hip -- C ABI (include/tdc_gpu.h): context life cycle, the option table, profiling, and the small host-side helpers.
#include "api.hpp"
#include "huffman_host.hpp"

#include <strings.h>
#include <ctype.h>

using namespace tdc;

namespace tdc {

int lcpcomp_enc_coder(int coder) {
    const int base = coder & 0xFF, k = coder >> 8;
    if (base == TDC_GPU_CODER_SLE) {
        if (k < 0 || k > 7) throw ArgError{TDC_GPU_ERR_ARG, "sle: kmer must be in 1..7"};       // SLECoder.hpp:12,86 (max_kmer = 7)
        return 3 | ((k ? k : 3) << 8);
    }
    if (k == 0 && base == TDC_GPU_CODER_HUFF) return 0;
    if (k == 0 && base == TDC_GPU_CODER_ARITH) return 1;
    if (k == 0 && base == TDC_GPU_CODER_ASCII) return 2;
    throw ArgError{TDC_GPU_ERR_UNSUPPORTED, "lcpcomp: coder must be huff, arithmetic, ascii or sle"};
}

void reserve_arena(Ctx& c, size_t bytes) {
    if (c.arena.size < bytes) {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess && fr + c.arena.size < bytes) {
            static thread_local char msg[256];
            snprintf(msg, sizeof(msg), "device %d has %.1f GB free of %.1f GB, this call needs an arena of %.1f GB (112 bytes per text byte + 192 MiB): "
                     "use smaller blocks (tdc_gpu_arena_bytes)", c.device, (double)(fr + c.arena.size) / 1e9, (double)tot / 1e9, (double)bytes / 1e9);
            throw ArgError{TDC_GPU_ERR_OOM, msg};
        }
        (void)hipGetLastError();
    }
    c.ensure_arena(bytes);
}

}  // namespace tdc

extern "C" {

const char* tdc_gpu_strerror(int status) {
    switch (status) {
        case TDC_GPU_OK: return "success";
        case TDC_GPU_ERR_HIP: return "HIP runtime error (is a gfx950 GPU visible?)";
        case TDC_GPU_ERR_ARG: return "invalid argument";
        case TDC_GPU_ERR_NO_SENTINEL: return "Expected a sentinel byte (0) at the end of the input text";
        case TDC_GPU_ERR_TOO_LARGE: return "input too large: text length must be < 2^31";
        case TDC_GPU_ERR_OOM: return "out of memory";
        case TDC_GPU_ERR_UNSUPPORTED: return "No implementation found for this coder/strategy";
        case TDC_GPU_ERR_INTERNAL: return "internal error";
        default: return "unknown status";
    }
}

const char* tdc_gpu_last_error(const tdc_gpu_ctx* ctx) { return ctx ? ctx->last_error.c_str() : ""; }

void tdc_gpu_free(void* p) { free(p); }

// ---- options ---------------------------------------------------------------------------------------------------------------------
// Every switch of the library, in ONE table: name (the environment variable of the development aid is TDC_GPU_ + upper case), the
// field, and the values it accepts (out-of-range values are clamped the way the environment parser of rounds 1-5 did).  README.md
// lists them with the test that exercises each.
namespace {
struct OptionDef { const char* name; void (*set)(Ctx&, long); };
inline int clampi(long v, long lo, long hi) { return (int)(v < lo ? lo : (v > hi ? hi : v)); }
const OptionDef OPTIONS[] = {
    { "fastread",         [](Ctx& c, long v) { c.fast_read = v ? 1 : 0; } },
    { "sa_local",         [](Ctx& c, long v) { c.sa_local_sort = (int)v; } },
    { "radix_waves",      [](Ctx& c, long v) { c.radix_waves = v == 8 ? 8 : 4; } },
    { "window_lcut",      [](Ctx& c, long v) { c.window_lcut = clampi(v, 0, 63); } },
    { "window_halo",      [](Ctx& c, long v) { c.window_halo = clampi(v, 0, 2048); } },
    { "dec_seg",          [](Ctx& c, long v) { c.dec_seg = v < 4096 ? 4096 : (v > (1l << 30) ? (size_t)1 << 30 : (size_t)v); } },
    { "dec_lean",         [](Ctx& c, long v) { c.dec_lean = v != 0; } },
    { "dec_parse",        [](Ctx& c, long v) { c.dec_parse = clampi(v, 0, 2); } },
    { "dec_done",         [](Ctx& c, long v) { c.dec_done = v != 0; } },
    { "dec_log",          [](Ctx& c, long v) { c.dec_log = v != 0; } },
    { "bwt_log",          [](Ctx& c, long v) { c.bwt_log = v != 0; } },
    { "pipe_log",         [](Ctx& c, long v) { c.pipe_log = v != 0; } },
    { "window_force_fail",[](Ctx& c, long v) { c.window_force_fail = v ? 1 : 0; } },
    { "window_large",     [](Ctx& c, long v) { c.window_large_lists = v ? 1 : 0; } },
    { "window_src",       [](Ctx& c, long v) { c.window_src = v ? 1 : 0; } },
    { "plcp_samples",     [](Ctx& c, long v) { c.plcp_samples = v != 0; } },
    { "small_pipeline",   [](Ctx& c, long v) { c.small_pipeline = v != 0; } },
    { "small_big",        [](Ctx& c, long v) { c.small_big = (int)v; } },
    { "small_prof",       [](Ctx& c, long v) { c.small_prof = v != 0; } },
    { "phi_lazy",         [](Ctx& c, long v) { c.phi_lazy = v != 0; } },
    { "fs_pair",          [](Ctx& c, long v) { c.fs_pair = v != 0; } },
    { "enc_early",        [](Ctx& c, long v) { c.enc_early = (int)v; } },
    { "owner_rem",        [](Ctx& c, long v) { c.owner_rem = (int)std::min<long>(std::max<long>(v, 0), 8); } },
    { "enc_rec",          [](Ctx& c, long v) { c.enc_rec = v != 0; } },
    { "level_purge",      [](Ctx& c, long v) { c.level_purge = v != 0; } },
    { "level_log",        [](Ctx& c, long v) { c.level_log = v != 0; } },
    { "eager",            [](Ctx& c, long v) { c.eager_levels = v != 0; } },
    { "eager_dump",       [](Ctx& c, long v) { c.eager_dump = v != 0; } },
    { "flen_bytes",       [](Ctx& c, long v) { c.flen_bytes = v != 0; } },
    { "flatten_steps",    [](Ctx& c, long v) { c.flatten_steps = v <= 0 ? (1 << 30) : clampi(v, 1, 1 << 30); } },
    { "flatten_growth",   [](Ctx& c, long v) { c.flatten_growth = clampi(v, 2, 1 << 20); } },
    { "sa_refine",        [](Ctx& c, long v) { c.sa_refine = v != 0; } },
    { "sa_pairs",         [](Ctx& c, long v) { c.sa_pairs = v != 0; } },
    { "sa_stars",         [](Ctx& c, long v) { c.sa_stars = v != 0; } },
    { "sa_fused_init",    [](Ctx& c, long v) { c.sa_fused_init = v != 0; } },
    { "sa_init_syms",     [](Ctx& c, long v) { c.sa_init_syms = clampi(v, 0, 64); } },
    { "radix_lds",        [](Ctx& c, long v) { c.radix_lds = (v >= 0 && v <= 2) ? (int)v : 2; } },
    { "xcd_remap",        [](Ctx& c, long v) { c.xcd_remap = (v >= 0 && v <= 2) ? (int)v : 0; } },
    { "bucket_scatter",   [](Ctx& c, long v) { c.bucket_scatter = v ? 1 : 0; } },
    { "ssort",            [](Ctx& c, long v) { c.ssort = v ? 1 : 0; } },
    { "ssort_levels",     [](Ctx& c, long v) { c.ssort_levels = (v >= 1 && v <= 3) ? (int)v : 0; } },
    { "msd_partition",    [](Ctx& c, long v) { c.msd_partition = v ? 1 : 0; } },
    { "wsort",            [](Ctx& c, long v) { c.wsort = v ? 1 : 0; } },
    { "wsort_min",        [](Ctx& c, long v) { c.wsort_min = v < 4096 ? 4096 : (size_t)v; } },
    { "wsort_syms",       [](Ctx& c, long v) { c.wsort_syms = (v >= 4 && v <= 64) ? (int)v : 0; } },
    { "wsort_kw",         [](Ctx& c, long v) { c.wsort_kw = (v == 1 || v == 2) ? (int)v : 0; } },
    { "wsort_rounds",     [](Ctx& c, long v) { c.wsort_rounds = clampi(v, 0, 100); } },
    { "wsort_smallrun",   [](Ctx& c, long v) { c.wsort_small = v ? 1 : 0; } },
    { "wsort_overlap",    [](Ctx& c, long v) { c.wsort_overlap = v ? 1 : 0; } },
    { "wsort_predig",     [](Ctx& c, long v) { c.wsort_predig = v ? 1 : 0; } },
    { "wsort_prehist",    [](Ctx& c, long v) { c.wsort_prehist = v ? 1 : 0; } },
    { "sa_seg_bigcap",    [](Ctx& c, long v) { c.sa_seg_bigcap = clampi(v, 0, 65536); } },
    { "sa_seg_rounds",    [](Ctx& c, long v) { c.sa_seg_rounds = clampi(v, 0, 2); } },
    { "wsort_run_streams",[](Ctx& c, long v) { c.wsort_run_streams = v != 0; } },
    { "wsort_predig_skip",[](Ctx& c, long v) { c.wsort_predig_skip = clampi(v, 0, 24); } },
    { "wsort_fuse",       [](Ctx& c, long v) { c.wsort_fuse = v ? 1 : 0; } },
    { "wsort_order",      [](Ctx& c, long v) { c.wsort_order = v ? 1 : 0; } },
    { "wsort_two",        [](Ctx& c, long v) { c.wsort_two = (v >= 0 && v <= 2) ? (int)v : 0; } },
    { "wsort_leaf",       [](Ctx& c, long v) { c.wsort_leaf = v == 1024 ? 1024 : 2048; } },
    { "wsort_pack",       [](Ctx& c, long v) { c.wsort_pack = (v == 1024 || v == 4096) ? (int)v : 2048; } },
    { "wsort_cmax",       [](Ctx& c, long v) { c.wsort_cmax = clampi(v, 8, 64); } },       // (the hand-over lists take 128 n / (cmax + 1) bytes: below 8 they outgrow the arena)
    { "wsort_log",        [](Ctx& c, long v) { c.wsort_log = v != 0; } },
    { "upload_chunks",    [](Ctx& c, long v) { c.upload_chunks = clampi(v, 4, 24); } },
    { "upload_tail_n",    [](Ctx& c, long v) { c.upload_tail_n = clampi(v, 0, 12); } },
    { "upload_tail_pct",  [](Ctx& c, long v) { c.upload_tail_pct = clampi(v, 30, 100); } },
    { "arena_log",        [](Ctx& c, long v) { c.arena_log = v != 0; } },
};
constexpr size_t NOPTIONS = sizeof(OPTIONS) / sizeof(OPTIONS[0]);
// Switches of passes folded into a neighbouring kernel: set like the others, but not enumerated by tdc_gpu_option_name() -- the enumerated
// set is the one tests/test_gpu_parity.py::test_every_option_value_is_bit_exact walks; these are walked by tests/test_gpu_fused_candidates.py.
// flatten_chunks (a schedule, not a fold) sits here for the same reason; tests/test_gpu_flatten_chunks.py walks it.  The repair_* switches
// (a cross-check mode, a forced table size, a log, the device decoder's depth cap) belong to one compressor; tests/test_gpu_repair.py and
// tests/test_gpu_repair_decode.py walk them.  lz_batch_hash_bits (the batch parse's table under long probe runs) is walked by
// tests/test_gpu_lz_batch.py; repair_batch_rounds and repair_batch_table (the batch grammar's launches and its table) by
// tests/test_gpu_repair_batch.py; bwt_batch_sample and bwt_batch_steps (the batch inverse's list heads and walk launches) by
// tests/test_gpu_bwt_batch.py; pipe_batch_threads (the host threads of the batch pipeline's Huffman table build: the same tables on any
// number) by tests/test_gpu_pipeline_batch.py.
const OptionDef FOLD_OPTIONS[] = {
    { "fused_cand",       [](Ctx& c, long v) { c.fused_cand = v != 0; } },
    { "sel_tile_counts",  [](Ctx& c, long v) { c.sel_tile_counts = v != 0; } },
    { "flatten_chunks",   [](Ctx& c, long v) { c.flatten_chunks = clampi(v, 0, (long)FLATTEN_MAX_CHUNKS); } },
    { "repair_recount",   [](Ctx& c, long v) { c.repair_recount = v != 0; } },
    { "repair_table_bits",[](Ctx& c, long v) { c.repair_table_bits = v == 0 ? 0 : clampi(v, 8, 30); } },
    { "repair_log",       [](Ctx& c, long v) { c.repair_log = v != 0; } },
    { "repair_dec_rounds",[](Ctx& c, long v) { c.repair_dec_rounds = clampi(v, 1, 1 << 24); } },
    { "lz_batch_hash_bits",[](Ctx& c, long v) { c.lz_batch_hash_bits = clampi(v, 0, 24); } },
    { "repair_batch_rounds",[](Ctx& c, long v) { c.repair_batch_rounds = clampi(v, 1, 1 << 24); } },
    { "repair_batch_table",[](Ctx& c, long v) { c.repair_batch_table = v != 0; } },
    { "bwt_batch_sample", [](Ctx& c, long v) { c.bwt_batch_sample = clampi(v, 0, 1 << 24); } },
    { "bwt_batch_steps",  [](Ctx& c, long v) { c.bwt_batch_steps = clampi(v, 0, 1 << 30); } },
    { "pipe_batch_threads",[](Ctx& c, long v) { c.pipe_batch_threads = clampi(v, 0, 16); } },
};
constexpr size_t NFOLD = sizeof(FOLD_OPTIONS) / sizeof(FOLD_OPTIONS[0]);
const OptionDef* find_option(const char* name) {
    if (!name) return nullptr;
    if (!strncasecmp(name, "TDC_GPU_", 8)) name += 8;
    for (size_t i = 0; i < NOPTIONS; ++i) if (!strcasecmp(name, OPTIONS[i].name)) return &OPTIONS[i];
    for (size_t i = 0; i < NFOLD; ++i) if (!strcasecmp(name, FOLD_OPTIONS[i].name)) return &FOLD_OPTIONS[i];
    return nullptr;
}
// the ONE place that reads TDC_GPU_* variables (besides TDC_GPU_LIB of the Python loader, which picks the library file)
void apply_env_options(tdc_gpu_ctx* ctx) {
    const char* on = getenv("TDC_GPU_DEBUG_KNOBS");
    if (!on || atoi(on) == 0) return;
    for (size_t i = 0; i < NOPTIONS + NFOLD; ++i) {
        const OptionDef& o = i < NOPTIONS ? OPTIONS[i] : FOLD_OPTIONS[i - NOPTIONS];
        char var[64] = "TDC_GPU_";
        size_t k = 8;
        for (const char* q = o.name; *q && k + 1 < sizeof(var); ++q) var[k++] = (char)toupper((unsigned char)*q);
        var[k] = 0;
        if (const char* m = getenv(var)) o.set(ctx->c, atol(m));
    }
}
}  // namespace

int tdc_gpu_ctx_set_option(tdc_gpu_ctx* ctx, const char* name, long value) {
    if (!ctx) return TDC_GPU_ERR_ARG;
    const OptionDef* o = find_option(name);
    if (!o) return TDC_GPU_ERR_ARG;
    o->set(ctx->c, value);
    return TDC_GPU_OK;
}
int tdc_gpu_option_count(void) { return (int)NOPTIONS; }
const char* tdc_gpu_option_name(int i) { return (i >= 0 && (size_t)i < NOPTIONS) ? OPTIONS[i].name : nullptr; }

int tdc_gpu_ctx_create(int device, tdc_gpu_ctx** out) {
    if (!out) return TDC_GPU_ERR_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { (void)hipGetLastError(); return TDC_GPU_ERR_HIP; }
    if (device < 0 || device >= count) return TDC_GPU_ERR_ARG;
    tdc_gpu_ctx* ctx = new (std::nothrow) tdc_gpu_ctx();
    if (!ctx) return TDC_GPU_ERR_OOM;
    // libstdc++ drift check: a C++ library whose heap / sort tie order differs from the reference build's would change every
    // Huffman stream silently (coders/HuffmanCoder.hpp:455 is an unstable std::sort).  Only what builds a Huffman table depends on
    // it: those calls fail (encode.hip), everything else -- other coders, lz78, decompression -- works
    ctx->c.huff_ok = huffman_selfcheck();
    ctx->c.device = device;
    ctx->c.wpre = &ctx->pre;
    DeviceGuard dg(device);                      // (the caller's current device is restored on every exit path)
    try {
        HIP_TRY(dg.enter());
        HIP_TRY(hipStreamCreateWithFlags(&ctx->c.stream, hipStreamNonBlocking));
        for (auto& e : ctx->c.ev) HIP_TRY(hipEventCreate(&e));
        HIP_TRY(hipStreamCreateWithFlags(&ctx->c.copy_stream, hipStreamNonBlocking));
        {   // the side stream takes the lowest priority the device offers
            int lo = 0, hi = 0;
            if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { lo = 0; (void)hipGetLastError(); }
            if (hipStreamCreateWithPriority(&ctx->c.aux_stream, hipStreamNonBlocking, lo) != hipSuccess) { ctx->c.aux_stream = nullptr; (void)hipGetLastError(); }
        }
        HIP_TRY(hipEventCreateWithFlags(&ctx->c.ev_join, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ctx->c.ev_dig2, hipEventDisableTiming));
        for (auto& e : ctx->c.ev_chunk) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->c.pinned_size = 4096;
        HIP_TRY(hipHostMalloc(&ctx->c.pinned, ctx->c.pinned_size, hipHostMallocDefault));
        HIP_TRY(hipHostMalloc((void**)&ctx->c.pinned_hdr, Ctx::PINNED_HDR, hipHostMallocDefault));
        if (ctx->c.fast_read) {
            void* zc = nullptr;
            if (hipHostMalloc(&zc, (size_t)Ctx::ZC_WORDS * Ctx::ZC_BLOCKS * 4, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) {
                void* dv = nullptr;
                if (hipHostGetDevicePointer(&dv, zc, 0) == hipSuccess) { ctx->c.zc_host = (u32*)zc; ctx->c.zc_dev = (u32*)dv; memset(zc, 0, (size_t)Ctx::ZC_WORDS * Ctx::ZC_BLOCKS * 4); }
                else { (void)hipHostFree(zc); (void)hipGetLastError(); }
            } else (void)hipGetLastError();
        }
        HIP_TRY(hipMalloc((void**)&ctx->c.d_err, 256));
        HIP_TRY(hipMemset(ctx->c.d_err, 0, 256));
        // Development aid: with TDC_GPU_DEBUG_KNOBS=1 every TDC_GPU_<OPTION> variable of the environment is applied through
        // tdc_gpu_ctx_set_option().  Without it the library never reads an option from the environment: an embedding process cannot change
        // the algorithm by accident.
        apply_env_options(ctx);
    } catch (const HipError&) {
        (void)hipGetLastError();
        tdc_gpu_ctx_destroy(ctx);
        return TDC_GPU_ERR_HIP;
    }
    *out = ctx;
    return TDC_GPU_OK;
}

void tdc_gpu_ctx_destroy(tdc_gpu_ctx* ctx) {
    if (!ctx) return;
    DeviceGuard dg(ctx->c.device);
    (void)dg.enter();
    (void)sync_streams(ctx->c);
    if (ctx->c.arena.base) (void)hipFree(ctx->c.arena.base);
    if (ctx->c.pinned) (void)hipHostFree(ctx->c.pinned);
    if (ctx->c.pinned_hdr) (void)hipHostFree(ctx->c.pinned_hdr);
    if (ctx->c.pinned_tab) (void)hipHostFree(ctx->c.pinned_tab);
    if (ctx->c.zc_host) (void)hipHostFree(ctx->c.zc_host);
    if (ctx->c.d_err) (void)hipFree(ctx->c.d_err);
    for (auto& e : ctx->c.ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : ctx->c.ev_chunk) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : {ctx->c.ev_join, ctx->c.ev_dig2}) if (e) (void)hipEventDestroy(e);
    if (ctx->c.copy_stream) (void)hipStreamDestroy(ctx->c.copy_stream);
    if (ctx->c.aux_stream) (void)hipStreamDestroy(ctx->c.aux_stream);
    if (ctx->c.ev_pool) { for (int i = 0; i < ctx->c.ev_pool_size; ++i) if (ctx->c.ev_pool[i]) (void)hipEventDestroy(ctx->c.ev_pool[i]); free(ctx->c.ev_pool); }
    free(ctx->c.pend);
    if (ctx->c.stream) (void)hipStreamDestroy(ctx->c.stream);
    delete ctx;
}

int tdc_gpu_ctx_set_profiling(tdc_gpu_ctx* ctx, int enabled) {
    return guarded(ctx, [&] {
        Ctx& c = ctx->c;
        if (enabled && !c.ev_pool) {
            c.ev_pool_size = 16384; c.pend_cap = 8192;
            c.ev_pool = (hipEvent_t*)calloc(c.ev_pool_size, sizeof(hipEvent_t));
            c.pend = (Ctx::Pending*)calloc(c.pend_cap, sizeof(Ctx::Pending));
            if (!c.ev_pool || !c.pend) throw std::bad_alloc();
            for (int i = 0; i < c.ev_pool_size; ++i) HIP_TRY(hipEventCreate(&c.ev_pool[i]));
        }
        c.profiling = enabled != 0;
    });
}

void tdc_gpu_ctx_reset_profile(tdc_gpu_ctx* ctx) {
    if (!ctx) return;
    for (auto& k : ctx->c.kprof) k = KernelProfile();
}

const char* tdc_gpu_ctx_kernel_profile(const tdc_gpu_ctx* ctx, int idx, double* ms, uint64_t* launches, uint64_t* bytes) {
    static const char* names[K_CLASS_COUNT] = {
        "rs_scatter_kernel<u64>", "rs_scatter_kernel<u32>", "rs_count_kernel", "scan_kernels",
        "sa_groups_kernel", "sa_build_keys_kernel", "phi_kernel", "plcp_kernel", "cand_kernels",
        "level_init_kernel", "mis_round_kernel", "resolve_kernel", "push_kernel", "apply_kernel", "pool_kernels", "small_level_kernel", "window_levels_kernel",
        "flatten_round_kernel", "gaps_kernel", "literal_hist_kernel", "tile_bits_kernel", "pack_kernel", "extract_kernels",
        "ss_leaf_sort_kernel", "sa_local_sort_kernel", "window_scatter_kernels",
        "ws_leaf_sort_kernel", "ws_leaf_count_kernel", "ws_run_kernels", "fs_image_kernel" };
    if (!ctx || idx < 0 || idx >= K_CLASS_COUNT) return nullptr;
    const KernelProfile& k = ctx->c.kprof[idx];
    if (ms) *ms = k.ms;
    if (launches) *launches = k.launches;
    if (bytes) *bytes = k.bytes;
    return names[idx];
}

size_t tdc_gpu_arena_bytes(size_t n) { return arena_need(n); }

int tdc_gpu_device_memory(int device, size_t* free_bytes, size_t* total_bytes) {
    if (!free_bytes || !total_bytes) return TDC_GPU_ERR_ARG;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) { (void)hipGetLastError(); return TDC_GPU_ERR_ARG; }
    DeviceGuard dg(device);
    if (dg.enter() != hipSuccess || hipMemGetInfo(free_bytes, total_bytes) != hipSuccess) { (void)hipGetLastError(); return TDC_GPU_ERR_HIP; }
    return TDC_GPU_OK;
}

int tdc_gpu_ctx_reserve(tdc_gpu_ctx* ctx, size_t n) {
    return guarded(ctx, [&] { reserve_arena(ctx->c, arena_need(ctx->c, n)); });
}

int tdc_gpu_host_register(void* p, size_t bytes) {
    if (!p || !bytes) return TDC_GPU_ERR_ARG;
    if (hipHostRegister(p, bytes, hipHostRegisterPortable) != hipSuccess) { (void)hipGetLastError(); return TDC_GPU_ERR_HIP; }
    return TDC_GPU_OK;
}
int tdc_gpu_host_unregister(void* p) {
    if (!p) return TDC_GPU_ERR_ARG;
    if (hipHostUnregister(p) != hipSuccess) { (void)hipGetLastError(); return TDC_GPU_ERR_HIP; }
    return TDC_GPU_OK;
}

int tdc_gpu_device_count(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return count;
}

void* tdc_gpu_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
void tdc_gpu_host_free(void* p) { if (p) (void)hipHostFree(p); }

// ---- host-side helpers ------------------------------------------------------------------------------------
size_t tdc_escape(const uint8_t* in, size_t n, uint8_t* out) {
    size_t o = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint8_t ch = in[i];
        if (ch == 0x00) { out[o++] = 0xFF; out[o++] = 0xFE; }
        else if (ch == 0xFF) { out[o++] = 0xFF; out[o++] = 0xFF; }
        else out[o++] = ch;
    }
    out[o++] = 0;
    return o;
}

size_t tdc_unescape(const uint8_t* in, size_t n, uint8_t* out) {
    size_t o = 0;
    if (n && in[n - 1] == 0) --n;
    for (size_t i = 0; i < n; ++i) {
        const uint8_t ch = in[i];
        if (ch == 0xFF && i + 1 < n) { const uint8_t d = in[++i]; out[o++] = (d == 0xFE) ? 0x00 : d; }
        else out[o++] = ch;
    }
    return o;
}

int tdc_huffman_selfcheck(void) { return huffman_selfcheck() ? TDC_GPU_OK : TDC_GPU_ERR_INTERNAL; }

int tdc_huffman_table(const uint32_t counts[256], uint32_t* sigma, uint32_t* longest, uint8_t order[256],
                      uint8_t len_of[256], uint64_t code_of[256]) {
    if (!counts) return TDC_GPU_ERR_ARG;
    try {
        HuffTable t;
        build_huffman_table(counts, &t);
        if (sigma) *sigma = t.sigma;
        if (longest) *longest = t.longest;
        if (order) memcpy(order, t.order, 256);
        if (len_of) memcpy(len_of, t.len_of, 256);
        if (code_of) memcpy(code_of, t.code_of, 256 * sizeof(uint64_t));
    } catch (...) { return TDC_GPU_ERR_OOM; }
    return TDC_GPU_OK;
}

}  // extern "C"
