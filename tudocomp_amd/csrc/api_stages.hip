// api_stages.hip -- C ABI (include/tdc_gpu.h): the stage-level entry points the tests drive -- the sorts, the text's arrays, the
// factorizer, flatten and the encoders on a given factor list.
#include "api.hpp"

using namespace tdc;

namespace {
void validate_factor_list(size_t n, const uint32_t* pos, const uint32_t* src, const uint32_t* len, size_t z) {
    uint64_t end = 0;
    for (size_t i = 0; i < z; ++i) {
        if (len[i] == 0) throw ArgError{TDC_GPU_ERR_ARG, "factor with length 0"};
        if (pos[i] < end) throw ArgError{TDC_GPU_ERR_ARG, "factors must be sorted by pos and must not overlap"};
        end = (uint64_t)pos[i] + len[i];
        if (end > n) throw ArgError{TDC_GPU_ERR_ARG, "factor exceeds the text"};
        if (src && (uint64_t)src[i] + len[i] > n) throw ArgError{TDC_GPU_ERR_ARG, "factor source exceeds the text"};
    }
}

// a factor list (validated) on the device, with room for one entry more, and scattered into the position space of a text of n bytes
struct DevFactors { u32 *pos, *src, *len; FactorSpace fs; };
DevFactors upload_factors(Ctx& c, size_t n, const uint32_t* pos, const uint32_t* src, const uint32_t* len, size_t z) {
    DevFactors F;
    F.fs.flen = c.arena.get<u32>(n); F.fs.owner = c.arena.get<u32>(n); F.fs.fsrc = c.arena.get<u32>(n);
    F.pos = c.arena.get<u32>(z + 1); F.src = c.arena.get<u32>(z + 1); F.len = c.arena.get<u32>(z + 1);
    if (z) {
        HIP_TRY(hipMemcpyAsync(F.pos, pos, z * 4, hipMemcpyHostToDevice, c.stream));
        HIP_TRY(hipMemcpyAsync(F.src, src, z * 4, hipMemcpyHostToDevice, c.stream));
        HIP_TRY(hipMemcpyAsync(F.len, len, z * 4, hipMemcpyHostToDevice, c.stream));
    }
    scatter_factors(c, n, F.pos, F.src, F.len, z, F.fs);
    return F;
}

int encode_entry(tdc_gpu_ctx* ctx, int coder, const uint8_t* text, size_t n, const uint32_t* pos, const uint32_t* src,
                 const uint32_t* len, size_t z, uint8_t** out, size_t* out_len) {
    return guarded(ctx, [&] {
        check_text_args(text, n);
        Sink s = sink_malloc(out, out_len);
        sink_check(s, "out/out_len is NULL");
        if (z && (!pos || !src || !len)) throw ArgError{TDC_GPU_ERR_ARG, "factor arrays are NULL"};
        validate_factor_list(n, pos, src, len, z);
        Ctx& c = ctx->c;
        reserve_arena(c, arena_need(c, n));
        const u8* d_text = upload_plain(c, text, n);
        const DevFactors F = upload_factors(c, n, pos, src, len, z);
        const size_t cap = align_up(encode_bound_coder(n, coder) + 16, 8);
        u8* d_out = c.arena.get<u8>(cap);
        const size_t l = encode_stream(c, d_text, n, F.fs, coder, d_out, cap, nullptr);
        sink_download(c, s, d_out, l);
        HIP_TRY(hipStreamSynchronize(c.stream));
        sink_commit(s, l);
    });
}
}  // namespace

extern "C" {

int tdc_gpu_sort_pairs_u64(tdc_gpu_ctx* ctx, uint64_t* keys, uint32_t* vals, size_t n, int algo) {
    return guarded(ctx, [&] {
        if (!keys || !vals) throw ArgError{TDC_GPU_ERR_ARG, "keys/vals is NULL"};
        if (n == 0) return;
        if (n >= 0xFFFFFFFFull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "at most 2^32 - 2 pairs"};
        Ctx& c = ctx->c;
        reserve_arena(c, 64 * n + ((size_t)256 << 20));
        u64* k[2] = { c.arena.get<u64>(n), c.arena.get<u64>(n) };
        u32* v[2] = { c.arena.get<u32>(n), c.arena.get<u32>(n) };
        HIP_TRY(hipMemcpyAsync(k[0], keys, n * 8, hipMemcpyHostToDevice, c.stream));
        HIP_TRY(hipMemcpyAsync(v[0], vals, n * 4, hipMemcpyHostToDevice, c.stream));
        int x;
        if (algo == 1) { SplitSortStats ss; x = splitter_sort_pairs_u64(c, k, v, n, nullptr, &ss); }
        else if (algo == 0) x = radix_sort_pairs_u64(c, k, v, n, 0, 64);
        else throw ArgError{TDC_GPU_ERR_ARG, "algo must be 0 (LSD radix) or 1 (splitter partition)"};
        HIP_TRY(hipMemcpyAsync(keys, k[x], n * 8, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipMemcpyAsync(vals, v[x], n * 4, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
    });
}

int tdc_gpu_suffix_array(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint32_t* sa, uint32_t* isa) {
    return tdc_gpu_textds(ctx, text, n, sa, isa, nullptr, nullptr, nullptr, nullptr);
}

int tdc_gpu_textds(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint32_t* sa, uint32_t* isa, uint32_t* phi,
                   uint32_t* plcp, uint32_t* lcp, uint32_t* maxlcp) {
    return guarded(ctx, [&] {
        check_host_text(text, n);
        Ctx& c = ctx->c;
        reserve_arena(c, arena_need(c, n));
        const u8* d_text = upload_plain(c, text, n);
        validate_device_text(c, d_text, n);
        DevArrays A;
        if (!phi && !plcp && !lcp && !maxlcp) {
            A.sa = c.arena.get<u32>(n);
            A.isa = c.arena.get<u32>(n);
            build_suffix_array(c, d_text, n, A.sa, A.isa, nullptr);
        } else {
            run_textds(c, d_text, n, A, nullptr, nullptr);
        }
        if (sa) HIP_TRY(hipMemcpyAsync(sa, A.sa, n * 4, hipMemcpyDeviceToHost, c.stream));
        if (isa) HIP_TRY(hipMemcpyAsync(isa, A.isa, n * 4, hipMemcpyDeviceToHost, c.stream));
        if (phi) HIP_TRY(hipMemcpyAsync(phi, A.phi, n * 4, hipMemcpyDeviceToHost, c.stream));
        if (plcp) HIP_TRY(hipMemcpyAsync(plcp, A.plcp, n * 4, hipMemcpyDeviceToHost, c.stream));
        if (lcp) {
            u32* d_lcp = c.arena.get<u32>(n);
            build_lcp(c, A.sa, A.plcp, n, d_lcp);
            HIP_TRY(hipMemcpyAsync(lcp, d_lcp, n * 4, hipMemcpyDeviceToHost, c.stream));
        }
        if (maxlcp) *maxlcp = A.maxlcp;
        HIP_TRY(hipStreamSynchronize(c.stream));
    });
}

int tdc_gpu_lcpcomp_factorize(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint32_t threshold, int flatten,
                              uint32_t** pos, uint32_t** src, uint32_t** len, size_t* z, tdc_gpu_stats* stats) {
    return guarded(ctx, [&] {
        check_host_text(text, n);
        if (!pos || !src || !len || !z) throw ArgError{TDC_GPU_ERR_ARG, "output pointer is NULL"};
        if (threshold == 0) throw ArgError{TDC_GPU_ERR_ARG, "threshold must be >= 1"};
        Ctx& c = ctx->c;
        if (stats) memset(stats, 0, sizeof(*stats));
        reserve_arena(c, arena_need(c, n));
        Events ev(c);
        const u8* d_text = upload_plain(c, text, n);
        validate_device_text(c, d_text, n);
        DevArrays A;
        run_textds(c, d_text, n, A, stats, &ev);
        run_factorize(c, n, A, threshold, flatten, stats, &ev);
        download_factors(c, n, A.fs, ev, pos, src, len, z);
        if (stats) { stats->n = n; stats->arena_bytes = c.arena.high; }
    });
}

int tdc_gpu_flatten(tdc_gpu_ctx* ctx, size_t n, const uint32_t* pos, uint32_t* src, const uint32_t* len, size_t z,
                    uint64_t* num_flattened, uint64_t* max_depth_lb) {
    return guarded(ctx, [&] {
        if (n == 0 || n >= 0x7FFFFFFFull) throw ArgError{TDC_GPU_ERR_ARG, "bad n"};
        if (z && (!pos || !src || !len)) throw ArgError{TDC_GPU_ERR_ARG, "factor arrays are NULL"};
        validate_factor_list(n, pos, src, len, z);
        Ctx& c = ctx->c;
        reserve_arena(c, arena_need(c, n));
        const DevFactors F = upload_factors(c, n, pos, src, len, z);
        FlattenStats fl;
        flatten_factors(c, n, F.fs, &fl);
        const size_t cnt = extract_factors(c, n, F.fs, F.pos, F.src, nullptr, z + 1);
        if (cnt != z) throw HipError{hipErrorUnknown, "flatten: factor count changed", (int)__LINE__};
        if (z) HIP_TRY(hipMemcpyAsync(src, F.src, z * 4, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        if (num_flattened) *num_flattened = fl.num_flattened;
        if (max_depth_lb) *max_depth_lb = fl.max_depth_lb;
    });
}

int tdc_gpu_encode_huff(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, const uint32_t* pos, const uint32_t* src,
                        const uint32_t* len, size_t z, uint8_t** out, size_t* out_len) {
    return encode_entry(ctx, 0, text, n, pos, src, len, z, out, out_len);
}
int tdc_gpu_encode_arith(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, const uint32_t* pos, const uint32_t* src,
                         const uint32_t* len, size_t z, uint8_t** out, size_t* out_len) {
    return encode_entry(ctx, 1, text, n, pos, src, len, z, out, out_len);
}
int tdc_gpu_encode_ascii(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, const uint32_t* pos, const uint32_t* src,
                         const uint32_t* len, size_t z, uint8_t** out, size_t* out_len) {
    return encode_entry(ctx, 2, text, n, pos, src, len, z, out, out_len);
}
int tdc_gpu_encode_sle(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, const uint32_t* pos, const uint32_t* src,
                       const uint32_t* len, size_t z, uint32_t kmer, uint8_t** out, size_t* out_len) {
    if (kmer > 7) return TDC_GPU_ERR_ARG;
    return encode_entry(ctx, 3 | ((int)(kmer ? kmer : 3) << 8), text, n, pos, src, len, z, out, out_len);
}

}  // extern "C"
