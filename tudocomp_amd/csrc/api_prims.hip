// api_prims.hip -- C ABI (include/tdc_gpu.h): the shared device primitives of prim.hpp and tile_chain.hpp one by one, for the tests.  Every entry point
// checks the primitive's preconditions ON THE HOST and refuses with TDC_GPU_ERR_ARG before anything is launched: a wrong test input
// must not become a store outside a buffer.  The product never calls these.
#include "api.hpp"
#include "tile_chain.hpp"

#include <algorithm>
#include <vector>

using namespace tdc;

namespace {
[[noreturn]] void bad(const char* msg) { throw ArgError{TDC_GPU_ERR_ARG, msg}; }

void check_count(size_t n) {
    if (n >= 0xFFFFFFFFull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "at most 2^32 - 2 elements"};
}

template <typename T>
T* upload(Ctx& c, const T* src, size_t n, size_t offset = 0) {
    T* d = c.arena.get<T>(n + offset + 4) + offset;           // (+ 4: never an empty allocation)
    if (n) HIP_TRY(hipMemcpyAsync(d, src, n * sizeof(T), hipMemcpyHostToDevice, c.stream));
    return d;
}
template <typename T>
void download(Ctx& c, T* dst, const T* d_src, size_t n) {
    if (n) HIP_TRY(hipMemcpyAsync(dst, d_src, n * sizeof(T), hipMemcpyDeviceToHost, c.stream));
}

// one bit per destination: every idx[j] < n_dst and no index twice
void check_distinct_indices(const uint32_t* idx, size_t m, size_t n_dst) {
    std::vector<uint64_t> seen((n_dst + 63) / 64, 0);
    for (size_t j = 0; j < m; ++j) {
        const size_t i = idx[j];
        if (i >= n_dst) bad("idx[j] >= n_dst");
        const uint64_t bit = 1ull << (i & 63);
        if (seen[i >> 6] & bit) bad("idx holds an index twice");
        seen[i >> 6] |= bit;
    }
}

template <typename T, typename F>
void scan_entry(Ctx& c, T* data, size_t n, int in_place, T* total, F&& scan) {
    reserve_arena(c, 4 * n * sizeof(T) + ((size_t)64 << 20));
    T* d_in = upload(c, data, n);
    T* d_out = in_place ? d_in : c.arena.get<T>(n + 4);
    T* d_total = total ? c.arena.get<T>(1) : nullptr;
    scan(d_in, d_out, d_total);
    download(c, data, d_out, n);
    if (total) download(c, total, d_total, 1);
    HIP_TRY(hipStreamSynchronize(c.stream));
}

template <typename K, typename F>
void sort_entry(Ctx& c, K* keys, uint32_t* vals, size_t n, F&& sort) {
    reserve_arena(c, 64 * n + ((size_t)256 << 20));
    K* k[2] = { upload(c, keys, n), c.arena.get<K>(n + 4) };
    u32* v[2] = { upload(c, vals, n), c.arena.get<u32>(n + 4) };
    const int x = sort(k, v);
    download(c, keys, k[x], n);
    download(c, vals, v[x], n);
    HIP_TRY(hipStreamSynchronize(c.stream));
}
}  // namespace

extern "C" {

int tdc_gpu_prim_scan(tdc_gpu_ctx* ctx, int op, void* data, size_t n, int in_place, void* total) {
    return guarded(ctx, [&] {
        if (op < 0 || op > 2) bad("op must be 0 (exclusive sum u32), 1 (exclusive sum u64) or 2 (inclusive max u32)");
        if (n && !data) bad("data is NULL");
        if (op == 2 && total) bad("inclusive_max_u32 has no total");
        check_count(n);
        Ctx& c = ctx->c;
        if (op == 0) scan_entry<u32>(c, (u32*)data, n, in_place, (u32*)total, [&](u32* i, u32* o, u32* t) { exclusive_sum_u32(c, i, o, n, t); });
        else if (op == 1) scan_entry<u64>(c, (u64*)data, n, in_place, (u64*)total, [&](u64* i, u64* o, u64* t) { exclusive_sum_u64(c, i, o, n, t); });
        else scan_entry<u32>(c, (u32*)data, n, in_place, nullptr, [&](u32* i, u32* o, u32*) { inclusive_max_u32(c, i, o, n); });
    });
}

int tdc_gpu_prim_sort_pairs(tdc_gpu_ctx* ctx, int kind, void* keys, uint32_t* vals, size_t n, int begin_bit, int end_bit) {
    return guarded(ctx, [&] {
        if (kind < 0 || kind > 2) bad("kind must be 0 (LSD, u32 keys), 1 (LSD, u64 keys) or 2 (distinct u64 keys)");
        if (n && (!keys || !vals)) bad("keys/vals is NULL");
        const int width = kind == 0 ? 32 : 64;
        if (begin_bit < 0 || begin_bit > end_bit) bad("0 <= begin_bit <= end_bit required");
        if (end_bit > width) bad("end_bit exceeds the key width");
        check_count(n);
        if (kind == 2 && n > 1) {
            if (end_bit == begin_bit) bad("keys are not pairwise distinct on the sorted bits (there are none)");
            const u64 mask = (end_bit - begin_bit >= 64) ? ~0ull : ((1ull << (end_bit - begin_bit)) - 1);
            std::vector<u64> f(n);
            for (size_t i = 0; i < n; ++i) f[i] = (((const u64*)keys)[i] >> begin_bit) & mask;
            std::sort(f.begin(), f.end());
            if (std::adjacent_find(f.begin(), f.end()) != f.end()) bad("keys are not pairwise distinct on the sorted bits");
        }
        Ctx& c = ctx->c;
        if (kind == 0) sort_entry<u32>(c, (u32*)keys, vals, n, [&](u32** k, u32** v) { return radix_sort_pairs_u32(c, k, v, n, begin_bit, end_bit); });
        else if (kind == 1) sort_entry<u64>(c, (u64*)keys, vals, n, [&](u64** k, u32** v) { return radix_sort_pairs_u64(c, k, v, n, begin_bit, end_bit); });
        else sort_entry<u64>(c, (u64*)keys, vals, n, [&](u64** k, u32** v) { return sort_pairs_u64_distinct(c, k, v, n, begin_bit, end_bit); });
    });
}

int tdc_gpu_prim_bucketed_scatter(tdc_gpu_ctx* ctx, const uint32_t* idx, const uint32_t* val, size_t m, uint32_t* dst, size_t n_dst,
                                  uint32_t fill, int permutation, int second_tmp, int offset) {
    return guarded(ctx, [&] {
        if ((m && (!idx || !val)) || !dst) bad("idx/val/dst is NULL");
        if (n_dst == 0 || n_dst > ((size_t)1 << 32)) bad("1 <= n_dst <= 2^32 required");
        if (m > n_dst) bad("more pairs than destinations");
        if (offset != 0 && offset != 1) bad("offset must be 0 or 1");
        check_distinct_indices(idx, m, n_dst);
        if (permutation) {
            if (m != n_dst && m + 1 != n_dst) bad("permutation: m must be n_dst or n_dst - 1");
            for (size_t j = 0; j < m; ++j) if (idx[j] >= m) bad("permutation: idx must hold every index of [0, m) once");
        }
        Ctx& c = ctx->c;
        reserve_arena(c, 4 * n_dst + 64 * m + ((size_t)256 << 20));
        const u32* d_idx = upload(c, idx, m, (size_t)offset);
        const u32* d_val = upload(c, val, m, (size_t)offset);
        u32* d_dst = c.arena.get<u32>(n_dst);
        u32* t1 = c.arena.get<u32>(m + 4); u32* tv1 = c.arena.get<u32>(m + 4);
        u32* t2 = second_tmp ? c.arena.get<u32>(m + 4) : nullptr; u32* tv2 = second_tmp ? c.arena.get<u32>(m + 4) : nullptr;
        fill_u32(c, d_dst, n_dst, fill);
        bucketed_scatter_u32(c, d_idx, d_val, m, d_dst, n_dst, t1, tv1, t2, tv2, permutation != 0);
        download(c, dst, d_dst, n_dst);
        HIP_TRY(hipStreamSynchronize(c.stream));
    });
}

int tdc_gpu_prim_msd_partition(tdc_gpu_ctx* ctx, uint32_t* idx, uint32_t* val, size_t m, int bits, int db) {
    return guarded(ctx, [&] {
        if (m && (!idx || !val)) bad("idx/val is NULL");
        if (db != 8 && db != 9) bad("db must be 8 or 9");
        if (bits <= 2 * db || bits > 32) bad("2 * db < bits <= 32 required");
        check_count(m);
        if (bits < 32) for (size_t j = 0; j < m; ++j) if (idx[j] >> bits) bad("idx[j] >= 2^bits");
        if (m == 0) return;
        Ctx& c = ctx->c;
        reserve_arena(c, 64 * m + ((size_t)256 << 20));
        const u32* d_idx = upload(c, idx, m);
        const u32* d_val = upload(c, val, m);
        u32* oi = c.arena.get<u32>(m + 4); u32* ov = c.arena.get<u32>(m + 4);
        u32* ti = c.arena.get<u32>(m + 4); u32* tv = c.arena.get<u32>(m + 4);
        msd_partition_pairs_u32(c, d_idx, d_val, m, bits, db, oi, ov, ti, tv);
        download(c, idx, oi, m);
        download(c, val, ov, m);
        HIP_TRY(hipStreamSynchronize(c.stream));
    });
}

int tdc_gpu_prim_select(tdc_gpu_ctx* ctx, const uint8_t* cls, uint8_t want, size_t m, const uint32_t* srcA, const uint64_t* srcB,
                        uint32_t fillA, uint64_t fillB, uint32_t* outA, uint64_t* outB, uint32_t* count) {
    return guarded(ctx, [&] {
        if (m && (!cls || !outA)) bad("cls/outA is NULL");
        if (!count) bad("count is NULL");
        if (m && ((srcB != nullptr) != (outB != nullptr))) bad("srcB and outB go together");
        check_count(m);
        Ctx& c = ctx->c;
        reserve_arena(c, 32 * m + ((size_t)64 << 20));
        const u8* d_cls = upload(c, cls, m);
        const u32* d_a = srcA ? upload(c, srcA, m) : nullptr;
        const u64* d_b = srcB ? upload(c, srcB, m) : nullptr;
        u32* d_oa = c.arena.get<u32>(m + 4);
        u64* d_ob = srcB ? c.arena.get<u64>(m + 4) : nullptr;
        u32* d_count = c.arena.get<u32>(1);
        fill_u32(c, d_oa, m, fillA);                            // nothing may be written behind the count: the tests see the fill words there
        if (d_ob) {
            std::vector<u64> f(m, fillB);
            if (m) HIP_TRY(hipMemcpyAsync(d_ob, f.data(), m * 8, hipMemcpyHostToDevice, c.stream));
            HIP_TRY(hipStreamSynchronize(c.stream));            // (f leaves scope)
        }
        select_by_class(c, d_cls, want, m, d_a, d_oa, d_b, d_ob, d_count);
        download(c, outA, d_oa, m);
        if (d_ob) download(c, outB, d_ob, m);
        download(c, count, d_count, 1);
        HIP_TRY(hipStreamSynchronize(c.stream));
    });
}

int tdc_gpu_prim_select_counts(tdc_gpu_ctx* ctx, const uint8_t* cls, uint8_t want, size_t m, const uint32_t* srcA, const uint32_t* tile_counts,
                               uint32_t fillA, uint32_t* outA, uint32_t* count) {
    return guarded(ctx, [&] {
        if (m && (!cls || !outA || !tile_counts)) bad("cls/outA/tile_counts is NULL");
        if (!count) bad("count is NULL");
        check_count(m);
        const size_t tiles = (m + SEL_TILE_CLASSES - 1) / SEL_TILE_CLASSES;
        for (size_t t = 0; t < tiles; ++t) {                    // the caller's promise: the counts are those of cls[]
            const size_t e = std::min(m, (t + 1) * SEL_TILE_CLASSES);
            if ((size_t)std::count(cls + t * SEL_TILE_CLASSES, cls + e, want) != tile_counts[t]) bad("tile_counts[t] is not the count of tile t");
        }
        Ctx& c = ctx->c;
        reserve_arena(c, 32 * m + ((size_t)64 << 20));
        const u8* d_cls = upload(c, cls, m);
        const u32* d_a = srcA ? upload(c, srcA, m) : nullptr;
        const u32* d_tc = upload(c, tile_counts, tiles);
        u32* d_oa = c.arena.get<u32>(m + 4);
        u32* d_count = c.arena.get<u32>(1);
        fill_u32(c, d_oa, m, fillA);
        select_by_class(c, d_cls, want, m, d_a, d_oa, nullptr, nullptr, d_count, d_tc);
        download(c, outA, d_oa, m);
        download(c, count, d_count, 1);
        HIP_TRY(hipStreamSynchronize(c.stream));
    });
}

int tdc_gpu_prim_mark_orbit(tdc_gpu_ctx* ctx, const uint32_t* next, size_t n, uint8_t* mark) {
    return guarded(ctx, [&] {
        if (n && (!next || !mark)) bad("next/mark is NULL");
        check_count(n);
        for (size_t i = 0; i < n; ++i) if (next[i] <= i || next[i] > n) bad("i < next[i] <= n required");
        if (n == 0) return;
        Ctx& c = ctx->c;
        reserve_arena(c, 16 * n + ((size_t)64 << 20));
        const u32* d_next = upload(c, next, n);
        u8* d_mark = c.arena.get<u8>(n + 4);
        u32* s1 = c.arena.get<u32>(n + 4); u32* s2 = c.arena.get<u32>(n + 4);
        mark_orbit_u32(c, d_next, n, d_mark, s1, s2);
        download(c, mark, d_mark, n);
        HIP_TRY(hipStreamSynchronize(c.stream));
    });
}

int tdc_gpu_prim_tile_entries(tdc_gpu_ctx* ctx, const uint16_t* exit0, size_t ntiles, uint32_t states, uint16_t* entry0) {
    return guarded(ctx, [&] {
        if (ntiles && (!exit0 || !entry0)) bad("exit0/entry0 is NULL");
        if (states == 0 || states >= DX_NONE) bad("1 <= states < 0xFFFF required");
        if (ntiles > ((size_t)1 << 27)) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "at most 2^27 tiles"};
        for (size_t i = 0; i < ntiles * states; ++i) if (exit0[i] >= states && exit0[i] != DX_NONE) bad("every exit must be < states or 0xFFFF");
        if (ntiles == 0) return;
        Ctx& c = ctx->c;
        reserve_arena(c, 2 * ntiles * states + dx_entries_scratch((u32)ntiles, states) + ((size_t)64 << 20));
        const u16* d_exit = upload(c, exit0, ntiles * states);
        const u16* d_entry = dx_entries(c, d_exit, (u32)ntiles, states, c.arena.alloc(dx_entries_scratch((u32)ntiles, states)));
        download(c, entry0, d_entry, ntiles);
        HIP_TRY(hipStreamSynchronize(c.stream));
    });
}

// Not a primitive: what the arena holds between two calls is chosen by the test (tests/test_gpu_arena_state.py).  top, top_hi and high
// stay as the call before left them.
int tdc_gpu_prim_arena_fill(tdc_gpu_ctx* ctx, int byte, uint64_t* base, uint64_t* size) {
    return guarded(ctx, [&] {
        if (!base || !size) bad("base/size is NULL");
        if (byte > 255) bad("byte must be 0 .. 255, or negative to fill nothing");
        Ctx& c = ctx->c;
        *base = (uint64_t)(uintptr_t)c.arena.base;
        *size = c.arena.base ? (uint64_t)c.arena.size : 0;
        if (byte < 0 || *size == 0) return;
        HIP_TRY(hipMemsetAsync(c.arena.base, byte, c.arena.size, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
    });
}

}  // extern "C"
