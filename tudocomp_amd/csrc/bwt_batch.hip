// bwt_batch.hip -- bwt over a batch of independent texts, both directions ("Batches" and "Batch decoder").
//
// Text k is in[off[k], off[k + 1]), result k lies in the same range of `out`: a transform has its text's length.  The rows of all texts,
// back to back, are ONE row space; a slot or a row is a global index into it.
//
// forward   The suffix sorter of the single call (suffix_array.hip, wsort.hip) rests on ONE smallest byte at n - 1; a concatenation has a
//           0 per text, and the escaped alphabet leaves no byte for separators.  So the batch has a prefix doubling of its own, built
//           from the grid-wide LSD sort (this is the GLOBAL form: one sort over the unresolved positions of all texts per round, not one
//           workgroup per text).  Ranks are global slots -- rank[p] = the first slot of p's group, and the groups of text k lie in
//           [off[k], off[k + 1]) --, so two positions compare by (rank[p], rank[p + h]) and never across texts: nothing carries a text id
//           but pass 0, whose key is (text, the 4 bytes at p, zeros behind the text's end).
//           Invariant: text k ends in its only 0, the smallest byte.  Two suffixes of it that agree in their first h symbols both have
//           p + h <= end_k - 1 (a suffix that holds the terminator among those h symbols differs from every other there), so rank[p + h]
//           is a rank of the same text.  The kernels pad with 0 behind a text's end all the same: they read nothing they do not own
//           whatever the bytes are.
//           A round sorts the positions of groups of two or more; a resolved suffix sits at sa[rank[p]] and is not touched again.  The
//           loop runs at most bits_for(longest accepted text) + 1 times by a counter; what is unresolved then gets TDC_GPU_ERR_INTERNAL.
//           Refused texts (no terminator, an inner 0, too long, empty) take no part: their positions are not selected.
// inverse   LF of all rows by ONE stable sort of the rows by (text, byte): the sorted index of row r is off[k] + C_k[b] + its rank among
//           the equal bytes of text k -- LF in the global row space, a permutation of every text's own rows on any input.  The LF cycles
//           of all texts are one forest of lists: hashed heads over the global rows as in bwt.hip, plus the first row of every accepted
//           text in a slot of its own (T + k).  A walk is cut where it steps ONTO such a row; those targets carry the top bit of their
//           LF word (why the rows of a call stay below 2^31 - 1).  bwt_jump_kernel ranks the heads unchanged.  Text k is a transform iff
//           the list of its first row then ends its cycle with n_k rows.  The byte of a row comes from the buffer itself (b[row]: LF[row]
//           lies in the bucket of b[row], so the search in C of the single call finds that byte) -- no table of count x 257 words.
//
// Nothing reads what the arena held before: every array is written for the positions of the accepted texts before it is read there, and
// the positions of refused texts are read by nobody.  Plain stores only; the atomics are the per-text 0 count (which stops counting behind two), the head counter of the
// first walk and the whole-word loads / stores of the jump.
#include "api.hpp"
#include "decode.hpp"
#include "bwt_passes.hpp"

#include <algorithm>
#include <vector>

namespace tdc {

namespace {

constexpr u64 BWTB_TEXT_CAP = (u64)1 << 20;                           // include/tdc_gpu.h: BWT_BATCH_TEXT_CAP
constexpr u32 LF_CUT = 0x80000000u, LF_ROW = 0x7FFFFFFFu;

// ---- both directions: the text of a row ------------------------------------------------------------------------------------------
// mark[off[k]] = k for every text that has bytes (mark is zero elsewhere); the running maximum is the text of every row
__global__ void __launch_bounds__(256) bwtb_mark_kernel(const u64* __restrict__ off, u32 count, u32* __restrict__ mark) {
    for (u64 k = (u64)blockIdx.x * 256 + threadIdx.x; k < count; k += (u64)gridDim.x * 256)
        if (off[k + 1] > off[k]) mark[off[k]] = (u32)k;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------
// a 0 that does not end its text refuses the text (status is 0 or a verdict of the host; every writer stores the same value)
__global__ void __launch_bounds__(256) bwtb_inner_zero_kernel(const u8* __restrict__ in, u64 n, const u32* __restrict__ tid, const u64* __restrict__ off,
                                                              int* status) {
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) {
        if (in[i] != 0) continue;
        const u32 k = tid[i];
        if (i + 1 != off[k + 1] && status[k] == 0) status[k] = TDC_GPU_ERR_ARG;
    }
}

__global__ void __launch_bounds__(256) bwtb_class_kernel(const u32* __restrict__ tid, const int* __restrict__ status, u64 n, u8* __restrict__ cls) {
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) cls[i] = status[tid[i]] == 0 ? 1 : 0;
}

// pass 0: record t = (text << 32 | the 4 bytes at p, big-endian, zeros behind the text's end; p)
__global__ void __launch_bounds__(256) bwtb_key0_kernel(const u8* __restrict__ in, const u64* __restrict__ off, const u32* __restrict__ tid,
                                                        const u32* __restrict__ U, u64 m, u64* __restrict__ K, u32* __restrict__ V) {
    for (u64 t = (u64)blockIdx.x * 256 + threadIdx.x; t < m; t += (u64)gridDim.x * 256) {
        const u32 p = U[t], k = tid[p];
        const u64 end = off[k + 1];
        u32 w = 0;
#pragma unroll
        for (u32 j = 0; j < 4; ++j) w = (w << 8) | ((u64)p + j < end ? (u32)in[(u64)p + j] : 0u);
        K[t] = ((u64)k << 32) | w;
        V[t] = p;
    }
}

// round h: record t = (rank[p] << 32 | rank[p + h] + 1, 0 behind the text's end; p)
__global__ void __launch_bounds__(256) bwtb_key_kernel(const u32* __restrict__ rank, const u64* __restrict__ off, const u32* __restrict__ tid,
                                                       const u32* __restrict__ U, u64 m, u64 h, u64* __restrict__ K, u32* __restrict__ V) {
    for (u64 t = (u64)blockIdx.x * 256 + threadIdx.x; t < m; t += (u64)gridDim.x * 256) {
        const u32 p = U[t];
        const u64 q = (u64)p + h;
        const u32 r2 = q < off[tid[p] + 1] ? rank[q] + 1u : 0u;
        K[t] = ((u64)rank[p] << 32) | r2;
        V[t] = p;
    }
}

// g1[t] = t where the upper word changes, g2[t] = t where the record's key changes, 0 elsewhere: their running maxima are the first
// record of t's group and of t's subgroup
__global__ void __launch_bounds__(256) bwtb_heads_kernel(const u64* __restrict__ K, u64 m, u32* __restrict__ g1, u32* __restrict__ g2) {
    for (u64 t = (u64)blockIdx.x * 256 + threadIdx.x; t < m; t += (u64)gridDim.x * 256) {
        const u64 a = K[t], b = t ? K[t - 1] : 0ull;
        g1[t] = (t && (a >> 32) == (b >> 32)) ? 0u : (u32)t;
        g2[t] = (t && a == b) ? 0u : (u32)t;
    }
}

// The sorted records take their slots: a group starts at `base` -- its rank, or (FIRST: the group is a text) the text's first slot --
// and record t is its (t - g1[t])-th member; the new rank is the slot of the subgroup's first member.  cls[t] = 1: the subgroup has two
// members or more, p stays unresolved.
template <bool FIRST>
__global__ void __launch_bounds__(256) bwtb_assign_kernel(const u64* __restrict__ K, const u32* __restrict__ V, const u32* __restrict__ g1,
                                                          const u32* __restrict__ g2, u64 m, const u64* __restrict__ off, u32* __restrict__ sa,
                                                          u32* __restrict__ rank, u8* __restrict__ cls) {
    for (u64 t = (u64)blockIdx.x * 256 + threadIdx.x; t < m; t += (u64)gridDim.x * 256) {
        const u32 hi = (u32)(K[t] >> 32), p = V[t];
        const u64 base = FIRST ? off[hi] : (u64)hi;
        const u32 a = g1[t], b = g2[t];
        sa[base + (t - a)] = p;
        rank[p] = (u32)(base + (b - a));
        cls[t] = (b != (u32)t || (t + 1 < m && g2[t + 1] == b)) ? 1 : 0;
    }
}

// the loop bound was reached: the texts of what is unresolved are refused
__global__ void __launch_bounds__(256) bwtb_stuck_kernel(const u32* __restrict__ U, u64 m, const u32* __restrict__ tid, int* status) {
    for (u64 t = (u64)blockIdx.x * 256 + threadIdx.x; t < m; t += (u64)gridDim.x * 256) status[tid[U[t]]] = TDC_GPU_ERR_INTERNAL;
}

// out[j] = T_k[SA_k[i] - 1] (T_k[n_k - 1] where SA_k[i] = 0) for the slots of the accepted texts; sa becomes the text's own positions
__global__ void __launch_bounds__(256) bwtb_gather_kernel(const u8* __restrict__ in, u32* __restrict__ sa, const u32* __restrict__ tid,
                                                          const u64* __restrict__ off, const int* __restrict__ status, u64 n, u8* __restrict__ out) {
    for (u64 j = (u64)blockIdx.x * 256 + threadIdx.x; j < n; j += (u64)gridDim.x * 256) {
        const u32 k = tid[j];
        if (status[k] != 0) continue;
        const u64 a = off[k], p = sa[j];
        out[j] = in[p == a ? off[k + 1] - 1 : p - 1];
        sa[j] = (u32)(p - a);
    }
}

// ---- inverse ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) bwtb_zero_count_kernel(const u8* __restrict__ b, u64 n, const u32* __restrict__ tid, u32* __restrict__ zeros) {
    for (u64 r = (u64)blockIdx.x * 256 + threadIdx.x; r < n; r += (u64)gridDim.x * 256)
        if (b[r] == 0) {                                      // (counted up to "more than one": a buffer of zeros does not queue its rows on one word)
            u32* z = &zeros[tid[r]];
            if (__hip_atomic_load(z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 2u) atomicAdd(z, 1u);
        }
}

// A buffer of 0 or 1 bytes decodes to nothing; one of two or more with another number of 0 bytes than one is refused.  walks[k] = 1: the
// buffer's rows are walked (so far it may be a transform).
__global__ void __launch_bounds__(256) bwtb_accept_kernel(const u64* __restrict__ off, u32 count, const u32* __restrict__ zeros, int* __restrict__ status,
                                                          u8* __restrict__ walks) {
    for (u64 k = (u64)blockIdx.x * 256 + threadIdx.x; k < count; k += (u64)gridDim.x * 256) {
        const u64 nk = off[k + 1] - off[k];
        const bool w = nk >= 2 && zeros[k] == 1;
        walks[k] = w ? 1 : 0;
        status[k] = (nk >= 2 && !w) ? TDC_GPU_ERR_ARG : 0;
    }
}

__global__ void __launch_bounds__(256) bwtb_lf_key_kernel(const u8* __restrict__ b, const u32* __restrict__ tid, u64 n, u64* __restrict__ K,
                                                          u32* __restrict__ V) {
    for (u64 r = (u64)blockIdx.x * 256 + threadIdx.x; r < n; r += (u64)gridDim.x * 256) { K[r] = ((u64)tid[r] << 8) | b[r]; V[r] = (u32)r; }
}

// the row at sorted index t has LF = t; the target that is the first row of a walked buffer is marked
__global__ void __launch_bounds__(256) bwtb_lf_kernel(const u32* __restrict__ V, u64 n, const u32* __restrict__ tid, const u64* __restrict__ off,
                                                      const u8* __restrict__ walks, u32* __restrict__ lf) {
    for (u64 t = (u64)blockIdx.x * 256 + threadIdx.x; t < n; t += (u64)gridDim.x * 256) {
        const u32 k = tid[t];
        lf[V[t]] = (u32)t | ((walks[k] && off[k] == t) ? LF_CUT : 0u);
    }
}

// slots [0, T): the hashed rows that lie in a walked buffer and are not its first row; slots [T, T + count): the first rows
__global__ void __launch_bounds__(256) bwtb_heads_init_kernel(Heads H, Mix m, u64 n, u32 count, const u32* __restrict__ tid, const u64* __restrict__ off,
                                                              const u8* __restrict__ walks) {
    const u64 slots = (u64)m.T + count;
    for (u64 kk = (u64)blockIdx.x * 256 + threadIdx.x; kk < slots; kk += (u64)gridDim.x * 256) {
        u32 row = NONE32;
        if (kk < m.T) {
            const u32 r = unmix((u32)kk, m);
            if (r < n) { const u32 k = tid[r]; if (walks[k] && off[k] != r) row = r; }
        } else {
            const u32 k = (u32)(kk - m.T);
            if (walks[k]) row = (u32)off[k];
        }
        H.hrow[kk] = row;
        H.hlen[kk] = 0;
        H.w[kk] = W_END;
    }
}

// First walk, slots [lo, hi): follow LF from the head until the step onto a buffer's first row (the cycle is cut there: the list ends),
// onto a hashed head, or max_steps steps -- then the row reached becomes a head of its own behind the slots in use, for the next launch.
// LF maps a buffer's rows onto themselves, so a walk never leaves the buffer of its head and the lists are disjoint.
__global__ void __launch_bounds__(256) bwtb_walk1_kernel(const u32* __restrict__ lf, Heads H, Mix m, u32 lo, u32 hi, u32 max_steps) {
    u32 longest = 0;
    for (u64 kk = (u64)lo + (u64)blockIdx.x * 256 + threadIdx.x; kk < hi; kk += (u64)gridDim.x * 256) {
        const u32 k = (u32)kk;
        u32 cur = H.hrow[k];
        if (cur == NONE32) continue;
        u32 steps = 0, link = NONE32;
        for (;;) {                                            // (at most max_steps turns)
            const u32 raw = lf[cur];
            cur = raw & LF_ROW;
            ++steps;
            if (raw & LF_CUT) break;
            const u32 g = mix(cur, m);
            if (g < m.T) { link = g; break; }
            if (steps == max_steps) {
                const u32 id = atomicAdd(&H.cnt[0], 1u);
                if (id < H.cap) { H.hrow[id] = cur; link = id; }
                else atomicOr(&H.cnt[2], 1u);
                break;
            }
        }
        H.hlen[k] = steps;
        H.w[k] = ((u64)link << 32) | steps;
        longest = max(longest, steps);
    }
    longest = wave_reduce_max(longest);
    if (lane_id() == 0 && longest) atomicMax(&H.cnt[1], longest);
}

// buffer k is a transform iff the list of its first row ends its cycle with n_k rows
__global__ void __launch_bounds__(256) bwtb_verdict_kernel(Heads H, u32 T, const u64* __restrict__ off, u32 count, const u8* __restrict__ walks,
                                                           int* __restrict__ status) {
    for (u64 k = (u64)blockIdx.x * 256 + threadIdx.x; k < count; k += (u64)gridDim.x * 256)
        if (walks[k] && H.w[(u64)T + k] != (W_END | (off[k + 1] - off[k]))) status[k] = TDC_GPU_ERR_ARG;
}

// Second walk over the heads of the transforms: the head of a slot starts n_k - w rows behind its buffer's first row; the row t behind
// the first row puts its byte at n_k - 2 - t of the text (the last row of the cycle holds the 0 that ends the text).  Positions fall by
// one per step: the bytes are collected into aligned words of the global position.
__global__ void __launch_bounds__(256) bwtb_walk2_kernel(const u32* __restrict__ lf, const u8* __restrict__ b, Heads H, u32 slots,
                                                         const u32* __restrict__ tid, const u64* __restrict__ off, const int* __restrict__ status,
                                                         u8* __restrict__ out) {
    for (u64 kk = (u64)blockIdx.x * 256 + threadIdx.x; kk < slots; kk += (u64)gridDim.x * 256) {
        const u32 k = (u32)kk;
        u32 cur = H.hrow[k];
        if (cur == NONE32) continue;
        const u32 text = tid[cur];
        if (status[text] != 0) continue;
        const u64 w = H.w[k];
        if ((w & W_END) != W_END) continue;                   // (never for a transform: all its lists end the cycle)
        const u64 base = off[text];
        const u32 nk = (u32)(off[text + 1] - base);
        const u32 len = H.hlen[k];
        const u32 r = nk - (u32)w;
        u32 acc = 0, hi = 0;
        bool open = false;                                    // a word is being filled: byte lanes (pos & 3) .. hi are in acc
        size_t pos = 0;
        for (u32 j = 0; j < len; ++j) {
            const u32 c = b[cur];
            const u32 t = r + j;
            if (t > nk - 2) { out[base + nk - 1] = (u8)c; break; }   // (the row of the 0: the last step of the last list)
            pos = (size_t)(base + nk - 2 - t);
            const u32 ln = (u32)pos & 3u;
            if (!open) { open = true; hi = ln; acc = 0; }
            acc |= c << (8 * ln);
            if (ln == 0) { put_bytes(out, pos, acc, 0, hi); open = false; }
            cur = lf[cur] & LF_ROW;
        }
        if (open) put_bytes(out, pos & ~(size_t)3, acc, (u32)pos & 3u, hi);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// the text of every row: tid (n entries); scratch: n entries
void bwtb_text_ids(Ctx& c, const u64* d_off, size_t count, size_t n, u32* scratch, u32* tid) {
    HIP_TRY(hipMemsetAsync(scratch, 0, n * sizeof(u32), c.stream));
    bwtb_mark_kernel<<<dec_grid(count), 256, 0, c.stream>>>(d_off, (u32)count, scratch);
    LAUNCH_CHECK();
    inclusive_max_u32(c, scratch, tid, n);
}

// Results of the texts with ok[k] != 0 from the device image `d` (elements of the global row space) into the same ranges of `host`;
// the other ranges are left alone.  Runs of neighbours travel in one copy; a batch cut into many runs goes through one staging copy.
template <typename T>
void bwtb_download(Ctx& c, const T* d, T* host, const uint64_t* off, size_t count, const std::vector<u8>& ok) {
    std::vector<std::pair<u64, u64>> runs;
    for (size_t k = 0; k < count; ++k) {
        const u64 a = off[k], b = off[k + 1];
        if (a == b || !ok[k]) continue;
        if (!runs.empty() && runs.back().second == a) runs.back().second = b;
        else runs.push_back({a, b});
    }
    if (runs.size() <= 64) {
        for (const auto& r : runs) HIP_TRY(hipMemcpyAsync(host + r.first, d + r.first, (size_t)(r.second - r.first) * sizeof(T), hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        return;
    }
    const u64 lo = runs.front().first, hi = runs.back().second;
    std::vector<T> stage((size_t)(hi - lo));
    HIP_TRY(hipMemcpyAsync(stage.data(), d + lo, stage.size() * sizeof(T), hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    for (const auto& r : runs) memcpy(host + r.first, stage.data() + (r.first - lo), (size_t)(r.second - r.first) * sizeof(T));
}

// ... and the inverse (sample / steps at the library's choice or smaller lists: more heads)
size_t bwtb_inverse_arena(size_t n, size_t count, size_t cap) { return 40 * n + 32 * count + 16 * cap + ((size_t)64 << 20); }

}  // namespace

// ---- what the entry points call (api.hpp; api_compress.hip, api_decompress.hip, api_chain.hip) ------------------------------------------
// what the forward call takes from the arena for n bytes in count texts (DESIGN.md section 5.2 "Batches" states it)
size_t bwtb_forward_arena(size_t n, size_t count) { return 64 * n + 64 * count + ((size_t)64 << 20); }

// the refusals decided from the arguments alone; throws ArgError
void bwtb_check(const uint8_t* in, const uint64_t* off, size_t count, const void* out, size_t out_cap, size_t elem, const int32_t* status, u64 total_max) {
    if (!off || !status) throw ArgError{TDC_GPU_ERR_ARG, "bwt batch: NULL argument"};
    if (off[0] != 0) throw ArgError{TDC_GPU_ERR_ARG, "bwt batch: off[0] must be 0"};
    for (size_t k = 0; k < count; ++k)
        if (off[k + 1] < off[k]) throw ArgError{TDC_GPU_ERR_ARG, "bwt batch: off must not decrease"};
    const u64 n = off[count];
    if (!in && n) throw ArgError{TDC_GPU_ERR_ARG, "bwt batch: NULL argument"};
    if (n > total_max || count > 0x7FFFFFFFull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "bwt batch: too many bytes or texts in one call"};
    if (out && n) {                                           // (of a size that is taken: the ranges are real)
        const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
        if (a < b + std::min<u64>(out_cap, n) * elem && b < a + n) throw ArgError{TDC_GPU_ERR_ARG, "bwt batch: out overlaps in"};
    }
}

// the verdict on text k that needs no device: the codes of tdc_gpu_bwt_compress in its order, but for the cap of one text in a batch
static int bwtb_host_status(const uint8_t* in, const uint64_t* off, size_t k) {
    const u64 nk = off[k + 1] - off[k];
    if (nk == 0) return TDC_GPU_ERR_NO_SENTINEL;
    if (nk > BWTB_TEXT_CAP) return TDC_GPU_ERR_TOO_LARGE;
    return in[off[k + 1] - 1] != 0 ? TDC_GPU_ERR_NO_SENTINEL : TDC_GPU_OK;
}

// out (nullable): the transforms; sa_out (nullable): the suffix arrays; keep (nullable): neither -- the transforms stay in the arena, which
// the caller has reserved
void bwtb_forward(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* off, size_t count, uint8_t* out, size_t out_cap, bool want_out, uint32_t* sa_out,
                  int32_t* status, tdc_gpu_stats* stats, BwtbKeep* keep) {
    Ctx& c = ctx->c;
    if (stats) memset(stats, 0, sizeof(*stats));
    const size_t n = (size_t)off[count];
    u64 longest = 0;
    for (size_t k = 0; k < count; ++k) {
        status[k] = bwtb_host_status(in, off, k);
        if (!status[k]) longest = std::max<u64>(longest, off[k + 1] - off[k]);
    }
    if (want_out && n && (!out || out_cap < n)) throw ArgError{TDC_GPU_ERR_OOM, "bwt batch: output buffer too small (off[count] bytes are needed)"};
    if (!want_out && n && !sa_out && !keep) throw ArgError{TDC_GPU_ERR_ARG, "bwt batch: NULL argument"};
    if (count == 0 || n == 0) return;
    if (!keep) reserve_arena(c, bwtb_forward_arena(n, count));
    hipStream_t s = c.stream;
    Events ev(c);
    const int e0 = ev.tick();
    u8* d_in = upload_plain(c, in, n);
    u64* d_off = c.arena.get<u64>(count + 1);
    int* d_status = c.arena.get<int>(count);
    HIP_TRY(hipMemcpyAsync(d_off, off, (count + 1) * sizeof(u64), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_status, status, count * sizeof(int), hipMemcpyHostToDevice, s));
    const int e1 = ev.tick();
    u32* tid = c.arena.get<u32>(n);
    u32* rank = c.arena.get<u32>(n);                          // (first the scratch of the text ids)
    u32* sa = c.arena.get<u32>(n);
    u32* U = c.arena.get<u32>(n);
    u8* cls = c.arena.get<u8>(n + 8);
    u32* d_cnt = c.arena.get<u32>(4);
    bwtb_text_ids(c, d_off, count, n, rank, tid);
    bwtb_inner_zero_kernel<<<dec_grid(n), 256, 0, s>>>(d_in, n, tid, d_off, d_status);
    LAUNCH_CHECK();
    bwtb_class_kernel<<<dec_grid(n), 256, 0, s>>>(tid, d_status, n, cls);
    LAUNCH_CHECK();
    select_by_class(c, cls, 1, n, nullptr, U, nullptr, nullptr, d_cnt);
    size_t m = c.read(d_cnt);
    u32 rounds = 0;
    u64 sorted = 0;
    if (m) {
        u64* K[2] = { c.arena.get<u64>(m), c.arena.get<u64>(m) };
        u32* V[2] = { c.arena.get<u32>(m), c.arena.get<u32>(m) };
        u32* g1 = c.arena.get<u32>(m);
        u32* g2 = c.arena.get<u32>(m);
        const u32 bound = (u32)bits_for(longest) + 1;
        const int rbits = (int)bits_for(n);                   // a rank + 1 is at most n
        u64 h = 4;
        for (bool first = true; m; first = false) {
            if (!first && rounds == bound) {                  // (the invariant says: never)
                bwtb_stuck_kernel<<<dec_grid(m), 256, 0, s>>>(U, m, tid, d_status);
                LAUNCH_CHECK();
                break;
            }
            const u64* Ks; const u32* Vs;
            if (first) {
                bwtb_key0_kernel<<<dec_grid(m), 256, 0, s>>>(d_in, d_off, tid, U, m, K[0], V[0]);
                LAUNCH_CHECK();
                const int x = radix_sort_pairs_u64(c, K, V, m, 0, 32 + (int)bits_for(count - 1));
                Ks = K[x]; Vs = V[x];
            } else {
                bwtb_key_kernel<<<dec_grid(m), 256, 0, s>>>(rank, d_off, tid, U, m, h, K[0], V[0]);
                LAUNCH_CHECK();
                // stable: by the lower word, then by the upper one
                const int x = radix_sort_pairs_u64(c, K, V, m, 0, rbits);
                u64* K2[2] = { K[x], K[x ^ 1] };
                u32* V2[2] = { V[x], V[x ^ 1] };
                const int y = radix_sort_pairs_u64(c, K2, V2, m, 32, 32 + rbits);
                Ks = K2[y]; Vs = V2[y];
                h *= 2;
                ++rounds;
            }
            sorted += m;
            bwtb_heads_kernel<<<dec_grid(m), 256, 0, s>>>(Ks, m, g1, g2);
            LAUNCH_CHECK();
            inclusive_max_u32(c, g1, g1, m);
            inclusive_max_u32(c, g2, g2, m);
            if (first) bwtb_assign_kernel<true><<<dec_grid(m), 256, 0, s>>>(Ks, Vs, g1, g2, m, d_off, sa, rank, cls);
            else bwtb_assign_kernel<false><<<dec_grid(m), 256, 0, s>>>(Ks, Vs, g1, g2, m, d_off, sa, rank, cls);
            LAUNCH_CHECK();
            select_by_class(c, cls, 1, m, Vs, U, nullptr, nullptr, d_cnt);
            m = c.read(d_cnt);
        }
    }
    const int e2 = ev.tick();
    u8* d_out = c.arena.get<u8>(n + 64);
    bwtb_gather_kernel<<<dec_grid(n), 256, 0, s>>>(d_in, sa, tid, d_off, d_status, n, d_out);
    LAUNCH_CHECK();
    const int e3 = ev.tick();
    c.read_n(d_status, (int*)status, count);
    std::vector<u8> ok(count);
    for (size_t k = 0; k < count; ++k) ok[k] = status[k] == 0;
    if (want_out) bwtb_download(c, d_out, out, off, count, ok);
    if (sa_out) bwtb_download(c, sa, sa_out, off, count, ok);
    if (keep) keep->d_out = d_out;
    const int e4 = ev.tick();
    if (stats) {
        stats->n = n; stats->out_len = n; stats->arena_bytes = c.arena.high;
        stats->len_rounds = rounds; stats->sa_rounds = rounds + 1; stats->sa_init_syms = 4; stats->sa_sorted_elems = sorted;
        ev.span(&stats->ms_h2d, e0, e1); ev.span(&stats->ms_sa, e1, e2); ev.span(&stats->ms_encode, e2, e3);
        ev.span(&stats->ms_d2h, e3, e4); ev.span(&stats->ms_total, e0, e4);
    }
    ev.finish();
}

void bwtb_inverse(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* off, size_t count, uint8_t* out, size_t out_cap, int32_t* status,
                  tdc_gpu_stats* stats) {
    Ctx& c = ctx->c;
    if (stats) memset(stats, 0, sizeof(*stats));
    const size_t n = (size_t)off[count];
    for (size_t k = 0; k < count; ++k) status[k] = TDC_GPU_OK;    // (what the lengths alone say: a buffer of 0 or 1 bytes decodes to nothing)
    if (n && (!out || out_cap < n)) throw ArgError{TDC_GPU_ERR_OOM, "bwt batch: output buffer too small (off[count] bytes are needed)"};
    if (count == 0 || n == 0) return;
    const u32 S = c.bwt_batch_sample ? (u32)c.bwt_batch_sample : BWT_SAMPLE;
    const u32 M = c.bwt_batch_steps ? (u32)c.bwt_batch_steps : (u32)std::min<u64>((u64)BWT_STEPS_PER_SAMPLE * S, 0x7FFFFFFFull);
    const Mix mx = make_mix(n, S);
    const u64 cap64 = (u64)mx.T + count + n / M + 2;          // hashed slots + first rows + one per max_steps rows walked
    if (cap64 > 0xFFFFFFFEull) throw ArgError{TDC_GPU_ERR_TOO_LARGE, "bwt batch: too many list heads (option bwt_batch_sample / bwt_batch_steps)"};
    const size_t cap = (size_t)cap64;
    reserve_arena(c, bwtb_inverse_arena(n, count, cap));
    hipStream_t s = c.stream;
    Events ev(c);
    const int e0 = ev.tick();
    u8* d_b = upload_plain(c, in, n);
    u64* d_off = c.arena.get<u64>(count + 1);
    HIP_TRY(hipMemcpyAsync(d_off, off, (count + 1) * sizeof(u64), hipMemcpyHostToDevice, s));
    const int e1 = ev.tick();
    int* d_status = c.arena.get<int>(count);
    u32* zeros = c.arena.get<u32>(count);
    u8* walks = c.arena.get<u8>(count);
    u32* tid = c.arena.get<u32>(n);
    u32* lf = c.arena.get<u32>(n);                            // (first the scratch of the text ids)
    u8* d_out = c.arena.get<u8>(n + 64);
    Heads H;
    H.cnt = c.arena.get<u32>(4);
    H.hrow = c.arena.get<u32>(cap); H.hlen = c.arena.get<u32>(cap); H.w = (unsigned long long*)c.arena.get<u64>(cap);
    H.cap = (u32)cap;
    bwtb_text_ids(c, d_off, count, n, lf, tid);
    HIP_TRY(hipMemsetAsync(zeros, 0, count * sizeof(u32), s));
    bwtb_zero_count_kernel<<<dec_grid(n), 256, 0, s>>>(d_b, n, tid, zeros);
    LAUNCH_CHECK();
    bwtb_accept_kernel<<<dec_grid(count), 256, 0, s>>>(d_off, (u32)count, zeros, d_status, walks);
    LAUNCH_CHECK();
    {   // LF: one stable sort of the rows by (text, byte)
        const size_t mk = c.arena.mark();
        u64* K[2] = { c.arena.get<u64>(n), c.arena.get<u64>(n) };
        u32* V[2] = { c.arena.get<u32>(n), c.arena.get<u32>(n) };
        bwtb_lf_key_kernel<<<dec_grid(n), 256, 0, s>>>(d_b, tid, n, K[0], V[0]);
        LAUNCH_CHECK();
        const int x = radix_sort_pairs_u64(c, K, V, n, 0, 8 + (int)bits_for(count - 1));
        bwtb_lf_kernel<<<dec_grid(n), 256, 0, s>>>(V[x], n, tid, d_off, walks, lf);
        LAUNCH_CHECK();
        HIP_TRY(hipStreamSynchronize(s));                     // (the records go back to the arena)
        c.arena.release(mk);
    }
    const int e2 = ev.tick();
    // first walk, launch by launch until no list is left open
    const u32 first_slots = mx.T + (u32)count;
    const u32 init[4] = { first_slots, 0, 0, 0 };
    HIP_TRY(hipMemcpyAsync(H.cnt, init, sizeof(init), hipMemcpyHostToDevice, s));
    bwtb_heads_init_kernel<<<dec_grid(first_slots), 256, 0, s>>>(H, mx, n, (u32)count, tid, d_off, walks);
    LAUNCH_CHECK();
    u32 lo = 0, hi = first_slots, launches = 0;
    u32 hc[4] = { 0, 0, 0, 0 };
    while (lo < hi) {
        bwtb_walk1_kernel<<<dec_grid(hi - lo), 256, 0, s>>>(lf, H, mx, lo, hi, M);
        LAUNCH_CHECK();
        ++launches;
        c.read_n(H.cnt, hc, 4);
        if (hc[2] || hc[0] > H.cap) throw HipError{hipErrorUnknown, "bwt batch: head table overflow", (int)__LINE__};
        lo = hi; hi = hc[0];
    }
    const u32 slots = hi;
    // ranks of the heads; the lists of a buffer that is no transform may still change when the bound is reached: its verdict, not the call's
    const u32 bound = (u32)bits_for(slots) + 2;
    u32 rounds = 0;
    while (rounds < bound) {
        HIP_TRY(hipMemsetAsync(H.cnt + 3, 0, sizeof(u32), s));
        bwt_jump_kernel<<<dec_grid(slots), 256, 0, s>>>(H, slots);
        LAUNCH_CHECK();
        ++rounds;
        if (c.read(H.cnt + 3) == 0) break;
    }
    bwtb_verdict_kernel<<<dec_grid(count), 256, 0, s>>>(H, mx.T, d_off, (u32)count, walks, d_status);
    LAUNCH_CHECK();
    bwtb_walk2_kernel<<<dec_grid(slots), 256, 0, s>>>(lf, d_b, H, slots, tid, d_off, d_status, d_out);
    LAUNCH_CHECK();
    const int e3 = ev.tick();
    c.read_n(d_status, (int*)status, count);
    std::vector<u8> ok(count);
    u64 written = 0;
    for (size_t k = 0; k < count; ++k) {
        const u64 nk = off[k + 1] - off[k];
        ok[k] = status[k] == 0 && nk >= 2;
        if (ok[k]) written += nk;
    }
    bwtb_download(c, d_out, out, off, count, ok);
    const int e4 = ev.tick();
    if (stats) {
        stats->n = n; stats->out_len = written; stats->arena_bytes = c.arena.high;
        stats->len_rounds = rounds; stats->levels = launches; stats->entries = slots; stats->flen_max = hc[1];
        ev.span(&stats->ms_h2d, e0, e1); ev.span(&stats->ms_sa, e1, e2); ev.span(&stats->ms_encode, e2, e3);
        ev.span(&stats->ms_d2h, e3, e4); ev.span(&stats->ms_total, e0, e4);
    }
    ev.finish();
    ctx->last_decode_device = 1;
}

}  // namespace tdc
