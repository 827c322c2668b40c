// repair.hip -- repair = RePairCompressor (compressors/RePairCompressor.hpp:96-178): the Re-Pair grammar built on the device (DESIGN.md
// section 5.8).  The host loop that specifies it: repair_host.cpp (tdc_repair_grammar); the passes below are stated once more, executable,
// as device_grammar() of tests/models/repair.py.
//
// State: the live sequence S[0 .. m) as a compacted u32 array (symbols 0 .. 255 are bytes, 256 + k is rule k) and a digram table in HBM --
// open addressing with linear probing, 64-bit keys l << 32 | r claimed with atomicCAS, u32 counts -- that holds the EXACT overlapping count
// of every adjacent pair of S.  A key never leaves its slot; a count that falls to 0 keeps the slot until the table is rebuilt.
//
// One round (one rule):
//   argmax     M = the largest count, T = the number of entries that hold it, one such key, whether one of them is a square (l == r);
//              one read-back through mapped host memory together with m and the table's fill.  M <= 1 ends the loop.
//   tie pass   (T > 1) the reference takes a pair over when its running count exceeds the best so far STRICTLY, so among the pairs that
//              count M the one whose M-th occurrence comes first wins.  The positions whose pair counts M are selected in position order
//              (T * M of them), stable-sorted by key; every group has exactly M members, the last one is that pair's M-th occurrence;
//              the group whose last position is smallest wins.
//   mark       l != r: every occurrence is taken.  l == r: the reference replaces left to right and goes on BEHIND a replaced pair, so a
//              maximal run of k takes floor(k / 2) pairs from its left end: run starts by an inclusive max over start markers, a position
//              is taken iff its offset in the run is even and a partner follows.
//   deltas     a taken occurrence owns its left boundary, and its right one unless the pair behind it is taken too: the old neighbour
//              pair loses one, the new one -- (x, A), (A, y), or (A, A) between two taken pairs -- gains one (new keys are inserted).  The
//              winner's entry is cleared and deltas that name it are dropped: no occurrence of it survives a round.
//   compact    keep flags, selection in position order; 256 + k stands where a taken pair began.
// The table is rebuilt by a recount of S, at twice the size, when a round could fill it beyond half; the recount drops the slots whose
// count had fallen to 0, and a table the live pairs would fill to less than an eighth is made to fit them.  Option repair_recount = 1
// rebuilds it in every round instead of applying the deltas.
//
// The grammar then goes through repair_encode: the cost pass, scan, pack and terminator of field_coder.hpp over RpFields (repair_fields.hpp).
#include "stages.hpp"
#include "field_coder.hpp"
#include "repair_fields.hpp"
#include "decode.hpp"

#include <chrono>
#include <stdio.h>

namespace tdc {

namespace {

constexpr unsigned long long RP_EMPTY = ~0ull;
constexpr u32 RP_ERR_FULL = 1, RP_ERR_TIE = 2, RP_ERR_MISSING = 4;

struct RpTable { unsigned long long* keys; u32* counts; u32 shift, mask; };      // 2^(64 - shift) = mask + 1 slots

// what a round reads back (16 words)
struct RpState {
    u32 M, T, sq, key_hi, key_lo;       // argmax
    u32 occupied, err;                  // slots claimed since the table was cleared; RP_ERR_*
    u32 m;                              // length of the live sequence
    u32 minpos, tiecnt;                 // tie pass
    u32 win_hi, win_lo;                 // the round's rule
    u32 pad[4];
};
static_assert(sizeof(RpState) == 64, "RpState: sixteen words");

__device__ __forceinline__ u64 rp_key(u32 l, u32 r) { return (u64)l << 32 | r; }
__device__ __forceinline__ u32 rp_slot0(const RpTable& t, u64 key) { return (u32)((key * 0x9E3779B97F4A7C15ull) >> t.shift); }

// the slot of a key that was in the table before the kernel began (slots in front of it were claimed before it and stay claimed)
__device__ __forceinline__ u32 rp_find(const RpTable& t, u64 key) {
    u32 h = rp_slot0(t, key);
    for (u32 probes = 0; probes <= t.mask; ++probes, h = (h + 1) & t.mask) {
        const u64 k = t.keys[h];
        if (k == key) return h;
        if (k == RP_EMPTY) return RP_NONE;
    }
    return RP_NONE;
}

// count(key) += d, the key inserted if it is new.  A slot changes once, from empty to its key: a stale read can only show `empty`, and
// the CAS then returns what is really there.
__device__ __forceinline__ void rp_add(const RpTable& t, u64 key, u32 d, RpState* st) {
    u32 h = rp_slot0(t, key);
    for (u32 probes = 0; probes <= t.mask; ++probes, h = (h + 1) & t.mask) {
        unsigned long long k = t.keys[h];
        if (k == RP_EMPTY) {
            k = atomicCAS(&t.keys[h], RP_EMPTY, (unsigned long long)key);
            if (k == RP_EMPTY) { atomicAdd(&st->occupied, 1u); k = key; }
        }
        if (k == key) { atomicAdd(&t.counts[h], d); return; }
    }
    atomicOr(&st->err, RP_ERR_FULL);
}

// ---- the first count, from the bytes ---------------------------------------------------------------------------------------------------
// The pairs of a text are 16-bit numbers and a few hundred of them take most of the occurrences: a workgroup counts its chunk in LDS --
// four passes over the chunk (it stays in L2), one per quarter of the first byte's values, 16384 counters each -- and adds the counters
// that are not 0 to a dense histogram in HBM, whose entries then go into the table once.
constexpr u32 RP_CHUNK = 1u << 18;
__global__ __launch_bounds__(256) void rp_byte_pairs_kernel(const u8* __restrict__ text, u64 n, u32* __restrict__ hist) {
    __shared__ u32 h[16384];
    const u64 p0 = (u64)blockIdx.x * RP_CHUNK;
    const u64 p1 = p0 + RP_CHUNK < n - 1 ? p0 + RP_CHUNK : n - 1;        // pairs start at [p0, p1); n >= 2
    for (u32 q = 0; q < 4; ++q) {
        for (u32 k = threadIdx.x; k < 16384; k += 256) h[k] = 0;
        __syncthreads();
        for (u64 p = p0 + 8ull * threadIdx.x; p < p1; p += 8 * 256) {    // (p0 and the text are 8-byte aligned)
            u64 w;
            u32 nxt = 0;
            if (p + 8 < n) { w = *(const u64*)(text + p); nxt = text[p + 8]; }
            else { w = 0; for (u32 b = 0; b < 8 && p + b < n; ++b) w |= (u64)text[p + b] << (8 * b); }
#pragma unroll
            for (u32 b = 0; b < 8; ++b) {
                const u32 x = (u32)(w >> (8 * b)) & 255u, y = b < 7 ? (u32)(w >> (8 * b + 8)) & 255u : nxt;
                if (p + b < p1 && (x >> 6) == q) atomicAdd(&h[((x & 63u) << 8) | y], 1u);
            }
        }
        __syncthreads();
        for (u32 k = threadIdx.x; k < 16384; k += 256) { const u32 v = h[k]; if (v) atomicAdd(&hist[(q << 14) | k], v); }
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void rp_hist_insert_kernel(const u32* __restrict__ hist, RpTable t, RpState* st) {
    const u32 k = blockIdx.x * 256 + threadIdx.x;                         // < 65536
    const u32 v = hist[k];
    if (v) rp_add(t, rp_key(k >> 8, k & 255u), v, st);
}
__global__ __launch_bounds__(256) void rp_widen_kernel(const u8* __restrict__ text, u64 n, u32* __restrict__ S) {
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) S[i] = text[i];
}
// the recount of a live sequence (its length is on the device: the kernel runs behind the compaction that set it)
__global__ __launch_bounds__(256) void rp_count_kernel(const u32* __restrict__ S, RpTable t, RpState* st) {
    const u64 m = st->m, stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i + 1 < m; i += stride) rp_add(t, rp_key(S[i], S[i + 1]), 1u, st);
}

// ---- argmax --------------------------------------------------------------------------------------------------------------------------------
__global__ void rp_round_begin_kernel(RpState* st) {
    st->M = 0; st->T = 0; st->sq = 0; st->key_hi = 0; st->key_lo = 0; st->minpos = RP_NONE; st->tiecnt = 0;
}
// Both passes run on at most RP_ARGMAX_BLOCKS workgroups and send one atomic per workgroup: atomics on one address are served one after
// the other, and a wave's worth of them per 64 slots made the first pass the longest kernel of a round by far.
constexpr unsigned RP_ARGMAX_BLOCKS = 512;
__global__ __launch_bounds__(256) void rp_max_kernel(RpTable t, RpState* st) {
    __shared__ u32 sm[4];
    const u64 cap = (u64)t.mask + 1, stride = (u64)gridDim.x * 256;
    u32 mx = 0;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < cap; i += stride) mx = max(mx, t.counts[i]);
    mx = wave_reduce_max(mx);
    if (lane_id() == 0) sm[wave_id()] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        mx = max(max(sm[0], sm[1]), max(sm[2], sm[3]));
        if (mx) atomicMax(&st->M, mx);
    }
}
// T, whether a square is among the entries that hold M, and one of their keys (T > 1: the halves may come from two of them -- the tie
// pass finds the winner then, the key is not read)
__global__ __launch_bounds__(256) void rp_tied_kernel(RpTable t, RpState* st) {
    __shared__ u32 sm[4];
    const u32 M = st->M;
    if (M <= 1) return;
    const u64 cap = (u64)t.mask + 1, stride = (u64)gridDim.x * 256;
    u32 cnt = 0, sq = 0;
    u64 key = RP_EMPTY;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < cap; i += stride) {
        if (t.counts[i] != M) continue;
        key = t.keys[i];
        ++cnt;
        sq |= (u32)(key >> 32) == (u32)key ? 1u : 0u;
    }
    if (cnt) { st->key_hi = (u32)(key >> 32); st->key_lo = (u32)key; }
    if (sq) st->sq = 1u;
    cnt = wave_reduce_sum(cnt);
    if (lane_id() == 0) sm[wave_id()] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) { cnt = sm[0] + sm[1] + sm[2] + sm[3]; if (cnt) atomicAdd(&st->T, cnt); }
}

// ---- tie pass ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rp_tie_class_kernel(const u32* __restrict__ S, u32 m, RpTable t, const RpState* __restrict__ st,
                                                            u8* __restrict__ cls) {
    const u32 M = st->M;
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i + 1 < m; i += stride) {
        const u32 h = rp_find(t, rp_key(S[i], S[i + 1]));
        cls[i] = (h != RP_NONE && t.counts[h] == M) ? 1 : 0;
    }
}
// sort key of a selected position: l and r in `bits` bits each (every symbol so far is below 2^bits)
__global__ __launch_bounds__(256) void rp_tie_keys_kernel(const u32* __restrict__ S, u32 m, const u32* __restrict__ pos, u32 cnt, u32 bits,
                                                           u64* __restrict__ keys) {
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 j = (u64)blockIdx.x * 256 + threadIdx.x; j < cnt; j += stride) {
        const u32 p = pos[j];
        keys[j] = p + 1 < m ? ((u64)S[p] << bits) | S[p + 1] : ~0ull;     // (p + 1 >= m: not a selected position -- rp_winner_kernel reports it)
    }
}
__global__ __launch_bounds__(256) void rp_tie_min_kernel(const u32* __restrict__ vals, u32 T, u32 M, RpState* st) {
    const u64 stride = (u64)gridDim.x * 256;
    u32 mn = RP_NONE;
    for (u64 g = (u64)blockIdx.x * 256 + threadIdx.x; g < T; g += stride) mn = min(mn, vals[g * M + M - 1]);
    mn = wave_reduce_min(mn);
    if (lane_id() == 0 && mn != RP_NONE) atomicMin(&st->minpos, mn);
}
__global__ void rp_winner_kernel(const u32* __restrict__ S, u32 m, RpState* st, u64* __restrict__ rules, u32 k, u32 tie, u32 TM) {
    u32 l = st->key_hi, r = st->key_lo;
    if (tie) {
        u32 p = st->minpos;
        if (st->tiecnt != TM || p + 1 >= m) { atomicOr(&st->err, RP_ERR_TIE); p = 0; }
        l = S[p]; r = S[p + 1];
    }
    st->win_hi = l; st->win_lo = r;
    rules[k] = rp_key(l, r);
}

// ---- mark ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rp_mark_kernel(const u32* __restrict__ S, u32 m, const RpState* __restrict__ st, u8* __restrict__ taken) {
    const u32 l = st->win_hi, r = st->win_lo;
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < m; i += stride) taken[i] = (i + 1 < m && S[i] == l && S[i + 1] == r) ? 1 : 0;
}
// l == r = a: marker[i] = i where a run of a's starts (and at every other symbol), 0 inside one
__global__ __launch_bounds__(256) void rp_run_marker_kernel(const u32* __restrict__ S, u32 m, const RpState* __restrict__ st, u32* __restrict__ marker) {
    const u32 a = st->win_hi;
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < m; i += stride) marker[i] = (i > 0 && S[i] == a && S[i - 1] == a) ? 0u : (u32)i;
}
__global__ __launch_bounds__(256) void rp_mark_sq_kernel(const u32* __restrict__ S, u32 m, const RpState* __restrict__ st,
                                                          const u32* __restrict__ run_start, u8* __restrict__ taken) {
    const u32 a = st->win_hi;
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < m; i += stride)
        taken[i] = (i + 1 < m && S[i] == a && S[i + 1] == a && (((u32)i - run_start[i]) & 1u) == 0) ? 1 : 0;
}

// ---- deltas --------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void rp_sub(const RpTable& t, u64 key, u64 win, RpState* st) {
    if (key == win) return;
    const u32 h = rp_find(t, key);
    if (h == RP_NONE) { atomicOr(&st->err, RP_ERR_MISSING); return; }
    atomicSub(&t.counts[h], 1u);
}
__global__ __launch_bounds__(256) void rp_delta_kernel(const u32* __restrict__ S, u32 m, RpState* st, const u8* __restrict__ taken, RpTable t, u32 A) {
    const u64 win = rp_key(st->win_hi, st->win_lo);
    if (blockIdx.x == 0 && threadIdx.x == 0) {                            // (no delta names the winner: nobody else touches its slot)
        const u32 h = rp_find(t, win);
        if (h != RP_NONE) t.counts[h] = 0;
    }
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i + 1 < m; i += stride) {
        if (!taken[i]) continue;
        if (i > 0) {
            const u32 x = S[i - 1];
            rp_sub(t, rp_key(x, S[i]), win, st);
            rp_add(t, rp_key((i >= 2 && taken[i - 2]) ? A : x, A), 1u, st);
        }
        if (i + 2 < m && !taken[i + 2]) {                                 // (taken[m - 1] is never set)
            const u32 y = S[i + 2];
            rp_sub(t, rp_key(S[i + 1], y), win, st);
            rp_add(t, rp_key(A, y), 1u, st);
        }
    }
}

// ---- compact -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rp_apply_kernel(u32* __restrict__ S, u32 m, const u8* __restrict__ taken, u32 A, u8* __restrict__ keep) {
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < m; i += stride) {
        keep[i] = (i > 0 && taken[i - 1]) ? 0 : 1;
        if (taken[i]) S[i] = A;
    }
}

u32 log2_ceil(u64 v) { u32 b = 0; while (((u64)1 << b) < v) ++b; return b; }
// the largest table a text of n bytes can ask for: four slots per symbol (a sequence of m symbols has fewer than m distinct pairs, and a
// round adds at most 2 M <= 2 m keys), at most 2^31; a forced first capacity above that counts
u32 table_bits_max(const Ctx& c, size_t n) {
    const u32 want = std::min<u32>(31u, std::max<u32>(8u, log2_ceil(4 * (u64)std::max<size_t>(n, 1))));
    return std::max<u32>(want, (u32)c.repair_table_bits);
}

struct Builder {
    Ctx& c;
    hipStream_t s;
    RpState* st;
    RpTable t;
    u32 bits;                     // log2 of the table's capacity
    u32 bits_max;
    RepairStats* rs;

    void set_bits(u32 b) { bits = b; t.shift = 64 - b; t.mask = (u32)(((u64)1 << b) - 1); }
    void clear_table() {
        const size_t cap = (size_t)1 << bits;
        HIP_TRY(hipMemsetAsync(t.keys, 0xFF, cap * sizeof(u64), s));
        HIP_TRY(hipMemsetAsync(t.counts, 0, cap * sizeof(u32), s));
        HIP_TRY(hipMemsetAsync(&st->occupied, 0, 2 * sizeof(u32), s));      // (occupied, err)
    }
    // fills the cleared table with `count`, at twice the size until it is at most half full; returns the state read back
    template <typename F> RpState fill(F&& count) {
        for (;;) {
            clear_table();
            count();
            const RpState h = c.read(st);
            if (!(h.err & RP_ERR_FULL) && 2 * (u64)h.occupied <= ((u64)1 << bits)) {
                if (h.err) throw HipError{hipErrorUnknown, "repair: digram table inconsistent", (int)__LINE__};
                return h;
            }
            if (bits >= bits_max) throw HipError{hipErrorUnknown, "repair: digram table cannot grow", (int)__LINE__};
            set_bits(bits + 1);
            ++rs->rebuilds;
        }
    }
};

}  // namespace

// every rule replaces at least one pair and a replaced pair leaves one symbol, so R rules leave at most n - R start
// symbols: 1 + 2R + (n - R) <= 2n + 1 fields for n >= 1 (R < n).  The costliest field: bit 1 + 31 (a rule index) against 9; ascii '1',
// ten digits and ':' = 96; gamma 1 + 63; delta 1 + 11 + 31.  + 16: the count (at most 96 bits) and the terminator.
size_t repair_bound(size_t n, int kind) {
    if (kind < 0 || kind > 3 || n > REPAIR_MAX_N) return 0;
    const u64 per = kind == 0 ? 32 : kind == 1 ? 96 : kind == 2 ? 64 : 43;
    return (size_t)(((2 * (u64)n + 1) * per + 7) / 8 + 16);
}

size_t repair_encode(Ctx& c, const u64* d_rules, size_t R, const u32* d_start, size_t m, int kind, u8* d_out, size_t out_cap) {
    if (kind < 0 || kind > 3) throw HipError{hipErrorInvalidValue, "repair: no such coder", (int)__LINE__};
    return encode_fields(c, RpFields{ d_rules, (u32)R, d_start }, 1 + 2 * (u64)R + m, kind, d_out, out_cap, "repair: output buffer too small");
}

size_t repair_arena(const Ctx& c, size_t n, u64 max_rules) {
    const u64 R = std::min<u64>(max_rules ? max_rules : n, n);
    return 43 * n + 8 * (size_t)R + 12 * ((size_t)1 << table_bits_max(c, n)) + ((size_t)8 << 20);
}

void repair_grammar(Ctx& c, const u8* d_text, size_t n, u64 max_rules, u64** d_rules, u32** d_start, RepairStats* rs) {
    RepairStats local;
    if (!rs) rs = &local;
    *rs = RepairStats();
    if (n > REPAIR_MAX_N) throw HipError{hipErrorInvalidValue, "repair: text length out of range", (int)__LINE__};
    hipStream_t s = c.stream;
    const u64 R = std::min<u64>(max_rules ? max_rules : n, n);
    u64* rules = c.arena.get<u64>((size_t)R + 1);
    u32* S = c.arena.get<u32>(n + 1), *S2 = c.arena.get<u32>(n + 1);
    *d_rules = rules; *d_start = S;
    if (n < 2) {                                                           // no pair: no round (n = 0 is defined as no symbols)
        if (n) { rp_widen_kernel<<<1, 256, 0, s>>>(d_text, (u64)n, S); LAUNCH_CHECK(); }
        rs->nstart = n;
        return;
    }
    u8* taken = c.arena.get<u8>(n + 8), *keep = c.arena.get<u8>(n + 8);
    u32* aux[2] = { c.arena.get<u32>(n + 1), c.arena.get<u32>(n + 1) };
    u32* tvals[2] = { c.arena.get<u32>(n + 1), c.arena.get<u32>(n + 1) };
    u64* tkeys[2] = { c.arena.get<u64>(n + 1), c.arena.get<u64>(n + 1) };
    u32* hist = c.arena.get<u32>(65536);
    Builder B{ c, s, (RpState*)c.arena.alloc(sizeof(RpState)), RpTable{}, 0, table_bits_max(c, n), rs };
    B.t.keys = c.arena.get<unsigned long long>((size_t)1 << B.bits_max);
    B.t.counts = c.arena.get<u32>((size_t)1 << B.bits_max);
    RpState* st = B.st;
    B.set_bits(c.repair_table_bits ? (u32)c.repair_table_bits
                                   : std::min<u32>(B.bits_max, std::max<u32>(8u, log2_ceil(4 * (u64)std::min<size_t>(n, 65536)))));

    // the first count
    HIP_TRY(hipMemsetAsync(st, 0, sizeof(RpState), s));
    HIP_TRY(hipMemsetAsync(hist, 0, 65536 * sizeof(u32), s));
    rp_widen_kernel<<<dec_grid(n), 256, 0, s>>>(d_text, (u64)n, S);
    LAUNCH_CHECK();
    rp_byte_pairs_kernel<<<(unsigned)((n - 1 + RP_CHUNK - 1) / RP_CHUNK), 256, 0, s>>>(d_text, (u64)n, hist);
    LAUNCH_CHECK();
    const u32 n32 = (u32)n;
    HIP_TRY(hipMemcpyAsync(&st->m, &n32, sizeof(u32), hipMemcpyHostToDevice, s));
    B.fill([&] { rp_hist_insert_kernel<<<256, 256, 0, s>>>(hist, B.t, st); LAUNCH_CHECK(); });

    // A round is timed on the host from read-back to read-back: what lies between the arrival of round k's argmax and that of round
    // k + 1's is round k's tie pass, mark, deltas and compaction and the next argmax.  No synchronisation is added for it.
    using clock = std::chrono::steady_clock;
    struct Pending { bool open = false, tie = false, square = false, rebuild = false; u32 m = 0, M = 0, T = 0; clock::time_point t0; } pend;
    auto close_round = [&](u64 idx, const RpState& h) {
        if (!pend.open) return;
        const float ms = std::chrono::duration<float, std::milli>(clock::now() - pend.t0).count();
        if (idx == 1) rs->ms_first = ms;
        if (pend.tie) rs->ms_tie += ms;
        rs->ms_last = ms;
        if (c.repair_log)
            fprintf(stderr, "repair: round %llu  m %u  M %u  T %u%s%s  table 2^%u (%u claimed)  %.3f ms\n", (unsigned long long)idx, pend.m, pend.M,
                    pend.T, pend.square ? "  square" : "", pend.rebuild ? "  rebuild" : "", B.bits, h.occupied, ms);
        pend.open = false;
    };
    u64 k = 0;
    u32 m = n32;
    while (k < R) {
        const unsigned tgrid = std::min(dec_grid((size_t)1 << B.bits), RP_ARGMAX_BLOCKS);
        rp_round_begin_kernel<<<1, 1, 0, s>>>(st);
        rp_max_kernel<<<tgrid, 256, 0, s>>>(B.t, st);
        rp_tied_kernel<<<tgrid, 256, 0, s>>>(B.t, st);
        LAUNCH_CHECK();
        const RpState h = c.read(st);
        close_round(k, h);
        if (h.err) throw HipError{hipErrorUnknown, "repair: digram table inconsistent", (int)h.err};
        m = h.m;
        if (h.M <= 1 || m < 2) break;
        const unsigned grid = dec_grid(m);
        const bool tie = h.T > 1;
        const u64 TM = (u64)h.T * h.M;
        pend.open = true; pend.tie = tie; pend.m = m; pend.M = h.M; pend.T = h.T; pend.t0 = clock::now();
        if (tie) {
            if (TM > m - 1) throw HipError{hipErrorUnknown, "repair: digram counts exceed the sequence", (int)__LINE__};
            ++rs->tie_rounds;
            rp_tie_class_kernel<<<grid, 256, 0, s>>>(S, m, B.t, st, keep);
            LAUNCH_CHECK();
            select_by_class(c, keep, 1, m - 1, nullptr, tvals[0], nullptr, nullptr, &st->tiecnt);
            const u32 sb = bits_for(255 + k);                              // symbols so far: < 256 + k
            rp_tie_keys_kernel<<<dec_grid((size_t)TM), 256, 0, s>>>(S, m, tvals[0], (u32)TM, sb, tkeys[0]);
            LAUNCH_CHECK();
            const int x = radix_sort_pairs_u64(c, tkeys, tvals, (size_t)TM, 0, 2 * (int)sb);
            rp_tie_min_kernel<<<dec_grid(h.T), 256, 0, s>>>(tvals[x], h.T, h.M, st);
            LAUNCH_CHECK();
        }
        rp_winner_kernel<<<1, 1, 0, s>>>(S, m, st, rules, (u32)k, tie ? 1u : 0u, (u32)TM);
        LAUNCH_CHECK();
        bool square = h.key_hi == h.key_lo;
        if (tie) {                                                         // a second read-back only where a square is among the tied pairs
            square = false;
            if (h.sq) { const RpState w = c.read(st); square = w.win_hi == w.win_lo; }
        }
        if (square) {
            rp_run_marker_kernel<<<grid, 256, 0, s>>>(S, m, st, aux[0]);
            LAUNCH_CHECK();
            inclusive_max_u32(c, aux[0], aux[1], m);
            rp_mark_sq_kernel<<<grid, 256, 0, s>>>(S, m, st, aux[1], taken);
        } else {
            rp_mark_kernel<<<grid, 256, 0, s>>>(S, m, st, taken);
        }
        LAUNCH_CHECK();
        // what a round inserts are pairs with the new symbol, (x, A), (A, y) and (A, A): at most two per taken pair -- M pairs at most --
        // and at most two per symbol there is
        const u64 cap = (u64)1 << B.bits;
        const u64 fresh = std::min<u64>(2 * (u64)h.M, 2 * (256 + k) + 1);
        const bool grow = (u64)h.occupied + fresh > cap / 2;
        const bool rebuild = c.repair_recount || grow;
        pend.square = square; pend.rebuild = rebuild;
        const u32 A = (u32)(256 + k);
        if (!rebuild) {
            rp_delta_kernel<<<grid, 256, 0, s>>>(S, m, st, taken, B.t, A);
            LAUNCH_CHECK();
        }
        rp_apply_kernel<<<grid, 256, 0, s>>>(S, m, taken, A, keep);
        LAUNCH_CHECK();
        select_by_class(c, keep, 1, m, S, S2, nullptr, nullptr, &st->m);
        std::swap(S, S2);
        ++k;
        ++rs->rounds;
        if (rebuild) {
            auto recount = [&] { rp_count_kernel<<<grid, 256, 0, s>>>(S, B.t, st); LAUNCH_CHECK(); };
            if (c.repair_recount) { B.fill(recount); continue; }
            // twice the size; slots whose count had fallen to 0 are gone after the recount, and where the pairs that are left would fill
            // less than an eighth of the table it is made to fit them (four slots per pair, room for the next round included)
            ++rs->rebuilds;
            B.set_bits(std::min(B.bits + 1, B.bits_max));
            const RpState f = B.fill(recount);
            const u32 fit = std::max<u32>(8u, log2_ceil(4 * ((u64)f.occupied + 2 * (256 + k) + 1)));
            if (fit + 1 < B.bits) { B.set_bits(fit); B.fill(recount); }
        }
    }
    const RpState h = c.read(st);
    close_round(k, h);
    if (h.err) throw HipError{hipErrorUnknown, "repair: digram table inconsistent", (int)h.err};
    rs->rules = k;
    rs->nstart = h.m;
    rs->replaced = n - h.m;
    *d_start = S;
}

}  // namespace tdc
