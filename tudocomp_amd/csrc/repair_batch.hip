// repair_batch.hip -- repair over many independent texts in one call ("Batches"): the kernels, the host side and
// the entry points of include/tdc_gpu.h.  The executable statement of the formulation is tests/models/repair_batch.py.
//
// The single call (repair.hip) is a host-driven loop, one rule per round and at least one read-back per round.  Across texts the grammars
// are independent: here ONE WORKGROUP runs the whole round loop of one text, without the host, and thousands of workgroups run side by
// side.  The grid is bounded and the texts are taken grid-stride, longest first (the host knows the lengths).  For text k the grammar is
// exactly what tdc_repair_grammar returns for it alone: nothing of a neighbour is visible, every array below is the text's own slice.
//   state      S[0 .. m) the live sequence (u32, compacted in place), taken[0 .. m), the rules, and a digram table of the layout of
//              repair.hip's RpTable -- a power of two of slots, at least 4 (option repair_batch_table = 1: 2) per text byte, linear
//              probing, exact 64-bit keys l << 32 | r, u32 counts -- with one more word per slot (`last`, 0 between rounds).  The host
//              plans the slices before the device is asked (rb_plan).
//   a round    argmax      one scan of the counts: M, the number T of slots that hold it, and (T = 1) the key
//              tie (T > 1) the table holds EXACT counts, so the M-th occurrence of a pair that counts M is its last one: every position
//                          whose pair counts M does atomicMax(last[slot], position); the winner is the pair whose `last` is smallest (a
//                          second scan, which also puts the words back to 0).  No selection, no sort.
//              mark        l != r: every occurrence.  l == r: run starts by an inclusive max over start markers, chunk by chunk with a
//                          carry; a position is taken iff its offset in the run is even and a partner follows.
//              deltas      as rp_delta_kernel of repair.hip
//              compact     in place, chunk by chunk with a carry: a chunk is read whole before the barrier of its scan and written
//                          behind it, to positions at or in front of the ones it read
//   the table  cannot grow inside a kernel.  INVARIANT: at most half of the slots are claimed whenever a pass inserts.  A sequence of m
//              symbols has fewer than m distinct pairs and the table has cap >= 2 m slots, so a recount claims fewer than cap / 2; a
//              round inserts at most `fresh` = min(2 * taken, 2 * (256 + R) + 1) new keys -- pairs with the new symbol --, and a round
//              with claimed + fresh > cap / 2 does not apply its deltas: the table is cleared and recounted from the compacted sequence
//              instead (the in-kernel rebuild).  So an empty slot always ends a probe run; every probe loop is bounded by the capacity
//              all the same, and a table that is full gives the text TDC_GPU_ERR_INTERNAL, not a spin.  The rebuild also halves the
//              capacity while the smaller table still has its 4 (2) slots per LIVE symbol: the argmax scan then costs what is left of
//              the text, not what it began with.
//   launches   a launch performs at most `repair_batch_rounds` rounds per text (fewer for a text above 128 KiB: rb_rounds) and leaves
//              every text's state in the arena (RbText); the
//              host relaunches while the 4-byte word `unfinished` says so, one read-back per launch.
// Termination: a text's loop runs at most `rounds` times per launch; a round that takes no pair ends the text with an error, so every
// round removes at least one symbol and adds one rule, and the loop ends at R = min(max_rules, n_k) at the latest; the host launches at
// most n_max / rb_rounds(n_max) + 2 times.  Every pass inside a round is a counted loop over the sequence, the chunks or the slots; every probe loop
// is bounded by the capacity.
// Memory: a text's arrays are written and re-read by different waves of its workgroup across __syncthreads(), and across launches.  None
// of them is const __restrict__ here, the table's words are read with agent-scope loads (never the scalar cache, never a stale line of
// the vector cache behind an atomic that ran in L2), and the state is carried in registers and LDS between the first and the last pass of
// a launch.  Workgroups do not communicate within a launch.
//
// Coding: RpFields (repair_fields.hpp) per text, placed as lz_batch.hip / lzss_sw_batch.hip place theirs: the bit cost of the text's
// 1 + 2 R_k + m_k fields -> its 8-byte aligned slot (0 for a refused text) | 64-bit scan: out_off | one read-back, which decides
// TDC_GPU_ERR_OOM | pack, a workgroup per text, chunks of 2048 fields with a carry | one terminator per stream.
#include "api.hpp"
#include "bitsink.hpp"
#include "decode.hpp"
#include "field_coder.hpp"
#include "repair_fields.hpp"

#include <algorithm>
#include <numeric>
#include <vector>

namespace tdc {

namespace {

constexpr u32 RB_TEXT_MAX = 1u << 24;            // bytes per text: one workgroup walks the text R_k times; the single call takes longer ones
constexpr unsigned long long RB_EMPTY = ~0ull;
constexpr u32 RB_F_INIT = 1, RB_F_DONE = 2;
constexpr u32 RB_ERR_FULL = 1, RB_ERR_TIE = 2, RB_ERR_MISSING = 4, RB_ERR_STUCK = 8;
constexpr u32 RB_ITEMS = 8, RB_CHUNK = 256 * RB_ITEMS;       // a thread's run of positions in the chunked passes
constexpr u32 RB_MIN_CAP = 8;
constexpr u32 RB_FLIGHT = 8, RB_SCAN = 8;                     // positions / table words a thread reads side by side: the loads are agent-scope,
                                                             // the compiler keeps their order, and a loop of single loads runs at one latency per word
constexpr unsigned RB_MAX_GRID = 2048;                       // twice what is resident: 4 workgroups of four waves per CU at the round kernel's 115 VGPRs, 256 CUs

// what a launch leaves of a text (32 bytes, zeroed by the call)
struct RbText { u32 m, R, cap, occupied, flags, err, tie_rounds, rebuilds; };
static_assert(sizeof(RbText) == 32, "RbText: eight words");

struct RbTable { unsigned long long* keys; u32* counts; u32* last; u32 shift, mask; };

struct RbArgs {
    const u8* __restrict__ text; const u32* __restrict__ off; const u32* __restrict__ order; u32 accepted;
    u32* S; u8* taken; u64* rules;                           // text k: S, taken and rules from off[k] on (a rule takes at least one symbol away)
    unsigned long long* keys; u32* counts; u32* last; const u64* __restrict__ tab_off;   // text k's slots: [tab_off[k], tab_off[k + 1])
    RbText* st; u32* unfinished;
    u32 rounds, spb; u64 max_rules;
};

__device__ __forceinline__ u32 rb_ld(u32* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ u64 rb_ld(unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void rb_st(u32* p, u32 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ u64 rb_key(u32 l, u32 r) { return (u64)l << 32 | r; }
__device__ __forceinline__ u32 rb_slot0(const RbTable& t, u64 key) { return (u32)((key * 0x9E3779B97F4A7C15ull) >> t.shift); }
__device__ __forceinline__ void rb_set_cap(RbTable& t, u32 cap) { t.shift = 64u - (u32)__builtin_ctz(cap); t.mask = cap - 1; }

// the slot of a key that an earlier pass put into the table
__device__ __forceinline__ u32 rb_find(const RbTable& t, u64 key) {
    u32 h = rb_slot0(t, key);
    for (u32 probes = 0; probes <= t.mask; ++probes, h = (h + 1) & t.mask) {
        const u64 k = rb_ld(&t.keys[h]);
        if (k == key) return h;
        if (k == RB_EMPTY) return RP_NONE;
    }
    return RP_NONE;
}
// count(key) += d, the key inserted if it is new.  sh[0] counts the claims, sh[1] takes RB_ERR_*.
__device__ __forceinline__ void rb_add(const RbTable& t, u64 key, u32 d, u32* sh) {
    u32 h = rb_slot0(t, key);
    for (u32 probes = 0; probes <= t.mask; ++probes, h = (h + 1) & t.mask) {
        unsigned long long k = rb_ld(&t.keys[h]);
        if (k == RB_EMPTY) {
            k = atomicCAS(&t.keys[h], RB_EMPTY, (unsigned long long)key);
            if (k == RB_EMPTY) { atomicAdd(&sh[0], 1u); k = key; }
        }
        if (k == key) { atomicAdd(&t.counts[h], d); return; }
    }
    atomicOr(&sh[1], RB_ERR_FULL);
}
__device__ __forceinline__ void rb_sub(const RbTable& t, u64 key, u64 win, u32* sh) {
    if (key == win) return;
    const u32 h = rb_find(t, key);
    if (h == RP_NONE) { atomicOr(&sh[1], RB_ERR_MISSING); return; }
    atomicSub(&t.counts[h], 1u);
}

// The rounds of one launch for a text of n bytes: option repair_batch_rounds up to 128 KiB, divided by n / 64 KiB beyond -- a round costs
// what the text is long, and a launch should stay near a second on a device that others share (16 MiB: 4 rounds at the default).
__host__ __device__ inline u32 rb_rounds(u32 n, u32 rounds) { const u32 by = n >> 16; const u32 r = by > 1 ? rounds / by : rounds; return r ? r : 1u; }

// workgroup reductions (256 threads; sm: four words; every thread gets the result)
__device__ __forceinline__ u32 rb_reduce_max(u32 v, u32* sm) {
    v = wave_reduce_max(v);
    if (lane_id() == 0) sm[wave_id()] = v;
    __syncthreads();
    v = max(max(sm[0], sm[1]), max(sm[2], sm[3]));
    __syncthreads();
    return v;
}
__device__ __forceinline__ u32 rb_reduce_min(u32 v, u32* sm) { return ~rb_reduce_max(~v, sm); }
__device__ __forceinline__ u32 rb_reduce_sum(u32 v, u32* sm) {
    v = wave_reduce_sum(v);
    if (lane_id() == 0) sm[wave_id()] = v;
    __syncthreads();
    v = sm[0] + sm[1] + sm[2] + sm[3];
    __syncthreads();
    return v;
}
// the max over the threads in front of this one; total: over all of them
__device__ __forceinline__ u32 rb_exclusive_max(u32 v, u32* sm, u32& total) {
    const u32 inc = wave_inclusive_max(v);
    u32 ex = __shfl_up(inc, 1, 64);
    if (lane_id() == 0) ex = 0;
    if (lane_id() == 63) sm[wave_id()] = inc;
    __syncthreads();
    u32 pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const u32 s = sm[w]; if (w < wave_id()) pre = max(pre, s); tot = max(tot, s); }
    __syncthreads();
    total = tot;
    return max(pre, ex);
}

// clears the table and counts the pairs of S[0 .. m); returns the slots claimed
__device__ __forceinline__ u32 rb_rebuild(const RbTable& t, u32* S, u32 m, u32* sh) {
    for (u32 i = threadIdx.x; i <= t.mask; i += 256) { t.keys[i] = RB_EMPTY; t.counts[i] = 0; t.last[i] = 0; }
    if (threadIdx.x == 0) sh[0] = 0;
    __syncthreads();
    for (u32 i = threadIdx.x; i + 1 < m; i += 256) rb_add(t, rb_key(S[i], S[i + 1]), 1u, sh);
    __syncthreads();
    return sh[0];
}

__global__ __launch_bounds__(256) void rb_rounds_kernel(const RbArgs P) {
    __shared__ u32 sm[8];
    __shared__ u32 sh[4];                                  // claims of the running pass, RB_ERR_*, the argmax key
    const u32 tid = threadIdx.x;
    for (u32 j = blockIdx.x; j < P.accepted; j += gridDim.x) {
        const u32 k = P.order[j];
        const u32 base = P.off[k], n = P.off[k + 1] - base;
        RbText* st = P.st + k;
        const u32 flags = rb_ld(&st->flags);
        if (flags & RB_F_DONE) continue;
        u32* S = P.S + base;
        u8* taken = P.taken + base;
        u64* rules = P.rules + base;
        const u64 t0 = P.tab_off[k];
        RbTable t{ P.keys + t0, P.counts + t0, P.last + t0, 0, 0 };
        u32 m = rb_ld(&st->m), R = rb_ld(&st->R), cap = rb_ld(&st->cap), occ = rb_ld(&st->occupied);
        u32 ties = rb_ld(&st->tie_rounds), rebuilds = rb_ld(&st->rebuilds), err = 0;
        bool done = false;
        if (tid == 0) { sh[0] = 0; sh[1] = 0; }
        __syncthreads();
        if (!(flags & RB_F_INIT)) {                            // the first visit: the bytes as symbols, the first count
            for (u32 i = tid; i < n; i += 256) S[i] = P.text[base + i];
            m = n; R = 0; cap = (u32)(P.tab_off[k + 1] - t0); occ = 0;
            __syncthreads();
            if (n >= 2) { rb_set_cap(t, cap); occ = rb_rebuild(t, S, m, sh); }
            else done = true;                                  // no pair: no round (n = 0: no symbols)
        } else rb_set_cap(t, cap);
        const u32 Rmax = P.max_rules && P.max_rules < n ? (u32)P.max_rules : n;
        const u32 rounds = rb_rounds(n, P.rounds);
        for (u32 round = 0; round < rounds && !done; ++round) {
            if (m < 2 || R >= Rmax) { done = true; break; }
            // ---- argmax: two counts per load
            u32 mx = 0, cnt = 0;
            u64 key = RB_EMPTY;
            for (u32 i0 = 2 * tid; i0 < cap; i0 += 512 * RB_SCAN) {
                u64 w[RB_SCAN];
#pragma unroll
                for (u32 q = 0; q < RB_SCAN; ++q) { const u32 i = i0 + 512 * q; w[q] = i < cap ? rb_ld((unsigned long long*)(t.counts + i)) : 0ull; }
#pragma unroll
                for (u32 q = 0; q < RB_SCAN; ++q) {
                    const u32 i = i0 + 512 * q, c0 = (u32)w[q], c1 = (u32)(w[q] >> 32);
                    if (c0 > mx) { mx = c0; cnt = 1; key = rb_ld(&t.keys[i]); } else if (c0 == mx && c0) ++cnt;
                    if (c1 > mx) { mx = c1; cnt = 1; key = rb_ld(&t.keys[i + 1]); } else if (c1 == mx && c1) ++cnt;
                }
            }
            const u32 M = rb_reduce_max(mx, sm);
            if (M <= 1) { done = true; break; }
            const u32 T = rb_reduce_sum(mx == M ? cnt : 0u, sm);
            if (mx == M) { sh[2] = (u32)(key >> 32); sh[3] = (u32)key; }      // (T = 1: one writer; T > 1: not read)
            __syncthreads();
            u32 l = sh[2], r = sh[3];
            // ---- tie: the pair whose last occurrence comes first
            if (T > 1) {
                for (u32 i0 = tid; i0 + 1 < m; i0 += 256 * RB_FLIGHT) {
                    u64 want[RB_FLIGHT], got[RB_FLIGHT];
                    u32 h[RB_FLIGHT], c[RB_FLIGHT];
#pragma unroll
                    for (u32 q = 0; q < RB_FLIGHT; ++q) {      // the home slots of RB_FLIGHT positions, read side by side
                        const u32 i = i0 + 256 * q;
                        const bool in = i + 1 < m;
                        want[q] = in ? rb_key(S[i], S[i + 1]) : RB_EMPTY;
                        h[q] = rb_slot0(t, want[q]);
                        got[q] = in ? rb_ld(&t.keys[h[q]]) : RB_EMPTY;
                    }
#pragma unroll
                    for (u32 q = 0; q < RB_FLIGHT; ++q) if (got[q] != want[q]) h[q] = rb_find(t, want[q]);      // (not at home: the probe run)
#pragma unroll
                    for (u32 q = 0; q < RB_FLIGHT; ++q) c[q] = (i0 + 256 * q + 1 < m && h[q] != RP_NONE) ? rb_ld(&t.counts[h[q]]) : 0u;
#pragma unroll
                    for (u32 q = 0; q < RB_FLIGHT; ++q) {
                        const u32 i = i0 + 256 * q;
                        if (i + 1 >= m) continue;
                        if (h[q] == RP_NONE) atomicOr(&sh[1], RB_ERR_MISSING);
                        else if (c[q] == M) atomicMax(&t.last[h[q]], i);
                    }
                }
                __syncthreads();
                u32 mn = RP_NONE;
                for (u32 i0 = 2 * tid; i0 < cap; i0 += 512 * RB_SCAN) {
                    u64 w[RB_SCAN];
#pragma unroll
                    for (u32 q = 0; q < RB_SCAN; ++q) { const u32 i = i0 + 512 * q; w[q] = i < cap ? rb_ld((unsigned long long*)(t.counts + i)) : 0ull; }
#pragma unroll
                    for (u32 q = 0; q < RB_SCAN; ++q) {
                        const u32 i = i0 + 512 * q;
                        if ((u32)w[q] == M) { mn = min(mn, rb_ld(&t.last[i])); rb_st(&t.last[i], 0u); }
                        if ((u32)(w[q] >> 32) == M) { mn = min(mn, rb_ld(&t.last[i + 1])); rb_st(&t.last[i + 1], 0u); }
                    }
                }
                const u32 p = rb_reduce_min(mn, sm);
                if (p == RP_NONE || p + 1 >= m) { err = RB_ERR_TIE | sh[1]; break; }
                l = rb_ld(&S[p]); r = rb_ld(&S[p + 1]);
                ++ties;
            }
            // ---- mark
            const u32 A = 256u + R;
            u32 nt = 0;
            if (l != r) {
                for (u32 i0 = tid; i0 < m; i0 += 256 * RB_FLIGHT) {          // (the loads of RB_FLIGHT positions in front of their stores)
                    u32 a[RB_FLIGHT], b[RB_FLIGHT];
#pragma unroll
                    for (u32 q = 0; q < RB_FLIGHT; ++q) {
                        const u32 i = i0 + 256 * q;
                        a[q] = i < m ? S[i] : RP_NONE;
                        b[q] = i + 1 < m ? S[i + 1] : RP_NONE;
                    }
#pragma unroll
                    for (u32 q = 0; q < RB_FLIGHT; ++q) {
                        const u32 i = i0 + 256 * q;
                        if (i >= m) continue;
                        const u32 tk = (a[q] == l && b[q] == r) ? 1u : 0u;
                        taken[i] = (u8)tk; nt += tk;
                    }
                }
            } else {
                u32 carry = 0;
                for (u32 c0 = 0; c0 < m; c0 += RB_CHUNK) {
                    const u32 i0 = c0 + tid * RB_ITEMS;
                    u32 x[RB_ITEMS + 2];                       // S[i0 - 1 .. i0 + 8]; RP_NONE off the sequence
#pragma unroll
                    for (u32 q = 0; q < RB_ITEMS + 2; ++q) { const u32 i = i0 + q; x[q] = (i >= 1 && i - 1 < m) ? S[i - 1] : RP_NONE; }
                    u32 mk[RB_ITEMS], run = 0;
#pragma unroll
                    for (u32 q = 0; q < RB_ITEMS; ++q) {       // marker: i where a run starts (and at every other symbol), 0 inside one
                        const u32 i = i0 + q;
                        const bool inside = x[q + 1] == l && x[q] == l;
                        run = max(run, (inside || i >= m) ? 0u : i);
                        mk[q] = run;
                    }
                    u32 total;
                    const u32 ex = max(carry, rb_exclusive_max(run, sm, total));
                    carry = max(carry, total);
#pragma unroll
                    for (u32 q = 0; q < RB_ITEMS; ++q) {
                        const u32 i = i0 + q;
                        if (i >= m) continue;
                        const u32 rs = max(ex, mk[q]);
                        const u32 tk = (x[q + 1] == l && x[q + 2] == l && ((i - rs) & 1u) == 0) ? 1u : 0u;
                        taken[i] = (u8)tk; nt += tk;
                    }
                }
            }
            const u32 ntaken = rb_reduce_sum(nt, sm);          // (its barriers stand between the marks and their readers)
            if (ntaken == 0 || sh[1]) { err = RB_ERR_STUCK | sh[1]; break; }
            // ---- the table after this round: deltas, or cleared and recounted (full, or small enough for half the slots)
            const u32 m_new = m - ntaken;
            const u32 fresh = min(2u * ntaken, 2u * A + 1u);
            u32 cap_new = cap;
            while (cap_new > RB_MIN_CAP && (u64)(cap_new >> 1) >= (u64)P.spb * m_new) cap_new >>= 1;
            const bool rebuild = occ + fresh > cap / 2 || cap_new != cap;
            if (!rebuild) {
                const u64 win = rb_key(l, r);
                if (tid == 0) sh[0] = 0;
                __syncthreads();
                if (tid == 0) {                                // (no delta names the winner: nobody else touches its slot)
                    const u32 h = rb_find(t, win);
                    if (h != RP_NONE) rb_st(&t.counts[h], 0u);
                }
                for (u32 i0 = tid; i0 + 1 < m; i0 += 256 * RB_FLIGHT) {
                    u8 tk[RB_FLIGHT];
#pragma unroll
                    for (u32 q = 0; q < RB_FLIGHT; ++q) { const u32 i = i0 + 256 * q; tk[q] = i + 1 < m ? taken[i] : (u8)0; }
#pragma unroll
                    for (u32 q = 0; q < RB_FLIGHT; ++q) {
                        const u32 i = i0 + 256 * q;
                        if (!tk[q]) continue;
                        if (i > 0) {
                            const u32 x = S[i - 1];
                            rb_sub(t, rb_key(x, S[i]), win, sh);
                            rb_add(t, rb_key((i >= 2 && taken[i - 2]) ? A : x, A), 1u, sh);
                        }
                        if (i + 2 < m && !taken[i + 2]) {      // (taken[m - 1] is never set)
                            const u32 y = S[i + 2];
                            rb_sub(t, rb_key(S[i + 1], y), win, sh);
                            rb_add(t, rb_key(A, y), 1u, sh);
                        }
                    }
                }
                __syncthreads();
                occ += sh[0];
            }
            // ---- compact, in place
            u32 outbase = 0;
            for (u32 c0 = 0; c0 < m; c0 += RB_CHUNK) {
                const u32 i0 = c0 + tid * RB_ITEMS;
                u32 v[RB_ITEMS];
                u32 keep = 0, cntk = 0;
                bool before = i0 >= 1 && i0 - 1 < m && taken[i0 - 1];
#pragma unroll
                for (u32 q = 0; q < RB_ITEMS; ++q) {
                    const u32 i = i0 + q;
                    const bool in = i < m;
                    const bool tk = in && taken[i];
                    v[q] = tk ? A : (in ? S[i] : 0u);
                    if (in && !before) { keep |= 1u << q; ++cntk; }
                    before = tk;
                }
                u32 total;
                u32 o = outbase + block_exclusive_sum<u32, 4>(cntk, sm, total);
#pragma unroll
                for (u32 q = 0; q < RB_ITEMS; ++q) if (keep >> q & 1u) S[o++] = v[q];
                outbase += total;
            }
            if (tid == 0) rules[R] = rb_key(l, r);
            __syncthreads();
            m = outbase;
            ++R;
            if (sh[1] || m != m_new) { err = RB_ERR_STUCK | sh[1]; break; }
            if (rebuild) {
                cap = cap_new;
                rb_set_cap(t, cap);
                occ = rb_rebuild(t, S, m, sh);
                ++rebuilds;
                if (sh[1]) { err = sh[1]; break; }
            }
        }
        if (!done && (m < 2 || R >= Rmax)) done = true;
        __syncthreads();                                       // (sh is rewritten for the next text)
        if (tid == 0) {
            st->m = m; st->R = R; st->cap = cap; st->occupied = occ; st->tie_rounds = ties; st->rebuilds = rebuilds; st->err = err;
            st->flags = RB_F_INIT | ((done || err) ? RB_F_DONE : 0u);
            if (!done && !err) *P.unfinished = 1u;
        }
    }
}

// ---- coding ------------------------------------------------------------------------------------------------------------------------------
struct RbEnc {
    const u32* __restrict__ off; const RbText* __restrict__ st; u32 count;
    const u64* __restrict__ rules; const u32* __restrict__ S;
    u64* tbits; u64* ooff;
};
__device__ __forceinline__ bool rb_refused(u32 n, const RbText& t) { return n > RB_TEXT_MAX || t.err != 0; }

// per text: the bits of its fields, and the bytes its stream takes in the output, rounded up to 8 (0 for a refused text)
template <int KIND>
__global__ __launch_bounds__(256) void rb_cost_kernel(const RbEnc E) {
    __shared__ u64 sm[4];
    for (u32 k = blockIdx.x; k < E.count; k += gridDim.x) {
        const u32 base = E.off[k], n = E.off[k + 1] - base;
        const RbText t = E.st[k];
        if (rb_refused(n, t)) { if (threadIdx.x == 0) { E.tbits[k] = 0; E.ooff[k] = 0; } continue; }
        const RpFields f{ E.rules + base, t.R, E.S + base };
        const u64 nf = 1 + 2ull * t.R + t.m;
        u64 sum = 0;
        for (u64 j0 = (u64)threadIdx.x * RB_ITEMS; j0 < nf; j0 += RB_CHUNK) {
            RpFields::Item it[RB_ITEMS];
#pragma unroll
            for (u32 q = 0; q < RB_ITEMS; ++q) f.load<KIND, true>(min(j0 + q, nf - 1), it[q]);
#pragma unroll
            for (u32 q = 0; q < RB_ITEMS; ++q) if (j0 + q < nf) sum += f.bits<KIND>(it[q]);
        }
        sum = wave_reduce_sum(sum);
        if (lane_id() == 0) sm[wave_id()] = sum;
        __syncthreads();
        if (threadIdx.x == 0) {
            const u64 tb = sm[0] + sm[1] + sm[2] + sm[3];
            const u64 len = (tb >> 3) + ((tb & 7) <= 5 ? 1 : 2);           // bit_stream_len
            E.tbits[k] = tb;
            E.ooff[k] = (len + 7) & ~7ull;
        }
        __syncthreads();
    }
}

// a workgroup per text: chunks of 2048 fields, the costs scanned inside the chunk, the chunks chained by a carry.  The output is zeroed.
template <int KIND>
__global__ __launch_bounds__(256) void rb_pack_kernel(const RbEnc E, u64* __restrict__ out) {
    __shared__ u32 sm[5];
    for (u32 k = blockIdx.x; k < E.count; k += gridDim.x) {
        const u32 base = E.off[k], n = E.off[k + 1] - base;
        const RbText t = E.st[k];
        if (rb_refused(n, t)) continue;
        const RpFields f{ E.rules + base, t.R, E.S + base };
        const u64 nf = 1 + 2ull * t.R + t.m;
        u64 carry = 8ull * E.ooff[k];
        for (u64 c0 = 0; c0 < nf; c0 += RB_CHUNK) {
            const u64 j0 = c0 + (u64)threadIdx.x * RB_ITEMS;
            RpFields::Item it[RB_ITEMS];
            u32 sum = 0;
#pragma unroll
            for (u32 q = 0; q < RB_ITEMS; ++q) f.load<KIND, false>(min(j0 + q, nf - 1), it[q]);
#pragma unroll
            for (u32 q = 0; q < RB_ITEMS; ++q) if (j0 + q < nf) sum += f.bits<KIND>(it[q]);
            u32 total;
            const u32 excl = block_exclusive_sum<u32, 4>(sum, sm, total);
            BitSink sink;
            sink.out = out; sink.pos = carry + excl; sink.acc = 0; sink.cnt = 0;
#pragma unroll
            for (u32 q = 0; q < RB_ITEMS; ++q) if (j0 + q < nf) f.put<KIND>(sink, it[q]);
            sink.flush();
            carry += total;
        }
    }
}

// io/BitOStream.hpp:53-64 for every stream, as lzb_terminators_kernel
__global__ __launch_bounds__(256) void rb_terminators_kernel(const RbEnc E, u8* __restrict__ out) {
    for (u32 k = blockIdx.x * 256 + threadIdx.x; k < E.count; k += gridDim.x * 256) {
        if (E.ooff[k + 1] == E.ooff[k]) continue;              // a refused text
        const u64 tb = E.tbits[k];
        u8* o = out + E.ooff[k] + (tb >> 3);
        const u32 u = (u32)(tb & 7);
        if (u <= 5) o[0] |= (u8)u; else o[1] = (u8)u;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------
int rb_kind(int coder) {                                       // public coder id -> kind of RpFields' coders; -1: none
    switch (coder) {
        case TDC_GPU_CODER_BIT: return ENC_TAB;
        case TDC_GPU_CODER_ASCII: return ENC_ASCII;
        case TDC_GPU_CODER_GAMMA: return ENC_GAMMA;
        case TDC_GPU_CODER_DELTA: return ENC_DELTA;
        default: return -1;
    }
}

// the slots of text k's table: the power of two from spb * n on; none for a text without a pair or one the batch refuses
u64 rb_table_slots(u64 n, u32 spb) {
    if (n < 2 || n > RB_TEXT_MAX) return 0;
    u64 cap = RB_MIN_CAP;
    while (cap < spb * n) cap <<= 1;
    return cap;
}

// what the host knows before the device is asked: the borders as 32-bit words, the accepted texts longest first, every text's table
struct RbPlan { std::vector<u32> off32, order; std::vector<u64> toff; u64 slots = 0; u32 n_max = 0; };

// what the arena holds per call: the text, S (4 n), taken (n), the rules (8 n), 16 bytes per slot -- 4 (2) slots per text byte rounded
// up to a power of two per text: 64 to 128 (32 to 64) bytes per text byte --, 160 bytes per text, and the streams in the room of the
// tables (a stream takes at most 24 bytes per text byte)
void rb_plan(Ctx& c, const uint64_t* in_off, size_t count, size_t out_bound, RbPlan& L) {
    const size_t n = (size_t)in_off[count];
    const u32 spb = c.repair_batch_table ? 2u : 4u;
    L.off32.resize(count + 1); L.toff.resize(count + 1);
    for (size_t k = 0; k <= count; ++k) {
        L.off32[k] = (u32)in_off[k];
        L.toff[k] = L.slots;
        if (k == count) break;
        const u64 nk = in_off[k + 1] - in_off[k];
        L.slots += rb_table_slots(nk, spb);
        if (nk <= RB_TEXT_MAX) { L.order.push_back((u32)k); L.n_max = std::max<u32>(L.n_max, (u32)nk); }
    }
    std::stable_sort(L.order.begin(), L.order.end(), [&](u32 a, u32 b) { return in_off[a + 1] - in_off[a] > in_off[b + 1] - in_off[b]; });
    reserve_arena(c, 14 * n + std::max<size_t>(16 * (size_t)L.slots, out_bound + 64 * count) + 160 * (count + 1) + ((size_t)4 << 20));
}

// the device side of one batch
struct RbBatch {
    const u8* text = nullptr; u32* off = nullptr; u32* S = nullptr; u64* rules = nullptr; RbText* st = nullptr;
    size_t table_mark = 0;                                     // the arena in front of the tables: they are dead once the grammars stand
    u32 launches = 0;
    std::vector<RbText> host;                                  // every text's state, read back behind the last launch
};

// uploads the texts and the plan, runs the launches until no text is unfinished and reads the states back (count >= 1)
void rb_grammars(Ctx& c, const uint8_t* in, size_t n, size_t count, const RbPlan& L, u64 max_rules, RbBatch& B, Events& ev, int* e_up) {
    hipStream_t s = c.stream;
    B.text = upload_plain(c, in, n);
    B.off = c.arena.get<u32>(count + 1);
    u32* d_order = c.arena.get<u32>(count + 1);
    u64* d_toff = c.arena.get<u64>(count + 1);
    HIP_TRY(hipMemcpyAsync(B.off, L.off32.data(), (count + 1) * sizeof(u32), hipMemcpyHostToDevice, s));
    if (!L.order.empty()) HIP_TRY(hipMemcpyAsync(d_order, L.order.data(), L.order.size() * sizeof(u32), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_toff, L.toff.data(), (count + 1) * sizeof(u64), hipMemcpyHostToDevice, s));
    *e_up = ev.tick();
    B.st = c.arena.get<RbText>(count);
    u32* d_unfinished = c.arena.get<u32>(1);
    B.S = c.arena.get<u32>(n + 1);
    B.rules = c.arena.get<u64>(n + 1);
    u8* taken = c.arena.get<u8>(n + 8);
    HIP_TRY(hipMemsetAsync(B.st, 0, count * sizeof(RbText), s));
    B.table_mark = c.arena.mark();
    RbArgs P;
    P.text = B.text; P.off = B.off; P.order = d_order; P.accepted = (u32)L.order.size();
    P.S = B.S; P.taken = taken; P.rules = B.rules;
    P.keys = c.arena.get<unsigned long long>((size_t)L.slots + 1);
    P.counts = c.arena.get<u32>((size_t)L.slots + 2);
    P.last = c.arena.get<u32>((size_t)L.slots + 2);
    P.tab_off = d_toff; P.st = B.st; P.unfinished = d_unfinished;
    P.rounds = (u32)c.repair_batch_rounds; P.spb = c.repair_batch_table ? 2u : 4u; P.max_rules = max_rules;
    if (P.accepted) {
        const unsigned grid = std::min<unsigned>(P.accepted, RB_MAX_GRID);
        const u64 most = (u64)L.n_max / rb_rounds(L.n_max, P.rounds) + 2;      // a text of n bytes needs fewer than n rounds and one visit that ends it
        for (;;) {
            HIP_TRY(hipMemsetAsync(d_unfinished, 0, sizeof(u32), s));
            rb_rounds_kernel<<<grid, 256, 0, s>>>(P);
            LAUNCH_CHECK();
            ++B.launches;
            if (!c.read(d_unfinished)) break;
            if (B.launches > most) throw HipError{hipErrorUnknown, "repair batch: the round loop does not end", (int)__LINE__};
        }
    }
    B.host.resize(count);
    HIP_TRY(hipMemcpyAsync(B.host.data(), B.st, count * sizeof(RbText), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
}

int rb_status(u64 n, const RbText& t) { return n > RB_TEXT_MAX ? TDC_GPU_ERR_TOO_LARGE : t.err ? TDC_GPU_ERR_INTERNAL : TDC_GPU_OK; }

// what can be said of the offsets without a device; throws ArgError
void rb_check_offsets(const uint64_t* in_off, size_t count) {
    if (in_off[0] != 0) throw ArgError{TDC_GPU_ERR_ARG, "repair batch: in_off[0] must be 0"};
    for (size_t k = 0; k < count; ++k)
        if (in_off[k + 1] < in_off[k]) throw ArgError{TDC_GPU_ERR_ARG, "repair batch: in_off must not decrease"};
    if (in_off[count] > 0xFFFFFFFEull || count > 0xFFFFFFFEull)
        throw ArgError{TDC_GPU_ERR_TOO_LARGE, "repair batch: the texts must be at most 2^32 - 2 bytes in all"};
}

size_t rb_bound(const uint64_t* in_off, size_t count, int coder) {
    const int kind = rb_kind(coder);
    if (kind < 0 || !in_off || in_off[0] != 0) return 0;
    size_t sum = 0;
    for (size_t k = 0; k < count; ++k) {
        if (in_off[k + 1] < in_off[k]) return 0;
        sum += align_up(repair_bound((size_t)(in_off[k + 1] - in_off[k]), kind), 8);
    }
    return in_off[count] > 0xFFFFFFFEull || count > 0xFFFFFFFEull ? 0 : sum;
}

template <int KIND>
void rb_encode_as(Ctx& c, const RbEnc& E, size_t count, size_t used, u8* d_out, bool cost) {
    hipStream_t s = c.stream;
    const unsigned grid = (unsigned)std::min<size_t>(count, (size_t)1 << 16);
    if (cost) { rb_cost_kernel<KIND><<<grid, 256, 0, s>>>(E); LAUNCH_CHECK(); return; }
    if (used) {
        HIP_TRY(hipMemsetAsync(d_out, 0, used, s));
        rb_pack_kernel<KIND><<<grid, 256, 0, s>>>(E, (u64*)d_out);
        LAUNCH_CHECK();
        rb_terminators_kernel<<<dec_grid(count), 256, 0, s>>>(E, d_out);
        LAUNCH_CHECK();
    }
}
void rb_encode(Ctx& c, int kind, const RbEnc& E, size_t count, size_t used, u8* d_out, bool cost) {
    switch (kind) {
        case ENC_TAB:   return rb_encode_as<ENC_TAB>(c, E, count, used, d_out, cost);
        case ENC_ASCII: return rb_encode_as<ENC_ASCII>(c, E, count, used, d_out, cost);
        case ENC_GAMMA: return rb_encode_as<ENC_GAMMA>(c, E, count, used, d_out, cost);
        default:        return rb_encode_as<ENC_DELTA>(c, E, count, used, d_out, cost);
    }
}

void repair_compress_batch(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* in_off, size_t count, uint64_t max_rules, int coder, uint8_t* out,
                           size_t out_cap, uint64_t* out_off, uint64_t* out_len, int32_t* status, tdc_gpu_stats* stats) {
    const int kind = rb_kind(coder);
    Ctx& c = ctx->c;
    if (stats) memset(stats, 0, sizeof(*stats));
    out_off[0] = 0;
    if (count == 0) return;
    const size_t n = (size_t)in_off[count];
    RbPlan L;
    rb_plan(c, in_off, count, rb_bound(in_off, count, coder), L);
    Events ev(c);
    const int e0 = ev.tick();
    int e1 = e0;
    RbBatch B;
    rb_grammars(c, in, n, count, L, max_rules, B, ev, &e1);
    c.arena.release(B.table_mark);
    RbEnc E;
    E.off = B.off; E.st = B.st; E.count = (u32)count; E.rules = B.rules; E.S = B.S;
    E.tbits = c.arena.get<u64>(count); E.ooff = c.arena.get<u64>(count + 1);
    rb_encode(c, kind, E, count, 0, nullptr, true);
    exclusive_sum_u64(c, E.ooff, E.ooff, count, E.ooff + count);
    std::vector<u64> tbits(count);
    c.read_n(E.ooff, (u64*)out_off, count + 1);
    c.read_n(E.tbits, tbits.data(), count);
    u64 rules = 0, replaced = 0, ties = 0, rebuilds = 0;
    for (size_t k = 0; k < count; ++k) {
        const u64 nk = in_off[k + 1] - in_off[k];
        const RbText& t = B.host[k];
        status[k] = rb_status(nk, t);
        out_len[k] = status[k] ? 0 : bit_stream_len(tbits[k]);
        if (!status[k]) { rules += t.R; replaced += nk - t.m; ties += t.tie_rounds; rebuilds += t.rebuilds; }
    }
    const int e2 = ev.tick();
    const size_t used = (size_t)out_off[count];
    if (used > out_cap) throw ArgError{TDC_GPU_ERR_OOM, "repair batch: output buffer too small (out_off[count] holds the required size)"};
    u8* d_out = c.arena.get<u8>(used + 8);
    rb_encode(c, kind, E, count, used, d_out, false);
    const int e3 = ev.tick();
    if (used) HIP_TRY(hipMemcpyAsync(out, d_out, used, hipMemcpyDeviceToHost, c.stream));
    const int e4 = ev.tick();
    if (stats) {
        stats->n = n; stats->out_len = used; stats->arena_bytes = c.arena.high;
        stats->rules = rules; stats->replaced = replaced;
        stats->tie_rounds = (uint32_t)std::min<u64>(ties, 0xFFFFFFFFull); stats->rebuilds = (uint32_t)std::min<u64>(rebuilds, 0xFFFFFFFFull);
        stats->len_rounds = B.launches;
        ev.span(&stats->ms_h2d, e0, e1); ev.span(&stats->ms_factorize, e1, e2); ev.span(&stats->ms_encode, e2, e3);
        ev.span(&stats->ms_d2h, e3, e4); ev.span(&stats->ms_total, e0, e4);
    }
    ev.finish();
}

void repair_grammar_batch(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* in_off, size_t count, uint64_t max_rules, uint64_t* rules,
                          uint64_t* rule_off, uint32_t* start, uint64_t* start_off, int32_t* status) {
    Ctx& c = ctx->c;
    rule_off[0] = 0; start_off[0] = 0;
    if (count == 0) return;
    const size_t n = (size_t)in_off[count];
    RbPlan L;
    rb_plan(c, in_off, count, 0, L);
    Events ev(c);
    int e1 = 0;
    RbBatch B;
    rb_grammars(c, in, n, count, L, max_rules, B, ev, &e1);
    // the slices as the device holds them, then back to back
    std::vector<u32> hs(n + 1);
    std::vector<u64> hr(n + 1);
    if (n) {
        HIP_TRY(hipMemcpyAsync(hs.data(), B.S, n * sizeof(u32), hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipMemcpyAsync(hr.data(), B.rules, n * sizeof(u64), hipMemcpyDeviceToHost, c.stream));
    }
    ev.finish();
    for (size_t k = 0; k < count; ++k) {
        const u64 nk = in_off[k + 1] - in_off[k];
        const RbText& t = B.host[k];
        status[k] = rb_status(nk, t);
        const u64 R = status[k] ? 0 : t.R, m = status[k] ? 0 : t.m;
        if (R) memcpy(rules + rule_off[k], hr.data() + in_off[k], R * sizeof(u64));
        if (m) memcpy(start + start_off[k], hs.data() + in_off[k], m * sizeof(u32));
        rule_off[k + 1] = rule_off[k] + R;
        start_off[k + 1] = start_off[k] + m;
    }
}

}  // namespace

}  // namespace tdc

using namespace tdc;

extern "C" {

size_t tdc_gpu_repair_batch_bound(const uint64_t* in_off, size_t count, int coder) { return rb_bound(in_off, count, coder); }

int tdc_gpu_repair_compress_batch(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* in_off, size_t count, uint64_t max_rules, int coder,
                                  uint8_t* out, size_t out_cap, uint64_t* out_off, uint64_t* out_len, int32_t* status, tdc_gpu_stats* stats) {
    try {                                                      // (before the context: no device needed)
        if (rb_kind(coder) < 0) throw ArgError{TDC_GPU_ERR_UNSUPPORTED, "repair: coder must be bit, ascii, gamma or delta"};
        if (!in_off || !out_off || (count && (!out || !out_len || !status))) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
        rb_check_offsets(in_off, count);
        if (!in && in_off[count]) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
    } catch (const ArgError& e) { if (ctx) ctx->last_error = e.msg; return e.code; }
    return guarded(ctx, [&] { repair_compress_batch(ctx, in, in_off, count, max_rules, coder, out, out_cap, out_off, out_len, status, stats); });
}

int tdc_gpu_repair_grammar_batch(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* in_off, size_t count, uint64_t max_rules, uint64_t* rules,
                                 uint64_t* rule_off, uint32_t* start, uint64_t* start_off, int32_t* status) {
    try {
        if (!in_off || !rule_off || !start_off || (count && !status)) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
        rb_check_offsets(in_off, count);
        if (in_off[count] && (!in || !rules || !start)) throw ArgError{TDC_GPU_ERR_ARG, "NULL argument"};
    } catch (const ArgError& e) { if (ctx) ctx->last_error = e.msg; return e.code; }
    return guarded(ctx, [&] { repair_grammar_batch(ctx, in, in_off, count, max_rules, rules, rule_off, start, start_off, status); });
}

}  // extern "C"
