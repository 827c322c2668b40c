// tile_chain.hpp -- the tile scheme by which the device decoders of lcpcomp's short-token streams (decode.hip, the lean path) and of
// rle, encode(huff) and encode(sle) (bytestages_decode.hip) find where their codes start; DESIGN.md 5, item 4.
// next(x) depends on the bits behind x alone and reaches at most LA positions far, so the chain of code starts can enter a tile only in
// one of its first LA offsets (rle: in one of 2 x 11 states).  Per tile "in which state does the chain that enters in state o enter the
// next tile" is computed from next() in LDS (tile_exits), the exits are composed over groups of DX_G tiles on three levels and the
// entries brought back down (dx_entries); the decoder then walks every tile from its entry, once to count and once to emit.
#pragma once
#include "common.hpp"

namespace tdc {

// exit[t * S + o] = the state in which the chain that enters tile t in state o enters tile t + 1 (DX_NONE: it ends or breaks in t)
constexpr u32 DX_G = 512;
constexpr u16 DX_NONE = 0xFFFFu;

// The exits of the TPW tiles of T positions whose next(x) - x stand in nxl[] (LDS; 0: no code starts at x, the chain ends), for the
// LA states "enters at offset o" of each: tile0 is the first of them, tiles from ntiles on do not exist.  Called by the whole
// workgroup of 256 behind the barrier that completes nxl[].
template <u32 T, u32 TPW, typename D>
__device__ __forceinline__ void tile_exits(const D* nxl, u32 LA, u32 tile0, u32 ntiles, u16* __restrict__ exit0) {
    for (u32 w = threadIdx.x; w < TPW * LA; w += 256) {
        const u32 tt = w / LA, o = w - tt * LA;
        const u32 tile = tile0 + tt;
        if (tile >= ntiles) continue;
        const u32 tend = (tt + 1) * T;
        u32 e = tt * T + o, res = DX_NONE;
        for (u32 guard = 0; guard <= T; ++guard) {
            if (e >= tend) { res = e - tend; break; }
            const u32 d = nxl[e];
            if (!d) break;
            e += d;
        }
        exit0[(size_t)tile * LA + o] = (u16)res;
    }
}

// entry[t] = the state in which the chain that enters tile 0 in state 0 enters tile t (DX_NONE behind its end), from the exits of N0
// tiles of S states (every exit < S or DX_NONE): at most 2^24 tiles -> 2^15 groups -> 64 groups of groups, walked by one thread.
// Where the scratch comes from is the caller's business: dx_entries_scratch(N0, S) bytes, 2-byte aligned; the entries are its tail.
size_t dx_entries_scratch(u32 N0, u32 S);
u16* dx_entries(Ctx& c, const u16* exit0, u32 N0, u32 S, void* scratch);

}  // namespace tdc
