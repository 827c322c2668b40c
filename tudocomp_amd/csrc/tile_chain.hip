// tile_chain.hip -- tile exits -> tile entries (tile_chain.hpp).  A thread walks at most one group of DX_G table rows.
#include "tile_chain.hpp"
#include "decode.hpp"

namespace tdc {
namespace {

__global__ void __launch_bounds__(256) dx_compose_kernel(const u16* __restrict__ lo, u32 nlo, u32 nhi, u32 S, u16* __restrict__ hi) {
    const u64 items = (u64)nhi * S;
    for (u64 w = (u64)blockIdx.x * 256 + threadIdx.x; w < items; w += (u64)gridDim.x * 256) {
        const u32 g = (u32)(w / S), o = (u32)(w - (u64)g * S);
        const u32 t1 = min((g + 1) * DX_G, nlo);
        u32 e = o;
        for (u32 t = g * DX_G; t < t1 && e != DX_NONE; ++t) e = lo[(size_t)t * S + e];
        hi[w] = (u16)e;
    }
}
// entries of the items of every group from the group's entry (entry_hi == nullptr: one group, entered in state e0)
__global__ void __launch_bounds__(256) dx_down_kernel(const u16* __restrict__ exit_lo, const u16* __restrict__ entry_hi, u32 nlo, u32 nhi, u32 S, u32 e0,
                                                      u16* __restrict__ entry_lo) {
    for (u32 g = blockIdx.x * 256 + threadIdx.x; g < nhi; g += gridDim.x * 256) {
        const u32 t1 = entry_hi ? min((g + 1) * DX_G, nlo) : nlo;
        u32 e = entry_hi ? entry_hi[g] : e0;
        for (u32 t = entry_hi ? g * DX_G : 0; t < t1; ++t) {
            entry_lo[t] = (u16)e;
            if (e != DX_NONE) e = exit_lo[(size_t)t * S + e];
        }
    }
}

}  // namespace

size_t dx_entries_scratch(u32 N0, u32 S) {
    const size_t N1 = cdiv(N0, DX_G), N2 = cdiv(N1, DX_G);
    return ((N1 + N2) * S + N2 + N1 + N0) * 2;
}

u16* dx_entries(Ctx& c, const u16* exit0, u32 N0, u32 S, void* scratch) {
    hipStream_t s = c.stream;
    const u32 N1 = cdiv(N0, DX_G), N2 = cdiv(N1, DX_G);
    if (N2 > DX_G) throw HipError{hipErrorUnknown, "tile entries: more than 2^27 tiles", (int)__LINE__};
    u16* exit1 = (u16*)scratch;
    u16* exit2 = exit1 + (size_t)N1 * S;
    u16* entry2 = exit2 + (size_t)N2 * S;
    u16* entry1 = entry2 + N2;
    u16* entry0 = entry1 + N1;
    dx_compose_kernel<<<dec_grid((size_t)N1 * S), 256, 0, s>>>(exit0, N0, N1, S, exit1);
    LAUNCH_CHECK();
    dx_compose_kernel<<<dec_grid((size_t)N2 * S), 256, 0, s>>>(exit1, N1, N2, S, exit2);
    LAUNCH_CHECK();
    dx_down_kernel<<<1, 256, 0, s>>>(exit2, nullptr, N2, 1, S, 0, entry2);
    LAUNCH_CHECK();
    dx_down_kernel<<<dec_grid(N2), 256, 0, s>>>(exit1, entry2, N1, N2, S, 0, entry1);
    LAUNCH_CHECK();
    dx_down_kernel<<<dec_grid(N1), 256, 0, s>>>(exit0, entry1, N0, N1, S, 0, entry0);
    LAUNCH_CHECK();
    return entry0;
}

}  // namespace tdc
