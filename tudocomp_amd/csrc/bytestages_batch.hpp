// bytestages_batch.hpp -- rle, mtf and encode(huff) over a batch of independent texts (bytestages_batch.hip, DESIGN.md section 5.3
// "Batches").  Between two stages the texts of a batch lie in ONE device buffer, text k at off[k] -- a multiple of 16, so that every
// 16-byte load of a kernel is aligned whatever the lengths are -- with len[k] bytes; the bytes between two texts are never read for
// a result.  A stage reads such a layout and returns the next one; its kernels walk tiles that belong to one text each.
#pragma once
#include "bytestages.hpp"

#include <functional>

namespace tdc {

constexpr u64 BATCH_TEXT_CAP = (u64)1 << 20;                  // include/tdc_gpu.h: BWT_BATCH_TEXT_CAP, the longest text of a batch pipeline
// Kernels that give a workgroup to a tile (or a thread to a text) are launched with at most this many workgroups and go on with
// `+= gridDim.x` (tests/test_gpu_pipeline_batch.py runs a batch with more tiles than that).
constexpr u32 BSB_MAX_BLOCKS = 1u << 16;

struct BatchLay {
    u8* d = nullptr;            // padded + 64 bytes
    u64* off = nullptr;         // device, count + 1: where text k starts (multiples of 16); off[count] = padded
    u64* len = nullptr;         // device, count
    u64 total = 0;              // the sum of len[]
    u64 padded = 0;
};

// called by the LAST stage of a chain once its output lengths are known (device array of count entries) and before it writes: the
// driver fills the caller's out_off / out_len there and throws if the caller's buffer does not take them
using BatchSizesHook = std::function<void(const u64* d_len)>;
// what the table build of encode(huff) took on the host, and on how many threads
struct BatchHuffInfo { float ms_tables = 0; u32 threads = 0; };

// off[] and padded for lengths on the device
void batch_layout(Ctx& c, BatchLay& lay, size_t count);
// bytes of the texts from `src` (text k at soff[k]) to dst (text k at doff[k]), len[k] bytes each; scratch from the arena
void batch_relayout(Ctx& c, const u8* src, const u64* soff, u8* dst, const u64* doff, const u64* len, size_t count);
// A stage whose output would pass STAGE_MAX_BYTES over the whole batch: StageTooLarge, before anything of it is written.
BatchLay rle_encode_batch(Ctx& c, const BatchLay& in, size_t count, u64 offset, const BatchSizesHook& hook);
BatchLay mtf_encode_batch(Ctx& c, const BatchLay& in, size_t count, const BatchSizesHook& hook);
// d_status (device, count): a text with a status other than 0 gets no stream (length 0); an accepted empty text gets its header and
// terminator.  threads: 0 = min(16, hardware threads)
BatchLay huff_literals_batch(Ctx& c, const BatchLay& in, size_t count, const int* d_status, const int32_t* status, u32 threads, BatchHuffInfo* info,
                             const BatchSizesHook& hook);
// what a stage takes from the arena besides its output, for L input bytes in count texts (DESIGN.md section 5.3 "Batches" states it)
inline u64 batch_stage_scratch(u64 L, u64 count) { return L / 2 + L / 16 + 4608 * count + ((u64)1 << 20); }

}  // namespace tdc
