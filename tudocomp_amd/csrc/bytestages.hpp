// bytestages.hpp -- the three byte-stream compressors behind bwt in the reference's `bwtzip = bwt:rle:mtf:encode(huff)` chain, on the
// device (bytestages.hip).  Citations are relative to the reference's include/tudocomp/.
//   rle           compressors/RunLengthEncoder.hpp:15-32 + util/vbyte.hpp:28-37
//   mtf           compressors/MTFCompressor.hpp:16-33
//   encode(huff)  compressors/LiteralEncoder.hpp:23-32 with coders/HuffmanCoder.hpp
//   encode(sle)   compressors/LiteralEncoder.hpp:23-32 with coders/SLECoder.hpp (encode.hip, next to lcpcomp's SLE encoder whose
//                 count, selection, fill scan and class codes it shares)
// Every function reads a device buffer of n bytes (n <= 2^32 - 2, at least 16 readable bytes behind it), takes its output buffer from
// the arena once the output length is known, and enqueues on c.stream.  An output of more than 2^32 - 2 bytes: StageTooLarge, thrown
// before anything of it is written.
#pragma once
#include "common.hpp"

namespace tdc {

constexpr u64 STAGE_MAX_BYTES = 0xFFFFFFFEull;
struct StageTooLarge { u64 bytes; };

// kernel geometry (the tests place their lengths around these borders)
constexpr u32 RLE_PER_THREAD = 16, RLE_TILE = 256 * RLE_PER_THREAD;
// mtf: one thread encodes MTF_CHUNK bytes from its own copy of the list.  Building that copy costs about 2 x 256 list steps whatever the
// chunk holds, encoding costs one step per unit of rank: with 1024 bytes per chunk the set-up is at most half a step per byte, and a
// text of 64 MiB still fills every compute unit with one workgroup (256 chunks = 256 KiB per workgroup).
constexpr u32 MTF_CHUNK = 1024, MTF_TILE = 256 * MTF_CHUNK;
constexpr u32 HUFF_PER_THREAD = 16, HUFF_TILE = 256 * HUFF_PER_THREAD;

// worst-case output lengths (64-bit: they may pass STAGE_MAX_BYTES)
u64 rle_bound(u64 n, u64 offset);
u64 huff_literals_bound(u64 n);
u64 sle_literals_bound(u64 n);
// device scratch a stage takes from the arena besides its output: rle, mtf and encode(huff); encode(sle) with its k-mer count
u64 stage_scratch_bound(u64 n);
u64 sle_literals_scratch_bound(u64 n, u32 kmer);

struct StageOut { u8* d = nullptr; u64 len = 0; };
StageOut rle_encode_device(Ctx& c, const u8* d_in, size_t n, u64 offset);
StageOut mtf_encode_device(Ctx& c, const u8* d_in, size_t n);
StageOut huff_literals_device(Ctx& c, const u8* d_in, size_t n);
StageOut sle_literals_device(Ctx& c, const u8* d_in, size_t n, u32 kmer);      // kmer 0 = 3; 1 .. 7

// The decoders (bytestages_decode.hip): the host loops of host/tdc_coders.hpp are their specification, including what they refuse.
// d_in: n bytes in the arena (256-byte aligned, 64 allocated bytes behind them).  The output comes from the bottom of the arena, scratch
// from its top (Arena::alloc_top: the caller releases it once the output exists).  Malformed input: StreamFormatError; an output of more
// than 2^32 - 2 bytes: StageTooLarge; an output the arena has no room for: StageArenaShort with its length and the scratch the stage
// holds at that moment -- each before anything of the output is written; a Huffman header that does not end inside the first 4 KiB (no
// encoder writes one): StageHostOnly.
struct StageArenaShort { u64 out_bytes, scratch_bytes; };
struct StageHostOnly {};
// What the driver reserves for a stage's scratch before it has run: n input bytes, `out` output bytes.  Enough for every stream an
// encoder writes; a stage that holds more (encode(huff) under a header that claims codes of more than 75 bits) says so in
// StageArenaShort::scratch_bytes.
u64 stage_decode_scratch_bound(u64 n, u64 out);
StageOut rle_decode_device(Ctx& c, const u8* d_in, size_t n, u64 offset);
StageOut mtf_decode_device(Ctx& c, const u8* d_in, size_t n);
StageOut huff_decode_device(Ctx& c, const u8* d_in, size_t n);
StageOut sle_decode_device(Ctx& c, const u8* d_in, size_t n, u32 kmer);

}  // namespace tdc
