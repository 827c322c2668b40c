// lzss_sw_host.cpp -- lzss = LZSSSlidingWindowCompressor<coder> (compressors/LZSSSlidingWindowCompressor.hpp:39-143), host side
// (g++, no HIP): the specification of the device factorizer (lzss_sw.hip) and the decoder of its streams.
//
// The reference slides a buffer of 2 * window bytes over the input.  What it holds when the loop looks at text position p is a
// function of p, n and w alone:
//   candidates   s in [max(0, p - w), p), ascending
//   look-ahead   L(p) = end(p) - p,  end(p) = n for n < 2w, else clamp(p - w, 0, n - 2w) + 2w
//                (2w - p in the first w positions -- a factor may be LONGER than the window there --, w in the steady state, n - p in
//                the last w positions)
//   match of s   j = min(lce(s, p), L(p)); it replaces the best so far if j >= threshold and j > best (:75: the smallest s among the
//                longest matches wins; threshold 0 behaves as 1 since best starts at 0)
// so the greedy parse needs no buffer: tdc_lzss_sw_factors walks the text with these three rules.
#include "../../include/tdc_gpu.h"
#include "../host/tdc_coders.hpp"

#include <stdlib.h>
#include <string.h>
#include <vector>

namespace {

using namespace tdc_amd;

// :120-143 with the Decoder of one coder.  Refused (std::runtime_error): distance 0 and a distance above the text so far (the reference
// reads out of bounds), a token cut off by the end of the stream (the reference reads zeros there), a gamma / delta prefix the field
// readers refuse.  More than 2^32 - 2 bytes of text: std::length_error.  A factor of length 0 decodes to nothing.
template <typename decoder_t>
void lzss_sw_decode_loop(const uint8_t* in, size_t len, size_t window, std::vector<uint8_t>& text) {
    auto bits = std::make_shared<BitIStream>(in, len);
    decoder_t decoder(bits);
    while (!decoder.eof()) {
        const bool is_factor = decoder.template decode<bool>(bit_r);
        if (is_factor) {
            const size_t dist = decoder.template decode<size_t>(Range(text.size()));
            const size_t fnum = decoder.template decode<size_t>(Range(window));
            if (bits->overrun()) throw std::runtime_error("corrupt stream: cut-off factor");
            if (dist == 0 || dist > text.size()) throw std::runtime_error("corrupt stream: factor source out of range");
            if (fnum > 0xFFFFFFFEull - text.size()) throw std::length_error("lzss: the stream decodes to more than 2^32 - 2 bytes");
            const size_t fsrc = text.size() - dist;
            for (size_t i = 0; i < fnum; ++i) { const uint8_t b = text[fsrc + i]; text.push_back(b); }      // (may overlap itself)
        } else {
            const uliteral_t c = decoder.template decode<uliteral_t>(literal_r);
            if (bits->overrun()) throw std::runtime_error("corrupt stream: cut-off literal");
            if (text.size() >= 0xFFFFFFFEull) throw std::length_error("lzss: the stream decodes to more than 2^32 - 2 bytes");
            text.push_back(c);
        }
    }
}

}  // namespace

extern "C" int tdc_lzss_sw_factors(const uint8_t* in, size_t n, uint32_t window, uint32_t threshold, uint32_t** pos_out, uint32_t** src_out,
                                   uint32_t** len_out, size_t* z_out) {
    if ((!in && n) || !pos_out || !src_out || !len_out || !z_out || window == 0) return TDC_GPU_ERR_ARG;
    *pos_out = *src_out = *len_out = nullptr; *z_out = 0;
    if (n > 0xFFFFFFFEull) return TDC_GPU_ERR_TOO_LARGE;
    try {
        const size_t w = window, t = threshold ? threshold : 1;
        std::vector<uint32_t> pos, src, len;
        for (size_t p = 0; p < n; ) {
            size_t end = n;
            if (n >= 2 * w) { const size_t off = p > w ? p - w : 0; end = (off < n - 2 * w ? off : n - 2 * w) + 2 * w; }
            const size_t L = end - p;
            size_t best = 0, bsrc = 0;
            for (size_t s = p > w ? p - w : 0; s < p && best < L; ++s) {          // (nothing beats a match of L: :75 asks for a longer one)
                size_t j = 0;
                while (j < L && in[s + j] == in[p + j]) ++j;
                if (j >= t && j > best) { best = j; bsrc = s; }
            }
            if (best) { pos.push_back((uint32_t)p); src.push_back((uint32_t)bsrc); len.push_back((uint32_t)best); p += best; }
            else ++p;
        }
        const size_t z = pos.size(), bytes = (z ? z : 1) * sizeof(uint32_t);
        uint32_t* a = (uint32_t*)malloc(bytes), *b = (uint32_t*)malloc(bytes), *c = (uint32_t*)malloc(bytes);
        if (!a || !b || !c) { free(a); free(b); free(c); return TDC_GPU_ERR_OOM; }
        if (z) { memcpy(a, pos.data(), z * 4); memcpy(b, src.data(), z * 4); memcpy(c, len.data(), z * 4); }
        *pos_out = a; *src_out = b; *len_out = c; *z_out = z;
    } catch (...) { return TDC_GPU_ERR_OOM; }
    return TDC_GPU_OK;
}

// the loop of one coder with its exceptions as statuses (coder and window checked by the caller); also the path of small streams of
// tdc_gpu_lzss_sw_decompress (api_decompress.hip)
namespace tdc {
int lzss_sw_decode_host(const uint8_t* in, size_t len, int coder, uint32_t window, std::vector<uint8_t>& text) {
    try {
        switch (coder) {
            case TDC_GPU_CODER_BIT:   lzss_sw_decode_loop<BitCoder::Decoder>(in, len, window, text); break;
            case TDC_GPU_CODER_GAMMA: lzss_sw_decode_loop<EliasGammaCoder::Decoder>(in, len, window, text); break;
            case TDC_GPU_CODER_DELTA: lzss_sw_decode_loop<EliasDeltaCoder::Decoder>(in, len, window, text); break;
            default:                  lzss_sw_decode_loop<ASCIICoder::Decoder>(in, len, window, text); break;
        }
        return TDC_GPU_OK;
    } catch (const std::length_error&) { return TDC_GPU_ERR_TOO_LARGE;
    } catch (const std::runtime_error&) { return TDC_GPU_ERR_ARG;
    } catch (const std::bad_alloc&) { return TDC_GPU_ERR_OOM;
    } catch (...) { return TDC_GPU_ERR_INTERNAL; }
}
}  // namespace tdc

extern "C" int tdc_lzss_sw_decode(const uint8_t* in, size_t len, int coder, uint32_t window, uint8_t* out, size_t out_cap, size_t* out_len) {
    if ((!in && len) || !out_len) return TDC_GPU_ERR_ARG;
    if (coder != TDC_GPU_CODER_BIT && coder != TDC_GPU_CODER_GAMMA && coder != TDC_GPU_CODER_DELTA && coder != TDC_GPU_CODER_ASCII)
        return TDC_GPU_ERR_UNSUPPORTED;
    if (coder == TDC_GPU_CODER_BIT && window == 0) return TDC_GPU_ERR_ARG;      // (the other coders ignore the range: no window needed)
    std::vector<uint8_t> text;
    const int rc = tdc::lzss_sw_decode_host(in, len, coder, window, text);
    if (rc) return rc;
    *out_len = text.size();
    if (!out) return TDC_GPU_OK;
    if (text.size() > out_cap) return TDC_GPU_ERR_ARG;
    if (!text.empty()) memcpy(out, text.data(), text.size());
    return TDC_GPU_OK;
}
