// repair_host.cpp -- repair = RePairCompressor<coder> (compressors/RePairCompressor.hpp:96-336), host side (g++, no HIP): the
// specification of the device grammar construction (repair.hip) and the decoder of its streams.
//
// tdc_repair_grammar is the reference's loop on one core, O(rules * n): per round one walk over the live sequence that counts every
// adjacent pair (occurrences overlap) and takes a pair over as the maximum when its running count exceeds the best so far STRICTLY
// (:144) -- so the winner is, among the pairs with the largest count M, the one whose M-th occurrence comes first --, then one walk that
// replaces it left to right and continues BEHIND a replaced pair (:165-173).  The reference keeps the sequence as text[] / next[]
// links; here it is compacted in place, which visits the same symbols in the same order.  The empty input, on which the reference is
// undefined (n - 1 wraps at :133), is defined as no rules and no symbols.
#include "../../include/tdc_gpu.h"
#include "../host/tdc_coders.hpp"

#include <algorithm>
#include <stdlib.h>
#include <string.h>
#include <vector>

namespace {

using namespace tdc_amd;

// digram -> count of the current round; entries of older rounds are recognised by their stamp, so a round clears nothing
struct PairCounter {
    struct Slot { uint64_t key; uint32_t count, stamp; };
    std::vector<Slot> slots;
    size_t mask = 0;
    uint32_t stamp = 0;
    void begin(size_t pairs) {
        size_t cap = 1024;
        while (cap < 2 * pairs) cap <<= 1;
        if (cap > slots.size() || ++stamp == 0) { slots.assign(std::max(cap, slots.size()), Slot{0, 0, 0}); stamp = 1; }
        mask = slots.size() - 1;
    }
    uint32_t add(uint64_t key) {
        size_t h = (size_t)((key * 0x9E3779B97F4A7C15ull) >> 20) & mask;
        for (;; h = (h + 1) & mask) {
            Slot& s = slots[h];
            if (s.stamp != stamp) { s.key = key; s.count = 1; s.stamp = stamp; return 1; }
            if (s.key == key) return ++s.count;
        }
    }
};

template <typename T> T* to_malloc(const std::vector<T>& v) {
    T* p = (T*)malloc((v.empty() ? 1 : v.size()) * sizeof(T));
    if (p && !v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

}  // namespace

extern "C" int tdc_repair_grammar(const uint8_t* in, size_t n, uint64_t max_rules, uint64_t** rules_out, size_t* nrules_out,
                                  uint32_t** start_out, size_t* nstart_out) {
    if ((!in && n) || !rules_out || !nrules_out || !start_out || !nstart_out) return TDC_GPU_ERR_ARG;
    *rules_out = nullptr; *start_out = nullptr; *nrules_out = 0; *nstart_out = 0;
    if (n > ((size_t)1 << 30)) return TDC_GPU_ERR_TOO_LARGE;
    try {
        std::vector<uint32_t> S(in, in + n);
        std::vector<uint64_t> rules;
        PairCounter count;
        if (max_rules == 0) max_rules = ~0ull;
        while (S.size() >= 2) {                                                // (do ... while (rules < max_rules), :123-178)
            const size_t m = S.size();
            count.begin(m - 1);
            uint64_t best = 0;
            uint32_t best_count = 0;
            for (size_t i = 0; i + 1 < m; ++i) {
                const uint64_t di = (uint64_t)S[i] << 32 | S[i + 1];
                const uint32_t c = count.add(di);
                if (c > best_count) { best = di; best_count = c; }             // :144
            }
            if (best_count <= 1) break;                                        // :155
            const uint32_t sym = (uint32_t)(256 + rules.size());
            rules.push_back(best);
            size_t o = 0;
            for (size_t i = 0; i < m; ) {
                if (i + 1 < m && ((uint64_t)S[i] << 32 | S[i + 1]) == best) { S[o++] = sym; i += 2; }     // :165-173
                else S[o++] = S[i++];
            }
            S.resize(o);
            if (rules.size() >= max_rules) break;
        }
        uint64_t* r = to_malloc(rules);
        uint32_t* s = to_malloc(S);
        if (!r || !s) { free(r); free(s); return TDC_GPU_ERR_OOM; }
        *rules_out = r; *nrules_out = rules.size(); *start_out = s; *nstart_out = S.size();
    } catch (...) { return TDC_GPU_ERR_OOM; }
    return TDC_GPU_OK;
}

extern "C" int tdc_repair_decode(const uint8_t* in, size_t len, int coder, uint8_t* out, size_t out_cap, size_t* out_len) {
    if ((!in && len) || !out_len) return TDC_GPU_ERR_ARG;
    if (coder != TDC_GPU_CODER_BIT && coder != TDC_GPU_CODER_GAMMA && coder != TDC_GPU_CODER_DELTA && coder != TDC_GPU_CODER_ASCII)
        return TDC_GPU_ERR_UNSUPPORTED;
    try {
        RepairGrammar g;
        switch (coder) {
            case TDC_GPU_CODER_BIT:   repair_parse<BitCoder::Decoder>(in, len, g); break;
            case TDC_GPU_CODER_GAMMA: repair_parse<EliasGammaCoder::Decoder>(in, len, g); break;
            case TDC_GPU_CODER_DELTA: repair_parse<EliasDeltaCoder::Decoder>(in, len, g); break;
            default:                  repair_parse<ASCIICoder::Decoder>(in, len, g); break;
        }
        const uint64_t total = repair_text_length(g);                          // before any text is written
        if (total > 0xFFFFFFFEull) return TDC_GPU_ERR_TOO_LARGE;
        *out_len = (size_t)total;
        if (!out) return TDC_GPU_OK;
        if (total > out_cap) return TDC_GPU_ERR_OOM;
        ByteSink sink(out, out_cap);
        repair_expand(g, sink);
        return TDC_GPU_OK;
    } catch (const std::length_error&) { return TDC_GPU_ERR_TOO_LARGE;
    } catch (const std::runtime_error&) { return TDC_GPU_ERR_ARG;
    } catch (const std::bad_alloc&) { return TDC_GPU_ERR_OOM;
    } catch (...) { return TDC_GPU_ERR_INTERNAL; }
}
