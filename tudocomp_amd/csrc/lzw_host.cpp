// lzw_host.cpp -- the LZW parse of LZWCompressor (compressors/LZWCompressor.hpp:39-108), host side (g++, no HIP).
//
// The LZ78 parse with 256 root nodes (ids 0 .. 255, which need no table slots: a root is its byte) and no explicit literal: phrase k
// is the longest dictionary string at its start, its code is that node's id, the node (phrase k + next byte) gets id 256 + k, and
// phrase k + 1 starts AT that next byte.  Sequential for the same reason as LZ78; the dictionary is the table
// of lz78_host.cpp (phrase_table.hpp): a node lives at the hash of the string it spells, the slots of the next depths are requested
// ahead of the walk that verifies them.  All trie back-ends of the reference yield the same ids by contract.
#include "stages_host.hpp"
#include "phrase_table.hpp"

namespace tdc {

size_t lzw_parse_host(const uint8_t* in, size_t n, std::vector<uint32_t>& codes) {
    codes.clear();
    if (n == 0) return 0;                                          // :68 nothing but the coder's terminator is written
    PhraseTable tab;
    size_t cap = 1024;
    while (cap < n / 4 + 16) cap <<= 1;
    if (cap > ((size_t)1 << 32)) cap = (size_t)1 << 32;            // (htop holds 32 placement bits)
    tab.init(cap);
    codes.reserve(n / 6 + 16);
    constexpr size_t RING = PHRASE_RING;
    size_t W = 12, nphr = 0, last_i = 0;
    uint32_t next_id = 256;                                        // roots 0 .. 255 (:53-63), then insertion order
    uint64_t hs[RING];
    size_t i = 0;                                                  // start of the current phrase
    while (i < n) {
        if ((tab.used + 1) * 2 >= tab.mask) tab.grow();
        uint32_t node = in[i];                                     // get_rootnode(c)  :70, :82
        uint64_t h = roll(PHRASE_HASH0, in[i]);
        size_t pa = i + 1;                                         // the prefixes text[i .. pa) have been hashed and their slots requested
        size_t j = i + 1;                                          // the next byte to match
        for (;;) {
            const size_t lim = (j + W < n) ? j + W : n;
            while (pa < lim) { h = roll(h, in[pa]); hs[pa % RING] = h; __builtin_prefetch(&tab.slots.p[tab.home(h)], 1, 0); ++pa; }
            if (j >= n) { codes.push_back(node); i = n; break; }   // :99 the left-over phrase
            const uint8_t c = in[j];
            const uint64_t hk = hs[j % RING];
            const uint64_t key = (((uint64_t)node << 8) | c) + 1;
            size_t at = tab.home(hk);
            PhraseTable::Slot* s = &tab.slots.p[at];
            while (s->key && s->key != key) { at = (at + 1) & tab.mask; s = &tab.slots.p[at]; }
            if (s->key) { node = s->val; ++j; continue; }          // :91-93 traverse further
            s->key = key; s->val = next_id++; s->htop = (uint32_t)(hk >> 32); ++tab.used;
            codes.push_back(node);                                 // :78 encode(node.id(), Range(factor_count + 256))
            i = j;                                                 // :82 the next phrase starts at the byte that did not match
            if ((++nphr & 0xFFFFu) == 0) {
                W = phrase_window((i - last_i + 0x8000u) >> 16);
                last_i = i;
            }
            break;
        }
    }
    return codes.size();
}

}  // namespace tdc

extern "C" int tdc_lzw_factors(const uint8_t* in, size_t n, uint32_t** codes_out, size_t* z_out) {
    if ((!in && n) || !codes_out || !z_out) return -2;
    *codes_out = nullptr; *z_out = 0;
    if (n >= 0xFFFFFF00ull) return -4;                             // (ids are 32-bit: 256 + z must fit)
    try {
        std::vector<uint32_t> codes;
        const size_t z = tdc::lzw_parse_host(in, n, codes);
        uint32_t* a = (uint32_t*)malloc((z ? z : 1) * sizeof(uint32_t));
        if (!a) return -5;
        if (z) memcpy(a, codes.data(), z * sizeof(uint32_t));
        *codes_out = a; *z_out = z;
    } catch (...) { return -5; }
    return 0;
}
