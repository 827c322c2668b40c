// phrase_table.hpp -- the hashed (parent, byte) -> child dictionary of the LZ78-family parses on the host (lz78_host.cpp, lzw_host.cpp).
// A node is kept at the hash of the STRING it spells (lz78_host.cpp explains why); what is compared is the exact key (parent id, byte).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <new>
#include <utility>

namespace tdc {

struct PhraseTable {                 // open addressing; key = (parent << 8 | byte) + 1 (0: empty), value = child id
    struct Slot { uint64_t key; uint32_t val; uint32_t htop; };     // htop: upper half of the string hash (placement after a growth)
    struct Buf {
        Slot* p = nullptr; size_t n = 0;
        ~Buf() { free(p); }
        void alloc(size_t count) {
            free(p); p = nullptr; n = count;
            const size_t bytes = (count * sizeof(Slot) + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
            p = (Slot*)aligned_alloc((size_t)2 << 20, bytes);       // the table of a 1 GB input is gigabytes large and every miss lands on
            if (!p) throw std::bad_alloc();                         // a random page: huge pages where the kernel grants them
#ifdef MADV_HUGEPAGE
            (void)madvise(p, bytes, MADV_HUGEPAGE);
#endif
            memset(p, 0, count * sizeof(Slot));
        }
        void swap(Buf& o) { std::swap(p, o.p); std::swap(n, o.n); }
    } slots;
    uint64_t mask = 0;
    int shift = 64;                                                 // slot of a hash: h >> shift
    size_t used = 0;
    void init(size_t cap_pow2) {
        slots.alloc(cap_pow2); mask = cap_pow2 - 1; used = 0;
        shift = 64; for (size_t c = cap_pow2; c > 1; c >>= 1) --shift;
    }
    size_t home(uint64_t h) const { return shift == 64 ? 0 : (size_t)(h >> shift); }
    void grow() {
        Buf os; os.swap(slots);
        init((mask + 1) * 2);
        for (size_t i = 0; i < os.n; ++i) if (os.p[i].key) {
            size_t at = home((uint64_t)os.p[i].htop << 32);
            while (slots.p[at].key) at = (at + 1) & mask;
            slots.p[at] = os.p[i]; ++used;
        }
    }
};

// hash of a phrase prefix from the hash of the prefix one byte shorter (a function of the string alone)
inline uint64_t roll(uint64_t h, uint8_t c) {
    h = (h ^ ((uint64_t)c + 1)) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 29);
}


constexpr uint64_t PHRASE_HASH0 = 0x243F6A8885A308D3ull;           // hash of the empty prefix
constexpr size_t PHRASE_RING = 64;                                 // ring of prefix hashes (a power of two > the largest window)
// the window of depths requested ahead follows the running mean phrase length (+ 3, within [8, 48]); measured in lz78_host.cpp
inline size_t phrase_window(size_t mean) { return mean + 3 < 8 ? 8 : (mean + 3 > 48 ? 48 : mean + 3); }

}  // namespace tdc
