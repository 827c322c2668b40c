// tdc_coders.hpp -- host-side mirror of tudocomp's Coder plugin surface for the lcpcomp / lz78 path.
//
//   tdc::Range, MinDistributedRange, TypeRange, FixedRange, LiteralRange, LengthRange, BitRange, literal_r / bit_r / len_r
//                                         include/tudocomp/Range.hpp:7-119          -> tdc_amd::Range ...
//   tdc::BitOStream                       include/tudocomp/io/BitOStream.hpp:17-164 -> tdc_amd::BitOStream
//   tdc::Encoder / tdc::Decoder           include/tudocomp/Coder.hpp:14-151         -> tdc_amd::Encoder / tdc_amd::Decoder
//   HuffmanCoder::{Encoder,Decoder}       coders/HuffmanCoder.hpp:521-613           -> tdc_amd::HuffmanCoder::{Encoder,Decoder}
//   EliasGammaCoder::{Encoder,Decoder}    coders/EliasGammaCoder.hpp:20-43          -> tdc_amd::EliasGammaCoder::...
//   ASCIICoder::{Encoder,Decoder}         coders/ASCIICoder.hpp:26-84               -> tdc_amd::ASCIICoder::...
//   BitCoder::{Encoder,Decoder}           coders/BitCoder.hpp                       -> tdc_amd::BitCoder::...
//   EliasDeltaCoder::{Encoder,Decoder}    coders/EliasDeltaCoder.hpp:20-43          -> tdc_amd::EliasDeltaCoder::...
//   lzss::encode_text / decode_text_internal  compressors/lzss/LZSSCoding.hpp:18-92, LCPCompressor.hpp:23-76
//
// As in the reference, overload resolution on the STATIC type of the range tag selects the literal coder (LiteralRange ->
// Huffman code) or the default binary coding (Range -> v - min in bits_for(max - min) bits, BitRange -> one bit).
// The GPU path never calls these per symbol (the whole token stream is produced on the device); they serve decompress(), the
// parity tests of the token format (tests/test_host_coders.py: host Encoder stream == oracle stream == device stream) and
// inputs too small to be worth a launch.  The Huffman table comes from tdc_huffman_table() of the C ABI, i.e. from the same
// std:: calls as the device path (huffman_host.cpp).
#pragma once

#include <cstdint>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/tdc_gpu.h"

namespace tdc_amd {

using uliteral_t = uint8_t;
using len_t = uint32_t;                                     // def.hpp:103

// ---- Range.hpp ---------------------------------------------------------------------------------------------------
class Range {
    size_t m_min, m_max;
public:
    constexpr Range(size_t max) : m_min(0), m_max(max) {}
    constexpr Range(size_t min, size_t max) : m_min(min), m_max(max) {}
    size_t min() const { return m_min; }
    size_t max() const { return m_max; }
    size_t delta() const { return m_max - m_min; }
};
class MinDistributedRange : public Range {
public:
    constexpr MinDistributedRange(size_t max) : Range(0, max) {}
    constexpr MinDistributedRange(size_t min, size_t max) : Range(min, max) {}
};
template <typename T> class TypeRange : public Range {
public:
    constexpr TypeRange() : Range(0, std::numeric_limits<T>::max()) {}
};
template <size_t t_min, size_t t_max> class FixedRange : public Range {
public:
    constexpr FixedRange() : Range(t_min, t_max) {}
};
class LiteralRange : public TypeRange<uliteral_t> { public: constexpr LiteralRange() {} };
class LengthRange : public TypeRange<len_t> { public: constexpr LengthRange() {} };
using BitRange = FixedRange<0, 1>;
constexpr auto bit_r = BitRange();
constexpr auto literal_r = LiteralRange();
constexpr auto len_r = LengthRange();

inline unsigned coder_bits_for(uint64_t v) { unsigned b = 0; if (!v) return 1; while (v) { ++b; v >>= 1; } return b; }   // util.hpp:194

// ---- io/BitOStream.hpp: MSB-first bit writer; the destructor (here: finish()) appends the 3-bit terminator (:53-64) ---
class BitOStream {
    std::vector<uint8_t>* m_sink;
    uint8_t m_next = 0;
    int m_cursor = 7;
    bool m_dirty = false, m_finished = false;
    void write_next() { if (m_dirty) { m_sink->push_back(m_next); m_next = 0; m_cursor = 7; m_dirty = false; } }
public:
    explicit BitOStream(std::vector<uint8_t>& sink) : m_sink(&sink) {}
    BitOStream(const BitOStream&) = delete;
    ~BitOStream() { finish(); }
    void finish() {
        if (m_finished) return;
        m_finished = true;
        const uint8_t set = (uint8_t)(7 - m_cursor);
        if (m_cursor >= 2) m_next |= set;
        else { write_next(); m_next = set; }
        m_dirty = true;
        write_next();
    }
    void write_bit(bool set) {
        if (set) m_next |= (uint8_t)(1u << m_cursor);
        m_dirty = true;
        if (--m_cursor < 0) write_next();
    }
    template <typename T> void write_int(T value, size_t bits = sizeof(T) * 8) {
        for (int i = (int)bits - 1; i >= 0; --i) write_bit(i < 64 ? (((uint64_t)value >> i) & 1u) != 0 : false);
    }
    template <typename T> void write_compressed_int(T v, size_t b = 7) {      // :150-163
        uint64_t x = (uint64_t)v;
        do {
            const uint64_t cur = x;
            x >>= b;
            write_bit(x > 0);
            write_int(cur, b);
        } while (x > 0);
    }
    template <typename T> void write_unary(T v) { uint64_t x = (uint64_t)v; while (x--) write_bit(0); write_bit(1); }
    template <typename T> void write_elias_gamma(T v) { write_unary(coder_bits_for((uint64_t)v)); write_int((uint64_t)v, coder_bits_for((uint64_t)v)); }
    template <typename T> void write_elias_delta(T v) { write_elias_gamma(coder_bits_for((uint64_t)v)); write_int((uint64_t)v, coder_bits_for((uint64_t)v)); }   // :131-135
};

// ---- io/BitIStream.hpp:16-195 ------------------------------------------------------------------------------------
class BitIStream {
    const uint8_t* m_p; size_t m_n, m_idx = 0;
    uint8_t m_current = 0, m_next = 0, m_final_bits = 0, m_cursor = 0;
    bool m_is_final = false, m_overrun = false;
    void read_next() {
        m_current = m_next; m_cursor = 7;
        if (m_idx < m_n) {
            m_next = m_p[m_idx++];
            if (m_idx == m_n) { m_final_bits = m_next & 7; if (m_final_bits >= 6) { m_is_final = true; m_next = 0; } }
        } else { m_is_final = true; m_final_bits = m_current & 7; m_next = 0; }
    }
public:
    BitIStream(const uint8_t* p, size_t n) : m_p(p), m_n(n) {
        if (n) { m_next = m_p[m_idx++]; read_next(); } else { m_is_final = true; }
    }
    bool eof() const { return m_is_final && m_cursor <= (7 - m_final_bits); }
    bool overrun() const { return m_overrun; }               // a bit has been asked for behind the end (it read as 0)
    size_t size_bytes() const { return m_n; }
    unsigned read_bit() {
        if (eof()) { m_overrun = true; return 0; }
        unsigned bit = (m_current >> m_cursor) & 1;
        if (m_cursor) --m_cursor; else read_next();
        return bit;
    }
    uint64_t read_int(unsigned bits) { uint64_t v = 0; while (bits--) v = (v << 1) | read_bit(); return v; }
    template <typename T> T read_int() { return (T)read_int(sizeof(T) * 8); }
    uint64_t read_compressed_int(unsigned b = 7) {
        uint64_t v = 0; unsigned i = 0; bool more;
        do { more = read_bit(); v |= read_int(b) << (b * i++); } while (more);
        return v;
    }
    uint64_t read_unary() { uint64_t v = 0; while (!read_bit()) { if (eof() || ++v > 64) throw std::runtime_error("corrupt unary code"); } return v; }
    uint64_t read_elias_gamma() { const unsigned b = (unsigned)read_unary(); return read_int(b); }
    // io/BitIStream.hpp:158-162; a width above 64 (the reference would shift out of range) is refused
    uint64_t read_elias_delta() { const uint64_t b = read_elias_gamma(); if (b > 64) throw std::runtime_error("corrupt delta code"); return read_int((unsigned)b); }
};

// ---- Coder.hpp:14-151 -----------------------------------------------------------------------------------------------
class Encoder {
protected:
    std::shared_ptr<BitOStream> m_out;
public:
    template <typename literals_t> Encoder(std::shared_ptr<BitOStream> out, literals_t&&) : m_out(std::move(out)) {}
    template <typename value_t> void encode(value_t v, const Range& r) { m_out->write_int((uint64_t)v - r.min(), coder_bits_for(r.max() - r.min())); }
    template <typename value_t> void encode(value_t v, const BitRange&) { m_out->write_bit(v != 0); }
    const std::shared_ptr<BitOStream>& stream() { return m_out; }
};
class Decoder {
protected:
    std::shared_ptr<BitIStream> m_in;
public:
    explicit Decoder(std::shared_ptr<BitIStream> in) : m_in(std::move(in)) {}
    bool eof() const { return m_in->eof(); }
    // the fewest bits a factor (src, len) of a text of n positions takes: decode_text's plausibility check of a header
    static unsigned min_factor_bits(size_t n) { return coder_bits_for(n); }
    template <typename value_t> value_t decode(const Range& r) { return (value_t)(r.min() + m_in->read_int(coder_bits_for(r.max() - r.min()))); }
    template <typename value_t> value_t decode(const BitRange&) { return (value_t)m_in->read_bit(); }
    const std::shared_ptr<BitIStream>& stream() { return m_in; }
};

// literal iterators (Literal.hpp: has_next() / next() yielding {c, pos})
struct Literal { uliteral_t c; size_t pos; };
struct NoLiterals { bool has_next() const { return false; } Literal next() { return {0, 0}; } };
// lzss::TextLiterals (compressors/lzss/LZSSLiterals.hpp:10-50): the positions no factor covers, in text order
struct Factor { len_t pos, src, len; };
class TextLiterals {
    const uint8_t* m_text; size_t m_n; const std::vector<Factor>* m_f; size_t m_pos = 0, m_next = 0;
    void skip() { while (m_next < m_f->size() && m_pos == (*m_f)[m_next].pos) { m_pos += (*m_f)[m_next].len; ++m_next; } }
public:
    TextLiterals(const uint8_t* text, size_t n, const std::vector<Factor>& f) : m_text(text), m_n(n), m_f(&f) { skip(); }
    bool has_next() const { return m_pos < m_n; }
    Literal next() { const Literal l{m_text[m_pos], m_pos}; ++m_pos; skip(); return l; }
};

// ---- coders/HuffmanCoder.hpp:521-613 ------------------------------------------------------------------------------
struct HuffmanCoder {
    class Encoder : public tdc_amd::Encoder {
        uint32_t m_sigma = 0;
        uint8_t m_len[256] = {0};
        uint64_t m_code[256] = {0};
    public:
        template <typename literals_t> Encoder(std::shared_ptr<BitOStream> out, literals_t&& literals) : tdc_amd::Encoder(out, NoLiterals()) {
            uint32_t C[256] = {0};                                           // huff::count_alphabet_literals :37-48
            while (literals.has_next()) ++C[literals.next().c];
            uint32_t longest = 0; uint8_t order[256];
            if (tdc_huffman_table(C, &m_sigma, &longest, order, m_len, m_code)) throw std::runtime_error("tdc_huffman_table failed");
            if (m_sigma <= 1) { m_out->write_bit(0); return; }               // :538-540
            m_out->write_bit(1);                                             // :542 + huffmantable_encode :264-273
            uint8_t numl[256] = {0};
            for (int s = 0; s < 256; ++s) if (m_len[s]) ++numl[m_len[s] - 1];
            m_out->write_compressed_int(longest);
            for (uint32_t i = 0; i < longest; ++i) m_out->write_compressed_int(numl[i]);
            m_out->write_compressed_int(m_sigma);
            for (uint32_t i = 0; i < m_sigma; ++i) m_out->write_int(order[i], 8);
        }
        using tdc_amd::Encoder::encode;                                      // default encoding as fallback
        template <typename value_t> void encode(value_t v, const LiteralRange&) {      // :562-569
            const uint8_t c = (uint8_t)v;
            if (m_sigma <= 1) m_out->write_int(c, 8);
            else m_out->write_int(m_code[c], m_len[c]);
        }
    };
    class Decoder : public tdc_amd::Decoder {
        bool m_table = false;
        uint8_t m_order[256]; uint64_t m_first[256]; size_t m_prefix[256]; uint8_t m_numl[256]; unsigned m_longest = 0; size_t m_sigma = 0;
    public:
        explicit Decoder(std::shared_ptr<BitIStream> in) : tdc_amd::Decoder(std::move(in)) {   // :581-597
            m_table = m_in->read_bit();
            if (!m_table) return;
            m_longest = (unsigned)(m_in->read_compressed_int() & 0xFF);
            if (!m_longest) throw std::runtime_error("corrupt Huffman table");
            for (unsigned i = 0; i < m_longest; ++i) m_numl[i] = (uint8_t)m_in->read_compressed_int();
            m_sigma = m_in->read_compressed_int();
            if (m_sigma > 256) throw std::runtime_error("corrupt Huffman table");
            for (size_t i = 0; i < m_sigma; ++i) m_order[i] = (uint8_t)m_in->read_int(8);
            m_first[m_longest - 1] = 0;                                      // gen_first_codes :192-198
            for (unsigned i = m_longest - 1; i > 0; --i) m_first[i - 1] = (m_first[i] + m_numl[i]) / 2;
            size_t acc = 0;                                                  // gen_prefix_sum_lengths :350-370
            for (unsigned l = 0; l < m_longest; ++l) { m_prefix[l] = acc; acc += m_numl[l]; }
        }
        using tdc_amd::Decoder::decode;
        template <typename value_t> value_t decode(const LiteralRange&) {     // :606-611, huffman_decode :377-397
            if (!m_table) return (value_t)m_in->read_int(8);
            uint64_t value = 0; unsigned length = 0;
            do { value = (value << 1) + m_in->read_bit(); ++length; } while (length <= m_longest && value < m_first[length - 1]);
            if (length > m_longest) throw std::runtime_error("corrupt Huffman code");
            --length;
            const uint64_t off = value - m_first[length];
            if (off >= m_numl[length] || m_prefix[length] + off >= m_sigma) throw std::runtime_error("corrupt Huffman code");   // a table that violates Kraft
            return (value_t)m_order[m_prefix[length] + off];
        }
    };
};

// ---- coders/EliasGammaCoder.hpp:20-43 -------------------------------------------------------------------------------
struct EliasGammaCoder {
    class Encoder : public tdc_amd::Encoder {
    public:
        using tdc_amd::Encoder::Encoder;
        using tdc_amd::Encoder::encode;
        template <typename value_t> void encode(value_t v, const Range&) { m_out->write_elias_gamma((uint64_t)v); }
    };
    class Decoder : public tdc_amd::Decoder {
    public:
        using tdc_amd::Decoder::Decoder;
        using tdc_amd::Decoder::decode;
        template <typename value_t> value_t decode(const Range&) { return (value_t)m_in->read_elias_gamma(); }
        static unsigned min_factor_bits(size_t) { return 4; }                 // the ranges are ignored: "1" (an empty field, src = 0) + gamma(1)
    };
};

// ---- coders/EliasDeltaCoder.hpp:20-43: as EliasGammaCoder with delta(v) = gamma(bits_for(v)), then v in bits_for(v) bits ------------
struct EliasDeltaCoder {
    class Encoder : public tdc_amd::Encoder {
    public:
        using tdc_amd::Encoder::Encoder;
        using tdc_amd::Encoder::encode;
        template <typename value_t> void encode(value_t v, const Range&) { m_out->write_elias_delta((uint64_t)v); }
    };
    class Decoder : public tdc_amd::Decoder {
    public:
        using tdc_amd::Decoder::Decoder;
        using tdc_amd::Decoder::decode;
        template <typename value_t> value_t decode(const Range&) { return (value_t)m_in->read_elias_delta(); }
        static unsigned min_factor_bits(size_t) { return 5; }                 // "1" + delta(1)
    };
};

// ---- coders/BitCoder.hpp: nothing but the default binary coding of Coder.hpp:60-77 (a literal is a TypeRange<uliteral_t>: 8 bits) -----
struct BitCoder {
    class Encoder : public tdc_amd::Encoder { public: using tdc_amd::Encoder::Encoder; };
    class Decoder : public tdc_amd::Decoder { public: using tdc_amd::Decoder::Decoder; };
};

// ---- coders/ASCIICoder.hpp:26-84 -------------------------------------------------------------------------------------
struct ASCIICoder {
    class Encoder : public tdc_amd::Encoder {
    public:
        using tdc_amd::Encoder::Encoder;
        template <typename value_t> void encode(value_t v, const Range&) {
            const std::string s = std::to_string((uint64_t)v);
            for (uint8_t c : s) m_out->write_int(c, 8);
            m_out->write_int((uint8_t)':', 8);
        }
        template <typename value_t> void encode(value_t v, const LiteralRange&) { m_out->write_int((uint8_t)v, 8); }
        template <typename value_t> void encode(value_t v, const BitRange&) { m_out->write_int((uint8_t)(v ? '1' : '0'), 8); }
    };
    class Decoder : public tdc_amd::Decoder {
    public:
        using tdc_amd::Decoder::Decoder;
        template <typename value_t> value_t decode(const Range&) {
            uint64_t v = 0; int digits = 0;
            for (uint8_t c = (uint8_t)m_in->read_int(8); c >= '0' && c <= '9'; c = (uint8_t)m_in->read_int(8)) {
                v = v * 10 + (c - '0'); ++digits;
                if (m_in->eof()) break;
            }
            if (!digits) throw std::runtime_error("corrupt stream: integer expected");
            return (value_t)v;
        }
        template <typename value_t> value_t decode(const LiteralRange&) { return (value_t)m_in->read_int(8); }
        template <typename value_t> value_t decode(const BitRange&) { return (value_t)((uint8_t)m_in->read_int(8) != '0'); }
    };
};

// ---- lzss::encode_text (compressors/lzss/LZSSCoding.hpp:18-92): factors sorted by pos -------------------------------
template <typename coder_t>
inline void encode_text(coder_t& coder, const uint8_t* text, size_t n, const std::vector<Factor>& factors) {
    size_t flen_min = std::numeric_limits<len_t>::max(), flen_max = 0, fdist_max = 0;      // FactorBuffer :41-47 (empty: max / 0)
    {
        size_t p = 0;
        for (const Factor& f : factors) {
            if (f.len < flen_min) flen_min = f.len;
            if (f.len > flen_max) flen_max = f.len;
            if (f.pos - p > fdist_max) fdist_max = f.pos - p;
            p = (size_t)f.pos + f.len;
        }
        if (n - p > fdist_max) fdist_max = n - p;
    }
    if (factors.empty()) { flen_min = std::numeric_limits<len_t>::max(); flen_max = 0; }
    const Range text_r(n);
    const MinDistributedRange flen_r(flen_min, flen_max);
    const Range fdist_r(fdist_max);
    coder.encode(n, len_r);
    coder.encode(flen_min, text_r);
    coder.encode(flen_max, text_r);
    coder.encode(fdist_max, text_r);
    size_t p = 0;
    for (const Factor& f : factors) {
        if (f.pos == p) coder.encode(false, bit_r);
        else { coder.encode(true, bit_r); coder.encode(f.pos - p, fdist_r); }
        while (p < f.pos) coder.encode(text[p++], literal_r);
        coder.encode(f.src, text_r);
        coder.encode(f.len, flen_r);
        p += (size_t)f.len;
    }
    if (p < n) { coder.encode(true, bit_r); coder.encode(n - p, fdist_r); }
    while (p < n) coder.encode(text[p++], literal_r);
}

// ---- lcpcomp::decode_text_internal (LCPCompressor.hpp:23-76): token stream -> text + reference forest --------------
// The decoded text is unique, so the references are resolved by following source chains instead of the reference's
// ScanDec buffers (forward and backward references alike: lcpcomp and lzss_lcp).
template <typename decoder_t>
inline void decode_text(decoder_t& decoder, std::vector<uint8_t>& text) {
    const size_t n = decoder.template decode<size_t>(len_r);
    if (n >= 0x7FFFFFFFull) throw std::runtime_error("corrupt stream: text length");       // 32-bit len_t, texts stay below 2^31 - 1
    const Range text_r(n);
    const size_t flen_min = decoder.template decode<size_t>(text_r);
    const size_t flen_max = decoder.template decode<size_t>(text_r);
    const size_t fdist_max = decoder.template decode<size_t>(text_r);
    {   // plausibility (corrupt headers would otherwise ask for gigabytes): a literal costs at least one bit, a factor at least
        // bits_for(n) (the universal codes: a few bits) and covers at most flen_max positions
        const size_t bits = decoder.stream()->size_bytes() * 8;
        if (n > bits + (bits / decoder_t::min_factor_bits(n) + 1) * (flen_max ? flen_max : 1)) throw std::runtime_error("corrupt stream: text length");
    }
    const MinDistributedRange flen_r(flen_min, flen_max >= flen_min ? flen_max : flen_min);
    const Range fdist_r(fdist_max);
    text.assign(n, 0);
    std::vector<uint32_t> ref(n, 0xFFFFFFFFu);
    size_t p = 0;
    while (!decoder.eof()) {
        size_t num = decoder.template decode<bool>(bit_r) ? decoder.template decode<size_t>(fdist_r) : 0;
        if (num > n - p) throw std::runtime_error("corrupt stream: too many literals");    // (p <= n; a gamma / delta field holds up to 64 bits)
        while (num--) text[p++] = decoder.template decode<uliteral_t>(literal_r);
        if (!decoder.eof()) {
            const size_t src = decoder.template decode<size_t>(text_r), len = decoder.template decode<size_t>(flen_r);
            if (len == 0 || len > n - p || src > n || len > n - src) throw std::runtime_error("corrupt stream: factor out of range");
            for (size_t j = 0; j < len; ++j) ref[p + j] = (uint32_t)(src + j);
            p += len;
        }
    }
    if (p != n) throw std::runtime_error("corrupt stream: length mismatch");
    std::vector<uint32_t> stack;
    for (size_t i = 0; i < n; ++i) {
        if (ref[i] == 0xFFFFFFFFu) continue;
        stack.clear();
        uint32_t q = (uint32_t)i;
        while (ref[q] != 0xFFFFFFFFu) {
            if (stack.size() > n) throw std::runtime_error("corrupt stream: reference cycle");
            stack.push_back(q); q = ref[q];
        }
        for (uint32_t r : stack) { text[r] = text[q]; ref[r] = 0xFFFFFFFFu; }
    }
}

// ---- the host loop behind tdc_lzss_decode (C ABI): decode_text with the Decoder of one of the five lzss_lcp coders (public coder ids).
// The specification of the device decoder for these streams and its path for small ones.  false: no such coder.
inline bool lzss_decode_coder(const uint8_t* in, size_t n, int coder, std::vector<uint8_t>& text) {
    auto bits = std::make_shared<BitIStream>(in, n);
    switch (coder) {
        case TDC_GPU_CODER_HUFF:  { HuffmanCoder::Decoder d(bits); decode_text(d, text); return true; }
        case TDC_GPU_CODER_GAMMA: { EliasGammaCoder::Decoder d(bits); decode_text(d, text); return true; }
        case TDC_GPU_CODER_ASCII: { ASCIICoder::Decoder d(bits); decode_text(d, text); return true; }
        case TDC_GPU_CODER_BIT:   { BitCoder::Decoder d(bits); decode_text(d, text); return true; }
        case TDC_GPU_CODER_DELTA: { EliasDeltaCoder::Decoder d(bits); decode_text(d, text); return true; }
        default: return false;
    }
}

// ---- the byte-stream compressors behind bwt (bwtzip = bwt:rle:mtf:encode(huff)) on the host ------------------------------------------
// They are the text of the C ABI's host decoders (tdc_rle_decode, tdc_mtf_decode, tdc_huff_decode_literals) and the host side of the
// CPU tests; the encoders restate what the reference's loops emit (the device kernels are pinned against the same rule).
// A sink that counts everything and stores what fits: out == nullptr measures.
struct ByteSink {
    uint8_t* out; size_t cap; uint64_t n = 0;
    ByteSink(uint8_t* o, size_t c) : out(o), cap(o ? c : 0) {}
    void put(uint8_t c) { if (n < cap) out[n] = c; if (~n) ++n; }
    void fill(uint8_t c, uint64_t k) {
        for (uint64_t i = n; i < cap && i - n < k; ++i) out[i] = c;
        n = k > ~n ? ~(uint64_t)0 : n + k;                     // (saturates: a ten-byte vbyte may ask for 2^64 - 1 bytes)
    }
};
// util/vbyte.hpp:28-37 (write) and :13-25 (read): seven bits per byte, least significant group first, bit 7 = "more"
template <typename sink_t> inline void write_vbyte(sink_t& os, uint64_t v) {
    while (v >= 128) { os.put((uint8_t)(0x80u | (v & 0x7Fu))); v >>= 7; }
    os.put((uint8_t)v);
}
inline uint64_t read_vbyte(const uint8_t* in, size_t n, size_t& i) {
    uint64_t v = 0;
    for (unsigned k = 0; ; ++k) {
        if (i >= n) throw std::runtime_error("corrupt rle stream: a vbyte runs off the end");
        if (k == 10) throw std::runtime_error("corrupt rle stream: a vbyte of more than ten bytes");
        const uint8_t b = in[i++];
        v |= (uint64_t)(b & 0x7Fu) << (7 * k);
        if (!(b & 0x80u)) return v;
    }
}
// rle_encode (compressors/RunLengthEncoder.hpp:15-32) as that loop behaves on x86-64: char is signed and istream::peek() yields 0 .. 255,
// so only bytes below 0x80 extend a run; the endless loop on a trailing 0xFF 0xFF (peek() == EOF == (char)0xFF) is cut off at the end of
// the input, where it emits what a 0xFF in mid-stream emits.
template <typename sink_t> inline void rle_encode(const uint8_t* in, size_t n, uint64_t offset, sink_t& os) {
    if (!n) return;
    uint8_t prev = in[0];
    os.put(prev);
    for (size_t i = 1; i < n; ) {
        const uint8_t c = in[i++];
        if (prev == c) {
            uint64_t run = 0;
            while (c < 0x80u && i < n && in[i] == c) { ++run; ++i; }
            os.put(c);
            write_vbyte(os, run + offset);
        } else os.put(c);
        prev = c;
    }
}
// rle_decode (:36-50): after two equal bytes a vbyte follows, run = vbyte - offset
template <typename sink_t> inline void rle_decode(const uint8_t* in, size_t n, uint64_t offset, sink_t& os) {
    if (!n) return;
    uint8_t prev = in[0];
    os.put(prev);
    for (size_t i = 1; i < n; ) {
        const uint8_t c = in[i++];
        if (prev == c) {
            const uint64_t v = read_vbyte(in, n, i);
            if (v < offset) throw std::runtime_error("corrupt rle stream: run length below the offset");
            os.fill(c, v - offset);
        }
        os.put(c);
        prev = c;
    }
}
// mtf_encode / mtf_decode (compressors/MTFCompressor.hpp:16-43): the list starts as 0 .. 255
template <typename sink_t> inline void mtf_encode(const uint8_t* in, size_t n, sink_t& os) {
    uint8_t list[256];
    for (int i = 0; i < 256; ++i) list[i] = (uint8_t)i;
    for (size_t i = 0; i < n; ++i) {
        const uint8_t c = in[i];
        unsigned j = 0;
        while (list[j] != c) ++j;
        os.put((uint8_t)j);
        for (; j > 0; --j) list[j] = list[j - 1];
        list[0] = c;
    }
}
template <typename sink_t> inline void mtf_decode(const uint8_t* in, size_t n, sink_t& os) {
    uint8_t list[256];
    for (int i = 0; i < 256; ++i) list[i] = (uint8_t)i;
    for (size_t i = 0; i < n; ++i) {
        unsigned j = in[i];
        const uint8_t c = list[j];
        os.put(c);
        for (; j > 0; --j) list[j] = list[j - 1];
        list[0] = c;
    }
}
// LiteralEncoder::compress / ::decompress (compressors/LiteralEncoder.hpp:23-41) with HuffmanCoder
struct BufferLiterals {
    const uint8_t* p; size_t n, i = 0;
    bool has_next() const { return i < n; }
    Literal next() { const Literal l{p[i], i}; ++i; return l; }
};
inline void huff_encode_literals(const uint8_t* in, size_t n, std::vector<uint8_t>& out) {
    auto bits = std::make_shared<BitOStream>(out);
    HuffmanCoder::Encoder coder(bits, BufferLiterals{in, n});
    for (size_t i = 0; i < n; ++i) coder.encode(in[i], literal_r);
    bits->finish();
}
template <typename sink_t> inline void huff_decode_literals(const uint8_t* in, size_t n, sink_t& os) {
    if (!n) throw std::runtime_error("corrupt stream: no Huffman header");
    // bits in front of the terminator (io/BitOStream.hpp:53-64): a header that needs more of them than there are is cut off
    const unsigned u = in[n - 1] & 7u;
    if (u >= 6 && n < 2) throw std::runtime_error("corrupt stream: no Huffman header");
    const uint64_t total = u >= 6 ? (uint64_t)(n - 2) * 8 + u : (uint64_t)(n - 1) * 8 + u;
    if (total < 1) throw std::runtime_error("corrupt stream: no Huffman header");
    if (in[0] & 0x80u) {                                     // "1" + table: longest, numl[], sigma as 8-bit groups, sigma bytes
        BitIStream probe(in, n);
        uint64_t need = 1;
        auto group = [&] { uint64_t v = probe.read_compressed_int(); need += 8; for (uint64_t x = v >> 7; x; x >>= 7) need += 8; return v; };
        probe.read_bit();
        const uint64_t longest = group() & 0xFF;
        for (uint64_t i = 0; i < longest && need <= total; ++i) (void)group();
        const uint64_t sigma = need <= total ? group() : 0;
        need += 8 * sigma;
        if (need > total || !longest || sigma > 256) throw std::runtime_error("corrupt stream: Huffman header cut off or inconsistent");
    }
    HuffmanCoder::Decoder dec(std::make_shared<BitIStream>(in, n));
    while (!dec.eof()) os.put(dec.template decode<uliteral_t>(literal_r));
}

// ---- LiteralEncoder::decompress (compressors/LiteralEncoder.hpp:34-41) with SLECoder::Decoder (coders/SLECoder.hpp:311-416) ----------
// The stream: the ranking (sigma and sigma symbols as compressed integers; a symbol is a byte, or 0xFF << 56 | the k bytes of a k-mer,
// first byte most significant), then one class code per symbol until the bit stream ends; a k-mer symbol stands for k bytes.  The class
// code of a rank depends on sigma_bits = bits_for(sigma - 1) alone (:378-404), and its length on its first three bits:
//   sigma_bits < 4:  sigma_bits plain bits
//   4, 5:            0 + 2 bits (ranks 0 .. 3) | 1 + sigma_bits bits
//   6:               00 + 3 | 01 + 3 (8 ..) | 10 + 4 (16 ..) | 11 + 6
//   >= 7:            0cc + 2 (4 cc ..) | 100, 101, 110 + 3 (16, 24, 32 ..) | 111 + sigma_bits
// sle_decode_literals is the specification of the device decoder (csrc/bytestages_decode.hip), its path for small streams, and the text
// of the C ABI's tdc_sle_decode.  Refused (std::runtime_error): a ranking that does not end inside the stream, sigma above 1024 (no
// encoder extends 256 bytes by more than 768 k-mers), a ranking entry that is neither a byte nor a k-mer of this k (marker byte, zero
// bytes between the marker and the k bytes), a rank >= sigma (the reference reads out of bounds there), a code cut off by the end of
// the stream (the reference reads zeros there).  More than 2^32 - 2 bytes of output: std::length_error.
#if defined(__HIPCC__)
#define TDC_CODERS_HD __host__ __device__
#else
#define TDC_CODERS_HD
#endif
constexpr uint32_t SLE_MAX_SIGMA = 1024;
constexpr uint32_t SLE_MAX_CODE_BITS = 13;                   // 3 + sigma_bits of 10
// header: at most ten groups for sigma and for every entry
constexpr size_t SLE_MAX_HEADER_BYTES = 10 * (1 + (size_t)SLE_MAX_SIGMA);
// length of the code whose first three bits are top3
TDC_CODERS_HD inline uint32_t sle_code_len(uint32_t sb, uint32_t top3) {
    if (sb < 4) return sb;
    if (sb < 6) return (top3 & 4u) ? 1 + sb : 3;
    if (sb == 6) return top3 < 4 ? 5 : top3 < 6 ? 6 : 8;
    return top3 < 4 ? 5 : top3 < 7 ? 6 : 3 + sb;
}
// rank of the code v (its sle_code_len bits, right-aligned)
TDC_CODERS_HD inline uint32_t sle_code_rank(uint32_t sb, uint32_t len, uint32_t v) {
    if (sb < 4) return v;
    if (sb < 6) return len == 3 ? (v & 3u) : (v & ((1u << sb) - 1));
    if (sb == 6) return len == 5 ? (v & 15u) : len == 6 ? 16 + (v & 15u) : (v & 63u);           // (01 + 3 bits = 8 + the three bits)
    return len == 5 ? v : len == 6 ? 16 + 8 * ((v >> 3) - 4) + (v & 7u) : (v & ((1u << sb) - 1));
}
struct SleRanking {
    uint32_t sigma = 0, sb = 1;
    uint64_t body = 0, total = 0;                            // first bit of the codes; bits in front of the terminator
    std::vector<uint64_t> ent;                               // rank -> its bytes (first byte most significant) | their number << 56
};
// 64 bits from bit x on, MSB first, zeros behind `total` (p: `avail` readable bytes)
inline uint64_t sle_peek(const uint8_t* p, size_t avail, uint64_t total, uint64_t x) {
    if (x >= total) return 0;
    const size_t b = (size_t)(x >> 3);
    uint64_t w = 0;
    for (size_t i = 0; i < 8; ++i) w = (w << 8) | (b + i < avail ? p[b + i] : 0);
    const unsigned sh = (unsigned)(x & 7);
    if (sh) w = (w << sh) | ((b + 8 < avail ? p[b + 8] : 0) >> (8 - sh));
    if (x + 64 > total) w &= ~0ull << (64 - (total - x));
    return w;
}
// the bits in front of the terminator (io/BitOStream.hpp:53-64) of a stream of n >= 1 bytes that ends with `last`
inline uint64_t sle_total_bits(size_t n, uint8_t last) {
    const unsigned u = last & 7u;
    if (u >= 6 && n < 2) throw std::runtime_error("corrupt stream: no SLE ranking");
    return u >= 6 ? (uint64_t)(n - 2) * 8 + u : (uint64_t)(n - 1) * 8 + u;
}
// Decoder ctor :333-346 from the first `avail` bytes of the stream (all of it, or at least SLE_MAX_HEADER_BYTES + 8)
inline void sle_parse_ranking(const uint8_t* p, size_t avail, uint64_t total, unsigned k, SleRanking& R) {
    if (k < 1 || k > 7) throw std::runtime_error("sle: kmer must be in 1..7");
    uint64_t pos = 0;
    auto cint = [&]() -> uint64_t {                          // io/BitIStream.hpp:174-188: groups of "more" + 7 bits, low group first
        uint64_t v = 0;
        for (unsigned i = 0; ; ++i) {
            if (pos + 8 > total) throw std::runtime_error("corrupt stream: the SLE ranking does not end inside the stream");
            const uint64_t g = sle_peek(p, avail, total, pos) >> 56;
            pos += 8;
            if (i == 10 || (i == 9 && (g & 0x7Eu))) throw std::runtime_error("corrupt stream: SLE ranking entry out of range");
            v |= (g & 0x7Fu) << (7 * i);
            if (!(g & 0x80u)) return v;
        }
    };
    const uint64_t sigma = cint();
    if (sigma > SLE_MAX_SIGMA) throw std::runtime_error("corrupt stream: SLE ranking of more than 1024 symbols");
    R.sigma = (uint32_t)sigma; R.total = total;
    R.sb = sigma ? coder_bits_for(sigma - 1) : 1;            // (no code is valid without a symbol)
    R.ent.assign((size_t)sigma, 0);
    for (uint64_t r = 0; r < sigma; ++r) {
        const uint64_t x = cint();
        if (x < 256) R.ent[r] = x | (1ull << 56);
        else if ((x >> 56) == 0xFF && ((x & 0x00FFFFFFFFFFFFFFull) >> (8 * k)) == 0) R.ent[r] = (x & 0x00FFFFFFFFFFFFFFull) | ((uint64_t)k << 56);
        else throw std::runtime_error("corrupt stream: SLE ranking entry is neither a byte nor a k-mer");
    }
    R.body = pos;
}
template <typename sink_t> inline void sle_decode_literals(const uint8_t* in, size_t n, unsigned k, sink_t& os) {
    if (!n) throw std::runtime_error("corrupt stream: no SLE ranking");
    SleRanking R;
    sle_parse_ranking(in, n, sle_total_bits(n, in[n - 1]), k, R);
    uint64_t len = 0;
    for (uint64_t pos = R.body; pos < R.total; ) {
        const uint64_t w = sle_peek(in, n, R.total, pos);
        const uint32_t l = sle_code_len(R.sb, (uint32_t)(w >> 61));
        if (pos + l > R.total) throw std::runtime_error("corrupt stream: cut-off SLE code");
        const uint32_t rank = sle_code_rank(R.sb, l, (uint32_t)(w >> (64 - l)));
        if (rank >= R.sigma) throw std::runtime_error("corrupt stream: SLE rank out of range");
        const uint64_t e = R.ent[rank];
        const unsigned m = (unsigned)(e >> 56);
        len += m;
        for (unsigned j = m; j-- > 0; ) os.put((uint8_t)(e >> (8 * j)));
        pos += l;
    }
    if (len > 0xFFFFFFFEull) throw std::length_error("sle: the stream decodes to more than 2^32 - 2 bytes");   // (a malformed code further on comes first)
}

// ---- LZWCompressor::decompress (compressors/LZWCompressor.hpp:110-133) with lzw::decode_step (lzw/LZWDecoding.hpp:12-99) restated ------
// The specification of the device decoder (csrc/lzw.hip), its path for small streams, and the text of the C ABI's tdc_lzw_decode.
// bit: BitCoder -- code k (0-based) in bits_for(k + 256) bits; else EliasGammaCoder.  dict_size = 0: the dictionary is never reset.
// Dictionary entry 256 + j = (code j, first byte of string j + 1); a string is rebuilt byte by byte along that chain (:31-47).
// Refused (std::runtime_error): code k above 255 + k (:72-76 "invalid compressed code"; code 0 = 256 would read an empty string), a code
// cut off by the end of the stream (the reference reads zeros there), a gamma field of more than 32 bits.  More than 2^32 - 2 bytes
// of text: std::length_error.
template <typename sink_t> inline void lzw_decode(const uint8_t* in, size_t n, bool bit, sink_t& os) {
    if (!n) return;
    const unsigned u = in[n - 1] & 7u;                           // io/BitIStream.hpp:27-63: the bits in front of the terminator
    if (u >= 6 && n < 2) throw std::runtime_error("corrupt stream: truncated stream");
    const uint64_t total = u >= 6 ? (uint64_t)(n - 2) * 8 + u : (uint64_t)(n - 1) * 8 + u;
    uint64_t pos = 0;
    auto peek = [&]() -> uint64_t {                              // the next 57 bits and more, left-aligned; zeros behind the end
        uint64_t w = 0;
        const size_t b = (size_t)(pos >> 3);
        for (size_t i = 0; i < 8; ++i) w = (w << 8) | (b + i < n ? in[b + i] : 0);
        w <<= (pos & 7);
        const uint64_t valid = total - pos;
        return valid >= 64 ? w : (valid ? w & (~0ull << (64 - valid)) : 0);
    };
    std::vector<uint32_t> parent;
    std::vector<uint8_t> last, tmp;
    auto rebuild = [&](uint64_t x) {                             // rebuild_string: tmp = the string of x behind its first byte, reversed
        tmp.clear();
        while (x >= 256) { tmp.push_back(last[x - 256]); x = parent[x - 256]; }
        return (uint8_t)x;
    };
    uint64_t k = 0, prev = 0, len = 0;
    while (pos < total) {
        uint64_t c;
        if (bit) {
            const unsigned w = coder_bits_for(k + 256);
            if (pos + w > total) throw std::runtime_error("corrupt stream: cut-off code");
            c = peek() >> (64 - w);
            pos += w;
        } else {
            const uint64_t v = peek();
            const unsigned b = v ? (unsigned)__builtin_clzll(v) : 64u;
            if (b > 32 || pos + 2 * b + 1 > total) throw std::runtime_error("corrupt stream: malformed or cut-off code");
            pos += b + 1;
            c = b ? peek() >> (64 - b) : 0;
            pos += b;
        }
        if (c > 255 + k) throw std::runtime_error("corrupt stream: invalid compressed code");
        uint8_t head;
        if (k && c == 255 + k) {                                 // :80-84 the entry is made first, from the previous string's first byte
            parent.push_back((uint32_t)prev); last.push_back(rebuild(prev));
            head = rebuild(c);
        } else {                                                 // :85-91
            head = rebuild(c);
            if (k) { parent.push_back((uint32_t)prev); last.push_back(head); }
        }
        len += tmp.size() + 1;
        if (len > 0xFFFFFFFEull) throw std::length_error("lzw: the stream decodes to more than 2^32 - 2 bytes");
        os.put(head);
        for (size_t i = tmp.size(); i-- > 0; ) os.put(tmp[i]);
        prev = c;
        ++k;
    }
}

// ---- RePairCompressor::decompress (compressors/RePairCompressor.hpp:287-336) --------------------------------------------------------------
// The stream: the number of rules under len_r; both sides of rule i, each a flag and the byte under literal_r or x - 256 under Range(i);
// then the start sequence under Range(rules) until the stream ends.  Symbols 0 .. 255 are bytes, 256 + k is rule k; a rule is l << 32 | r.
// Refused (std::runtime_error): a side of rule i that names a rule >= i (the reference would recurse for ever: Range(i) holds i itself
// under BitCoder when i is a power of two), a start symbol that names a rule >= rules, a field cut off by the end of the stream (the
// reference reads zeros there), more rules than the stream has room for (a rule takes at least four bits), and what the field readers
// refuse.
struct RepairGrammar { std::vector<uint64_t> rules; std::vector<uint32_t> start; };
template <typename decoder_t> inline void repair_parse(const uint8_t* in, size_t n, RepairGrammar& g) {
    auto bits = std::make_shared<BitIStream>(in, n);
    decoder_t decoder(bits);
    auto decode_sym = [&](size_t hi, uint64_t limit) -> uint32_t {      // :292-301
        if (decoder.template decode<bool>(bit_r)) {
            const uint64_t v = decoder.template decode<uint64_t>(Range(hi));
            if (bits->overrun()) throw std::runtime_error("corrupt stream: cut-off field");
            if (v >= limit) throw std::runtime_error("corrupt stream: rule index out of range");
            return (uint32_t)(256 + v);
        }
        const uliteral_t c = decoder.template decode<uliteral_t>(literal_r);
        if (bits->overrun()) throw std::runtime_error("corrupt stream: cut-off field");
        return c;
    };
    const uint64_t num_rules = decoder.template decode<uint64_t>(len_r);
    if (bits->overrun()) throw std::runtime_error("corrupt stream: cut-off field");
    if (num_rules > 2 * (uint64_t)n) throw std::runtime_error("corrupt stream: more rules than the stream can hold");
    g.rules.reserve((size_t)num_rules);
    for (uint64_t i = 0; i < num_rules; ++i) {
        const uint32_t l = decode_sym((size_t)i, i);
        const uint32_t r = decode_sym((size_t)i, i);
        g.rules.push_back((uint64_t)l << 32 | r);
    }
    while (!decoder.eof()) g.start.push_back(decode_sym((size_t)num_rules, num_rules));
}
// the length of the text a grammar stands for, summed in 64 bits with saturation (A_i = A_{i-1} A_{i-1} doubles per rule) -- known
// before any text is allocated
inline uint64_t repair_text_length(const RepairGrammar& g) {
    auto sat_add = [](uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; };
    std::vector<uint64_t> len(g.rules.size());
    auto of = [&](uint32_t x) -> uint64_t { return x < 256 ? 1 : len[x - 256]; };
    for (size_t i = 0; i < g.rules.size(); ++i) len[i] = sat_add(of((uint32_t)(g.rules[i] >> 32)), of((uint32_t)g.rules[i]));
    uint64_t total = 0;
    for (uint32_t x : g.start) total = sat_add(total, of(x));
    return total;
}
// :274-284 with an explicit stack instead of the recursion (a rule chain may be as deep as there are rules)
template <typename sink_t> inline void repair_expand(const RepairGrammar& g, sink_t& os) {
    std::vector<uint32_t> stack;
    for (uint32_t x : g.start) {
        stack.push_back(x);
        while (!stack.empty()) {
            const uint32_t y = stack.back(); stack.pop_back();
            if (y < 256) { os.put((uint8_t)y); continue; }
            const uint64_t di = g.rules[y - 256];
            stack.push_back((uint32_t)di);
            stack.push_back((uint32_t)(di >> 32));
        }
    }
}

}  // namespace tdc_amd
