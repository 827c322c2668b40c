// tdc_amd.hpp -- host-side C++ mirror of the slice of tudocomp's plugin surface that the lcpcomp hot path needs.
//
// Same names, argument meaning and error behaviour as the reference, so that its tests and driver read the same:
//   tdc::Compressor          include/tudocomp/Compressor.hpp:19-43        -> tdc_amd::Compressor
//   tdc::LCPCompressor       include/tudocomp/compressors/LCPCompressor.hpp:79-151 -> tdc_amd::LCPCompressor
//   Input / Output wrapping  include/tudocomp/io/{Input,Output}.hpp, restrictions "escape {0} + null-terminate"
//   Registry                 include/tudocomp/pre_header/Registry.hpp:11-25,204-231 (parse_algorithm_id / select_algorithm)
// compress() forwards to the C ABI (include/tdc_gpu.h) -- there is no CPU compress path.
// decompress() is host code, like in the reference (decode_text_internal + HuffmanCoder::Decoder, LCPCompressor.hpp:23-76,
// coders/HuffmanCoder.hpp:572-612, io/BitIStream.hpp); the decoded text is unique, so references are resolved by
// following source chains instead of the reference's ScanDec buffers.
#pragma once

#include <cstdint>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/tdc_gpu.h"
#include "tdc_coders.hpp"

namespace tdc_amd {

using bytes = std::vector<uint8_t>;

// ---- Input / Output ---------------------------------------------------------------------------------------
struct InputRestrictions {
    bool escape_zero = false;       // escape {0}        (ds/SADivSufSort.hpp:20-25)
    bool null_terminate = false;    // append sentinel
    bool has_restrictions() const { return escape_zero || null_terminate; }
};

class Input {
    bytes m_data;
    InputRestrictions m_restr;
public:
    Input() = default;
    explicit Input(bytes data) : m_data(std::move(data)) {}
    static Input from_memory(const void* p, size_t n) { return Input(bytes((const uint8_t*)p, (const uint8_t*)p + n)); }
    static Input from_file(const std::string& path) {
        std::ifstream f(path, std::ios::binary);
        if (!f) throw std::runtime_error("Could not open file for reading: " + path);
        return Input(bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>()));
    }
    Input(const Input& other, InputRestrictions r) : m_data(other.m_data), m_restr(r) {}
    Input(const Input& other, size_t from) : m_data(other.m_data.begin() + from, other.m_data.end()), m_restr(other.m_restr) {}
    size_t size() const { return m_data.size(); }
    const bytes& raw() const { return m_data; }
    // Input::as_view(): materialises the restricted view (io/RestrictedBuffer.hpp:108-254)
    bytes as_view() const {
        if (!m_restr.has_restrictions()) return m_data;
        bytes out(2 * m_data.size() + 1);
        out.resize(tdc_escape(m_data.data(), m_data.size(), out.data()));
        return out;
    }
};

class Output {
    bytes* m_vec = nullptr;
    InputRestrictions m_restr;
public:
    Output() = default;
    explicit Output(bytes& v) : m_vec(&v) {}
    Output(const Output& other, InputRestrictions r) : m_vec(other.m_vec), m_restr(r) {}
    // bytes that are already unrestricted (the blocks of a container remove their own restrictions)
    void write_plain(const uint8_t* p, size_t n) { m_vec->insert(m_vec->end(), p, p + n); }
    void write(const uint8_t* p, size_t n) {
        if (m_restr.has_restrictions()) {                       // un-escaping ostream filter (io/RestrictedIOStream.hpp:13-89)
            bytes tmp(n + 1);
            tmp.resize(tdc_unescape(p, n, tmp.data()));
            m_vec->insert(m_vec->end(), tmp.begin(), tmp.end());
        } else m_vec->insert(m_vec->end(), p, p + n);
    }
};

// ---- options ------------------------------------------------------------------------------------------------
struct AlgorithmValue {
    std::string name;
    std::map<std::string, std::string> args;      // key -> value text ("huff", "2", "scan(scans=6)")
    std::string get(const std::string& k, const std::string& dflt) const {
        auto it = args.find(k);
        return it == args.end() ? dflt : it->second;
    }
    long get_int(const std::string& k, long dflt) const {
        auto it = args.find(k);
        return it == args.end() ? dflt : std::stol(it->second);
    }
};

// name(arg, key=value, key=algo(...))  -- the subset of AlgorithmStringParser.hpp:94-300 this path needs
inline AlgorithmValue parse_algorithm_id(const std::string& s, const std::vector<std::string>& positional = {}) {
    AlgorithmValue av;
    size_t i = 0;
    auto skip = [&] { while (i < s.size() && isspace((unsigned char)s[i])) ++i; };
    skip();
    size_t b = i;
    while (i < s.size() && (isalnum((unsigned char)s[i]) || s[i] == '_')) ++i;
    av.name = s.substr(b, i - b);
    if (av.name.empty()) throw std::runtime_error("Expected an algorithm name in '" + s + "'");
    skip();
    if (i == s.size()) return av;
    if (s[i] != '(') throw std::runtime_error("Unexpected character in algorithm string '" + s + "'");
    ++i;
    size_t pos_idx = 0;
    while (true) {
        skip();
        if (i < s.size() && s[i] == ')') { ++i; break; }
        size_t st = i; int depth = 0;
        while (i < s.size() && (depth > 0 || (s[i] != ',' && s[i] != ')'))) {
            if (s[i] == '(') ++depth;
            if (s[i] == ')') --depth;
            ++i;
        }
        if (i >= s.size()) throw std::runtime_error("Unbalanced parentheses in algorithm string '" + s + "'");
        std::string item = s.substr(st, i - st);
        while (!item.empty() && isspace((unsigned char)item.back())) item.pop_back();
        size_t eq = std::string::npos; depth = 0;
        for (size_t j = 0; j < item.size(); ++j) {
            if (item[j] == '(') ++depth; else if (item[j] == ')') --depth;
            else if (item[j] == '=' && depth == 0) { eq = j; break; }
        }
        if (eq == std::string::npos) {
            if (pos_idx >= positional.size()) throw std::runtime_error("Too many positional arguments in '" + s + "'");
            av.args[positional[pos_idx++]] = item;
        } else {
            std::string k = item.substr(0, eq), v = item.substr(eq + 1);
            while (!k.empty() && isspace((unsigned char)k.back())) k.pop_back();
            while (!v.empty() && isspace((unsigned char)v.front())) v.erase(v.begin());
            av.args[k] = v;
        }
        if (s[i] == ',') ++i;
    }
    return av;
}

inline unsigned bits_for(uint64_t v) { return coder_bits_for(v); }

// ---- Compressor ---------------------------------------------------------------------------------------------
class Compressor {
public:
    virtual ~Compressor() = default;
    virtual void compress(Input& input, Output& output) = 0;      // Compressor.hpp:36
    virtual void decompress(Input& input, Output& output) = 0;    // Compressor.hpp:42
    virtual InputRestrictions input_restrictions() const { return {}; }
};

struct GpuContext {
    tdc_gpu_ctx* h = nullptr;
    explicit GpuContext(int device = 0) {
        int rc = tdc_gpu_ctx_create(device, &h);
        if (rc) throw std::runtime_error(std::string("tdc_gpu_ctx_create: ") + tdc_gpu_strerror(rc));
    }
    ~GpuContext() { tdc_gpu_ctx_destroy(h); }
    GpuContext(const GpuContext&) = delete;
    GpuContext& operator=(const GpuContext&) = delete;
};

// coder_t::Decoder + lzss token stream (decode_text_internal / lzss::decode_text), shared by lcpcomp and lzss_lcp: the
// Decoder classes of tdc_coders.hpp (HuffmanCoder::Decoder, coders/HuffmanCoder.hpp:572-612; ASCIICoder::Decoder,
// coders/ASCIICoder.hpp:53-84).  References may point forwards (lcpcomp) or backwards (lzss_lcp).
template <typename coder_t>
inline void lzss_decode(Input& input, Output& output) {
    const bytes& in = input.raw();
    typename coder_t::Decoder decoder(std::make_shared<BitIStream>(in.data(), in.size()));
    bytes text;
    decode_text(decoder, text);
    output.write(text.data(), text.size());
}
inline void lzss_huff_decode(Input& input, Output& output) { lzss_decode<HuffmanCoder>(input, output); }
inline void lzss_ascii_decode(Input& input, Output& output) { lzss_decode<ASCIICoder>(input, output); }

// ---- block container (written by tdc_gpu_blocks_compress / tudocomp_amd.blocks): "tdcgpu-blocks%" | u32 G |
//      G x { u64 raw_len, u64 comp_len } | payloads, little endian.  Every payload is a complete stream of its block.
struct BlockContainer {
    struct Block { uint64_t raw_len; const uint8_t* data; size_t len; };
    static constexpr const char* MAGIC = "tdcgpu-blocks%";
    static bool is_container(const uint8_t* p, size_t n) { return n >= 14 && std::memcmp(p, MAGIC, 14) == 0; }
    static std::vector<Block> parse(const uint8_t* p, size_t n) {
        if (!is_container(p, n) || n < 18) throw std::runtime_error("not a tdcgpu-blocks container");
        auto u32at = [&](size_t o) { uint32_t v = 0; for (int i = 0; i < 4; ++i) v |= (uint32_t)p[o + i] << (8 * i); return v; };
        auto u64at = [&](size_t o) { uint64_t v = 0; for (int i = 0; i < 8; ++i) v |= (uint64_t)p[o + i] << (8 * i); return v; };
        const size_t G = u32at(14);
        if (n < 18 + 16 * G) throw std::runtime_error("corrupt container: directory");
        std::vector<Block> out;
        size_t at = 18 + 16 * G;
        for (size_t k = 0; k < G; ++k) {
            const uint64_t raw = u64at(18 + 16 * k), comp = u64at(18 + 16 * k + 8);
            if (comp > n - at) throw std::runtime_error("corrupt container: payload exceeds the file");
            out.push_back(Block{raw, p + at, (size_t)comp});
            at += comp;
        }
        if (at != n) throw std::runtime_error("corrupt container: trailing bytes");
        return out;
    }
};

// SLECoder::Decoder (coders/SLECoder.hpp:301-453) + the same token stream: ranking header, rank class codes, k-mer
// symbols expand to k literals; the factor length is a MinDistributedRange (:413-431).
inline void lzss_sle_decode(Input& input, Output& output, unsigned k) {
    const bytes& in = input.raw();
    BitIStream bs(in.data(), in.size());
    const size_t sigma = (size_t)bs.read_compressed_int();                   // Decoder ctor :325-340
    if (sigma == 0 || sigma > 4096) throw std::runtime_error("corrupt SLE ranking");
    const unsigned sb = bits_for(sigma - 1);
    std::vector<uint64_t> inv(sigma);
    for (size_t r = 0; r < sigma; ++r) inv[r] = bs.read_compressed_int();
    auto read_rank = [&]() -> uint64_t {                                      // :367-397
        if (sb < 4) return bs.read_int(sb);
        if (sb < 6) return bs.read_bit() ? bs.read_int(sb) : bs.read_int(2);
        if (sb == 6) {
            switch (bs.read_int(2)) {
                case 0: return bs.read_int(3);
                case 1: return 8 + bs.read_int(3);
                case 2: return 16 + bs.read_int(4);
                default: return bs.read_int(sb);
            }
        }
        const uint64_t cls = bs.read_int(3);
        if (cls < 4) return 4 * cls + bs.read_int(2);
        if (cls < 7) return 16 + 8 * (cls - 4) + bs.read_int(3);
        return bs.read_int(sb);
    };
    uint8_t kmer[8]; size_t kread = (size_t)-1;
    const uint64_t n = bs.read_int(32);
    const unsigned W = bits_for(n);
    const uint64_t flen_min = bs.read_int(W), flen_max = bs.read_int(W), fdist_max = bs.read_int(W);
    const unsigned lbits = bits_for(flen_max - flen_min), dbits = bits_for(fdist_max);
    bytes text(n);
    std::vector<uint32_t> ref(n, 0xFFFFFFFFu);
    uint64_t p = 0;
    auto eof = [&] { return kread < k ? false : bs.eof(); };                  // :351-359
    while (!eof()) {
        kread = (size_t)-1;                                                   // decode(BitRange) resets the k-mer :433-437
        uint64_t num = bs.read_bit() ? bs.read_int(dbits) : 0;
        while (num--) {
            uint8_t ch;
            if (kread < k) ch = kmer[kread++];
            else {
                const uint64_t r = read_rank();
                if (r >= sigma) throw std::runtime_error("corrupt stream: rank out of range");
                const uint64_t x = inv[r];
                if ((x >> 56) == 0xFF) { for (unsigned i = 0; i < k; ++i) kmer[k - 1 - i] = (uint8_t)(x >> (8 * i)); kread = 1; ch = kmer[0]; }
                else ch = (uint8_t)x;
            }
            if (p >= n) throw std::runtime_error("corrupt stream: too many literals");
            text[p++] = ch;
        }
        if (!eof()) {
            kread = (size_t)-1;
            const uint64_t src = bs.read_int(W);
            uint64_t v;
            if (lbits <= 5) v = bs.read_int(lbits);
            else switch (bs.read_int(2)) {
                case 0: v = bs.read_int(3); break;
                case 1: v = 8 + bs.read_int(3); break;
                case 2: v = 16 + bs.read_int(4); break;
                default: v = bs.read_int(lbits); break;
            }
            const uint64_t len = flen_min + v;
            if (len == 0 || p + len > n || src + len > n) throw std::runtime_error("corrupt stream: factor out of range");
            for (uint64_t j = 0; j < len; ++j) ref[p + j] = (uint32_t)(src + j);
            p += len;
        }
    }
    if (p != n) throw std::runtime_error("corrupt stream: length mismatch");
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t q = (uint32_t)i; uint64_t guard = 0;
        while (ref[q] != 0xFFFFFFFFu) { q = ref[q]; if (++guard > n) throw std::runtime_error("corrupt stream: reference cycle"); }
        text[i] = text[q];
    }
    output.write(text.data(), text.size());
}

class LCPCompressor : public Compressor {
    AlgorithmValue m_opts;
    std::shared_ptr<GpuContext> m_ctx;       // created lazily by the first compress(): decompress() needs no GPU
    int m_device = 0;
    int m_coder = TDC_GPU_CODER_HUFF;
    int m_comp = TDC_GPU_COMP_ARRAYS;
    unsigned m_kmer = 3;
public:
    tdc_gpu_stats last_stats{};
    void set_device(int d) { m_device = d; }
    long threshold() const { return m_opts.get_int("threshold", 5); }
    // meta: type "compressor", name "lcpcomp", options coder, comp=arrays, dec=scan, threshold=5, flatten=1 (LCPCompressor.hpp:85-95)
    LCPCompressor(AlgorithmValue opts, std::shared_ptr<GpuContext> ctx) : m_opts(std::move(opts)), m_ctx(std::move(ctx)) {
        const std::string coder = m_opts.get("coder", ""), comp = m_opts.get("comp", "arrays");
        // `arithmetic` is not in the reference's lcpcomp registry (etc/registry_config.py:138-142) but the template
        // instantiates; BASELINE.json configs[2] asks for it, compress side only
        m_comp = (comp == "plcppeaks" || comp == "plcppeaks()") ? TDC_GPU_COMP_PLCPPEAKS
               : (comp == "max_lcp" || comp == "max_lcp()") ? TDC_GPU_COMP_MAXLCP
               : (comp == "heap" || comp == "heap()") ? TDC_GPU_COMP_HEAP : TDC_GPU_COMP_ARRAYS;
        const AlgorithmValue cv = coder.empty() ? AlgorithmValue() : parse_algorithm_id(coder, {"kmer"});
        const std::string& cname = cv.name;
        if ((cname != "huff" && cname != "arithmetic" && cname != "ascii" && cname != "sle") ||
            (comp != "arrays" && comp != "arrays()" && comp != "plcppeaks" && comp != "plcppeaks()" && comp != "max_lcp" && comp != "max_lcp()" &&
             comp != "heap" && comp != "heap()"))
            throw std::runtime_error("No implementation found for compressor lcpcomp(coder=" + coder + ",comp=" + comp + ")");   // Registry.hpp:214
        m_coder = (cname == "huff") ? TDC_GPU_CODER_HUFF : (cname == "ascii" ? TDC_GPU_CODER_ASCII : TDC_GPU_CODER_ARITH);
        if (cname == "sle") {                                                 // option kmer = 3 (SLECoder.hpp:38)
            m_kmer = (unsigned)cv.get_int("kmer", 3);
            if (m_kmer < 1 || m_kmer > 7) throw std::runtime_error("sle: kmer must be in 1..7");
            m_coder = TDC_GPU_CODER_SLE_K((int)m_kmer);
        }
    }
    InputRestrictions input_restrictions() const override { return {true, true}; }   // uses_textds (Meta.hpp:277-282)

    void compress(Input& input, Output& output) override {
        if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
        const bytes view = input.as_view();
        uint8_t* out = nullptr; size_t out_len = 0;
        const int rc = tdc_gpu_lcpcomp_compress_comp(m_ctx->h, view.data(), view.size(), (uint32_t)m_opts.get_int("threshold", 5),
                                                     (int)m_opts.get_int("flatten", 1), m_coder, m_comp, &out, &out_len, &last_stats);
        if (rc == TDC_GPU_ERR_NO_SENTINEL) throw std::logic_error(tdc_gpu_strerror(rc));          // ds/TextDS.hpp:132-138
        if (rc) throw std::runtime_error(std::string(tdc_gpu_strerror(rc)) + ": " + tdc_gpu_last_error(m_ctx->h));
        output.write(out, out_len);
        tdc_gpu_free(out);
    }

    // block mode (tdc --blocks SIZE): the UNRESTRICTED input is cut into blocks of block_size bytes, every block is compressed
    // on one of the visible devices as a stream of its own (tdc_gpu_blocks_compress) and framed in the block container
    void compress_blocks(const bytes& raw, size_t block_size, Output& output, int ndev = 0) {
        int have = tdc_gpu_device_count();
        if (have <= 0) throw std::runtime_error(std::string("tdc_gpu_blocks_compress: ") + tdc_gpu_strerror(TDC_GPU_ERR_HIP));
        if (ndev > 0 && ndev < have) have = ndev;
        std::vector<int> devs((size_t)have);
        for (int i = 0; i < have; ++i) devs[(size_t)i] = i;
        uint8_t* out = nullptr; size_t out_len = 0;
        const int rc = tdc_gpu_blocks_compress(devs.data(), have, raw.data(), raw.size(), block_size, (uint32_t)m_opts.get_int("threshold", 5),
                                               (int)m_opts.get_int("flatten", 1), m_coder, &out, &out_len, nullptr);
        if (rc) throw std::runtime_error(std::string("tdc_gpu_blocks_compress: ") + tdc_gpu_strerror(rc));
        output.write(out, out_len);
        tdc_gpu_free(out);
    }

    void decompress(Input& input, Output& output) override {
        if (BlockContainer::is_container(input.raw().data(), input.raw().size())) {      // every payload is a stream of its own
            const bytes& in = input.raw();
            for (const BlockContainer::Block& b : BlockContainer::parse(in.data(), in.size())) {
                Input part = Input::from_memory(b.data, b.len);
                bytes plain;
                Output po(plain);
                Output restricted(po, input_restrictions());                              // the block's own escaping + sentinel
                decompress(part, restricted);
                if (plain.size() != b.raw_len) throw std::runtime_error("corrupt container: block length mismatch");
                output.write_plain(plain.data(), plain.size());
            }
            return;
        }
        if (m_coder == TDC_GPU_CODER_ARITH)
            throw std::runtime_error("lcpcomp(coder=arithmetic) streams cannot be decoded (neither can the reference: "
                                     "consuming coders corrupt interleaved streams, docs/Documentation.md:1190-1203)");
        const bool on_device = m_opts.get("dec", "scan") == "gpu";
        if (!on_device && m_coder == TDC_GPU_CODER_ASCII) { lzss_ascii_decode(input, output); return; }
        if (!on_device && (m_coder & 0xFF) == TDC_GPU_CODER_SLE) { lzss_sle_decode(input, output, m_kmer); return; }
        // dec=gpu (an addition to the reference's decoder strategies scan / compact / ..., LCPCompressor.hpp:88): huff and
        // sle streams of 1 MiB and more are parsed on the device, the others on the host; the references are resolved on the device
        // (tdc_gpu_lcpcomp_decompress_coder)
        if (m_opts.get("dec", "scan") == "gpu") {
            if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
            const bytes& in = input.raw();
            uint8_t* out = nullptr; size_t out_len = 0;
            const int rc = tdc_gpu_lcpcomp_decompress_coder(m_ctx->h, in.data(), in.size(), m_coder, &out, &out_len, nullptr, nullptr);
            if (rc) throw std::runtime_error(std::string(tdc_gpu_strerror(rc)) + ": " + tdc_gpu_last_error(m_ctx->h));
            output.write(out, out_len);
            tdc_gpu_free(out);
            return;
        }
        lzss_huff_decode(input, output);
    }
};

// tdc::LZSSLCPCompressor<coder>  (compressors/LZSSLCPCompressor.hpp:22-132) with the coders the reference registers it with
// (etc/registry_config.py:33-34: ascii, bit, gamma, delta, huff); threshold defaults to 3.
class LZSSLCPCompressor : public Compressor {
    AlgorithmValue m_opts;
    std::shared_ptr<GpuContext> m_ctx;
    int m_device = 0;
    int m_coder = TDC_GPU_CODER_HUFF;
public:
    tdc_gpu_stats last_stats{};
    void set_device(int d) { m_device = d; }
    LZSSLCPCompressor(AlgorithmValue opts, std::shared_ptr<GpuContext> ctx) : m_opts(std::move(opts)), m_ctx(std::move(ctx)) {
        const std::string coder = m_opts.get("coder", "");
        if (coder == "huff") m_coder = TDC_GPU_CODER_HUFF;
        else if (coder == "bit") m_coder = TDC_GPU_CODER_BIT;
        else if (coder == "gamma") m_coder = TDC_GPU_CODER_GAMMA;
        else if (coder == "delta") m_coder = TDC_GPU_CODER_DELTA;
        else if (coder == "ascii") m_coder = TDC_GPU_CODER_ASCII;
        else throw std::runtime_error("No implementation found for compressor lzss_lcp(coder=" + coder + ")");   // Registry.hpp:214
    }
    InputRestrictions input_restrictions() const override { return {true, true}; }
    void compress(Input& input, Output& output) override {
        if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
        const bytes view = input.as_view();
        uint8_t* out = nullptr; size_t out_len = 0;
        const int rc = tdc_gpu_lzss_lcp_compress(m_ctx->h, view.data(), view.size(), (uint32_t)m_opts.get_int("threshold", 3),
                                                 m_coder, &out, &out_len, &last_stats);
        if (rc == TDC_GPU_ERR_NO_SENTINEL) throw std::logic_error(tdc_gpu_strerror(rc));
        if (rc) throw std::runtime_error(std::string(tdc_gpu_strerror(rc)) + ": " + tdc_gpu_last_error(m_ctx->h));
        output.write(out, out_len);
        tdc_gpu_free(out);
    }
    // :125-130 (DecodeBackBuffer): the host loop decode_text with the coder's Decoder, which needs no device; dec=gpu (an addition, as
    // for lz78 / lzw): tdc_gpu_lzss_lcp_decompress.  The stream is the same either way.
    void decompress(Input& input, Output& output) override {
        const bytes& in = input.raw();
        if (m_opts.get("dec", "host") == "gpu") {
            if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
            uint8_t* out = nullptr; size_t out_len = 0;
            const int rc = tdc_gpu_lzss_lcp_decompress(m_ctx->h, in.data(), in.size(), m_coder, &out, &out_len, nullptr, nullptr);
            if (rc) throw std::runtime_error(std::string(tdc_gpu_strerror(rc)) + ": " + tdc_gpu_last_error(m_ctx->h));
            output.write(out, out_len);
            tdc_gpu_free(out);
            return;
        }
        bytes text;
        lzss_decode_coder(in.data(), in.size(), m_coder, text);
        output.write(text.data(), text.size());
    }
};

// lzw / lz78 over a batch (tdc_gpu_lzw_compress_batch, tdc_gpu_lz78_compress_batch): every text on its own, all of them parsed and coded
// in one device call.  streams[k] is what compress() writes for texts[k]; where status[k] is not TDC_GPU_OK (the single call's refusal of
// that text) the stream is empty.
template <class Call, class Bound>
inline void lz_compress_batch(tdc_gpu_ctx* h, Call call, Bound bound, int coder, const std::vector<bytes>& texts, std::vector<bytes>& streams,
                              std::vector<int32_t>& status, tdc_gpu_stats* stats) {
    const size_t count = texts.size();
    std::vector<uint64_t> in_off(count + 1, 0), out_off(count + 1, 0), out_len(count ? count : 1, 0);
    for (size_t k = 0; k < count; ++k) in_off[k + 1] = in_off[k] + texts[k].size();
    bytes in((size_t)in_off[count] ? (size_t)in_off[count] : 1);
    for (size_t k = 0; k < count; ++k) std::copy(texts[k].begin(), texts[k].end(), in.begin() + (size_t)in_off[k]);
    bytes out(bound(in_off.data(), count, coder) + 8);
    status.assign(count ? count : 1, 0);
    const int rc = call(h, in.data(), in_off.data(), count, coder, out.data(), out.size(), out_off.data(), out_len.data(), status.data(), stats);
    if (rc) throw std::runtime_error(std::string(tdc_gpu_strerror(rc)) + ": " + tdc_gpu_last_error(h));
    status.resize(count);
    streams.clear();
    for (size_t k = 0; k < count; ++k) streams.emplace_back(out.begin() + (size_t)out_off[k], out.begin() + (size_t)(out_off[k] + out_len[k]));
}

// The decoders of such batches (tdc_gpu_lzw_decompress_batch, tdc_gpu_lz78_decompress_batch): all streams in one pass on the device, the
// sizes first, then the call.  status[k] is the single decoder's verdict on streams[k] alone, a refused stream yields an empty text.
template <class Call>
inline void lz_decompress_batch(tdc_gpu_ctx* h, Call call, int coder, const std::vector<bytes>& streams, std::vector<bytes>& texts,
                                std::vector<int32_t>& status, tdc_gpu_stats* stats) {
    const size_t count = streams.size();
    texts.assign(count, bytes());
    std::vector<uint64_t> s_off(count ? count : 1, 0), s_len(count ? count : 1, 0), out_off(count + 1, 0);
    size_t pos = 0;
    for (size_t k = 0; k < count; ++k) { s_off[k] = pos; s_len[k] = streams[k].size(); pos += (streams[k].size() + 7) / 8 * 8; }
    bytes blob(pos ? pos : 1);
    for (size_t k = 0; k < count; ++k) std::copy(streams[k].begin(), streams[k].end(), blob.begin() + (size_t)s_off[k]);
    status.assign(count ? count : 1, 0);
    int rc = call(h, blob.data(), s_off.data(), s_len.data(), count, coder, nullptr, 0, out_off.data(), status.data(), nullptr);      // the sizes
    bytes out((size_t)out_off[count] ? (size_t)out_off[count] : 1);
    if (rc == TDC_GPU_ERR_OOM || rc == TDC_GPU_OK)
        rc = call(h, blob.data(), s_off.data(), s_len.data(), count, coder, out.data(), out.size(), out_off.data(), status.data(), stats);
    if (rc) throw std::runtime_error(std::string(tdc_gpu_strerror(rc)) + ": " + tdc_gpu_last_error(h));
    status.resize(count);
    for (size_t k = 0; k < count; ++k) texts[k].assign(out.begin() + (size_t)out_off[k], out.begin() + (size_t)out_off[k + 1]);
}

// tdc::LZ78Compressor<EliasGammaCoder, trie>  (compressors/LZ78Compressor.hpp:45-161): no input restrictions.
class LZ78Compressor : public Compressor {
    AlgorithmValue m_opts;
    std::shared_ptr<GpuContext> m_ctx;
    int m_device = 0;
public:
    tdc_gpu_stats last_stats{};
    void set_device(int d) { m_device = d; }
    LZ78Compressor(AlgorithmValue opts, std::shared_ptr<GpuContext> ctx) : m_opts(std::move(opts)), m_ctx(std::move(ctx)) {
        const std::string coder = m_opts.get("coder", "bit");                 // the reference's default coder is BitCoder
        if (coder != "gamma")
            throw std::runtime_error("No implementation found for compressor lz78(coder=" + coder + ")");   // Registry.hpp:214
    }
    void compress(Input& input, Output& output) override {
        if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
        const bytes& in = input.raw();
        uint8_t* out = nullptr; size_t out_len = 0;
        const int rc = tdc_gpu_lz78_compress(m_ctx->h, in.data(), in.size(), TDC_GPU_CODER_GAMMA, &out, &out_len, &last_stats);
        if (rc) throw std::runtime_error(std::string(tdc_gpu_strerror(rc)) + ": " + tdc_gpu_last_error(m_ctx->h));
        output.write(out, out_len);
        tdc_gpu_free(out);
    }
    void compress_batch(const std::vector<bytes>& texts, std::vector<bytes>& streams, std::vector<int32_t>& status) {
        if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
        lz_compress_batch(m_ctx->h, tdc_gpu_lz78_compress_batch, tdc_gpu_lz78_batch_bound, TDC_GPU_CODER_GAMMA, texts, streams, status, &last_stats);
    }
    void decompress_batch(const std::vector<bytes>& streams, std::vector<bytes>& texts, std::vector<int32_t>& status) {
        if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
        lz_decompress_batch(m_ctx->h, tdc_gpu_lz78_decompress_batch, TDC_GPU_CODER_GAMMA, streams, texts, status, &last_stats);
    }
    // LZ78Compressor::decompress (:142-160) with EliasGammaCoder::Decoder: pairs until BitIStream eof.
    // dec=gpu (an addition, as for lcpcomp): the stream is parsed and the phrases are expanded on the device (tdc_gpu_lz78_decompress);
    // the stream itself is the same either way.
    void decompress(Input& input, Output& output) override {
        const bytes& in = input.raw();
        if (m_opts.get("dec", "host") == "gpu") {
            if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
            uint8_t* out = nullptr; size_t out_len = 0;
            const int rc = tdc_gpu_lz78_decompress(m_ctx->h, in.data(), in.size(), TDC_GPU_CODER_GAMMA, &out, &out_len, nullptr, nullptr);
            if (rc) throw std::runtime_error(std::string(tdc_gpu_strerror(rc)) + ": " + tdc_gpu_last_error(m_ctx->h));
            output.write(out, out_len);
            tdc_gpu_free(out);
            return;
        }
        EliasGammaCoder::Decoder decoder(std::make_shared<BitIStream>(in.data(), in.size()));
        std::vector<uint32_t> parent(1, 0);
        std::vector<uint8_t> chr(1, 0);
        bytes text, tmp;
        const Range factor_r(0, std::numeric_limits<uint32_t>::max());       // the ranges are ignored by this coder (:26-29)
        while (!decoder.eof()) {
            const uint64_t id = decoder.decode<uint64_t>(factor_r);
            const uint64_t c = decoder.decode<uint64_t>(factor_r);
            if (id >= parent.size()) throw std::runtime_error("corrupt stream: unknown phrase id");
            tmp.clear();
            for (uint64_t x = id; x != 0; x = parent[x]) tmp.push_back(chr[x]);
            text.insert(text.end(), tmp.rbegin(), tmp.rend());
            text.push_back((uint8_t)c);
            parent.push_back((uint32_t)id);
            chr.push_back((uint8_t)c);
        }
        output.write(text.data(), text.size());
    }
};

// tdc::LZWCompressor<BitCoder | EliasGammaCoder, trie>  (compressors/LZWCompressor.hpp:19-135): no input restrictions.  coder defaults to
// bit, as in the reference; lz78trie is accepted and ignored (every back-end yields the same ids); dict_size must be 0 (no resets).
class LZWCompressor : public Compressor {
    AlgorithmValue m_opts;
    std::shared_ptr<GpuContext> m_ctx;
    int m_device = 0;
    int m_coder = TDC_GPU_CODER_BIT;
public:
    tdc_gpu_stats last_stats{};
    void set_device(int d) { m_device = d; }
    LZWCompressor(AlgorithmValue opts, std::shared_ptr<GpuContext> ctx) : m_opts(std::move(opts)), m_ctx(std::move(ctx)) {
        const std::string coder = m_opts.get("coder", "bit");
        if (coder == "gamma") m_coder = TDC_GPU_CODER_GAMMA;
        else if (coder != "bit") throw std::runtime_error("No implementation found for compressor lzw(coder=" + coder + ")");   // Registry.hpp:214
        if (m_opts.get("dict_size", "0") != "0")
            throw std::runtime_error("lzw: dict_size=" + m_opts.get("dict_size", "0") + " is not available (only dict_size=0, the unlimited dictionary)");
    }
    void compress(Input& input, Output& output) override {
        if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
        const bytes& in = input.raw();
        uint8_t* out = nullptr; size_t out_len = 0;
        const int rc = tdc_gpu_lzw_compress(m_ctx->h, in.data(), in.size(), m_coder, &out, &out_len, &last_stats);
        if (rc) throw std::runtime_error(std::string(tdc_gpu_strerror(rc)) + ": " + tdc_gpu_last_error(m_ctx->h));
        output.write(out, out_len);
        tdc_gpu_free(out);
    }
    void compress_batch(const std::vector<bytes>& texts, std::vector<bytes>& streams, std::vector<int32_t>& status) {
        if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
        lz_compress_batch(m_ctx->h, tdc_gpu_lzw_compress_batch, tdc_gpu_lzw_batch_bound, m_coder, texts, streams, status, &last_stats);
    }
    void decompress_batch(const std::vector<bytes>& streams, std::vector<bytes>& texts, std::vector<int32_t>& status) {
        if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
        lz_decompress_batch(m_ctx->h, tdc_gpu_lzw_decompress_batch, m_coder, streams, texts, status, &last_stats);
    }
    // LZWCompressor::decompress (:110-133): the host loop of tdc_coders.hpp (lzw::decode_step restated), which needs no device;
    // dec=gpu (an addition, as for lz78): the device decoder (tdc_gpu_lzw_decompress).  The stream is the same either way.
    void decompress(Input& input, Output& output) override {
        const bytes& in = input.raw();
        if (m_opts.get("dec", "host") == "gpu") {
            if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
            uint8_t* out = nullptr; size_t out_len = 0;
            const int rc = tdc_gpu_lzw_decompress(m_ctx->h, in.data(), in.size(), m_coder, &out, &out_len, nullptr, nullptr);
            if (rc) throw std::runtime_error(std::string(tdc_gpu_strerror(rc)) + ": " + tdc_gpu_last_error(m_ctx->h));
            output.write(out, out_len);
            tdc_gpu_free(out);
            return;
        }
        struct { bytes v; void put(uint8_t c) { v.push_back(c); } } text;
        lzw_decode(in.data(), in.size(), m_coder == TDC_GPU_CODER_BIT, text);
        output.write(text.v.data(), text.v.size());
    }
};

// tdc::LZSSSlidingWindowCompressor<ASCIICoder | BitCoder | EliasGammaCoder | EliasDeltaCoder>  (compressors/
// LZSSSlidingWindowCompressor.hpp:15-144), the algorithm `lzss`: no input restrictions.  The reference's meta gives coder no default, so
// `lzss` without one is refused; window (16) must be in 1 .. 4096, threshold defaults to 3.  The parse runs on the device.
class LZSSSlidingWindowCompressor : public Compressor {
    AlgorithmValue m_opts;
    std::shared_ptr<GpuContext> m_ctx;
    int m_device = 0;
    int m_coder = TDC_GPU_CODER_BIT;
    long m_window = 16;
public:
    tdc_gpu_stats last_stats{};
    void set_device(int d) { m_device = d; }
    LZSSSlidingWindowCompressor(AlgorithmValue opts, std::shared_ptr<GpuContext> ctx) : m_opts(std::move(opts)), m_ctx(std::move(ctx)) {
        const std::string coder = m_opts.get("coder", "");
        if (coder == "bit") m_coder = TDC_GPU_CODER_BIT;
        else if (coder == "ascii") m_coder = TDC_GPU_CODER_ASCII;
        else if (coder == "gamma") m_coder = TDC_GPU_CODER_GAMMA;
        else if (coder == "delta") m_coder = TDC_GPU_CODER_DELTA;
        else throw std::runtime_error("No implementation found for compressor lzss(coder=" + coder + ")");   // Registry.hpp:214
        m_window = m_opts.get_int("window", 16);
        if (m_window < 1 || m_window > 4096) throw std::runtime_error("lzss: window=" + m_opts.get("window", "16") + " is not available (1 .. 4096)");
        if (m_opts.get_int("threshold", 3) < 0) throw std::runtime_error("lzss: threshold must not be negative");
    }
    void compress(Input& input, Output& output) override {
        if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
        const bytes& in = input.raw();
        uint8_t* out = nullptr; size_t out_len = 0;
        const int rc = tdc_gpu_lzss_sw_compress(m_ctx->h, in.data(), in.size(), (uint32_t)m_window, (uint32_t)m_opts.get_int("threshold", 3),
                                                m_coder, &out, &out_len, &last_stats);
        if (rc) throw std::runtime_error(std::string(tdc_gpu_strerror(rc)) + ": " + tdc_gpu_last_error(m_ctx->h));
        output.write(out, out_len);
        tdc_gpu_free(out);
    }
    // Every text on its own, all of them in one device call (tdc_gpu_lzss_sw_compress_batch): streams[k] is what compress() writes for
    // texts[k]; status[k] is TDC_GPU_ERR_UNSUPPORTED, and the stream empty, where coder=bit would truncate a length of text k.
    void compress_batch(const std::vector<bytes>& texts, std::vector<bytes>& streams, std::vector<int32_t>& status) {
        if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
        const size_t count = texts.size();
        std::vector<uint64_t> in_off(count + 1, 0), out_off(count + 1, 0), out_len(count ? count : 1, 0);
        for (size_t k = 0; k < count; ++k) in_off[k + 1] = in_off[k] + texts[k].size();
        bytes in((size_t)in_off[count] ? (size_t)in_off[count] : 1);
        for (size_t k = 0; k < count; ++k) std::copy(texts[k].begin(), texts[k].end(), in.begin() + (size_t)in_off[k]);
        const uint32_t w = (uint32_t)m_window, t = (uint32_t)m_opts.get_int("threshold", 3);
        bytes out(tdc_gpu_lzss_sw_batch_bound(in_off.data(), count, w, m_coder) + 8);
        status.assign(count ? count : 1, 0);
        const int rc = tdc_gpu_lzss_sw_compress_batch(m_ctx->h, in.data(), in_off.data(), count, w, t, m_coder, out.data(), out.size(), out_off.data(),
                                                      out_len.data(), status.data(), &last_stats);
        if (rc) throw std::runtime_error(std::string(tdc_gpu_strerror(rc)) + ": " + tdc_gpu_last_error(m_ctx->h));
        status.resize(count);
        streams.clear();
        for (size_t k = 0; k < count; ++k) streams.emplace_back(out.begin() + (size_t)out_off[k], out.begin() + (size_t)(out_off[k] + out_len[k]));
    }
    // The decoder of such a batch, on the device, one wave per stream (tdc_gpu_lzss_sw_decompress_batch; bit, gamma, delta -- coder=ascii
    // loops the host decoder): status[k] is the host loop's verdict on streams[k] alone, a refused stream yields an empty text.
    void decompress_batch(const std::vector<bytes>& streams, std::vector<bytes>& texts, std::vector<int32_t>& status) {
        const size_t count = streams.size();
        texts.assign(count, bytes());
        status.assign(count, 0);
        if (m_coder == TDC_GPU_CODER_ASCII) {
            for (size_t k = 0; k < count; ++k) {
                size_t n = 0;
                status[k] = tdc_lzss_sw_decode(streams[k].data(), streams[k].size(), m_coder, (uint32_t)m_window, nullptr, 0, &n);
                texts[k].resize(status[k] ? 0 : n);
                if (!status[k] && n) status[k] = tdc_lzss_sw_decode(streams[k].data(), streams[k].size(), m_coder, (uint32_t)m_window, texts[k].data(), n, &n);
            }
            return;
        }
        if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
        std::vector<uint64_t> s_off(count ? count : 1, 0), s_len(count ? count : 1, 0), out_off(count + 1, 0);
        size_t pos = 0;
        for (size_t k = 0; k < count; ++k) { s_off[k] = pos; s_len[k] = streams[k].size(); pos += (streams[k].size() + 7) / 8 * 8; }
        bytes blob(pos ? pos : 1);
        for (size_t k = 0; k < count; ++k) std::copy(streams[k].begin(), streams[k].end(), blob.begin() + (size_t)s_off[k]);
        status.assign(count ? count : 1, 0);
        int rc = tdc_gpu_lzss_sw_decompress_batch(m_ctx->h, blob.data(), s_off.data(), s_len.data(), count, m_coder, (uint32_t)m_window, nullptr, 0,
                                                  out_off.data(), status.data(), nullptr);                      // the sizes
        bytes out((size_t)out_off[count] ? (size_t)out_off[count] : 1);
        if (rc == TDC_GPU_ERR_OOM || rc == TDC_GPU_OK)
            rc = tdc_gpu_lzss_sw_decompress_batch(m_ctx->h, blob.data(), s_off.data(), s_len.data(), count, m_coder, (uint32_t)m_window, out.data(), out.size(),
                                                  out_off.data(), status.data(), &last_stats);
        if (rc) throw std::runtime_error(std::string(tdc_gpu_strerror(rc)) + ": " + tdc_gpu_last_error(m_ctx->h));
        status.resize(count);
        for (size_t k = 0; k < count; ++k) texts[k].assign(out.begin() + (size_t)out_off[k], out.begin() + (size_t)out_off[k + 1]);
    }
    // :120-143 -- tokens until the stream ends: the host loop (tdc_lzss_sw_decode), which needs no device; dec=gpu (an addition, as for
    // lz78 / lzw): the device decoder (tdc_gpu_lzss_sw_decompress).  The stream is the same either way.  The window comes from the
    // algorithm id in the file's header (16 if it names none); only coder=bit needs it.
    void decompress(Input& input, Output& output) override {
        const bytes& in = input.raw();
        if (m_opts.get("dec", "host") == "gpu") {
            if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
            uint8_t* out = nullptr; size_t out_len = 0;
            const int rc = tdc_gpu_lzss_sw_decompress(m_ctx->h, in.data(), in.size(), m_coder, (uint32_t)m_window, &out, &out_len, nullptr, nullptr);
            if (rc) throw std::runtime_error(std::string(tdc_gpu_strerror(rc)) + ": " + tdc_gpu_last_error(m_ctx->h));
            output.write(out, out_len);
            tdc_gpu_free(out);
            return;
        }
        size_t n = 0;
        int rc = tdc_lzss_sw_decode(in.data(), in.size(), m_coder, (uint32_t)m_window, nullptr, 0, &n);
        bytes text(n ? n : 1);
        if (!rc) rc = tdc_lzss_sw_decode(in.data(), in.size(), m_coder, (uint32_t)m_window, text.data(), n, &n);
        if (rc) throw std::runtime_error(std::string("lzss: corrupt stream (") + tdc_gpu_strerror(rc) + ")");
        output.write(text.data(), n);
    }
};

// tdc::RePairCompressor<BitCoder | ASCIICoder | EliasGammaCoder | EliasDeltaCoder>  (compressors/RePairCompressor.hpp:14-337), the
// algorithm `repair`: no input restrictions.  coder defaults to bit (:89), max_rules to 0 = unlimited (:90).  The grammar is built on the
// device; coder=huff needs the literal order of :36-84, which is not built.
class RePairCompressor : public Compressor {
    AlgorithmValue m_opts;
    std::shared_ptr<GpuContext> m_ctx;
    int m_device = 0;
    int m_coder = TDC_GPU_CODER_BIT;
    long m_max_rules = 0;
public:
    tdc_gpu_stats last_stats{};
    void set_device(int d) { m_device = d; }
    RePairCompressor(AlgorithmValue opts, std::shared_ptr<GpuContext> ctx) : m_opts(std::move(opts)), m_ctx(std::move(ctx)) {
        const std::string coder = m_opts.get("coder", "bit");
        if (coder == "bit") m_coder = TDC_GPU_CODER_BIT;
        else if (coder == "ascii") m_coder = TDC_GPU_CODER_ASCII;
        else if (coder == "gamma") m_coder = TDC_GPU_CODER_GAMMA;
        else if (coder == "delta") m_coder = TDC_GPU_CODER_DELTA;
        else throw std::runtime_error("No implementation found for compressor repair(coder=" + coder + ")");   // Registry.hpp:214
        m_max_rules = m_opts.get_int("max_rules", 0);
        if (m_max_rules < 0) throw std::runtime_error("repair: max_rules must not be negative");
    }
    void compress(Input& input, Output& output) override {
        if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
        const bytes& in = input.raw();
        uint8_t* out = nullptr; size_t out_len = 0;
        const int rc = tdc_gpu_repair_compress(m_ctx->h, in.data(), in.size(), (uint64_t)m_max_rules, m_coder, &out, &out_len, &last_stats);
        if (rc) throw std::runtime_error(std::string(tdc_gpu_strerror(rc)) + ": " + tdc_gpu_last_error(m_ctx->h));
        output.write(out, out_len);
        tdc_gpu_free(out);
    }
    // every text on its own in one device call, one workgroup per grammar (tdc_gpu_repair_compress_batch): streams[k] is what compress()
    // writes for texts[k]; where status[k] is not TDC_GPU_OK (a text beyond the cap of one text in a batch) the stream is empty
    void compress_batch(const std::vector<bytes>& texts, std::vector<bytes>& streams, std::vector<int32_t>& status) {
        if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
        const uint64_t max_rules = (uint64_t)m_max_rules;
        lz_compress_batch(m_ctx->h,
                          [max_rules](tdc_gpu_ctx* h, const uint8_t* in, const uint64_t* in_off, size_t count, int coder, uint8_t* out, size_t out_cap,
                                      uint64_t* out_off, uint64_t* out_len, int32_t* st, tdc_gpu_stats* stats) {
                              return tdc_gpu_repair_compress_batch(h, in, in_off, count, max_rules, coder, out, out_cap, out_off, out_len, st, stats);
                          },
                          tdc_gpu_repair_batch_bound, m_coder, texts, streams, status, &last_stats);
    }
    // The decoder of such a batch, or of any collection of repair streams, on the device: the grammars of all streams as one forest, one
    // pass, whatever dec says (tdc_gpu_repair_decompress_batch; bit, gamma, delta -- coder=ascii is refused as the call refuses it).
    // texts[k] is what decompress() writes for streams[k], empty where status[k] is not TDC_GPU_OK.
    void decompress_batch(const std::vector<bytes>& streams, std::vector<bytes>& texts, std::vector<int32_t>& status) {
        if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
        lz_decompress_batch(m_ctx->h, tdc_gpu_repair_decompress_batch, m_coder, streams, texts, status, &last_stats);
    }
    // :287-336 -- the host loop (tdc_repair_decode: the rules expanded with an explicit stack), which needs no device; dec=gpu (an
    // addition, as for lzss): the device decoder (tdc_gpu_repair_decompress, which keeps the host loop for coder=ascii).  The stream is
    // the same either way.
    void decompress(Input& input, Output& output) override {
        const bytes& in = input.raw();
        if (m_opts.get("dec", "host") == "gpu") {
            if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
            uint8_t* out = nullptr; size_t out_len = 0;
            const int rc = tdc_gpu_repair_decompress(m_ctx->h, in.data(), in.size(), m_coder, &out, &out_len);
            if (rc) throw std::runtime_error(std::string(tdc_gpu_strerror(rc)) + ": " + tdc_gpu_last_error(m_ctx->h));
            output.write(out, out_len);
            tdc_gpu_free(out);
            return;
        }
        size_t n = 0;
        int rc = tdc_repair_decode(in.data(), in.size(), m_coder, nullptr, 0, &n);
        bytes text(n ? n : 1);
        if (!rc) rc = tdc_repair_decode(in.data(), in.size(), m_coder, text.data(), n, &n);
        if (rc) throw std::runtime_error(std::string("repair: corrupt stream (") + tdc_gpu_strerror(rc) + ")");
        output.write(text.data(), n);
    }
};

// tdc::BWTCompressor (compressors/BWTCompressor.hpp:14-67, ds/bwt.hpp): the Burrows-Wheeler transform of the escaped, 0-terminated view;
// n bytes out, no header.
class BWTCompressor : public Compressor {
    AlgorithmValue m_opts;
    std::shared_ptr<GpuContext> m_ctx;
    int m_device = 0;
public:
    tdc_gpu_stats last_stats{};
    void set_device(int d) { m_device = d; }
    BWTCompressor(AlgorithmValue opts, std::shared_ptr<GpuContext> ctx) : m_opts(std::move(opts)), m_ctx(std::move(ctx)) {}   // (textds: accepted, ignored)
    InputRestrictions input_restrictions() const override { return {true, true}; }   // uses_textds (BWTCompressor.hpp:23)
    void compress(Input& input, Output& output) override {
        if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
        const bytes view = input.as_view();
        uint8_t* out = nullptr; size_t out_len = 0;
        const int rc = tdc_gpu_bwt_compress(m_ctx->h, view.data(), view.size(), &out, &out_len, &last_stats);
        if (rc) throw std::runtime_error(std::string(tdc_gpu_strerror(rc)) + ": " + tdc_gpu_last_error(m_ctx->h));
        output.write(out, out_len);
        tdc_gpu_free(out);
    }
    // every text on its own in one device call (tdc_gpu_bwt_compress_batch): streams[k] is what compress() writes for texts[k] -- each
    // escaped and terminated like a view; where status[k] is not TDC_GPU_OK (a view beyond the cap of one text in a batch) it is empty
    void compress_batch(const std::vector<bytes>& texts, std::vector<bytes>& streams, std::vector<int32_t>& status) {
        if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
        bytes in, piece;
        std::vector<uint64_t> off(texts.size() + 1, 0);
        for (size_t k = 0; k < texts.size(); ++k) {
            piece.resize(2 * texts[k].size() + 1);
            piece.resize(tdc_escape(texts[k].data(), texts[k].size(), piece.data()));
            in.insert(in.end(), piece.begin(), piece.end());
            off[k + 1] = in.size();
        }
        batch_call(tdc_gpu_bwt_compress_batch, in, off, streams, status, 0);
    }
    // The inverse of such a batch, or of any collection of transforms, on the device in one pass whatever dec says
    // (tdc_gpu_bwt_decompress_batch): texts[k] is what decompress() writes for streams[k], empty where status[k] is not TDC_GPU_OK.
    void decompress_batch(const std::vector<bytes>& streams, std::vector<bytes>& texts, std::vector<int32_t>& status) {
        if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
        bytes in;
        std::vector<uint64_t> off(streams.size() + 1, 0);
        for (size_t k = 0; k < streams.size(); ++k) { in.insert(in.end(), streams[k].begin(), streams[k].end()); off[k + 1] = in.size(); }
        batch_call(tdc_gpu_bwt_decompress_batch, in, off, texts, status, 1);
        for (bytes& t : texts) {
            if (t.empty()) continue;
            bytes raw(t.size());
            raw.resize(tdc_unescape(t.data(), t.size(), raw.data()));
            t.swap(raw);
        }
    }
private:
    // results longer than `shortest` bytes are handed out (a buffer of at most one byte inverts to nothing)
    template <typename Call>
    void batch_call(Call call, const bytes& in, const std::vector<uint64_t>& off, std::vector<bytes>& res, std::vector<int32_t>& status, size_t shortest) {
        const size_t count = off.size() - 1;
        bytes out(in.size() ? in.size() : 1);
        status.assign(count ? count : 1, 0);
        const int rc = call(m_ctx->h, in.data(), off.data(), count, out.data(), out.size(), status.data(), &last_stats);
        if (rc) throw std::runtime_error(std::string(tdc_gpu_strerror(rc)) + ": " + tdc_gpu_last_error(m_ctx->h));
        status.resize(count);
        res.assign(count, bytes());
        for (size_t k = 0; k < count; ++k)
            if (!status[k] && off[k + 1] - off[k] > shortest) res[k].assign(out.begin() + off[k], out.begin() + off[k + 1]);
    }
public:
    // decode_bwt (ds/bwt.hpp:77-98): LF[i] = C[b[i]] + rank of b[i] among the equal bytes in front; n - 1 steps from row 0, then the 0.
    // C is accumulated over ALL byte values here (the reference's loop stops in front of 255, which breaks texts that hold 0xFF --
    // every escaped 0x00 or 0xFF byte).  Like the reference the host loop does not look at what it is given beyond staying inside the
    // buffer.  dec=gpu: LF and the list ranking of its cycle on the device (tdc_gpu_bwt_decompress), which refuses what is no transform.
    void decompress(Input& input, Output& output) override {
        const bytes& in = input.raw();
        if (m_opts.get("dec", "host") == "gpu") {
            if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
            uint8_t* out = nullptr; size_t out_len = 0;
            const int rc = tdc_gpu_bwt_decompress(m_ctx->h, in.data(), in.size(), &out, &out_len, nullptr);
            if (rc) throw std::runtime_error(std::string(tdc_gpu_strerror(rc)) + ": " + tdc_gpu_last_error(m_ctx->h));
            output.write(out, out_len);
            tdc_gpu_free(out);
            return;
        }
        const size_t n = in.size();
        if (n <= 1) return;
        if (n >= 0x7FFFFFFFull) throw std::runtime_error("bwt: input too large (32-bit len_t)");
        size_t C[257] = {0};
        for (size_t i = 0; i < n; ++i) ++C[in[i] + 1];
        for (int c = 0; c < 256; ++c) C[c + 1] += C[c];
        std::vector<uint32_t> lf(n);
        for (size_t i = 0; i < n; ++i) lf[i] = (uint32_t)C[in[i]]++;
        bytes text(n);
        size_t i = 0;
        for (size_t j = 1; j < n; ++j) { text[n - 1 - j] = in[i]; i = lf[i]; }
        text[n - 1] = 0;
        output.write(text.data(), text.size());
    }
};

// tdc::ChainCompressor (tudocomp_driver/ChainCompressor.hpp) over bwt, rle, mtf, encode(huff) and encode(sle) -- e.g. the reference's
// bwtzip = bwt:rle:mtf:encode(huff) -- and the three single compressors as chains of one stage: tdc::RunLengthEncoder
// (compressors/RunLengthEncoder.hpp:52-74, option offset), tdc::MTFCompressor (compressors/MTFCompressor.hpp:45-69), tdc::LiteralEncoder
// (compressors/LiteralEncoder.hpp:11-42, `encode(coder)`, coder huff or sle(kmer=1 .. 7)).  compress(): every stage on the device, intermediates in device
// memory (tdc_gpu_pipeline_compress).  decompress(): tdc_gpu_pipeline_decompress -- the stages backwards on the device for streams of
// 1 MiB and more, the host loops of tdc_coders.hpp below that (option dec_parse) and on a machine without a device.  Only a leading bwt
// has input restrictions.
class ChainCompressor : public Compressor {
protected:
    std::vector<tdc_gpu_stage> m_stages;
    std::shared_ptr<GpuContext> m_ctx;
    int m_device = 0;
    static tdc_gpu_stage parse_stage(const std::string& part) {
        const AlgorithmValue av = parse_algorithm_id(part, {part.compare(0, 6, "encode") == 0 ? "coder" : "offset"});
        if (av.name == "bwt") return {TDC_GPU_STAGE_BWT, 0};
        if (av.name == "mtf") return {TDC_GPU_STAGE_MTF, 0};
        if (av.name == "rle") {
            const long o = av.get_int("offset", 0);
            if (o < 0) throw std::runtime_error("rle: offset must not be negative");
            return {TDC_GPU_STAGE_RLE, (uint64_t)o};
        }
        if (av.name == "encode" && av.get("coder", "huff") == "huff") return {TDC_GPU_STAGE_HUFF, 0};
        if (av.name == "encode") {                                            // encode(sle), encode(sle(kmer=K)), encode(coder=sle(kmer=K))
            const AlgorithmValue cv = parse_algorithm_id(av.get("coder", ""), {"kmer"});
            if (cv.name == "sle") {
                const long k = cv.get_int("kmer", 3);                         // SLECoder.hpp:38
                if (k < 1 || k > 7) throw std::runtime_error("sle: kmer must be in 1..7");
                return {TDC_GPU_STAGE_SLE, (uint64_t)k};
            }
        }
        throw std::runtime_error("No implementation found for compressor " + part);       // Registry.hpp:214
    }
public:
    tdc_gpu_stats last_stats{};
    void set_device(int d) { m_device = d; }
    // `a:b:c` (util/algorithm_parser/AlgorithmAST.hpp:119-129: chain(chain(a, b), c))
    ChainCompressor(const std::string& spec, std::shared_ptr<GpuContext> ctx) : m_ctx(std::move(ctx)) {
        size_t b = 0; int depth = 0;
        for (size_t i = 0; i <= spec.size(); ++i) {
            if (i < spec.size() && spec[i] == '(') ++depth;
            if (i < spec.size() && spec[i] == ')') --depth;
            if (i == spec.size() || (spec[i] == ':' && depth == 0)) { m_stages.push_back(parse_stage(spec.substr(b, i - b))); b = i + 1; }
        }
        for (size_t i = 1; i < m_stages.size(); ++i)
            if (m_stages[i].kind == TDC_GPU_STAGE_BWT) throw std::runtime_error("bwt is only available as the first stage of a chain");
        if (m_stages.size() > TDC_GPU_PIPELINE_MAX_STAGES) throw std::runtime_error("a chain has at most 8 stages");
    }
    const std::vector<tdc_gpu_stage>& stages() const { return m_stages; }
    InputRestrictions input_restrictions() const override {
        return m_stages[0].kind == TDC_GPU_STAGE_BWT ? InputRestrictions{true, true} : InputRestrictions{};
    }
    void compress(Input& input, Output& output) override {
        if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
        const bytes view = input.as_view();
        uint8_t* out = nullptr; size_t out_len = 0;
        const int rc = tdc_gpu_pipeline_compress(m_ctx->h, m_stages.data(), (int)m_stages.size(), view.data(), view.size(), &out, &out_len, &last_stats);
        if (rc == TDC_GPU_ERR_NO_SENTINEL) throw std::logic_error(tdc_gpu_strerror(rc));
        if (rc) throw std::runtime_error(std::string(tdc_gpu_strerror(rc)) + ": " + tdc_gpu_last_error(m_ctx->h));
        output.write(out, out_len);
        tdc_gpu_free(out);
    }
    // every text on its own in one device call (tdc_gpu_pipeline_compress_batch): streams[k] is what compress() writes for texts[k] --
    // under a leading bwt each escaped and terminated like a view; where status[k] is not TDC_GPU_OK (a text or view beyond the cap of
    // one text in a batch) it is empty.  The buffer is sized by the call's own sizes pass.  A chain with encode(sle) has no batch form.
    void compress_batch(const std::vector<bytes>& texts, std::vector<bytes>& streams, std::vector<int32_t>& status) {
        if (!m_ctx) m_ctx = std::make_shared<GpuContext>(m_device);
        const size_t count = texts.size();
        const bool lead = m_stages[0].kind == TDC_GPU_STAGE_BWT;
        bytes in, piece;
        std::vector<uint64_t> in_off(count + 1, 0), out_off(count + 1, 0), out_len(count ? count : 1, 0);
        for (size_t k = 0; k < count; ++k) {
            if (lead) {
                piece.resize(2 * texts[k].size() + 1);
                piece.resize(tdc_escape(texts[k].data(), texts[k].size(), piece.data()));
                in.insert(in.end(), piece.begin(), piece.end());
            } else in.insert(in.end(), texts[k].begin(), texts[k].end());
            in_off[k + 1] = in.size();
        }
        if (in.empty()) in.resize(1);
        status.assign(count ? count : 1, 0);
        const int k = (int)m_stages.size();
        int rc = tdc_gpu_pipeline_compress_batch(m_ctx->h, m_stages.data(), k, in.data(), in_off.data(), count, nullptr, 0, out_off.data(), out_len.data(),
                                                 status.data(), nullptr);                                              // the sizes
        bytes out((size_t)out_off[count] ? (size_t)out_off[count] : 1);
        if (rc == TDC_GPU_ERR_OOM || rc == TDC_GPU_OK)
            rc = tdc_gpu_pipeline_compress_batch(m_ctx->h, m_stages.data(), k, in.data(), in_off.data(), count, out.data(), out.size(), out_off.data(),
                                                 out_len.data(), status.data(), &last_stats);
        if (rc) throw std::runtime_error(std::string(tdc_gpu_strerror(rc)) + ": " + tdc_gpu_last_error(m_ctx->h));
        status.resize(count);
        streams.clear();
        for (size_t t = 0; t < count; ++t) streams.emplace_back(out.begin() + (size_t)out_off[t], out.begin() + (size_t)(out_off[t] + out_len[t]));
    }
    // without a device (no context can be created) the byte stages are still decodable: the host loops, which need none
    void decompress_host(Input& input, Output& output) {
        bytes a = input.raw(), b;
        for (size_t i = m_stages.size(); i-- > 0; ) {
            const tdc_gpu_stage& st = m_stages[i];
            auto run = [&](uint8_t* o, size_t cap) {
                ByteSink sink(o, cap);
                if (st.kind == TDC_GPU_STAGE_RLE) rle_decode(a.data(), a.size(), st.param, sink);
                else if (st.kind == TDC_GPU_STAGE_MTF) mtf_decode(a.data(), a.size(), sink);
                else if (st.kind == TDC_GPU_STAGE_SLE) sle_decode_literals(a.data(), a.size(), (unsigned)st.param, sink);
                else huff_decode_literals(a.data(), a.size(), sink);
                return sink.n;
            };
            const uint64_t need = run(nullptr, 0);
            if (need > 0xFFFFFFFEull) throw std::runtime_error("corrupt stream: a stage decodes to more than 2^32 - 2 bytes");
            b.assign((size_t)need, 0);
            run(b.data(), b.size());
            a.swap(b);
        }
        output.write(a.data(), a.size());
    }
    void decompress(Input& input, Output& output) override {
        if (!m_ctx) {
            try { m_ctx = std::make_shared<GpuContext>(m_device); }
            catch (const std::exception&) {
                if (m_stages[0].kind == TDC_GPU_STAGE_BWT) throw;
                decompress_host(input, output);
                return;
            }
        }
        const bytes& in = input.raw();
        uint8_t* out = nullptr; size_t out_len = 0;
        const int rc = tdc_gpu_pipeline_decompress(m_ctx->h, m_stages.data(), (int)m_stages.size(), in.data(), in.size(), &out, &out_len);
        if (rc) throw std::runtime_error(std::string(tdc_gpu_strerror(rc)) + ": " + tdc_gpu_last_error(m_ctx->h));
        output.write(out, out_len);
        tdc_gpu_free(out);
    }
};
class RunLengthEncoder : public ChainCompressor {
public:
    RunLengthEncoder(const AlgorithmValue& opts, std::shared_ptr<GpuContext> ctx) : ChainCompressor("rle(offset=" + opts.get("offset", "0") + ")", std::move(ctx)) {}
};
class MTFCompressor : public ChainCompressor {
public:
    explicit MTFCompressor(std::shared_ptr<GpuContext> ctx) : ChainCompressor("mtf", std::move(ctx)) {}
};
class LiteralEncoder : public ChainCompressor {
public:
    LiteralEncoder(const AlgorithmValue& opts, std::shared_ptr<GpuContext> ctx) : ChainCompressor("encode(coder=" + opts.get("coder", "huff") + ")", std::move(ctx)) {}
};

// ---- registry (what is actually registered; Registry.hpp:204-231) ---------------------------------------------
struct Selection {
    std::string id_string;
    std::unique_ptr<Compressor> compressor;
    InputRestrictions restrictions;
};

inline std::vector<std::string> registered_algorithms() {
    return { "lcpcomp(coder=huff, comp=arrays, dec=scan(scans=6), threshold=5, flatten=1)   [MI355X, libtdc_gpu.so]",
             "lcpcomp(coder=huff, comp=plcppeaks, threshold=5, flatten=1)                 [MI355X, peak scan as an orbit marking]",
             "lcpcomp(coder=huff, dec=gpu)                                                [decompression: host parse, references resolved on the MI355X]",
             "lcpcomp(coder=ascii, comp=arrays, threshold=5, flatten=1)                   [MI355X; host decoder]",
             "lcpcomp(coder=sle(kmer=3), comp=arrays, threshold=5, flatten=1)             [MI355X; host decoder]",
             "lcpcomp(coder=..., comp=max_lcp | plcppeaks, ...)                           [MI355X]",
             "lcpcomp(coder=..., comp=heap, ...)                                          [MI355X, sequential replay of the reference's heap: a parity row, about a minute per MiB -- inputs of a few hundred KiB at most]",
             "lcpcomp(coder=arithmetic, comp=arrays, threshold=5, flatten=1)              [MI355X, compress only]",
             "lzss_lcp(coder=huff, threshold=3)                                           [MI355X, libtdc_gpu.so]",
             "lzss_lcp(coder=bit | gamma | delta | ascii, threshold=3)                    [MI355X: the position-space encoder with fixed-width fields / self-delimiting codes]",
             "lzss_lcp(coder=huff | bit | gamma | delta, dec=gpu)                         [decompression parsed on the MI355X for streams of 1 MiB and more; ascii: host parse]",
             "lz78(coder=gamma)                                                           [host parse + MI355X gamma packer]",
             "lz78(coder=gamma, dec=gpu)                                                  [decompression parsed and expanded on the MI355X]",
             "lzw(coder=bit)                                                              [host parse + MI355X packer from closed-form bit offsets]",
             "lzw(coder=gamma)                                                            [host parse + MI355X gamma packer]",
             "lzw(coder=bit, dec=gpu)                                                     [decompression on the MI355X: codes read side by side, phrases expanded by pointer jumping]",
             "lzw(coder=gamma, dec=gpu)                                                   [decompression parsed and expanded on the MI355X]",
             "lzss(coder=bit | ascii | gamma | delta, window=16, threshold=3)             [sliding-window LZ77 factorized on the MI355X, window 1 .. 4096; host decoder]",
             "lzss(coder=bit | gamma | delta, dec=gpu)                                    [decompression parsed and resolved on the MI355X for streams of 1 MiB and more; ascii: host loop]",
             "repair(coder=bit | ascii | gamma | delta, max_rules=0)                      [Re-Pair grammar built on the MI355X: digram table, one rule per round; host decoder]",
             "repair(coder=bit | gamma | delta, dec=gpu)                                  [decompression on the MI355X for streams of 1 MiB and more: tokens parsed side by side, grammar -> factor list; ascii: host loop]",
             "bwt                                                                         [MI355X: suffix array + one gather; host inverse loop]",
             "bwt(dec=gpu)                                                                [inverse on the MI355X: LF by a counting rank + list ranking of its cycle]",
             "rle                                                                         [MI355X; host decoder]",
             "rle(offset=0)                                                               [MI355X; host decoder]",
             "mtf                                                                         [MI355X: chunk summaries + one list per thread; host decoder]",
             "encode(huff)                                                                [MI355X; host decoder]",
             "encode(sle)                                                                 [MI355X: k-mer count, fill-state scan, one cost / scan / pack pass; decompression on the MI355X for streams of 1 MiB and more]",
             "encode(sle(kmer=3))                                                         [kmer = 1 .. 7]" };
}

inline Selection select_algorithm(const std::string& id, std::shared_ptr<GpuContext> ctx = nullptr, int device = 0) {
    // chains (`a:b`) are reached through the library and the facade classes, not through the command line
    if (id.find(':') != std::string::npos) throw std::runtime_error("No implementation found for compressor " + id + " (chains are not available on the command line)");
    AlgorithmValue av = parse_algorithm_id(id, {"coder", "comp", "dec", "textds"});
    Selection s;
    s.id_string = id;
    if (av.name == "rle" || av.name == "mtf" || av.name == "encode") {
        std::unique_ptr<ChainCompressor> z;
        if (av.name == "rle") z = std::make_unique<RunLengthEncoder>(parse_algorithm_id(id, {"offset"}), std::move(ctx));
        else if (av.name == "mtf") z = std::make_unique<MTFCompressor>(std::move(ctx));
        else z = std::make_unique<LiteralEncoder>(parse_algorithm_id(id, {"coder"}), std::move(ctx));
        z->set_device(device);
        s.compressor = std::move(z);
        return s;
    }
    if (av.name == "lz78") {
        auto z = std::make_unique<LZ78Compressor>(parse_algorithm_id(id, {"coder", "lz78trie", "dec"}), std::move(ctx));
        z->set_device(device);
        s.compressor = std::move(z);
        return s;
    }
    if (av.name == "lzw") {
        auto z = std::make_unique<LZWCompressor>(parse_algorithm_id(id, {"coder", "lz78trie", "dict_size", "dec"}), std::move(ctx));
        z->set_device(device);
        s.compressor = std::move(z);
        return s;
    }
    if (av.name == "lzss") {
        auto z = std::make_unique<LZSSSlidingWindowCompressor>(parse_algorithm_id(id, {"coder", "window", "threshold", "dec"}), std::move(ctx));
        z->set_device(device);
        s.compressor = std::move(z);
        return s;
    }
    if (av.name == "repair") {
        auto z = std::make_unique<RePairCompressor>(parse_algorithm_id(id, {"coder", "max_rules", "dec"}), std::move(ctx));
        z->set_device(device);
        s.compressor = std::move(z);
        return s;
    }
    if (av.name == "bwt") {
        auto z = std::make_unique<BWTCompressor>(parse_algorithm_id(id, {"textds", "dec"}), std::move(ctx));
        z->set_device(device);
        s.restrictions = z->input_restrictions();
        s.compressor = std::move(z);
        return s;
    }
    if (av.name == "lzss_lcp") {
        auto z = std::make_unique<LZSSLCPCompressor>(parse_algorithm_id(id, {"coder", "textds", "threshold", "dec"}), std::move(ctx));
        z->set_device(device);
        s.restrictions = z->input_restrictions();
        s.compressor = std::move(z);
        return s;
    }
    if (av.name != "lcpcomp") throw std::runtime_error("No implementation found for compressor " + id);
    auto c = std::make_unique<LCPCompressor>(av, std::move(ctx));
    c->set_device(device);
    s.restrictions = c->input_restrictions();
    s.compressor = std::move(c);
    return s;
}

}  // namespace tdc_amd
