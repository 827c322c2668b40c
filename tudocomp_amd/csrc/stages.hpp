// stages.hpp -- host-callable stage functions of the device pipeline (all arrays are device pointers).
// Each stage replaces one row of SURVEY.md section 8a; citations are relative to
// /root/reference/include/tudocomp/.
#pragma once
#include "common.hpp"
#include <functional>

namespace tdc {

// a1: io/RestrictedBuffer.hpp:43-74 + io/EscapeMap.hpp:39-64 on the device (d_out: n + #escapes + 1 bytes); returns the escaped length
size_t escape_device(Ctx& c, const u8* d_in, size_t n, u8* d_out);
size_t count_escapes_device(Ctx& c, const u8* d_in, size_t n);     // bytes the escaping adds

struct SAStats { u32 rounds = 0; u32 sym_bits = 0; u32 init_syms = 0; u64 sorted_elems = 0;
                 u32 wide_kw = 0; /* key words of the wide initial sort (0: classic path) */ u32 text_rounds = 0; u64 wide_nonheads = 0;
                 u32 overlapped = 0; /* 1: level 1 of the wide sort ran behind the upload */
                 u64 pair_resolved = 0; /* suffixes of two-member groups ordered by the one-pass pair step in front of the doubling rounds */
                 u64 star_chains = 0; /* chains of the star step (round 6: every group ordered against its smallest member in one pass) */ };
// Optional sink of the wide path (suffix_array.hip): lcp8 = n bytes for the LCP (in symbols) of every suffix-array slot with its
// predecessor.  mode (out): 0 = classic result (sa and isa written), 1 = sa final and lcp8 valid but isa NOT written -- the caller
// derives ISA, Phi and PLCP with build_isa_phi_plcp_fused().
struct SAExtra { u8* lcp8 = nullptr; int mode = 0; };

// a2+a3: ds/SADivSufSort.hpp:27-51 and ds/ISAFromSA.hpp:30-43.
// Prefix doubling; text[n-1] must be the unique 0.  sa and isa are caller-provided (n entries each).
void build_suffix_array(Ctx& c, const u8* text, size_t n, u32* sa, u32* isa, SAStats* st, SAExtra* ex = nullptr);
// a3 + a4 + a5 in one pass over a final suffix array whose neighbour LCPs are known (lcp8[i] = lcp(T[sa[i-1]..], T[sa[i]..]), i >= 1):
// isa[sa[i]] = i, phi[sa[i]] = sa[i-1] (phi[sa[0]] = sa[n-1]), plcp[sa[i]] = lcp8[i] (plcp[sa[0]] = 0); d_maxlcp receives the maximum.
// ds/ISAFromSA.hpp:30-43, ds/PhiFromSA.hpp:35-45, ds/PLCPFromPhi.hpp:27-53 (same arrays, computed from the sort instead of the text)
// What cand_class_kernel (factorize.hip) derives from the PLCP values, produced by the image kernel of the fused scatter while it holds a
// window's values in LDS (option fused_cand): the caller allocates the arrays BEFORE the scatter takes its scratch and sets threshold and
// lcut (the window pass's cut as known before maxlcp is: min(window_lcut, window_levels_max_lcut()), 0 where the pass cannot run); the
// scatter sets `filled` where its image kernel ran (not on the direct path of small texts), and factorize_arrays then skips its own pass.
struct CandFused {
    u32 threshold = 0, lcut = 0;
    u8* cls = nullptr;          // n bytes: 1 = candidate of a level above lcut
    u8* res8 = nullptr;         // n bytes, lcut != 0 only: min(PLCP, 255) of a candidate, 0 elsewhere
    u8* flen8 = nullptr;        // FactorSpace::flen8 (zero-filled), or
    u32* flen = nullptr;        // FactorSpace::flen where there is no byte array
    u32* tilecnt = nullptr;     // nullable (option sel_tile_counts): class-1 bytes per SEL_TILE positions, for select_by_class
    u32* acc = nullptr;         // CF_COPIES x CF_ACC words the workgroups add to (sampled level histogram [0, 64), candidate count [64])
    u32* lvlhist = nullptr;     // 64 words: the sampled level histogram (lcut != 0 only meaningful), folded from acc
    u32* entries = nullptr;     // 1 word behind it: the number of candidates
    bool filled = false;
};
constexpr u32 CF_COPIES = 64, CF_ACC = 80;
void build_isa_phi_plcp_fused(Ctx& c, const u32* sa, const u8* lcp8, size_t n, u32* isa, u32* phi, u32* plcp, u32* d_maxlcp, CandFused* cf = nullptr);
bool fused_scatter_has_image(const Ctx& c, size_t n);      // false: a text this short takes the direct kernel (cf is left unfilled)
u32 factorize_arrays_lcut0(const Ctx& c, size_t n, u32 threshold);     // CandFused::lcut for factorize_arrays(threshold) on this context
// byte histogram of a text into the context's cache (c.hist_cache / hist_ptr / hist_n): add() per part, finish() once
void text_histogram_add(Ctx& c, const u8* part, size_t len, u32* d_hist);
void text_histogram_finish(Ctx& c, const u8* text, size_t n, const u32* d_hist);

// a4: ds/PhiFromSA.hpp:35-45
void build_phi(Ctx& c, const u32* sa, size_t n, u32* phi);
// a5: ds/PLCPFromPhi.hpp:27-53 ; plcp[n-1] := 0 ; d_maxlcp (device u32) receives max PLCP
void build_plcp(Ctx& c, const u8* text, size_t n, const u32* phi, u32* plcp, u32* d_maxlcp);
// len[i] = lcp(T[i..], T[src[i]..]) for sources with len[i] >= len[i-1] - 1 (same chunked carry as build_plcp);
// src[i] == NONE32 -> 0.  d_max receives the maximum.
void build_lce_with_carry(Ctx& c, const u8* text, size_t n, const u32* src, u32* len, u32* d_max);
// a6 (debug/fixtures only): ds/LCPFromPLCP.hpp:27-56
void build_lcp(Ctx& c, const u32* sa, const u32* plcp, size_t n, u32* lcp);

// Position-space factor representation shared by factorize / flatten / encode:
//   flen[p]  : length of the factor that STARTS at p, 0 otherwise (after mark_literal_runs: run length at
//              the first position of every literal run)
//   owner[p] : identifies the factor covering p (its index in position order; lzss_lcp writes the start position
//              instead), NONE32 if p is a literal.  A factor starts at p iff owner[p] != NONE32 and owner[p-1] != owner[p].
//   fsrc[p]  : source of the factor starting at p (valid where flen[p] > 0 and owner[p] == p)
struct FactorSpace {
    u32* flen = nullptr;
    // optional (round 5, the metric's path): the factor lengths as BYTES until build_owner() has turned them into the list -- flen8[p] = length
    // of the factor that starts at p (255: the length is flen[p]), 0 elsewhere.  Only flen8 is zero-filled then (2 instead of 8 bytes of
    // traffic per position for the fill and for either pass of build_owner); flen[] is valid at the starts of factors of 255 and more
    // positions only, until expand_flen8() fills it for a caller that wants the dense array after all.
    u8* flen8 = nullptr;
    u32* owner = nullptr;
    u32* fsrc = nullptr;
    // optional: the factor starts in position order (n entries of capacity).  build_owner() fills it and sets
    // have_list; flatten and encode then skip their own extraction (factor positions never change after that).
    u32* fpos = nullptr;
    u32* flenl = nullptr;      // optional companion of fpos: the factor lengths in the same order (filled with it)
    size_t nfact = 0;
    bool have_list = false;
    // optional: one class byte per position -- 0 literal, 2 factor start, 3 covered by a factor that started earlier.  build_owner()
    // fills it (have_cls); the encoder's streaming passes then read 1 byte instead of the 4-byte owner word per position.
    u8* cls = nullptr;
    bool have_cls = false;
    // optional (round 6, the metric's path): the top owner_rem_bits bits of a covered position's owner word hold how far its factor still
    // reaches -- q = min(end of the factor - p - 1, 2^bits - 1); the rank sits in the bits below.  A flatten step that lands on p with a
    // copy longer than q + 1 (q not saturated) knows that the copy does not fit WITHOUT fetching the covering factor's record: 43 % of all
    // chain visits on English text.  Requested with want_owner_rem by a caller whose later stages never read owner[] (they read cls[] and
    // the flatten records); build_owner() takes the bits the ranks leave free (at most want_owner_rem, at most 8) and sets owner_rem_bits.  NONE32 stays NONE32.
    u32 want_owner_rem = 0;     // 0: plain ranks; else the most bits to take (8 is all build_owner() ever takes)
    u32 owner_rem_bits = 0;
    // lazy sources (round 4): set by factorize_arrays when there is no Phi array -- fsrc[] then holds the sources of the factors of the
    // global levels only; the source of any factor start p is  src_prio[p] < src_n ? src_sa[src_prio[p] - 1] : fsrc[p]  (src_prio = ISA
    // unless a push at a global level overwrote it, and such a position had its source saved first).  flatten_factors computes it
    // while it builds its records; everyone else calls materialize_sources() first.
    const u32* src_prio = nullptr;
    const u32* src_sa = nullptr;
    size_t src_n = 0;
};
// owner[] for a reader that compares whole words (everyone but the flatten rounds): refuses an array that carries remainder bits
inline const u32* plain_owner(const FactorSpace& fs) {
    if (fs.owner_rem_bits) throw HipError{hipErrorUnknown, "owner[] carries remainder bits (FactorSpace::owner_rem_bits): this stage reads plain ranks", (int)__LINE__};
    return fs.owner;
}
void materialize_sources(Ctx& c, size_t n, FactorSpace& fs);    // fills fsrc[] at every factor start, clears src_prio

struct FactorizeStats { u64 factors = 0; u32 maxlcp = 0; u32 levels = 0; u32 rounds = 0; u64 pushes = 0; u64 entries = 0; u32 small_levels = 0; u32 purges = 0;
                        u32 window_pass = 0; /* 0 not used, 1 low levels done window-local, 2 window pass failed -> global loop */
                        u32 window_lcut = 0; /* highest level of the last window pass */
                        u32 probes = 0; /* skip-ahead probes over runs of erased levels */
                        u32 max_push_targets = 0; /* most push-target levels of one level */
                        u32 eager_levels = 0, eager_phases = 0; /* levels inside one-launch runs of small levels (factorize_eager.hip), runs */ };

// a8: compressors/lcpcomp/compress/ArraysComp.hpp:36-117 in position space.
// Inputs: isa, phi, plcp.  isa and plcp are consumed: they become the working priority / LCP arrays.
// Outputs: fs.flen / fs.owner filled, fs.fsrc[p] = phi[p] at factor starts.
// cf (optional, cf->filled): the candidate classes, residence bytes, zero-filled lengths and counters are in place already (CandFused)
void factorize_arrays(Ctx& c, size_t n, const u32* sa, u32* isa, const u32* phi, u32* plcp, u32 maxlcp,
                      u32 threshold, FactorSpace& fs, FactorizeStats* st, const CandFused* cf = nullptr);

// owner[] from the factor starts (flen[p] != 0 exactly at factor starts): owner[q] = start of the factor covering q, else NONE32
void build_owner(Ctx& c, size_t n, FactorSpace& fs);
// compact lengths (fs.flen8) -> the dense flen[] array; fs.flen8 is cleared
void expand_flen8(Ctx& c, size_t n, FactorSpace& fs);

// lcpcomp(comp=plcppeaks): lcpcomp::PLCPPeaksStrategy (compressors/lcpcomp/compress/PLCPPeaksStrategy.hpp:36-80); fills fs
// (flen, fsrc, owner, factor list) like factorize_arrays
void plcp_peaks_factorize(Ctx& c, size_t n, const u32* phi, const u32* plcp, u32 threshold, FactorSpace& fs, u64* nfactors);
// lcpcomp::MaxLCPStrategy (compressors/lcpcomp/compress/MaxLCPStrategy.hpp:36-100) in position space; isa and plcp are
// consumed like in factorize_arrays
void factorize_max_lcp(Ctx& c, size_t n, u32* isa, const u32* phi, u32* plcp, u32 maxlcp, u32 threshold, FactorSpace& fs,
                       FactorizeStats* st);

// lcpcomp::MaxHeapStrategy (compressors/lcpcomp/compress/MaxHeapStrategy.hpp:36-101, ds/ArrayMaxHeap.hpp): sequential replay on
// the device (a parity row: its tie order is the layout history of a binary heap); sa / isa / plcp are only read
void factorize_max_heap(Ctx& c, size_t n, const u32* sa, const u32* isa, const u32* plcp, u32 maxlcp, u32 threshold, FactorSpace& fs,
                        FactorizeStats* st);

struct FlattenStats { u64 num_flattened = 0; u64 max_depth_lb = 0; u32 rounds = 0; };      // rounds: summed over the rank ranges of a chunked run
// Rank ranges of a chunked flatten (option flatten_chunks): K = want clamped to [1, min(z, FLATTEN_MAX_CHUNKS)] ranges of equal counts,
// range k = [z k / K, z (k + 1) / K).  The pack that follows the ranges (encode_early_chunks) takes its bounds from the same two functions.
constexpr u32 FLATTEN_MAX_CHUNKS = 16;
inline u32 flatten_chunk_count(u32 want, size_t z) { return (u32)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(want, FLATTEN_MAX_CHUNKS), z)); }
inline size_t flatten_chunk_start(size_t z, u32 k, u32 K) { return (size_t)((u64)z * k / K); }
// a10: compressors/lzss/LZSSFactors.hpp:79-132 ; rewrites fs.fsrc in place.
// `between` (optional) is called with r = 1, 2, ... once round r has been enqueued and before the host waits for its count, and with 0
// when the rounds are over: the place for work that does not need the flattened sources (api_compress.hip runs the first half of the encoder
// there, step by step on another stream), whatever range the round belongs to.  Whatever it takes from the arena is gone when flatten_factors returns.
// rec_keep (optional, room for 16 bytes per factor): the records {pos, len, original source, final source} in position order are built
// there and stay valid for the caller; fs.fsrc is NOT rewritten then.
// chunks: rank ranges the rounds run on one after the other (flatten.hip; 0: what option flatten_chunks forces, else one); chunk_done(k, r)
// (optional) is called when the last round of range k is over, with c.stream behind it: the final sources of ranks < r stand in the records.
void flatten_factors(Ctx& c, size_t n, FactorSpace fs, FlattenStats* st, const std::function<void(int)>& between = {}, void* rec_keep = nullptr,
                     u32 chunks = 0, const std::function<void(u32, size_t)>& chunk_done = {});

// a9: extract the factor list sorted by pos (LZSSFactors.hpp:69-76): pos[], src[], len[] (z entries each,
// arrays caller-provided with capacity cap).  Returns z.
size_t extract_factors(Ctx& c, size_t n, FactorSpace fs, u32* pos, u32* src, u32* len, size_t cap);
// inverse: scatter a sorted factor list into position space (used by the stage-level test entry points)
void scatter_factors(Ctx& c, size_t n, const u32* pos, const u32* src, const u32* len, size_t z, FactorSpace fs);

struct EncodeStats { u64 factors = 0; u64 flen_min = 0, flen_max = 0, fdist_max = 0; u64 out_bits = 0; u32 sigma = 0; };
// a11-a14: LZSSLiterals.hpp:10-50, HuffmanCoder.hpp:37-48/442-474/526-569, LZSSCoding.hpp:18-92, BitOStream.hpp:53-64.
// Writes the complete stream (incl. terminator) to d_out (capacity out_cap bytes); returns its length.
// fs.flen is modified (literal-run lengths are stored at run starts).
size_t encode_huff(Ctx& c, const u8* text, size_t n, FactorSpace fs, u8* d_out, size_t out_cap, EncodeStats* st);
// the same with a selectable coder: 0 = HuffmanCoder, 1 = ArithmeticCoder (a15: coders/ArithmeticCoder.hpp:35-177),
// 2 = ASCIICoder (coders/ASCIICoder.hpp:29-50; every integer and bit of the token stream as text)
// 4 = BitCoder (the raw-literal stream of coder 0 without its table bit), 5 = EliasGammaCoder, 6 = EliasDeltaCoder (every field and
// every literal as a self-delimiting code; factor spaces without class bytes only: lzss_lcp)
// `early`: the first half (everything in front of the pack: gaps, histogram, coder header, bits per tile and their scan -- none of
// it reads the factors' sources) has already run, see encode_early_*
struct EncodeEarly;
size_t encode_stream(Ctx& c, const u8* text, size_t n, FactorSpace fs, int coder, u8* d_out, size_t out_cap, EncodeStats* st, EncodeEarly* early = nullptr);
// the first half on its own, for coder 0 and a factor space with list and class bytes (build_owner): _reserve takes the scratch from
// the arena (call it BEFORE flatten_factors takes its lists), _run enqueues on c.stream and waits for the results
// z_rec > 0: also room for the z_rec records of the flatten stage (encode_early_rec; hand it to flatten_factors as rec_keep): the pack
// then takes lengths and flattened sources from the records and flatten_factors leaves fs.fsrc as it is
EncodeEarly* encode_early_reserve(Ctx& c, size_t n, size_t z_rec = 0);
void* encode_early_rec(EncodeEarly* e);
// _run: the next of its three steps (gaps + histogram | code table, bits per tile, scans | collect), or with finish = true all that are left.
// Only the last one waits for the device if the steps are spread over time (their read-backs travel through the mapped host area).
void encode_early_run(Ctx& c, const u8* text, size_t n, FactorSpace fs, int coder, EncodeEarly* e, bool finish = true);
void encode_early_free(EncodeEarly* e);
// Pack and download behind the rank ranges of a chunked flatten (K >= 2 ranges of fs.nfact factors; call it between _reserve and
// flatten_factors).  false: this call does not overlap pack and download (no host buffer of the caller's, a text of fewer than
// 64 * PACK_CH tiles, no records, no second side stream) -- nothing was taken, flatten in one range.  true: the output buffer is reserved
// (encode_early_out), the pack's chunks end at the tiles that hold the first factor of every range, and encode_early_chunk_done -- from
// flatten_factors' chunk_done, c.stream being the compute stream -- packs the tiles in front of range k + 1 on the copy stream and sends
// their bytes to the host on the aux stream, as soon as the first half's results are there; encode_stream does what is left.
bool encode_early_chunks(Ctx& c, size_t n, const FactorSpace& fs, EncodeEarly* e, u32 K, size_t out_cap);
void encode_early_chunk_done(Ctx& c, const u8* text, size_t n, const FactorSpace& fs, EncodeEarly* e, u32 k);
u8* encode_early_out(EncodeEarly* e, size_t* out_cap);      // the buffer encode_early_chunks reserved and its size (NULL: none, *out_cap untouched)
u32 encode_early_packed(const EncodeEarly* e);              // ranges whose pack has been enqueued so far

// worst-case output size of encode_huff for a text of n bytes
size_t encode_bound(size_t n);
size_t encode_bound_coder(size_t n, int coder);    // coder as in encode_stream (2 = ASCIICoder needs twice as much)
size_t encode_bound_uni(size_t n, int coder);      // coder 4 / 5 / 6 (lzss_lcp's BitCoder, EliasGammaCoder, EliasDeltaCoder)

struct LzssStats { u64 factors = 0; };
// a18: compressors/LZSSLCPCompressor.hpp:60-115 (lzss_lcp): greedy LZ77 parse from the previous / next smaller values of
// the suffix array (ANSV) -- fills fs like factorize_arrays (no flatten for this compressor).
void lzss_lcp_factorize(Ctx& c, const u8* text, size_t n, const u32* sa, const u32* isa, u32 threshold, FactorSpace fs,
                        LzssStats* st);

}  // namespace tdc
#include <vector>
namespace tdc {
// LCPCompressor::decompress (LCPCompressor.hpp:140-150; also lzss_lcp streams): host parse of the Huffman token stream,
// references resolved on the device by pointer jumping.  `text` receives the (still escaped, 0-terminated) text.
struct DecodeStats { u64 factors = 0; u32 rounds = 0; u32 device_parse = 0; };
struct StreamFormatError { const char* what; };          // malformed input
// Where the bytes a call produces go: the caller's buffer `into` of `cap` bytes, or a buffer allocated during the call (`owned`: by
// decode_dest for the decoders, by sink_host of the C ABI layer for everything else) that is handed to the caller through *out by
// release() once the call has succeeded and freed otherwise, or -- `keep`, lcpcomp only -- nowhere: the stream stays on the device.
// *out_len receives the length (api.hpp: how the entry points build one, and the "too small" rule).
struct Sink {
    u8* into = nullptr; size_t cap = 0;
    u8* owned = nullptr;
    uint8_t** out = nullptr; size_t* out_len = nullptr;
    bool keep = false;
    Sink() = default;
    Sink(Sink&& o) : into(o.into), cap(o.cap), owned(o.owned), out(o.out), out_len(o.out_len), keep(o.keep) { o.owned = nullptr; }
    Sink(const Sink&) = delete;
    Sink& operator=(const Sink&) = delete;
    ~Sink() { free(owned); }
    u8* release() { u8* r = owned; owned = nullptr; return r; }
};
// the same for streams written with another coder: 0 = HuffmanCoder, 2 = ASCIICoder, 3 | kmer << 8 = SLECoder
size_t decode_lzss(Ctx& c, const u8* stream, size_t len, int coder, Sink& out, DecodeStats* st);
// lzss_lcp streams of the universal coders (kind 0 = BitCoder, 1 = EliasGammaCoder, 2 = EliasDeltaCoder) parsed on the device; false:
// this stream keeps the host loop (tdc_coders.hpp decode_text), nothing has been written.  *n_out: the text length.
bool decode_lzss_uni(Ctx& c, const u8* stream, size_t len, int kind, Sink& out, DecodeStats* st, size_t* n_out);
// LZ78Compressor::decompress (compressors/LZ78Compressor.hpp:142-160) for coder=gamma, parsed on the device (lz78_decode.hip).
// Returns the text length; *need (nullable) receives it as soon as it is known -- also when out.into is too small (HipError
// hipErrorOutOfMemory).  Malformed input: StreamFormatError; a text of more than 2^32 - 2 bytes: DecodeTooLarge.
struct DecodeTooLarge { u64 n; };
size_t decode_lz78_gamma(Ctx& c, const u8* stream, size_t len, Sink& out, size_t* need, DecodeStats* st);
// a17: compressors/LZ78Compressor.hpp:64-140 -- sequential parse on the host; returns the number of (id, char) pairs
size_t lz78_parse_host(const u8* in, size_t n, std::vector<u32>& ids, std::vector<u8>& chars, bool* leftover_is_high);
// a16: coders/EliasGammaCoder.hpp:26-29 + io/BitOStream.hpp:105-129 on the device; returns the stream length
size_t lz78_gamma_encode(Ctx& c, const u32* d_ids, const u8* d_chars, size_t z, u8* d_out, size_t out_cap);
// the same for items of one value (d_chars == NULL) or two
size_t gamma_encode_items(Ctx& c, const u32* d_ids, const u8* d_chars, size_t z, u8* d_out, size_t out_cap);

// ---- lzw (compressors/LZWCompressor.hpp, lzw/LZWDecoding.hpp; lzw_host.cpp, lzw.hip) -----------------------
// :39-108 -- the sequential parse on the host: codes[k] = id of the node phrase k ends in; returns the number of codes
size_t lzw_parse_host(const u8* in, size_t n, std::vector<u32>& codes);
// the codes (device) -> the stream in d_out, terminator included; bit: BitCoder (code k in bits_for(k + 256) bits), else EliasGammaCoder.
// Returns the stream length.  d_out needs no zeroing for BitCoder (every word is written whole).
size_t lzw_encode(Ctx& c, const u32* d_codes, size_t z, bool bit, u8* d_out, size_t out_cap);
// :110-133 -- on the device for streams of LZW_DEVICE_MIN bytes and more (option dec_parse: 2 = every stream, 0 = never), else the host
// loop (decode_step restated).  Results and exceptions as decode_lz78_gamma; st->device_parse tells which path ran.
constexpr size_t LZW_DEVICE_MIN = (size_t)64 << 10;
size_t decode_lzw(Ctx& c, const u8* stream, size_t len, bool bit, Sink& out, size_t* need, DecodeStats* st);

// ---- lzss (compressors/LZSSSlidingWindowCompressor.hpp; lzss_sw.hip, lzss_sw_host.cpp) ----------------------------
constexpr u32 LZSS_SW_MAX_WINDOW = 4096;      // the match kernel holds a tile of positions, its window and its look-ahead in LDS
// :57-99 for every text position at once, then the greedy parse as the orbit of position 0.  Returns the number of tokens; tokpos[i] =
// text position of token i (ascending) and fac[p] = distance << 16 | length of the factor the parse would start AT p (0: a literal) are
// taken from the arena and stay valid until the caller releases its mark.  1 <= window <= LZSS_SW_MAX_WINDOW, n <= 2^32 - 2.
size_t lzss_sw_tokens(Ctx& c, const u8* d_text, size_t n, u32 window, u32 threshold, u32** tokpos, u32** fac);
// the factors among the tokens as a list sorted by pos (d_pos / d_src / d_len: ntok entries of capacity each); returns their number
size_t lzss_sw_factor_list(Ctx& c, const u32* tokpos, const u32* fac, size_t ntok, u32* d_pos, u32* d_src, u32* d_len);
// :85-95 -- the tokens through one coder (field_coder.hpp): kind 0 = BitCoder, 1 = ASCIICoder, 2 = EliasGammaCoder, 3 = EliasDeltaCoder.
// Writes the stream, terminator included, to d_out and returns its length -- or 0 with st->truncates set and nothing packed: BitCoder
// and a length that does not fit bits_for(window) bits.  bound: lzss_sw_bound (0: this kind or window is not taken).
struct LzssSwStats { u64 factors = 0; u32 flen_max = 0; bool truncates = false; };
size_t lzss_sw_encode_tokens(Ctx& c, const u8* d_text, const u32* tokpos, const u32* fac, size_t ntok, u32 window, int kind,
                             u8* d_out, size_t out_cap, LzssSwStats* st);
size_t lzss_sw_bound(size_t n, u32 window, int kind);
// :120-143 -- streams of BitCoder (kind 0), EliasGammaCoder (1) and EliasDeltaCoder (2) parsed and resolved on the device
// (lzss_sw_decode.hip); false: this stream keeps the host loop (option dec_parse, or more tokens than 32-bit indices count), nothing has
// been written.  *n_out: the text length; *need (nullable) receives it as soon as it is known -- also when out.into is too small
// (HipError hipErrorOutOfMemory).  Malformed input: StreamFormatError; a text of more than 2^32 - 2 bytes: DecodeTooLarge.
bool decode_lzss_sw(Ctx& c, const u8* stream, size_t len, int kind, u32 window, Sink& out, size_t* need, DecodeStats* st, size_t* n_out);
// the host loop behind tdc_lzss_sw_decode (lzss_sw_host.cpp): a status of tdc_gpu.h, the text
int lzss_sw_decode_host(const u8* in, size_t len, int coder, u32 window, std::vector<u8>& text);

// ---- lzss over a batch of independent texts (lzss_sw_batch.hip, DESIGN.md section 5.7 "Batches") -------------------------------------------
// The texts lie back to back on the device, off[0 .. count] are their borders.  The caller provides the per-text arrays (24 bytes per
// text); lzss_sw_batch_sizes fills the rest from the arena, where it stays valid until the caller releases its mark.
struct LzssSwBatch {
    const u32* off = nullptr;     // count + 1: text k = [off[k], off[k + 1])
    u64* gfirst = nullptr;        // count + 1: the bit of text k's first token in the concatenated token stream; [count]: all bits
    u64* ooff = nullptr;          // count + 1: the byte of stream k in the output, a multiple of 8; [count]: the bytes used
    u32* flag = nullptr;          // count: 1 = BitCoder would truncate a length of this text; it takes no bytes of the output
    size_t ntok = 0; u64 factors = 0;
    const u32* tokpos = nullptr, *fac = nullptr; const u64* gpos = nullptr;
};
// match, parse, costs and the two scans: everything the output's size depends on (count >= 1; synchronises: token count, factor count)
void lzss_sw_batch_sizes(Ctx& c, const u8* d_text, size_t n, size_t count, u32 window, u32 threshold, int kind, LzssSwBatch& B);
// zeroes d_out[0, used), used = ooff[count], packs every token at its bit of its stream and writes the terminators; enqueued only
void lzss_sw_batch_pack(Ctx& c, const u8* d_text, size_t count, u32 window, int kind, const LzssSwBatch& B, u8* d_out, size_t used);
// Streams of kind 0 = BitCoder, 1 = EliasGammaCoder, 2 = EliasDeltaCoder, one wave per stream.  Stream k = blob[s_off[k] - sub, + s_len[k]),
// the blob 4-byte aligned and padded with 64 zero bytes.  _sizes: tlen[k], status[k] (a status of tdc_gpu.h: what tdc_lzss_sw_decode
// says of the stream), ooff[0 .. count] (the scan of tlen) and *factors; _write: the accepted texts into d_text + ooff[k].  Enqueued only.
struct LzssSwBatchDec {
    const u8* blob = nullptr; u64 sub = 0;
    const u64* s_off = nullptr, *s_len = nullptr;
    u32* tlen = nullptr; int* status = nullptr; u64* ooff = nullptr; u64* factors = nullptr;
};
void lzss_sw_batch_decode_sizes(Ctx& c, int kind, u32 window, size_t count, LzssSwBatchDec& D);
void lzss_sw_batch_decode_write(Ctx& c, int kind, u32 window, size_t count, const LzssSwBatchDec& D, u8* d_text);

// ---- lzw / lz78 streams in a batch (lz_batch_decode.hip, DESIGN.md section 5.4 "Batch decoder") ----------------------------------------------
// Stream k = blob[s_off[k] - sub, + s_len[k]), the blob 4-byte aligned and padded with 64 zero bytes.  The items of all streams lie back
// to back (stream k: item_off[k] .. item_off[k + 1]) with their links rebased to global item indices: one forest, whose text is the
// texts back to back.  The caller provides every array; all three functions only enqueue, but for the pointer-jumping rounds of _sizes.
struct LzBatchDec {
    const u8* blob = nullptr; u64 sub = 0;
    const u64* s_off = nullptr, *s_len = nullptr;
    u64* bits = nullptr;          // count: the payload bits of stream k
    int* status = nullptr;        // count: a status of tdc_gpu.h
    u64* item_off = nullptr;      // count + 1: the item counts, then their scan; [count]: all items
    u64* ooff = nullptr;          // count + 1: the scan of the accepted text lengths
    u64* factors = nullptr;       // 1: the items of the accepted streams
};
// The items of one batch (z = item_off[count] of them).  ids / chars / owner / J / S (z + 1) are scratch of the length stages; fpos, fsrc,
// flen and lit are what the text is made of: the factor list for resolve_and_download and the literal of every item.
struct LzBatchItems {
    size_t z = 0;
    u32* ids = nullptr; u8* chars = nullptr; u32* owner = nullptr; u64* J = nullptr, *S = nullptr;
    u32* fpos = nullptr, *fsrc = nullptr, *flen = nullptr; u8* lit = nullptr;
};
// bits, the verdicts that need no item (a cut-off terminator; bit: a cut-off code), the item count of every stream -- bit: from the closed
// form, gamma: by the first walk, one wave per stream -- and item_off
void lz_batch_decode_count(Ctx& c, bool lzw, bool bit, size_t count, LzBatchDec& D);
// the items at item_off[k] + j, links rebased (bit: one thread per code of the batch; gamma: the second walk); lengths, starts, the
// per-stream sums and verdicts, ooff, *factors, and the factor list.  z >= 1.  Returns the pointer-jumping rounds.
u32 lz_batch_decode_sizes(Ctx& c, bool lzw, bool bit, size_t count, LzBatchDec& D, LzBatchItems& I, u32* d_changed);
// the literals of the accepted streams at their text positions
void lz_batch_decode_literals(Ctx& c, bool lzw, const LzBatchItems& I, u8* d_text);

// ---- repair (compressors/RePairCompressor.hpp; repair.hip, repair_host.cpp) ------------------------------------------
constexpr size_t REPAIR_MAX_N = (size_t)1 << 30;
// ms_first / ms_last / ms_tie: the first round, the last one and the sum over the tie rounds, on the host clock from one round's read-back
// to the next one's
struct RepairStats { u64 rules = 0, replaced = 0; u32 tie_rounds = 0, rebuilds = 0, rounds = 0; size_t nstart = 0; float ms_first = 0, ms_last = 0, ms_tie = 0; };
// :96-178 on the device: the rules (l << 32 | r, rule k stands for symbol 256 + k) and the start sequence, taken from the arena and valid
// until the caller releases its mark.  max_rules 0: unlimited.  n <= REPAIR_MAX_N.  What the arena has to hold: repair_arena(n, max_rules,
// table_bits) -- checked by the caller before anything is written.
void repair_grammar(Ctx& c, const u8* d_text, size_t n, u64 max_rules, u64** d_rules, u32** d_start, RepairStats* st);
size_t repair_arena(const Ctx& c, size_t n, u64 max_rules);
// :208-263 -- the grammar through one coder (field_coder.hpp): kind 0 = BitCoder, 1 = ASCIICoder, 2 = EliasGammaCoder, 3 = EliasDeltaCoder.
// Writes the stream, terminator included, to d_out and returns its length.  bound: repair_bound (0: this kind is not taken).
size_t repair_encode(Ctx& c, const u64* d_rules, size_t nrules, const u32* d_start, size_t nstart, int kind, u8* d_out, size_t out_cap);
size_t repair_bound(size_t n, int kind);
// :287-336 on the device (repair_decode.hip): kind 0 = BitCoder, 1 = EliasGammaCoder, 2 = EliasDeltaCoder.  True: the text is in `out`.
// False: this stream keeps the host loop (option dec_parse, a grammar deeper than option repair_dec_rounds, a field beyond the device's
// caps, more items than 32-bit indices count), nothing has been written.  *need, *n_out, what it throws: as decode_lzss_sw.
// ms_h2d: the upload; ms_grammar: parse, lengths, positions, first occurrences; ms_text: items, reference resolver and download (host
// clock around synchronisations).
struct RepairDecodeStats { DecodeStats dec; u64 rules = 0, nstart = 0; u32 segments = 0, len_rounds = 0, first_rounds = 0; float ms_h2d = 0, ms_grammar = 0, ms_text = 0; };
bool decode_repair(Ctx& c, const u8* stream, size_t len, int kind, Sink& out, size_t* need, RepairDecodeStats* st, size_t* n_out);
// ---- repair streams in a batch (repair_batch_decode.hip, DESIGN.md section 5.8 "Batch decoder") ------------------------------------------
// Stream k = blob[s_off[k] - sub, + s_len[k]), the blob 4-byte aligned and padded with 64 zero bytes; kind as decode_repair.  The rules of
// all streams lie back to back (stream k: rule_off[k] .. rule_off[k + 1]) with their references rebased to global rule indices, the start
// sequences likewise behind them: one forest, whose text is the texts back to back.  The caller provides every array.
struct RepairBatchDec {
    const u8* blob = nullptr; u64 sub = 0;
    const u64* s_off = nullptr, *s_len = nullptr;
    u64* bits = nullptr;          // count: the payload bits of stream k; behind _sizes: the scan of all start symbols at its first one
    int* status = nullptr;        // count: a status of tdc_gpu.h
    u64* rule_off = nullptr;      // count + 1: the rule counts, then their scan; [count]: all rules
    u64* start_off = nullptr;     // count + 1: the same for the start symbols
    u64* ooff = nullptr;          // count + 1: the scan of the accepted text lengths
    u64* rules = nullptr;         // 1: the rules of the accepted streams
};
// The forest: R = rule_off[count] rules, M = start_off[count] start symbols.  sym (2 R + M): the sides of rule k at 2 k and 2 k + 1, start
// symbol j at 2 R + j; len, len2, first: R + 1 entries each (entry R is the rule `nothing`, of length 0; len2 is the second buffer of the
// length rounds and dead behind _sizes); pos: M + 1, the text position of every start symbol, [M] the scan's total.
struct RepairBatchGrammar {
    size_t R = 0, M = 0;
    u32* sym = nullptr, *len = nullptr, *len2 = nullptr, *first = nullptr; u64* pos = nullptr;
};
// bits, the first walk (one wave per stream: R_k, m_k and the verdict), rule_off and start_off; enqueued only
void repair_batch_decode_count(Ctx& c, int kind, size_t count, RepairBatchDec& D);
// The second walk (the symbols, rebased), the lengths in at most `cap` strict rounds -- a stream that owns a rule higher than cap is
// TDC_GPU_ERR_UNSUPPORTED --, positions, the per-stream sizes and verdicts, ooff and *rules; the start symbols of refused streams become
// `nothing`.  2 R + M >= 1.  d_flags: 8 words.  Returns the length rounds that ran up to the quiet one; it synchronises once per 8 rounds.
u32 repair_batch_decode_sizes(Ctx& c, int kind, size_t count, RepairBatchDec& D, RepairBatchGrammar& G, u32 cap, u32* d_flags);
// first occurrences at the global positions, seeded from the start symbols; the rounds that ran, 0: `cap` rounds did not come to rest
u32 repair_batch_decode_first(Ctx& c, const RepairBatchGrammar& G, u32 cap, u32* d_flags);
// the literals to d_text (n + 64 bytes), cls / fidx (2 R + M entries each): the items that are factors; returns their number (synchronises)
size_t repair_batch_decode_items(Ctx& c, const RepairBatchGrammar& G, size_t n, u8* d_text, u8* cls, u32* fidx, u32* d_cnt);
// the factor list for resolve_and_download (zf + 1 entries each)
void repair_batch_decode_factors(Ctx& c, const RepairBatchGrammar& G, const u32* fidx, size_t zf, u32* fpos, u32* fsrc, u32* flen);

// ---- bwt (compressors/BWTCompressor.hpp, ds/bwt.hpp; bwt.hip) ---------------------------------------------
// forward: d_out[i] = T[SA[i] - 1] (T[n - 1] where SA[i] = 0), i < n; d_out holds n + 64 bytes.  host_dst (nullable): where the transform
// goes afterwards.  True: it is on its way there already, chunk by chunk on the copy stream behind the gather (page-locked memory, texts
// of 128 MiB and more), and c.stream waits for the last copy; false: the caller downloads d_out.
bool bwt_gather(Ctx& c, const u8* d_text, const u32* d_sa, size_t n, u8* d_out, u8* host_dst);
// inverse (decode_bwt with the complete C table): LF by a stable counting rank, then list ranking of its one cycle from sampled heads.
// sample = expected rows per list, max_steps = most steps a walk takes per launch (0: BWT_SAMPLE, BWT_STEPS_PER_SAMPLE x sample).
// `bwt` is a host buffer; the text goes to decode_dest(out, len); host_lf (nullable, len entries) receives the LF table.  Inputs of at
// most one byte decode to nothing.  A buffer that is no transform (not exactly one 0 byte, LF not one cycle): StreamFormatError;
// len >= 2^31 - 1: DecodeTooLarge; out.into too small: HipError hipErrorOutOfMemory -- each before anything is written to `out`.
constexpr u32 BWT_SAMPLE = 256, BWT_STEPS_PER_SAMPLE = 4;
struct BwtInvStats { u64 heads = 0; u32 launches = 0, rounds = 0, longest = 0, sample = 0, max_steps = 0; };
// on_device: `bwt` lies in the arena already (256-byte aligned, 64 allocated bytes behind it) and stays where it is; the inverse takes
// what it needs from the room above the arena's current top (bwt_inverse_arena(len) bytes at most with the default sample).
size_t bwt_inverse_arena(size_t n);
size_t bwt_inverse(Ctx& c, const u8* bwt, size_t len, u32 sample, u32 max_steps, Sink& out, u32* host_lf, BwtInvStats* st, bool on_device = false);

}  // namespace tdc
