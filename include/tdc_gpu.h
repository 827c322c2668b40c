/*
 * tdc_gpu.h -- C ABI of the MI355X-native lcpcomp hot path (libtdc_gpu.so).
 *
 * This is the drop-in boundary for tudocomp's lcpcomp compressor: a tudocomp maintainer binds these entry
 * points from  tdc::LCPCompressor<HuffmanCoder, lcpcomp::ArraysComp, ...>::compress
 * (/root/reference/include/tudocomp/compressors/LCPCompressor.hpp:100-138); INTEGRATION.md shows the binding.
 * Plain pointers and sizes only; no C++/torch types; no exception crosses the boundary.
 *
 * Conventions
 *   - `text`/`n` is what Input::as_view() hands to compress(): already escaped, terminated by ONE 0 byte that
 *     occurs nowhere else (ds/SADivSufSort.hpp:20-25, ds/TextDS.hpp:132-138).  n < 2^31 (32-bit len_t, def.hpp:103).
 *   - every function returns 0 on success or a negative tdc_gpu_status; tdc_gpu_strerror() explains it.
 *   - host output buffers returned through `uint8_t** out` are malloc'd by the library: free with tdc_gpu_free().
 *   - a context owns three HIP streams (compute, copy, low-priority side work) and one device arena on one GPU; every call
 *     returns with all three streams idle.  A context is not thread-safe, use one per thread.
 *     Every call switches the calling thread to the context's device and restores the previous current device on return.
 *     The library NEVER falls back to a CPU path: without a usable GPU every compute call fails with TDC_GPU_ERR_HIP.
 */
#ifndef TDC_GPU_H
#define TDC_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    TDC_GPU_OK = 0,
    TDC_GPU_ERR_HIP = -1,          /* HIP runtime error (no device, launch failure, ...) */
    TDC_GPU_ERR_ARG = -2,          /* invalid argument (NULL pointer, threshold 0, extra 0 bytes in the text, ...) */
    TDC_GPU_ERR_NO_SENTINEL = -3,  /* text does not end with 0: reference throws std::logic_error (TextDS.hpp:132-138) */
    TDC_GPU_ERR_TOO_LARGE = -4,    /* n >= 2^31 */
    TDC_GPU_ERR_OOM = -5,          /* device or host memory exhausted */
    TDC_GPU_ERR_UNSUPPORTED = -6,  /* coder / strategy not available in this build */
    TDC_GPU_ERR_INTERNAL = -7      /* invariant violated */
} tdc_gpu_status;

/* coder ids (option `coder`, etc/registry_config.py:28-31,138-142) */
enum { TDC_GPU_CODER_HUFF = 0, TDC_GPU_CODER_GAMMA = 1, TDC_GPU_CODER_ARITH = 2, TDC_GPU_CODER_ASCII = 3, TDC_GPU_CODER_SLE = 4,
       TDC_GPU_CODER_BIT = 5 /* BitCoder: lzw, lzss_lcp, lzss, repair */, TDC_GPU_CODER_DELTA = 6 /* EliasDeltaCoder: lzss_lcp, lzss, repair */ };
/* coder=sle(kmer=K) (coders/SLECoder.hpp:36-40; the reference's default is 3): the option travels in bits 8.. of `coder` */
#define TDC_GPU_CODER_SLE_K(K) (TDC_GPU_CODER_SLE | ((K) << 8))
/* factorization strategy of lcpcomp (option `comp`, LCPCompressor.hpp:87): ArraysComp or PLCPPeaksStrategy */
enum { TDC_GPU_COMP_ARRAYS = 0, TDC_GPU_COMP_PLCPPEAKS = 1, TDC_GPU_COMP_MAXLCP = 2, TDC_GPU_COMP_HEAP = 3 };

typedef struct tdc_gpu_ctx tdc_gpu_ctx;

/* Replaces the StatPhase log of LCPCompressor::compress (same keys: LCPCompressor.hpp:117-118, ArraysComp.hpp:43,60,
 * LZSSFactors.hpp:130-131) plus device timings per phase in milliseconds (hipEvent). */
typedef struct {
    uint64_t n;                 /* text length incl. sentinel                                  */
    uint64_t out_len;           /* compressed bytes                                            */
    uint64_t factors;           /* "factors"                                                   */
    uint64_t maxlcp;            /* "maxlcp"                                                    */
    uint64_t entries;           /* "entries" (initial candidates)                              */
    uint64_t num_flattened;     /* "num_flattened"                                             */
    uint64_t max_depth_lb;      /* "max_depth_lb"                                              */
    uint64_t flen_min, flen_max, fdist_max;
    uint64_t pushes;            /* lazily pushed-down candidates                               */
    uint32_t sa_rounds;         /* prefix-doubling rounds (incl. the initial sort)             */
    uint32_t sa_init_syms;      /* symbols packed into the initial sort key                    */
    uint32_t levels;            /* non-empty LCP levels processed                              */
    uint32_t mis_rounds;        /* selection rounds over all levels                            */
    uint32_t flatten_rounds;
    uint32_t sigma;             /* literal alphabet size                                       */
    uint64_t sa_sorted_elems;   /* total elements that went through the radix sort during SA   */
    uint64_t arena_bytes;       /* device memory high-water mark                               */
    float ms_h2d, ms_sa, ms_phi, ms_plcp, ms_factorize, ms_flatten, ms_encode, ms_d2h, ms_total;
    uint32_t small_levels;      /* levels processed by the one-workgroup kernel                 */
    uint32_t purges;            /* bulk removals of erased candidates                           */
    uint32_t window_pass;       /* low levels window-local in one launch: 0 not used, 1 done, 2 fell back to the level loop */
    uint32_t window_lcut;       /* highest level handed to the (last) window pass                */
    uint32_t sa_key_words;      /* 64-bit words of the initial suffix-sort key (0: classic path, 1 | 2: wide bit-packed keys) */
    uint32_t sa_text_rounds;    /* rank-free refinement rounds keyed from the text (wide path)     */
    uint32_t sa_mode;           /* 1: ISA / Phi / PLCP came from the fused scatter of the final suffix array, 0: classic */
    uint32_t sa_overlapped;     /* 1: the first partition level of the suffix sort ran chunk by chunk behind the upload */
    uint32_t eager_levels;      /* levels processed inside one-launch runs of small levels (factorize_eager.hip)           */
    uint32_t eager_phases;      /* such runs                                                                            */
    uint32_t sa_star_chains;    /* chains of the star step of the suffix array's doubling fall-back (0: the step was not taken) */
    uint32_t probes;            /* skip-ahead probes over runs of erased levels (arrays, max_lcp)                              */
    uint32_t max_push_targets;  /* most target levels the pushes of one level went to (arrays, max_lcp)                        */
    uint64_t d2h_early;         /* tdc_gpu_lcpcomp_compress_into: stream bytes copied to `out` while the pack still ran            */
    uint32_t pipe_stages;       /* tdc_gpu_pipeline_compress: number of stages, ...                                                 */
    uint32_t pipe_dev;          /* tdc_gpu_pipeline_decompress_stats: bit i = stage i was decoded (bwt: inverted) on the device      */
    uint64_t pipe_len[8];       /* ... the length in bytes behind stage i, ...                                                      */
    float    pipe_ms[8];        /* ... and what stage i took (host clock around a synchronisation; only with option pipe_log)       */
    uint32_t ranges_early;      /* tdc_gpu_lcpcomp_compress_into: rank ranges of the flatten stage whose pack was enqueued before the stage returned (flatten_chunks) */
    uint32_t len_rounds;        /* tdc_gpu_repair_decompress_stats: rounds of the length pass over the rules                          */
    uint64_t rules;             /* tdc_gpu_repair_*: "rules" (RePairCompressor.hpp:204), ...                                          */
    uint64_t replaced;          /* ... "replaced" (:205): pairs replaced over all rounds, ...                                        */
    uint32_t tie_rounds;        /* ... rounds in which more than one pair held the largest count, ...                               */
    uint32_t rebuilds;          /* ... and how often the digram table was rebuilt by a recount of the live sequence                   */
    float ms_round_first, ms_round_last, ms_round_tie;   /* repair: the first round, the last one, the sum over the tie rounds (host clock, read-back to read-back) */
    float reserved1;
} tdc_gpu_stats;

/* ---- context -------------------------------------------------------------------------------------------- */
int  tdc_gpu_ctx_create(int device, tdc_gpu_ctx** ctx);
void tdc_gpu_ctx_destroy(tdc_gpu_ctx* ctx);
/* Options (round 6).  The library's defaults are the product; every switch that tests, A/B measurements and diagnostics need is an
 * option of the context, set through this function and through nothing else: the library does not read TDC_GPU_* environment variables
 * (an embedding process cannot change the algorithm by accident) -- unless TDC_GPU_DEBUG_KNOBS=1 is set, in which case
 * tdc_gpu_ctx_create() applies every TDC_GPU_<OPTION NAME IN UPPER CASE> variable through this same function (development aid,
 * tools/ab.sh).  `name`: an option name (README.md lists them; "wsort_min" and "TDC_GPU_WSORT_MIN" are the same option); out-of-range
 * values are clamped.  TDC_GPU_ERR_ARG for an unknown name.  tdc_gpu_option_count / _name enumerate the table -- all of it but
 * the switches of folded passes (fused_cand, sel_tile_counts: README.md) and flatten_chunks (the flatten stage in rank ranges, with pack
 * and download behind each range: README.md), which this function accepts like any other. */
int tdc_gpu_ctx_set_option(tdc_gpu_ctx* ctx, const char* name, long value);
int tdc_gpu_option_count(void);
const char* tdc_gpu_option_name(int i);
/* Pre-size the device arena for texts up to n bytes (optional; otherwise grown on demand). */
int  tdc_gpu_ctx_reserve(tdc_gpu_ctx* ctx, size_t n);
/* Device memory a context holds while it works on a text of n bytes (its arena; 112 bytes per text byte + 192 MiB), and what the
 * device has: callers that place several contexts on one device (block mode, one process per GPU next to RCCL buffers) size
 * their shards with it.  A call whose arena does not fit fails with TDC_GPU_ERR_OOM and a message that names both numbers. */
size_t tdc_gpu_arena_bytes(size_t n);
int  tdc_gpu_device_memory(int device, size_t* free_bytes, size_t* total_bytes);
/* Live kernel timing for bench.py's roofline: when enabled, HIP events are recorded (on the launching stream) around
 * every launch of the instrumented kernels; tdc_gpu_ctx_kernel_profile() returns the sums since the last reset.
 * idx enumerates the instrumented kernel classes from 0; the function returns the class name, or NULL once idx is
 * out of range. `bytes` = algorithmic bytes summed over the launches. */
int  tdc_gpu_ctx_set_profiling(tdc_gpu_ctx* ctx, int enabled);
void tdc_gpu_ctx_reset_profile(tdc_gpu_ctx* ctx);
const char* tdc_gpu_ctx_kernel_profile(const tdc_gpu_ctx* ctx, int idx, double* ms, uint64_t* launches, uint64_t* bytes);
const char* tdc_gpu_strerror(int status);
/* Human-readable detail of the last failure on this context ("" if none). */
const char* tdc_gpu_last_error(const tdc_gpu_ctx* ctx);
void tdc_gpu_free(void* p);

/* ---- the hot path: replaces LCPCompressor::compress (LCPCompressor.hpp:100-138) --------------------------- */
/* Host buffers in, host buffer out (H2D + all kernels + D2H).  threshold/flatten = the dynamic options of the
 * same name (LCPCompressor.hpp:92-93, defaults 5 and 1).  `stats` may be NULL.
 * coder: TDC_GPU_CODER_HUFF (HuffmanCoder) or TDC_GPU_CODER_ARITH (ArithmeticCoder, coders/ArithmeticCoder.hpp:35-177 --
 * compress side only: the reference itself cannot decode lcpcomp + arithmetic; returns
 * TDC_GPU_ERR_UNSUPPORTED for inputs on which the reference divides by zero), TDC_GPU_CODER_ASCII (ASCIICoder) or
 * TDC_GPU_CODER_SLE / TDC_GPU_CODER_SLE_K(k) (SLECoder, the coder of the reference's published lcpcomp runs,
 * etc/compare-suites/default.suite:5; k in 1..7 = the reference's max_kmer, SLECoder.hpp:12). */
int tdc_gpu_lcpcomp_compress(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint32_t threshold, int flatten,
                             int coder, uint8_t** out, size_t* out_len, tdc_gpu_stats* stats);
/* The same with a selectable factorization strategy: comp = TDC_GPU_COMP_ARRAYS (lcpcomp::ArraysComp, the default of the
 * entry point above) or TDC_GPU_COMP_PLCPPEAKS (lcpcomp::PLCPPeaksStrategy, compressors/lcpcomp/compress/PLCPPeaksStrategy.hpp:36-80:
 * strict local maxima of the PLCP array, one left-to-right scan) or TDC_GPU_COMP_MAXLCP (lcpcomp::MaxLCPStrategy,
 * compressors/lcpcomp/compress/MaxLCPStrategy.hpp:36-100: the same greedy rule as ArraysComp with the tie order of its
 * per-level stacks and eager key decreases) or TDC_GPU_COMP_HEAP (lcpcomp::MaxHeapStrategy, MaxHeapStrategy.hpp:36-101 over
 * ds/ArrayMaxHeap.hpp: the strategy of the reference's published heap run; its tie order is the layout history of a binary
 * heap, so the device replays the reference's loop with ONE thread -- a parity row, about a minute per MiB of text). */
int tdc_gpu_lcpcomp_compress_comp(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint32_t threshold, int flatten, int coder,
                                  int comp, uint8_t** out, size_t* out_len, tdc_gpu_stats* stats);

/* The metric's entry point (pinned host text -> compressed bytes in host memory): the same as
 * tdc_gpu_lcpcomp_compress_comp, but the stream is written into the CALLER's buffer `out` of out_cap bytes (no allocation
 * in the call).  *out_len receives the stream length; if it exceeds out_cap the call fails with TDC_GPU_ERR_OOM and *out_len
 * holds the required size.  `text` and `out` should be pinned host memory (tdc_gpu_host_alloc, or hipHostMalloc /
 * hipHostRegister by the embedding program): the two transfers then run at PCIe rate; pageable memory works but is staged
 * by the runtime.  stats->ms_h2d / ms_d2h / ms_total cover the transfers. */
int tdc_gpu_lcpcomp_compress_into(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint32_t threshold, int flatten, int coder,
                                  int comp, uint8_t* out, size_t out_cap, size_t* out_len, tdc_gpu_stats* stats);
/* One process per GPU, one container per node (SURVEY.md 8e replaces nothing of the reference: its 32-bit len_t has
 * no block mode).  tdc_gpu_lcpcomp_compress_keep is tdc_gpu_lcpcomp_compress_into without the download: the stream STAYS on the
 * device inside the context until the next call on it, *out_len receives its length.  Once the ranks have exchanged their lengths,
 * tdc_gpu_stream_fetch copies the kept stream to `dst` -- this rank's offset in a container that all ranks map, e.g. a POSIX
 * shared-memory segment page-locked with tdc_gpu_host_register -- so every shard travels over its own GPU's host link instead of
 * all of them through rank 0.  tdc_gpu_stream_fetch: *len (nullable) receives the stream length; TDC_GPU_ERR_OOM if cap is smaller. */
int tdc_gpu_lcpcomp_compress_keep(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint32_t threshold, int flatten, int coder,
                                  int comp, size_t* out_len, tdc_gpu_stats* stats);
int tdc_gpu_stream_fetch(tdc_gpu_ctx* ctx, uint8_t* dst, size_t cap, size_t* len);
/* The same with a DEVICE destination on the context's GPU (e.g. the send buffer of an RCCL gather of the per-block streams to one
 * rank, SURVEY.md 8e "Collective"): a device-to-device copy on the context's stream, synchronised before the call returns. */
int tdc_gpu_stream_fetch_dev(tdc_gpu_ctx* ctx, void* d_dst, size_t cap, size_t* len);
/* Page-lock / release host memory the embedding program allocated itself (hipHostRegister): transfers then run at PCIe rate. */
int tdc_gpu_host_register(void* p, size_t bytes);
int tdc_gpu_host_unregister(void* p);
/* Pinned (page-locked) host memory for the buffers above; NULL on failure.  Free with tdc_gpu_host_free. */
void* tdc_gpu_host_alloc(size_t bytes);
void  tdc_gpu_host_free(void* p);

/* Raw input variant: `data`/`n` is the UNRESTRICTED input (any bytes, no sentinel).  The library applies the
 * compressor's input restrictions on the device -- escape {0} + null-terminate, i.e. what Input(inp, restrictions) does
 * in tudocomp_driver.cpp:268-270 (io/RestrictedBuffer.hpp:43-74) -- and then compresses.  The escaped text (n + number of
 * 0x00 / 0xFF bytes + 1) must stay below 2^31 - 1 bytes. */
int tdc_gpu_lcpcomp_compress_raw(tdc_gpu_ctx* ctx, const uint8_t* data, size_t n, uint32_t threshold, int flatten,
                                 int coder, uint8_t** out, size_t* out_len, tdc_gpu_stats* stats);
/* Device-resident variant: d_text and d_out are device pointers on ctx's GPU (d_out 8-byte aligned, capacity out_cap
 * bytes; tdc_gpu_lcpcomp_bound_coder(n, coder) always suffices -- tdc_gpu_lcpcomp_bound(n) is that bound for huff and
 * arithmetic; ascii needs twice as much).  The call runs on the context's own stream: the caller must have finished
 * (synchronised) whatever produced d_text before calling, and the stream is synchronised before the call returns. */
int tdc_gpu_lcpcomp_compress_dev(tdc_gpu_ctx* ctx, const void* d_text, size_t n, uint32_t threshold, int flatten,
                                 int coder, void* d_out, size_t out_cap, size_t* out_len, tdc_gpu_stats* stats);
size_t tdc_gpu_lcpcomp_bound(size_t n);
size_t tdc_gpu_lcpcomp_bound_coder(size_t n, int coder);     /* 0 for an unknown coder */

/* ---- block mode (north_star: inputs above one-GPU size shard into independent blocks; BASELINE.json configs[4]) ----
 * `data`/`n` is the UNRESTRICTED input.  It is cut into ceil(n / block_size) blocks of block_size bytes (the last one shorter;
 * block_size < 2^31 - 2 and small enough that the ESCAPED block stays below 2^31 - 1 bytes); block k is compressed exactly like
 * tdc_gpu_lcpcomp_compress_raw(data + k * block_size, ...) -- own escaping + sentinel, own suffix array, factors and Huffman
 * table -- on one of the `ndev` devices listed in `devices` (one host thread and one context per device, blocks handed out
 * from a shared counter).  *out (malloc'd, tdc_gpu_free) receives the container
 *     "tdcgpu-blocks%" | u32 G | G x { u64 raw_len, u64 comp_len } | payload_0 | ... | payload_{G-1}      (little endian)
 * whose payloads are byte-identical to the single-block streams.  per_block (nullable): G stats records.
 * The reference has no counterpart (32-bit len_t: an input is at most 2^31 - 1 bytes, def.hpp:103). */
size_t tdc_gpu_blocks_count(size_t n, size_t block_size);
int tdc_gpu_blocks_compress(const int* devices, int ndev, const uint8_t* data, size_t n, size_t block_size, uint32_t threshold,
                            int flatten, int coder, uint8_t** out, size_t* out_len, tdc_gpu_stats* per_block);
/* Inverse: every payload through tdc_gpu_lcpcomp_decompress_coder on ctx's device, restrictions removed (unescape, sentinel
 * dropped), blocks concatenated.  A malformed container: TDC_GPU_ERR_ARG. */
int tdc_gpu_blocks_decompress(tdc_gpu_ctx* ctx, const uint8_t* container, size_t len, int coder, uint8_t** out, size_t* out_len);
/* number of visible devices (0 if none / no runtime) */
int tdc_gpu_device_count(void);

/* ---- LZ78 (BASELINE.json configs[3]): replaces LZ78Compressor<EliasGammaCoder, ...>::compress
 * (compressors/LZ78Compressor.hpp:64-140).  No input restrictions (no escaping, no sentinel).  The parse is sequential
 * and runs on the host; the Elias-gamma stream is packed on the GPU.  coder must be TDC_GPU_CODER_GAMMA.
 * stats (may be NULL): n, out_len, factors (= number of phrases) and ms_encode / ms_total are filled. */
int tdc_gpu_lz78_compress(tdc_gpu_ctx* ctx, const uint8_t* in, size_t n, int coder, uint8_t** out, size_t* out_len,
                          tdc_gpu_stats* stats);

/* ---- lzss_lcp (SURVEY.md 8a row a18 / 8f "next" #1): replaces LZSSLCPCompressor<coder>::compress
 * (compressors/LZSSLCPCompressor.hpp:41-123): greedy LZ77 parse via previous / next smaller values of the suffix array.
 * Same text contract as lcpcomp (escaped, 0-terminated); option threshold (default 3, :30).
 * coder: the reference's non-consuming coders (etc/registry_config.py:33-34) -- TDC_GPU_CODER_HUFF, TDC_GPU_CODER_BIT (BitCoder: every
 * field v - min in bits_for(max - min) bits, a literal in 8), TDC_GPU_CODER_GAMMA / TDC_GPU_CODER_DELTA (every field and every literal
 * as a self-delimiting code, the ranges ignored) or TDC_GPU_CODER_ASCII; anything else: TDC_GPU_ERR_UNSUPPORTED.  DESIGN.md 5.5. */
int tdc_gpu_lzss_lcp_compress(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint32_t threshold, int coder,
                              uint8_t** out, size_t* out_len, tdc_gpu_stats* stats);
/* The same into the CALLER's buffer of out_cap bytes; TDC_GPU_ERR_OOM with the required size in *out_len if it is too small. */
int tdc_gpu_lzss_lcp_compress_into(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint32_t threshold, int coder,
                                   uint8_t* out, size_t out_cap, size_t* out_len, tdc_gpu_stats* stats);
/* worst-case stream length for a text of n bytes (what an _into buffer needs at most, and what the call sizes its device buffer by);
 * 0 for a coder lzss_lcp does not take */
size_t tdc_gpu_lzss_lcp_bound(size_t n, int coder);
/* LZSSLCPCompressor::decompress (:125-130) for a stream of one of the five coders.  huff: tdc_gpu_lcpcomp_decompress_coder.  bit, gamma,
 * delta: streams of 1 MiB and more whose longest literal run is at most 512 are parsed ON THE DEVICE (option dec_parse = 2: every
 * stream, 0: never; dec_lean, dec_seg as for lcpcomp), the others by the host loop tdc_lzss_decode restates; ascii: host parse,
 * references resolved on the device.  tdc_gpu_ctx_last_decode_on_device tells which.  Malformed input: TDC_GPU_ERR_ARG.  _into:
 * TDC_GPU_ERR_OOM if the text does not fit the caller's buffer. */
int tdc_gpu_lzss_lcp_decompress(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint8_t** out, size_t* out_len,
                                uint64_t* factors, uint32_t* rounds);
int tdc_gpu_lzss_lcp_decompress_into(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint8_t* out, size_t out_cap,
                                     size_t* out_len, uint64_t* factors, uint32_t* rounds);
/* the factor list of LZSSLCPCompressor.hpp:60-115 (sorted by pos), three malloc'd arrays */
int tdc_gpu_lzss_lcp_factorize(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint32_t threshold,
                               uint32_t** pos, uint32_t** src, uint32_t** len, size_t* z);

/* ---- stage-level entry points (host buffers), used by the parity tests ------------------------------------ */
/* the device sorts behind the suffix array (no reference counterpart; for the tests): sorts n (key, value) pairs in place by
 * the 64-bit key; algo 0 = stable 8-bit LSD radix sort, 1 = splitter-partition sort (unstable) */
int tdc_gpu_sort_pairs_u64(tdc_gpu_ctx* ctx, uint64_t* keys, uint32_t* vals, size_t n, int algo);
/* ds/SADivSufSort.hpp:27-51 + ds/ISAFromSA.hpp:30-43 : sa / isa may be NULL */
int tdc_gpu_suffix_array(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint32_t* sa, uint32_t* isa);
/* TextDS::require(SA|ISA|PHI|PLCP|LCP) (ds/TextDS.hpp:247-292); any output may be NULL; plcp[n-1] = 0 */
int tdc_gpu_textds(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint32_t* sa, uint32_t* isa, uint32_t* phi,
                   uint32_t* plcp, uint32_t* lcp, uint32_t* maxlcp);
/* ArraysComp::factorize + FactorBuffer::sort (+ flatten if requested): factors sorted by pos in three malloc'd arrays */
int tdc_gpu_lcpcomp_factorize(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint32_t threshold, int flatten,
                              uint32_t** pos, uint32_t** src, uint32_t** len, size_t* z, tdc_gpu_stats* stats);
/* FactorBuffer::flatten on a caller-supplied factor list sorted by pos (LZSSFactors.hpp:79-132); src rewritten in place */
int tdc_gpu_flatten(tdc_gpu_ctx* ctx, size_t n, const uint32_t* pos, uint32_t* src, const uint32_t* len, size_t z,
                    uint64_t* num_flattened, uint64_t* max_depth_lb);
/* ---- the shared device primitives (csrc/prim.hpp) one by one, for tests/test_gpu_prims.py; no reference counterpart.  Host buffers in
 * and out.  Every precondition of a primitive is checked on the host first: TDC_GPU_ERR_ARG, and nothing is launched. ---- */
/* op 0: exclusive_sum_u32, 1: exclusive_sum_u64, 2: inclusive_max_u32 over the n words (4 / 8 / 4 bytes each) of `data`, which the result
 * replaces.  in_place != 0: in == out on the device as well, else two buffers.  total (NULL: the primitive gets a null d_total; op 2
 * has none): one word that receives the grand total. */
int tdc_gpu_prim_scan(tdc_gpu_ctx* ctx, int op, void* data, size_t n, int in_place, void* total);
/* kind 0: radix_sort_pairs_u32, 1: radix_sort_pairs_u64 (stable), 2: sort_pairs_u64_distinct (keys pairwise distinct on the sorted
 * bits), on bits [begin_bit, end_bit) of the keys (4 / 8 / 8 bytes each); end_bit <= 32 / 64 / 64.  keys / vals are replaced by the
 * contents of the buffer pair the primitive names. */
int tdc_gpu_prim_sort_pairs(tdc_gpu_ctx* ctx, int kind, void* keys, uint32_t* vals, size_t n, int begin_bit, int end_bit);
/* bucketed_scatter_u32: dst (n_dst words, every one `fill` beforehand) with dst[idx[j]] = val[j], j < m; idx pairwise distinct and
 * < n_dst.  permutation != 0: idx holds every index of [0, m) once and m is n_dst or n_dst - 1.  second_tmp = 0: without the second
 * pair of temporaries.  offset (0 or 1): idx / val start that many elements behind an aligned device address. */
int tdc_gpu_prim_bucketed_scatter(tdc_gpu_ctx* ctx, const uint32_t* idx, const uint32_t* val, size_t m, uint32_t* dst, size_t n_dst,
                                  uint32_t fill, int permutation, int second_tmp, int offset);
/* msd_partition_pairs_u32: the m pairs grouped by idx >> (bits - 2 * db), in place; db 8 or 9, 2 * db < bits <= 32, idx < 2^bits */
int tdc_gpu_prim_msd_partition(tdc_gpu_ctx* ctx, uint32_t* idx, uint32_t* val, size_t m, int bits, int db);
/* select_by_class: outA (m words, every one fillA beforehand) / outB (m words of fillB; NULL iff srcB is NULL) receive the selected
 * elements of srcA (NULL: their indices) / srcB in order, *count their number */
int tdc_gpu_prim_select(tdc_gpu_ctx* ctx, const uint8_t* cls, uint8_t want, size_t m, const uint32_t* srcA, const uint64_t* srcB,
                        uint32_t fillA, uint64_t fillB, uint32_t* outA, uint64_t* outB, uint32_t* count);
/* select_by_class with the per-tile counts handed in (tile_counts[t] = number of cls[k] == want, 2048 t <= k < 2048 (t + 1); anything
 * else is refused): outA as above */
int tdc_gpu_prim_select_counts(tdc_gpu_ctx* ctx, const uint8_t* cls, uint8_t want, size_t m, const uint32_t* srcA, const uint32_t* tile_counts,
                               uint32_t fillA, uint32_t* outA, uint32_t* count);
/* mark_orbit_u32: mark[i] = 1 on the chain 0, next[0], next[next[0]], ... and 0 elsewhere; i < next[i] <= n for every i */
int tdc_gpu_prim_mark_orbit(tdc_gpu_ctx* ctx, const uint32_t* next, size_t n, uint8_t* mark);
/* dx_entries (the tile scheme of the device decoders): exit0[t * states + o] = the state in which the chain that enters tile t in
 * state o enters tile t + 1, 0xFFFF: it ends in t.  entry0[t] = the state in which the chain that enters tile 0 in state 0 enters
 * tile t, 0xFFFF behind its end.  Every exit must be < states or 0xFFFF (anything else is refused); at most 2^27 tiles */
int tdc_gpu_prim_tile_entries(tdc_gpu_ctx* ctx, const uint16_t* exit0, size_t ntiles, uint32_t states, uint16_t* entry0);
/* For tests/test_gpu_arena_state.py: what a call finds in the scratch arena.  byte 0..255: fill the whole arena [base, base + size) with
 * it on the context's stream and synchronise; byte < 0: fill nothing; byte > 255: TDC_GPU_ERR_ARG.  Either way *base / *size report
 * where the arena is and how large.  An arena that does not exist yet: *size = 0, nothing filled, status OK.  The allocation marks of
 * the arena are not touched.  Not between tdc_gpu_lcpcomp_compress_keep and tdc_gpu_stream_fetch*: the kept stream lives in the arena
 * (and, as after every call on the context, it is no longer there to fetch). */
int tdc_gpu_prim_arena_fill(tdc_gpu_ctx* ctx, int byte, uint64_t* base, uint64_t* size);

/* ---- LCPCompressor::decompress (LCPCompressor.hpp:140-150 -> decode_text_internal :23-76, HuffmanCoder::Decoder
 * coders/HuffmanCoder.hpp:572-612); lzss_lcp(coder=huff) streams have the same format (LZSSLCPCompressor.hpp:125-130).
 * Streams of 1 MiB and more whose longest literal run is at most 512 are parsed ON THE DEVICE (rounds 4-5, DESIGN.md section 5: where
 * the token that starts at a bit position ends is evaluated for every bit position, the real token starts are the orbit of the
 * first one) -- coder=huff and coder=sle (every kmer; rankings of up to 1024 entries, which is all the encoder writes) alike;
 * smaller streams, longer literal runs and the ASCII coder take the host parse.  The references -- what ScanDec /
 * CompactDec spend their time on (lcpcomp/decompress/ScanDec.hpp:146-247) -- are resolved on the device by pointer jumping.
 * *out (malloc'd, free with tdc_gpu_free) receives the escaped, 0-terminated text exactly as compress() was given it.
 * factors / rounds (nullable): number of factors in the stream / pointer-jumping rounds.  Malformed input: TDC_GPU_ERR_ARG. */
int tdc_gpu_lcpcomp_decompress(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, uint8_t** out, size_t* out_len,
                               uint64_t* factors, uint32_t* rounds);
/* The same for a stream written with another coder: TDC_GPU_CODER_HUFF, TDC_GPU_CODER_ASCII (ASCIICoder::Decoder,
 * coders/ASCIICoder.hpp:53-84) or TDC_GPU_CODER_SLE / TDC_GPU_CODER_SLE_K(k) (SLECoder::Decoder, coders/SLECoder.hpp:301-453). */
int tdc_gpu_lcpcomp_decompress_coder(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint8_t** out, size_t* out_len,
                                     uint64_t* factors, uint32_t* rounds);
/* The same into the CALLER's buffer `out` of out_cap bytes (pinned host memory -- tdc_gpu_host_alloc -- receives the text at the host
 * link's rate; the malloc'd variants pay for the page faults of a fresh buffer).  TDC_GPU_ERR_OOM if the text does not fit. */
int tdc_gpu_lcpcomp_decompress_into(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint8_t* out, size_t out_cap,
                                    size_t* out_len, uint64_t* factors, uint32_t* rounds);
/* 1 if the last tdc_gpu_lcpcomp_decompress / _decompress_coder / _decompress_into (or tdc_gpu_lzss_lcp_decompress / _into, tdc_gpu_lzw_decompress /
 * _into) call on this context succeeded and parsed the token
 * stream on the device (coder=huff and coder=sle streams of 1 MiB and more whose longest literal run is at most 512; option dec_parse =
 * 0 never / 2 every size; option dec_lean = 0: the general marking also for streams of short tokens -- tests), 0 if on the host. */
int tdc_gpu_ctx_last_decode_on_device(const tdc_gpu_ctx* ctx);

/* ---- LZ78Compressor::decompress (compressors/LZ78Compressor.hpp:142-160 -> lz78::Decompressor :16-37, EliasGammaCoder::Decoder
 * coders/EliasGammaCoder.hpp:31-42) for streams of tdc_gpu_lz78_compress or the reference's lz78(coder=gamma).  Parsed ON THE DEVICE
 * (where the pair that starts at a bit position ends is evaluated for every bit position, the real pair starts
 * are the orbit of bit 0), phrase lengths by pointer jumping over the parent ids, the text by the reference resolver of the lcpcomp
 * decoder.  The reference walks every phrase's parent chain one byte at a time instead.  coder must be TDC_GPU_CODER_GAMMA
 * (else TDC_GPU_ERR_UNSUPPORTED).  *out (malloc'd, free with tdc_gpu_free) receives the text; the empty stream decodes to 0 bytes.
 * phrases / rounds (nullable): number of (id, char) pairs / pointer-jumping rounds (phrase lengths + text references).
 * Malformed input -- a pair cut off by the end of the stream, an id field wider than 32 bits, a char field wider than 64 bits, the
 * k-th pair (0-based) naming a phrase id > k --: TDC_GPU_ERR_ARG.  A text of more than 2^32 - 2 bytes: TDC_GPU_ERR_TOO_LARGE (found
 * before anything of the text's size is allocated). */
int tdc_gpu_lz78_decompress(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint8_t** out, size_t* out_len,
                            uint64_t* phrases, uint32_t* rounds);
/* The same into the CALLER's buffer `out` of out_cap bytes (pinned host memory -- tdc_gpu_host_alloc -- receives the text at the host
 * link's rate).  TDC_GPU_ERR_OOM if the text does not fit; *out_len then holds the required size. */
int tdc_gpu_lz78_decompress_into(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint8_t* out, size_t out_cap,
                                 size_t* out_len, uint64_t* phrases, uint32_t* rounds);

/* ---- lzw: LZWCompressor<BitCoder | EliasGammaCoder, ...> (compressors/LZWCompressor.hpp:39-133, lzw/LZWDecoding.hpp:12-99; DESIGN.md
 * section 5.4).  No input restrictions.  coder: TDC_GPU_CODER_BIT (the reference's default: code k in bits_for(k + 256) bits) or
 * TDC_GPU_CODER_GAMMA; anything else: TDC_GPU_ERR_UNSUPPORTED.  dict_size is 0 (unlimited), as in the reference's default.
 * compress: the parse is sequential and runs on the host (tdc_lzw_factors), the codes are packed on the device.  Inputs of 2^32 - 256
 * bytes and more: TDC_GPU_ERR_TOO_LARGE.  stats (may be NULL): n, out_len, factors (= number of codes), ms_h2d / ms_encode / ms_d2h /
 * ms_total. */
int tdc_gpu_lzw_compress(tdc_gpu_ctx* ctx, const uint8_t* in, size_t n, int coder, uint8_t** out, size_t* out_len,
                         tdc_gpu_stats* stats);
/* decompress: on the device for streams of 64 KiB and more (option dec_parse = 2: every stream, 0: never), else a host loop that restates
 * lzw::decode_step; tdc_gpu_ctx_last_decode_on_device tells which.  On the device the codes are read side by side (coder=bit: from
 * closed-form offsets; coder=gamma: the orbit parse of the lz78 decoder), a code c >= 256 is the copy of phrase c - 256 and the byte
 * behind it in the text, lengths come from pointer jumping and the text from the reference resolver.  codes / rounds (nullable): number
 * of codes / pointer-jumping rounds.  Malformed input -- code k (0-based) above 255 + k, a code cut off by the end of the stream, a
 * gamma field wider than 32 bits --: TDC_GPU_ERR_ARG.  A text of more than 2^32 - 2 bytes: TDC_GPU_ERR_TOO_LARGE (found before
 * anything of the text's size is allocated). */
int tdc_gpu_lzw_decompress(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint8_t** out, size_t* out_len,
                           uint64_t* codes, uint32_t* rounds);
/* The same into the CALLER's buffer `out` of out_cap bytes.  TDC_GPU_ERR_OOM if the text does not fit; *out_len then holds the
 * required size. */
int tdc_gpu_lzw_decompress_into(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint8_t* out, size_t out_cap,
                                size_t* out_len, uint64_t* codes, uint32_t* rounds);

/* ---- lzss: LZSSSlidingWindowCompressor<ASCIICoder | BitCoder | EliasGammaCoder | EliasDeltaCoder> (compressors/
 * LZSSSlidingWindowCompressor.hpp:39-143): the classic LZ77 parse over a sliding window, factorized ON THE DEVICE.
 * No input restrictions (raw bytes, no sentinel); the empty input has no tokens.  Options: window (the reference's default: 16) and
 * threshold (3; 0 behaves as 1).  At text position p the candidates are the sources s in [max(0, p - window), p), the look-ahead is
 * L(p) = end(p) - p with end(p) = n for n < 2 window, else clamp(p - window, 0, n - 2 window) + 2 window -- so a factor in the first
 * `window` positions may be as long as 2 window - 1 --, and the smallest s among the longest matches of at least `threshold` bytes wins;
 * a source may overlap p.  The stream has no header: a literal is the flag 0 and the byte under literal_r, a factor the flag 1,
 * p - s under Range(0, p) and the length under Range(0, window); the bit stream's terminator ends it.
 * coder: TDC_GPU_CODER_ASCII, _BIT, _GAMMA or _DELTA; anything else (huff among it): TDC_GPU_ERR_UNSUPPORTED.
 * window: 1 .. 4096 (the match kernel keeps a tile's text and its window in LDS); 0: TDC_GPU_ERR_ARG, above 4096: TDC_GPU_ERR_UNSUPPORTED.
 * n above 2^32 - 2: TDC_GPU_ERR_TOO_LARGE.
 * One defect of the reference is not reproduced: under coder=bit with a window that is no power of two, a length of up to
 * 2 window - 1 may not fit the bits_for(window) bits of its field; the reference truncates it and its own decoder then yields another
 * text (window 3, "aaaaaaaa": lengths 4 and 5 in 2 bits).  On such inputs the call returns TDC_GPU_ERR_UNSUPPORTED and writes nothing to
 * `out`; the other three coders ignore the range and code them normally.
 * stats (may be NULL): n, out_len, factors, flen_max, ms_h2d, ms_factorize, ms_encode, ms_d2h, ms_total, arena_bytes.
 * Streams are decoded by tdc_gpu_lzss_sw_decompress (on the device) or by tdc_lzss_sw_decode (the host loop, its specification). */
int tdc_gpu_lzss_sw_compress(tdc_gpu_ctx* ctx, const uint8_t* in, size_t n, uint32_t window, uint32_t threshold, int coder,
                             uint8_t** out, size_t* out_len, tdc_gpu_stats* stats);
/* The same into the CALLER's buffer of out_cap bytes; TDC_GPU_ERR_OOM with the required size in *out_len if it is too small. */
int tdc_gpu_lzss_sw_compress_into(tdc_gpu_ctx* ctx, const uint8_t* in, size_t n, uint32_t window, uint32_t threshold, int coder,
                                  uint8_t* out, size_t out_cap, size_t* out_len, tdc_gpu_stats* stats);
/* worst-case stream length for n input bytes (what an _into buffer needs at most); 0 for a coder or a window the call does not take */
size_t tdc_gpu_lzss_sw_bound(size_t n, uint32_t window, int coder);
/* the factors of the parse on their own, sorted by pos: pos / src / len are malloc'd (tdc_gpu_free), z entries each; what
 * tdc_lzss_sw_factors computes on the host */
int tdc_gpu_lzss_sw_factorize(tdc_gpu_ctx* ctx, const uint8_t* in, size_t n, uint32_t window, uint32_t threshold,
                              uint32_t** pos, uint32_t** src, uint32_t** len, size_t* z);
/* LZSSSlidingWindowCompressor::decompress (:120-143) of a stream of tdc_gpu_lzss_sw_compress or of the reference's lzss(coder=...).
 * coder = TDC_GPU_CODER_BIT, _GAMMA or _DELTA: the token stream is parsed and the references are resolved on the device for streams of
 * 1 MiB and more (option dec_parse: 2 = every stream, 0 = never; dec_seg, dec_log as for the other decoders); smaller streams and
 * TDC_GPU_CODER_ASCII go through tdc_lzss_sw_decode, which stays the specification.  tdc_gpu_ctx_last_decode_on_device reports the path.
 * Any other coder: TDC_GPU_ERR_UNSUPPORTED.  window: the compressor's option -- only coder=bit reads it (the width of the length field;
 * 0: TDC_GPU_ERR_ARG), and distances may reach back further than it, up to the token's text position.  The empty stream decodes to 0 bytes.
 * TDC_GPU_ERR_ARG, as from the host loop: a token cut off by the end of the stream, a distance of 0 or above the token's text position,
 * a malformed gamma / delta field, a token chain that does not advance.  The device reads gamma / delta distance and length fields of
 * at most 32 value bits and literal codes of at most 8; a wider field (no encoder writes one) is refused there with TDC_GPU_ERR_ARG even
 * where the host loop would read it -- coder=bit has no such case.  A text of more than 2^32 - 2 bytes: TDC_GPU_ERR_TOO_LARGE, decided
 * before anything of the text's size is allocated.
 * *out is malloc'd (tdc_gpu_free).  factors (may be NULL): the number of factor tokens; rounds (may be NULL): pointer-jumping rounds of
 * the reference resolver (both 0 on the host path). */
int tdc_gpu_lzss_sw_decompress(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint32_t window,
                               uint8_t** out, size_t* out_len, uint64_t* factors, uint32_t* rounds);
/* The same into the CALLER's buffer of out_cap bytes; TDC_GPU_ERR_OOM with the required size in *out_len if it is too small (nothing
 * is written to `out` then). */
int tdc_gpu_lzss_sw_decompress_into(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint32_t window,
                                    uint8_t* out, size_t out_cap, size_t* out_len, uint64_t* factors, uint32_t* rounds);

/* ---- lzss over a batch: many independent texts in one call, both directions (lzss_sw_batch.hip, DESIGN.md section 5.7 "Batches").
 * The texts lie back to back in `in`: text k = in[in_off[k], in_off[k + 1]); in_off has count + 1 entries, does not decrease, and
 * in_off[0] = 0.  Stream k = out[out_off[k], out_off[k] + out_len[k]) is byte for byte what tdc_gpu_lzss_sw_compress returns for text k
 * alone with the same window, threshold and coder (TDC_GPU_CODER_ASCII, _BIT, _GAMMA, _DELTA), the empty text included: nothing of one
 * text reaches another one's stream -- candidates, look-ahead and, under coder=bit, the width of a distance are those of the position
 * inside its own text.  out_off[k] is a multiple of 8, out_off[count] the number of bytes used; the bytes between two streams are
 * unspecified.  The device makes ONE pass over the concatenation and the call synchronises a constant number of times, whatever count is.
 * status[k]: TDC_GPU_OK, or -- coder=bit and a length of text k that bits_for(window) bits do not hold, the single call's refusal --
 * TDC_GPU_ERR_UNSUPPORTED with out_len[k] = 0; the other texts are coded normally and the call returns TDC_GPU_OK.
 * The call itself: TDC_GPU_ERR_ARG for a NULL argument, window 0, in_off[0] != 0 or a decreasing in_off; TDC_GPU_ERR_UNSUPPORTED for a
 * window above 4096 or another coder; TDC_GPU_ERR_TOO_LARGE for more than 2^32 - 2 bytes in all (these are decided from the arguments
 * alone, before the context is looked at); TDC_GPU_ERR_OOM with the required size in out_off[count] if out_cap is too small -- nothing is
 * written to `out` then.  count = 0 is valid and writes only out_off[0] = 0.
 * stats (may be NULL): n (all input bytes), out_len (bytes used), factors (summed over the batch), ms_h2d, ms_factorize, ms_encode,
 * ms_d2h, ms_total, arena_bytes. */
int tdc_gpu_lzss_sw_compress_batch(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* in_off, size_t count,
                                   uint32_t window, uint32_t threshold, int coder,
                                   uint8_t* out, size_t out_cap, uint64_t* out_off /* count + 1 */, uint64_t* out_len /* count */,
                                   int32_t* status /* count */, tdc_gpu_stats* stats);
/* what `out` of tdc_gpu_lzss_sw_compress_batch needs at most: the sum of tdc_gpu_lzss_sw_bound of every text, each rounded up to 8.
 * 0 where tdc_gpu_lzss_sw_bound returns 0 (coder, window), for offsets the call refuses, or for more than 2^32 - 2 bytes in all. */
size_t tdc_gpu_lzss_sw_batch_bound(const uint64_t* in_off, size_t count, uint32_t window, int coder);
/* The decoder of such a batch, or of any collection of lzss streams: stream k = streams[s_off[k], s_off[k] + s_len[k]) (any order, any
 * alignment; together they must lie within 2^32 - 2 bytes), coder = TDC_GPU_CODER_BIT, _GAMMA or _DELTA (TDC_GPU_CODER_ASCII and every
 * other coder: TDC_GPU_ERR_UNSUPPORTED -- loop tdc_lzss_sw_decode for ascii).  Always on the device, one wave per stream; option
 * dec_parse is not consulted.  Text k = out[out_off[k], out_off[k + 1]), the texts back to back.  status[k] is the verdict
 * tdc_lzss_sw_decode gives on stream k alone -- TDC_GPU_OK, TDC_GPU_ERR_ARG or TDC_GPU_ERR_TOO_LARGE -- and the text is the same bytes
 * where it is TDC_GPU_OK; a refused stream contributes 0 bytes and disturbs no neighbour.  A distance is checked against the token's
 * position in its OWN text: the text in front of it in `out` is never reachable.  The device caps of tdc_gpu_lzss_sw_decompress hold
 * here too: a gamma / delta distance or length field of more than 32 value bits, or a literal code of more than 8, is
 * TDC_GPU_ERR_ARG although the host loop reads it (no encoder writes one).
 * out == NULL or out_cap too small: TDC_GPU_ERR_OOM with the required total in out_off[count] and all of out_off / status filled -- the
 * sizes pass alone, so that a caller can size its buffer; nothing is written to `out`.  More than 2^32 - 2 bytes of text in all:
 * TDC_GPU_ERR_TOO_LARGE.  TDC_GPU_ERR_ARG: a NULL s_off, s_len, out_off or status, coder=bit with window 0 (only coder=bit reads it).
 * stats (may be NULL): n (all stream bytes), out_len (all text bytes), factors (factor tokens of the accepted streams), ms_h2d,
 * ms_factorize (the sizes pass), ms_encode (the write pass), ms_d2h, ms_total, arena_bytes. */
int tdc_gpu_lzss_sw_decompress_batch(tdc_gpu_ctx* ctx, const uint8_t* streams, const uint64_t* s_off, const uint64_t* s_len,
                                     size_t count, int coder, uint32_t window,
                                     uint8_t* out, size_t out_cap, uint64_t* out_off /* count + 1 */,
                                     int32_t* status /* count */, tdc_gpu_stats* stats);

/* ---- lzw and lz78 over a batch: many independent texts in one call, PARSED ON THE DEVICE (lz_batch.hip, DESIGN.md section 5.4 "Batches").
 * The single calls parse on the host, because the parse of one text is sequential; across texts the parses are independent, and here one
 * wave takes one text.  The texts lie back to back in `in`: text k = in[in_off[k], in_off[k + 1]); in_off has count + 1 entries, does not
 * decrease, and in_off[0] = 0.  Stream k = out[out_off[k], out_off[k] + out_len[k]) is byte for byte what tdc_gpu_lzw_compress /
 * tdc_gpu_lz78_compress returns for text k alone with the same coder, the empty text (the terminator alone) included.  out_off[k] is a
 * multiple of 8, out_off[count] the number of bytes used; the bytes between two streams are unspecified.  The call synchronises a constant
 * number of times, whatever count is.
 * coder: what the single calls take -- lzw: TDC_GPU_CODER_BIT or _GAMMA, lz78: TDC_GPU_CODER_GAMMA; anything else:
 * TDC_GPU_ERR_UNSUPPORTED for the call.
 * status[k]: TDC_GPU_OK, or the code of the single call on text k alone, with out_len[k] = 0 and no byte of `out` taken; the other texts
 * are coded normally and the call returns TDC_GPU_OK.  lz78: TDC_GPU_ERR_UNSUPPORTED for a text whose left-over phrase ends in a byte
 * >= 0x80 (the reference encodes it as a signed char).  Both: TDC_GPU_ERR_TOO_LARGE for a text of more than 2^25 - 256 = 33 554 176
 * bytes -- the cap of ONE text in a batch (a table word holds the key in 33 bits and the id in 25); the single calls take such a text.
 * The call itself: TDC_GPU_ERR_ARG for a NULL argument, in_off[0] != 0 or a decreasing in_off; TDC_GPU_ERR_UNSUPPORTED for the coder;
 * TDC_GPU_ERR_TOO_LARGE for more than 2^32 - 2 bytes in all (these are decided from the arguments alone, before the context is looked
 * at); TDC_GPU_ERR_OOM with the required size in out_off[count] if out_cap is too small -- decided from the sizes before anything is
 * packed, nothing is written to `out` then -- or if the device cannot hold the arena: the tables take at most 32 bytes per text byte.
 * count = 0 is valid and writes only out_off[0] = 0.
 * Option of the context: lz_batch_hash_bits (tests; 0: the whole hash of a phrase picks its home slot in the table, k = 1 .. 24: only k
 * bits of it do -- long probe runs, the same streams).
 * stats (may be NULL): n (all input bytes), out_len (bytes used), factors (items summed over the accepted texts), ms_h2d, ms_factorize
 * (the parse and the placement), ms_encode (the pack), ms_d2h, ms_total, arena_bytes.
 * The batch decoders are tdc_gpu_lzw_decompress_batch / tdc_gpu_lz78_decompress_batch below; the streams are also ordinary streams for
 * tdc_lzw_decode, tdc_gpu_lzw_decompress and tdc_gpu_lz78_decompress. */
int tdc_gpu_lzw_compress_batch(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* in_off, size_t count, int coder,
                               uint8_t* out, size_t out_cap, uint64_t* out_off /* count + 1 */, uint64_t* out_len /* count */,
                               int32_t* status /* count */, tdc_gpu_stats* stats);
int tdc_gpu_lz78_compress_batch(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* in_off, size_t count, int coder,
                                uint8_t* out, size_t out_cap, uint64_t* out_off /* count + 1 */, uint64_t* out_len /* count */,
                                int32_t* status /* count */, tdc_gpu_stats* stats);
/* what `out` of the batch calls needs at most: per text of n bytes the stream of n items with every field at its widest for such a
 * text -- lzw + bit: S(n) bits, the offset of code n; lzw + gamma: n (2 bits_for(n + 255) + 1); lz78: n (2 bits_for(n) + 1 + 17) --, its
 * terminator (bits / 8 + 1 bytes, + 2 where bits mod 8 > 5), rounded up to 8; summed.  0 for a coder the call does not take, for offsets
 * it refuses, or for more than 2^32 - 2 bytes in all. */
size_t tdc_gpu_lzw_batch_bound(const uint64_t* in_off, size_t count, int coder);
size_t tdc_gpu_lz78_batch_bound(const uint64_t* in_off, size_t count, int coder);
/* The parse of such a batch alone, what tdc_lzw_factors (lzw != 0) / tdc_lz78_factors (lzw = 0) compute for every text on the host: the
 * items of text k are items[item_off[k] .. item_off[k + 1]) -- lzw: the codes; lz78: the phrase ids, with their bytes in chars (NULL for
 * lzw).  items and chars hold in_off[count] entries (a text has at most as many items as bytes), item_off count + 1.  status[k]:
 * TDC_GPU_OK; TDC_GPU_ERR_UNSUPPORTED (lz78: the left-over byte is >= 0x80 -- the items are there all the same);
 * TDC_GPU_ERR_TOO_LARGE (the text is beyond the cap: no items).  Arguments are refused as by the batch calls. */
int tdc_gpu_lz_parse_batch(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* in_off, size_t count, int lzw,
                           uint32_t* items /* n */, uint8_t* chars /* n */, uint64_t* item_off /* count + 1 */, int32_t* status /* count */);

/* The decoders of such batches, or of any collection of lzw / lz78 streams (lz_batch_decode.hip, DESIGN.md section 5.4 "Batch decoder").
 * The arguments are those of tdc_gpu_lzss_sw_decompress_batch, one by one: stream k = streams[s_off[k], s_off[k] + s_len[k]) (any order,
 * any alignment; together they must lie within 2^32 - 2 bytes), text k = out[out_off[k], out_off[k + 1]), the texts back to back; a
 * refused stream contributes 0 bytes and disturbs no neighbour.  coder: lzw TDC_GPU_CODER_BIT or _GAMMA, lz78 _GAMMA; anything else is
 * TDC_GPU_ERR_UNSUPPORTED for the call.  Always on the device -- option dec_parse is not consulted, no stream is too small -- and in ONE
 * pass: the items of all streams form one forest of backward links, expanded as tdc_gpu_lzw_decompress expands one stream's; under
 * coder=bit every code of every stream is read side by side from its closed-form offset.  The call synchronises a constant number of
 * times (plus the pointer-jumping rounds, which depend on the deepest chain), whatever count is.
 * status[k], lzw: the verdict of tdc_lzw_decode on stream k alone -- TDC_GPU_OK with the same bytes; TDC_GPU_ERR_ARG for a code j above
 * 255 + j, a cut-off code, a cut-off terminator or a gamma field wider than 32 bits; TDC_GPU_ERR_TOO_LARGE for a text above 2^32 - 2
 * bytes.  lz78: what tdc_gpu_lz78_decompress returns on stream k alone (the rules are stated there).  An item is counted from its OWN
 * stream's first item: a code or id that a global count would allow -- the second stream of a batch opening with lzw code 256, or with
 * the lz78 pair (1, c) -- is refused, and nothing in front of a stream's own text is reachable from it.  A stream that holds a bad item
 * AND claims too much text is TDC_GPU_ERR_ARG: the device reads every item before it knows a length, as the single device decoders do
 * (the host loop reports whichever comes first in the stream).
 * out == NULL or out_cap too small: TDC_GPU_ERR_OOM with the required total in out_off[count] and all of out_off / status filled -- the
 * sizes alone, so that a caller can size its buffer; nothing is written to `out`.  More than 2^32 - 2 bytes of text in all, or
 * 2^32 - 258 items and more in all: TDC_GPU_ERR_TOO_LARGE for the call, before anything text-sized is allocated.  Decided from the
 * arguments alone, before the context is looked at: TDC_GPU_ERR_ARG for a NULL s_off, s_len, out_off or status, a stream whose end
 * overflows, streams == NULL with a non-empty stream; the coder.  count = 0 is valid and writes only out_off[0] = 0.
 * stats (may be NULL): n (all stream bytes), out_len (all text bytes), factors (the items of the accepted streams), ms_h2d, ms_factorize
 * (parse, lengths, starts and sizes, up to the read-back of out_off and status), ms_encode (literals, the resolver and -- the resolver
 * hands the text over as it finishes -- its download; ms_d2h stays 0), ms_total, arena_bytes, len_rounds and flatten_rounds (the
 * pointer-jumping rounds over the items and over the text). */
int tdc_gpu_lzw_decompress_batch(tdc_gpu_ctx* ctx, const uint8_t* streams, const uint64_t* s_off, const uint64_t* s_len,
                                 size_t count, int coder, uint8_t* out, size_t out_cap, uint64_t* out_off /* count + 1 */,
                                 int32_t* status /* count */, tdc_gpu_stats* stats);
int tdc_gpu_lz78_decompress_batch(tdc_gpu_ctx* ctx, const uint8_t* streams, const uint64_t* s_off, const uint64_t* s_len,
                                  size_t count, int coder, uint8_t* out, size_t out_cap, uint64_t* out_off /* count + 1 */,
                                  int32_t* status /* count */, tdc_gpu_stats* stats);

/* ---- repair: RePairCompressor<BitCoder | ASCIICoder | EliasGammaCoder | EliasDeltaCoder> (compressors/RePairCompressor.hpp:96-336;
 * DESIGN.md section 5.8): the Re-Pair grammar, built ON THE DEVICE.  No input restrictions (raw bytes, no sentinel).  Symbols are 32-bit:
 * 0 .. 255 are bytes, 256 + k is rule k; a rule is l << 32 | r.  Per round every adjacent pair of the live sequence is counted
 * (occurrences overlap: aaa counts (a,a) twice); with M the largest count, the pair whose M-th occurrence comes first among the pairs
 * that count M becomes the next rule (the reference takes a pair over when its running count exceeds the best so far strictly); M <= 1
 * ends the loop.  The pair is replaced left to right, continuing behind a replaced pair: a run a^k loses floor(k / 2) pairs from its
 * left end.  max_rules (the reference's option; 0 = unlimited) ends the loop after that many rules.  The empty input, on which the
 * reference is undefined, is defined as no rules and no symbols.
 * The stream: the number of rules under len_r, both sides of rule i -- a flag, then the byte under literal_r or x - 256 under Range(i) --,
 * then the start sequence under Range(rules); the bit stream's terminator ends it.
 * coder: TDC_GPU_CODER_BIT (the reference's default), _ASCII, _GAMMA or _DELTA; anything else (huff among it, whose literal order is not
 * built): TDC_GPU_ERR_UNSUPPORTED.  n above 2^30: TDC_GPU_ERR_TOO_LARGE.  A device that cannot hold the arena (DESIGN.md section 5.8 states
 * the formula): TDC_GPU_ERR_OOM before anything is written.
 * Options of the context: repair_recount (1: the digram table is recounted in every round instead of taking the round's deltas),
 * repair_table_bits (8 .. 30: the first capacity of the table), repair_log.
 * stats (may be NULL): n, out_len, rules, replaced, tie_rounds, rebuilds, ms_round_first / _last / _tie, ms_h2d, ms_factorize (the grammar),
 * ms_encode, ms_d2h, ms_total, arena_bytes. */
int tdc_gpu_repair_compress(tdc_gpu_ctx* ctx, const uint8_t* in, size_t n, uint64_t max_rules, int coder, uint8_t** out, size_t* out_len,
                            tdc_gpu_stats* stats);
/* The same into the CALLER's buffer of out_cap bytes; TDC_GPU_ERR_OOM with the required size in *out_len if it is too small. */
int tdc_gpu_repair_compress_into(tdc_gpu_ctx* ctx, const uint8_t* in, size_t n, uint64_t max_rules, int coder, uint8_t* out, size_t out_cap,
                                 size_t* out_len, tdc_gpu_stats* stats);
/* worst-case stream length for n input bytes (what an _into buffer needs at most); 0 for a coder or a length the call does not take */
size_t tdc_gpu_repair_bound(size_t n, int coder);
/* the grammar on its own: *rules (nrules entries, l << 32 | r) and *start (nstart symbols) are malloc'd (tdc_gpu_free); what
 * tdc_repair_grammar computes on the host.  stats (may be NULL): the repair fields and ms_factorize. */
int tdc_gpu_repair_grammar(tdc_gpu_ctx* ctx, const uint8_t* in, size_t n, uint64_t max_rules, uint64_t** rules, size_t* nrules,
                           uint32_t** start, size_t* nstart, tdc_gpu_stats* stats);
/* ---- repair over a batch: many independent texts in one call, ONE WORKGROUP PER GRAMMAR (repair_batch.hip, DESIGN.md section 5.8
 * "Batches").  The single call is a host-driven loop with a read-back per rule; across texts the grammars are independent, and here one
 * workgroup runs the whole round loop of one text on the device.  The texts lie back to back in `in`: text k = in[in_off[k], in_off[k + 1]);
 * in_off has count + 1 entries, does not decrease, and in_off[0] = 0.  Stream k = out[out_off[k], out_off[k] + out_len[k]) is byte for byte
 * what tdc_gpu_repair_compress returns for text k alone with the same max_rules and coder, the empty text included; no pair spans a
 * border.  out_off[k] is a multiple of 8, out_off[count] the number of bytes used; the bytes between two streams are unspecified.
 * coder: TDC_GPU_CODER_BIT, _ASCII, _GAMMA or _DELTA; anything else: TDC_GPU_ERR_UNSUPPORTED for the call.
 * status[k]: TDC_GPU_OK, or TDC_GPU_ERR_TOO_LARGE for a text of more than 2^24 = 16 777 216 bytes -- the cap of ONE text in a batch (one
 * workgroup walks the text once per rule; tdc_gpu_repair_compress is the tool for such a text) --, with out_len[k] = 0 and no byte of
 * `out` taken; the other texts are coded normally and the call returns TDC_GPU_OK.
 * status[k] can also be TDC_GPU_ERR_INTERNAL: the text's round loop met a broken invariant (a full table, a tie without a winner, a round
 * that took no pair).  That is a bug of the library, not a property of the text; the text is then treated like a refused one, and callers
 * should check for it as for TOO_LARGE.
 * The call itself, decided from the arguments alone before the context is looked at, in this order: TDC_GPU_ERR_UNSUPPORTED for the
 * coder; TDC_GPU_ERR_ARG for a NULL argument, in_off[0] != 0 or a decreasing in_off; TDC_GPU_ERR_TOO_LARGE for more than 2^32 - 2 bytes
 * in all; TDC_GPU_ERR_ARG for a NULL context.  TDC_GPU_ERR_OOM with the required size in out_off[count] if out_cap is too small --
 * decided from the sizes before anything is packed, nothing is written to `out` then -- or if the device cannot hold the arena (DESIGN.md
 * section 5.8 states the formula: at most 142 bytes per text byte).  count = 0 is valid and writes only out_off[0] = 0.
 * Options of the context (not enumerated by tdc_gpu_option_name): repair_batch_rounds (rounds per text and launch, divided by n_k / 64 KiB for a text above 128 KiB; the host relaunches
 * while a text is unfinished, one read-back per launch), repair_batch_table (0: a text's digram table has 4 slots per text byte; 1: 2
 * slots, so that small texts reach the in-kernel rebuild -- tests; the same streams).
 * stats (may be NULL): n (all input bytes), out_len (bytes used), rules, replaced, tie_rounds and rebuilds (summed over the accepted
 * texts), len_rounds (the LAUNCHES of the round kernel), ms_h2d, ms_factorize (the grammars and the placement), ms_encode (the pack),
 * ms_d2h, ms_total, arena_bytes.
 * The batch decoder is tdc_gpu_repair_decompress_batch below; the streams are also ordinary streams for tdc_repair_decode and
 * tdc_gpu_repair_decompress. */
int tdc_gpu_repair_compress_batch(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* in_off, size_t count, uint64_t max_rules, int coder,
                                  uint8_t* out, size_t out_cap, uint64_t* out_off /* count + 1 */, uint64_t* out_len /* count */,
                                  int32_t* status /* count */, tdc_gpu_stats* stats);
/* what `out` of tdc_gpu_repair_compress_batch needs at most: the sum of tdc_gpu_repair_bound of every text, each rounded up to 8.  0 for
 * a coder the call does not take, for offsets it refuses, or for more than 2^32 - 2 bytes in all. */
size_t tdc_gpu_repair_batch_bound(const uint64_t* in_off, size_t count, int coder);
/* The grammars of such a batch alone, what tdc_repair_grammar computes for every text on the host: the rules of text k are
 * rules[rule_off[k] .. rule_off[k + 1]) (l << 32 | r), its start sequence start[start_off[k] .. start_off[k + 1]).  rules and start hold
 * in_off[count] entries, rule_off and start_off count + 1.  status[k]: TDC_GPU_OK, or TDC_GPU_ERR_TOO_LARGE / TDC_GPU_ERR_INTERNAL as in the
 * batch call (no rules, no symbols).
 * Arguments are refused as by the batch call (there is no coder). */
int tdc_gpu_repair_grammar_batch(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* in_off, size_t count, uint64_t max_rules,
                                 uint64_t* rules /* in_off[count] */, uint64_t* rule_off /* count + 1 */,
                                 uint32_t* start /* in_off[count] */, uint64_t* start_off /* count + 1 */, int32_t* status /* count */);

/* RePairCompressor::decompress.  bit, gamma and delta streams are decoded ON THE DEVICE ("Device decoder"): the
 * tokens are parsed side by side, the grammar becomes a factor list (lengths bottom-up, first occurrences top-down) and the reference
 * resolver of the other decoders writes the text.  Option dec_parse picks the path: 1 (default) = streams of 1 MiB and more, 2 = every
 * stream, 0 = the host loop tdc_repair_decode, which also keeps the ascii streams.  Option repair_dec_rounds (default 1024) bounds the
 * rounds of the two grammar passes; a grammar that needs more (a chain of rules) is decoded by the host loop, as is a stream with a gamma /
 * delta field wider than the device reads (an index above 32 bits, a literal above 8).  Verdict and text are tdc_repair_decode's on
 * every stream; tdc_gpu_ctx_last_decode_on_device reports the path a successful call took.  *out is malloc'd (tdc_gpu_free); _into:
 * TDC_GPU_ERR_OOM with the required size in *out_len if out_cap is too small. */
int tdc_gpu_repair_decompress(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint8_t** out, size_t* out_len);
int tdc_gpu_repair_decompress_into(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint8_t* out, size_t out_cap, size_t* out_len);
/* _into with what the call did.  stats (may be NULL): n and out_len (the text), rules, factors, arena_bytes, len_rounds (rounds of the
 * length pass), levels (rounds of the first-occurrence pass), flatten_rounds (pointer-jumping rounds of the reference resolver),
 * small_levels (segments of the parse), ms_h2d (the upload), ms_factorize (parse and grammar passes), ms_d2h (items, resolver and
 * download), ms_total -- host clock around synchronisations; all zero but n, out_len and ms_total where the host loop decoded. */
int tdc_gpu_repair_decompress_stats(tdc_gpu_ctx* ctx, const uint8_t* stream, size_t len, int coder, uint8_t* out, size_t out_cap, size_t* out_len,
                                    tdc_gpu_stats* stats);
/* The decoder of repair batches, or of any collection of repair streams (repair_batch_decode.hip, DESIGN.md section 5.8 "Batch decoder").
 * The arguments are those of tdc_gpu_lzw_decompress_batch, one by one: stream k = streams[s_off[k], s_off[k] + s_len[k]) (any order, any
 * alignment; together they must lie within 2^32 - 2 bytes), text k = out[out_off[k], out_off[k + 1]), the texts back to back; a refused
 * stream contributes 0 bytes and disturbs no neighbour.  coder: TDC_GPU_CODER_BIT, _GAMMA or _DELTA; _ASCII and anything else is
 * TDC_GPU_ERR_UNSUPPORTED for the call (ascii streams: loop tdc_repair_decode).  Always on the device -- option dec_parse is not
 * consulted, no stream is too small, nothing is handed to the host loop -- and in ONE pass: one wave per stream finds the token borders,
 * the rules of all streams with their references rebased form one forest, and the grammar passes of tdc_gpu_repair_decompress run over
 * it once.  The call synchronises a constant number of times (plus the rounds of the length pass, of the first-occurrence pass and of
 * the resolver, which depend on the deepest accepted grammar), whatever count is.  tdc_gpu_ctx_last_decode_on_device is 1 after a
 * successful call.
 * status[k]: the verdict of tdc_repair_decode on stream k alone -- TDC_GPU_OK with the same bytes; TDC_GPU_ERR_ARG for a cut-off field, a
 * stream that ends inside its rules, more rules than twice the stream's bytes, a rule index out of range, a cut-off terminator, the
 * stream of no bytes; TDC_GPU_ERR_TOO_LARGE for a text above 2^32 - 2 bytes.  An index is checked against its OWN stream: a side of
 * rule i names a rule below i of that stream, a start symbol a rule below its R; nothing in front of a stream's own rules or text is
 * reachable.  A stream that holds a bad token AND claims too much text is TDC_GPU_ERR_ARG, as on the host (both parse the whole stream
 * before they look at a length).  Two deviations from the host's verdict, and no other:
 *   1. the device caps of the single decoder: a gamma / delta index field (the count field among them) of more than 32 value bits is
 *      TDC_GPU_ERR_ARG -- the host refuses it too --, and so is a literal code of more than 8 value bits, although the host loop keeps
 *      its low byte (no encoder writes one);
 *   2. depth: a stream whose grammar is higher than option repair_dec_rounds (default 1024) is TDC_GPU_ERR_UNSUPPORTED and contributes 0
 *      bytes; tdc_gpu_repair_decompress decodes it through the host loop.  A byte has height 0, a rule 1 + the larger height of its sides,
 *      and the height counts over ALL rules of the stream: a deep rule that nothing names refuses an otherwise shallow stream too.  The
 *      verdict is a function of the stream and the option alone.
 * out == NULL or out_cap too small: TDC_GPU_ERR_OOM with the required total in out_off[count] and all of out_off / status filled -- the
 * sizes alone, so that a caller can size its buffer; nothing is written to `out`.  More than 2^32 - 2 bytes of text in all, or
 * 2^32 - 258 tokens (sides of rules and start symbols) and more in all: TDC_GPU_ERR_TOO_LARGE for the call, before anything text-sized
 * is allocated.  Decided from the arguments alone, before the context is looked at, in this order: TDC_GPU_ERR_UNSUPPORTED for the
 * coder; TDC_GPU_ERR_ARG for a NULL s_off, s_len, out_off or status, for a stream whose end overflows, for streams == NULL with a
 * non-empty stream; TDC_GPU_ERR_ARG for a NULL context.  count = 0 is valid and writes only out_off[0] = 0.  TDC_GPU_ERR_INTERNAL: the
 * first-occurrence pass did not come to rest within its bound -- a bug of the library, not a property of a stream.
 * stats (may be NULL): n (all stream bytes), out_len (all text bytes), rules (summed over the accepted streams), factors (the factor
 * list of the accepted streams), len_rounds (rounds of the length pass), levels (rounds of the first-occurrence pass), flatten_rounds
 * (pointer-jumping rounds of the resolver), ms_h2d, ms_factorize (walks, lengths and sizes, up to the read-back of out_off and status),
 * ms_encode (first occurrences, items, the resolver and -- the resolver hands the text over as it finishes -- its download; ms_d2h stays
 * 0), ms_total, arena_bytes. */
int tdc_gpu_repair_decompress_batch(tdc_gpu_ctx* ctx, const uint8_t* streams, const uint64_t* s_off, const uint64_t* s_len,
                                    size_t count, int coder, uint8_t* out, size_t out_cap, uint64_t* out_off /* count + 1 */,
                                    int32_t* status /* count */, tdc_gpu_stats* stats);

/* ---- bwt: BWTCompressor::compress / ::decompress (compressors/BWTCompressor.hpp:29-60, ds/bwt.hpp:20-98), the Burrows-Wheeler transform
 * of the text.  Text contract and error codes of tdc_gpu_lcpcomp_compress (escaped, ONE terminating 0; TDC_GPU_ERR_NO_SENTINEL, TDC_GPU_ERR_ARG
 * for an inner 0, TDC_GPU_ERR_TOO_LARGE).  out[i] = T[SA[i] - 1] (T[n - 1] where SA[i] = 0): n bytes, no header.  The suffix array is the one
 * tdc_gpu_suffix_array builds; the transform is one gather over it, downloaded chunk by chunk behind the gather into page-locked memory.
 * stats (nullable): n, out_len, ms_h2d, ms_sa, ms_encode (the gather), ms_d2h, ms_total and the sa_* fields. */
int tdc_gpu_bwt_compress(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint8_t** out, size_t* out_len, tdc_gpu_stats* stats);
/* The same into the CALLER's buffer of out_cap bytes; TDC_GPU_ERR_OOM with the required size in *out_len if it is too small. */
int tdc_gpu_bwt_compress_into(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, uint8_t* out, size_t out_cap, size_t* out_len,
                              tdc_gpu_stats* stats);
/* Inverse (decode_bwt, ds/bwt.hpp:77-98, with the complete C table -- DESIGN.md section 5.2): LF by a stable counting rank, then list ranking
 * of its one cycle from sampled heads on the device; the reference walks LF one byte at a time.  *out (malloc'd, tdc_gpu_free) receives the
 * escaped, 0-terminated text exactly as compress() was given it; a buffer of at most one byte decodes to nothing.  rounds (nullable):
 * pointer-jumping rounds over the heads.  A buffer of two bytes or more that is no transform -- not exactly one 0 byte, or an LF mapping that
 * is not one cycle --: TDC_GPU_ERR_ARG, nothing written to the destination.  len >= 2^31 - 1: TDC_GPU_ERR_TOO_LARGE. */
int tdc_gpu_bwt_decompress(tdc_gpu_ctx* ctx, const uint8_t* bwt, size_t len, uint8_t** out, size_t* out_len, uint32_t* rounds);
int tdc_gpu_bwt_decompress_into(tdc_gpu_ctx* ctx, const uint8_t* bwt, size_t len, uint8_t* out, size_t out_cap, size_t* out_len,
                                uint32_t* rounds);
/* tests: the inverse with its two parameters exposed (0 = the library's choice): sample = expected rows between two list heads, max_steps =
 * most steps a walk takes in one launch.  out: len bytes; lf (nullable): len entries, the LF table; heads / launches (nullable): list heads
 * in the end, launches of the first walk. */
int tdc_gpu_bwt_inverse_stage(tdc_gpu_ctx* ctx, const uint8_t* bwt, size_t len, uint32_t sample, uint32_t max_steps, uint8_t* out,
                              uint32_t* lf, uint64_t* heads, uint32_t* launches);

/* bwt over a batch of independent texts, both directions (bwt_batch.hip; DESIGN.md section 5.2 "Batches" and "Batch decoder").  Text k
 * is in[off[k], off[k + 1]) (off: count + 1 entries, off[0] = 0, the texts back to back); a transform has exactly its text's length, so
 * result k is written to the same range of `out`, out[off[k], off[k + 1]): `out` needs off[count] bytes, there is no out_off and no bound
 * function.  The range of a refused text is left untouched, a refused text costs its neighbours nothing, and the call returns TDC_GPU_OK.
 * Result k is byte for byte what the single call returns for text k alone.
 * tdc_gpu_bwt_compress_batch: text k has the contract of tdc_gpu_bwt_compress (escaped, ONE terminating 0) and status[k] is that call's
 * code for it -- TDC_GPU_OK, TDC_GPU_ERR_NO_SENTINEL (also for the text of no bytes), TDC_GPU_ERR_ARG for an inner 0 -- with one
 * exception: a text of more than BWT_BATCH_TEXT_CAP = 2^20 = 1 048 576 bytes is TDC_GPU_ERR_TOO_LARGE, refused before any work (the batch
 * is built for many small texts; tdc_gpu_bwt_compress is the tool for a long one).  status[k] can also be TDC_GPU_ERR_INTERNAL: the text's
 * doubling rounds did not come to rest within the call's bound, bits_for(the longest accepted text) + 1 -- a bug of the library, not a
 * property of the text.  The suffix sort is
 * a prefix doubling over the unresolved positions of all texts at once, ranks never compared across texts.
 * tdc_gpu_bwt_decompress_batch: status[k] is the verdict of tdc_gpu_bwt_decompress on buffer k alone -- TDC_GPU_OK with the same bytes (a
 * buffer of 0 or 1 bytes is TDC_GPU_OK and writes nothing), TDC_GPU_ERR_ARG for a buffer of two or more bytes that has not exactly one 0
 * byte or whose LF mapping is not one cycle.  There is no cap per buffer; the LF cycles of all buffers are ranked as one forest of lists.
 * The call synchronises a constant number of times plus the launches of the first walk and the pointer-jumping rounds, whatever count is.
 * The call itself, decided from the arguments alone before the context is looked at, in this order: TDC_GPU_ERR_ARG for a NULL off or
 * status, off[0] != 0, a decreasing off or in == NULL with off[count] > 0; TDC_GPU_ERR_TOO_LARGE for off[count] > 2^32 - 2 (forward),
 * off[count] >= 2^31 - 1 (inverse: the top bit of an LF word marks a cut) or 2^31 texts and more; TDC_GPU_ERR_ARG for `out` overlapping
 * `in` and for a NULL context.  out == NULL or out_cap < off[count]: TDC_GPU_ERR_OOM, nothing written to `out`, status filled with
 * what needs no device (forward: the terminator and the lengths; inverse: TDC_GPU_OK).  TDC_GPU_ERR_OOM also if the device cannot hold the
 * arena: 64 bytes per text byte forward, 40 inverse, plus 64 MiB (DESIGN.md states the formulas).  count = 0 is valid.
 * Options of the context (tests; not enumerated by tdc_gpu_option_name): bwt_batch_sample (expected rows per list of the inverse) and
 * bwt_batch_steps (most steps of a walk per launch), 0 = the library's choice; the same bytes whatever they are.
 * stats (may be NULL): n, out_len, ms_h2d, ms_sa (forward: the sort; inverse: LF), ms_encode (forward: the gather; inverse: the walks and
 * the ranking), ms_d2h, ms_total, arena_bytes; len_rounds = the doubling rounds behind the initial sort (forward: the most any text
 * took) or the pointer-jumping rounds (inverse); forward: sa_sorted_elems = records sorted over all rounds; inverse: levels = launches
 * of the first walk, entries = list heads in the end, flen_max = the longest list. */
#define BWT_BATCH_TEXT_CAP ((size_t)1 << 20)
int tdc_gpu_bwt_compress_batch(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* off /* count + 1 */, size_t count, uint8_t* out,
                               size_t out_cap, int32_t* status /* count */, tdc_gpu_stats* stats);
int tdc_gpu_bwt_decompress_batch(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* off /* count + 1 */, size_t count, uint8_t* out,
                                 size_t out_cap, int32_t* status /* count */, tdc_gpu_stats* stats);
/* tests and later batches: the suffix arrays alone, sa[off[k] + i] = the i-th smallest suffix of text k, counted from the text's start
 * (off[count] entries; the range of a refused text is left untouched).  Arguments and status as for tdc_gpu_bwt_compress_batch. */
int tdc_gpu_suffix_array_batch(tdc_gpu_ctx* ctx, const uint8_t* in, const uint64_t* off /* count + 1 */, size_t count,
                               uint32_t* sa /* off[count] */, int32_t* status /* count */);

/* ---- rle, mtf, encode(huff), encode(sle) and chains of them behind bwt: the reference's `bwtzip = bwt:rle:mtf:encode(huff)`
 * (etc/compare-suites/default.suite).  A pipeline is a sequence of 1 .. 8 stages; every stage's whole output is the
 * next stage's input (tudocomp_driver/ChainCompressor.hpp: `a:b:c` = chain(chain(a, b), c)) and stays in device memory, only the last
 * one is downloaded.  One stage alone is a valid pipeline: that is how the three single compressors are reached.
 *   TDC_GPU_STAGE_BWT   BWTCompressor::compress (compressors/BWTCompressor.hpp:29-44).  Only as the FIRST stage: its input is the escaped,
 *                       0-terminated view, with the contract and the error codes of tdc_gpu_bwt_compress.
 *   TDC_GPU_STAGE_RLE   RunLengthEncoder::compress (compressors/RunLengthEncoder.hpp:15-32, util/vbyte.hpp:28-37), param = its option
 *                       `offset`.  The reference's loop compares a signed char with istream::peek(): a run of k bytes below 0x80 becomes
 *                       `c c vbyte(k - 2 + offset)`, bytes from 0x80 up never extend a run (every repeated one becomes `c vbyte(offset)`).
 *                       On an input that ends in 0xFF 0xFF the reference does not terminate; this library emits what it emits for such bytes
 *                       in mid-stream, which the reference's decoder decodes.
 *   TDC_GPU_STAGE_MTF   MTFCompressor::compress (compressors/MTFCompressor.hpp:16-33): move-to-front ranks, list 0 .. 255 at the start.
 *   TDC_GPU_STAGE_HUFF  LiteralEncoder<HuffmanCoder>::compress (compressors/LiteralEncoder.hpp:23-32): the algorithm `encode(huff)`.
 *   TDC_GPU_STAGE_SLE   LiteralEncoder<SLECoder>::compress (the same with coders/SLECoder.hpp): the algorithm `encode(sle)`, param = its
 *                       option `kmer`: 1 .. 7, 0 means the reference's default 3.  The stream is the ranking -- the bytes and the eta most
 *                       frequent k-byte windows of the input in Counter::getSorted order --, one class code per symbol (a k-mer symbol stands
 *                       for k bytes) and the bit stream's terminator.  The k-mer count of kmer 4 .. 7 sorts the
 *                       windows of the whole input: about 38 bytes of arena per input byte, TDC_GPU_ERR_OOM before anything is written if the
 *                       device cannot hold that.
 * Inputs of up to 2^32 - 2 bytes (bwt: < 2^31 - 1); a stage whose output would be longer fails with TDC_GPU_ERR_TOO_LARGE before it writes.
 * 0 or more than 8 stages, an unknown kind, bwt behind the first stage, an rle offset above 2^62, a kmer above 7: TDC_GPU_ERR_ARG. */
enum { TDC_GPU_STAGE_BWT = 0, TDC_GPU_STAGE_RLE = 1, TDC_GPU_STAGE_MTF = 2, TDC_GPU_STAGE_HUFF = 3, TDC_GPU_STAGE_SLE = 4 };
#define TDC_GPU_PIPELINE_MAX_STAGES 8
typedef struct { int kind; uint64_t param; } tdc_gpu_stage;      /* param: rle offset, sle kmer, 0 for the other kinds */
/* worst-case output length of the pipeline on n input bytes (what an _into buffer needs at most); 0 for an invalid pipeline or one
 * whose worst case passes 2^32 - 2 bytes */
size_t tdc_gpu_pipeline_bound(const tdc_gpu_stage* stages, int nstages, size_t n);
/* stats (nullable): n, out_len, pipe_stages, pipe_len[], pipe_ms[] (option pipe_log), ms_total, arena_bytes, and for a leading bwt the
 * fields tdc_gpu_bwt_compress fills. */
int tdc_gpu_pipeline_compress(tdc_gpu_ctx* ctx, const tdc_gpu_stage* stages, int nstages, const uint8_t* in, size_t n, uint8_t** out,
                              size_t* out_len, tdc_gpu_stats* stats);
/* into the CALLER's buffer of out_cap bytes; TDC_GPU_ERR_OOM with the required size in *out_len if it is too small.  The download runs
 * on the copy stream (page-locked memory -- tdc_gpu_host_alloc -- receives it at the host link's rate). */
int tdc_gpu_pipeline_compress_into(tdc_gpu_ctx* ctx, const tdc_gpu_stage* stages, int nstages, const uint8_t* in, size_t n, uint8_t* out,
                                   size_t out_cap, size_t* out_len, tdc_gpu_stats* stats);
/* ---- a chain over a batch: many independent texts in one call (bytestages_batch.hip, bwt_batch.hip; DESIGN.md section 5.3 "Batches").
 * Any chain of bwt (first only), rle, mtf and encode(huff).  The texts lie back to back in `in`: text k = in[in_off[k], in_off[k + 1]);
 * in_off has count + 1 entries, does not decrease, and in_off[0] = 0.  Stream k = out[out_off[k], out_off[k] + out_len[k]) is byte for byte
 * what tdc_gpu_pipeline_compress returns for text k alone with the same stages, the empty text included wherever that call accepts it:
 * nothing of one text reaches another one's stream -- no run spans a border, every text starts from the list 0 .. 255 and has its own
 * histogram, table, header and terminator.  out_off[k] is a multiple of 8, out_off[count] the number of bytes used; the bytes between two
 * streams are unspecified.  The intermediates of all texts stay in device memory; the call makes a constant number of launches and
 * synchronisations whatever count is (but for the doubling rounds of a leading bwt: tdc_gpu_bwt_compress_batch).
 * status[k] is the single call's code for text k alone -- under a leading bwt TDC_GPU_ERR_NO_SENTINEL, TDC_GPU_ERR_ARG for an inner 0 and
 * TDC_GPU_ERR_INTERNAL as documented for tdc_gpu_bwt_compress_batch -- with one exception that holds for every chain: a text of more than
 * BWT_BATCH_TEXT_CAP = 2^20 bytes is TDC_GPU_ERR_TOO_LARGE, refused before any work (the single call is the tool for a long text).  A
 * refused text has out_len[k] = 0 and costs its neighbours nothing; the call returns TDC_GPU_OK.
 * The call itself, decided from the arguments alone before the context is looked at, in this order: TDC_GPU_ERR_ARG for a NULL in_off,
 * out_off, out_len or status, in_off[0] != 0, a decreasing in_off, in == NULL with bytes to read; for the stage list what
 * tdc_gpu_pipeline_compress says (TDC_GPU_ERR_NO_SENTINEL for a bwt behind the first stage, TDC_GPU_ERR_ARG for an invalid list);
 * TDC_GPU_ERR_UNSUPPORTED for a list that holds TDC_GPU_STAGE_SLE; TDC_GPU_ERR_TOO_LARGE for more than 2^32 - 2 input bytes in all or
 * 2^31 texts and more; TDC_GPU_ERR_ARG for a NULL context.
 * The exact sizes are known before the last stage writes: out == NULL or an out_cap that is too small gives TDC_GPU_ERR_OOM with out_off,
 * out_len and status completely filled and the required total in out_off[count] -- nothing is written to `out`, the sizes pass alone.  A
 * stage whose output over the whole batch would pass 2^32 - 2 bytes: TDC_GPU_ERR_TOO_LARGE for the call, before anything is written to
 * `out`.  count = 0 is valid and writes only out_off[0] = 0.
 * Arena, reserved before any work (TDC_GPU_ERR_OOM if the device cannot hold it): n + 80 count bytes for the input, then the larger of
 * what tdc_gpu_bwt_compress_batch takes (64 n + 64 count + 64 MiB) and, summed over the byte stages with L = the stage's worst-case input,
 * 0.5625 L + 4624 count + 1 MiB of scratch plus the stage's worst-case output (tdc_gpu_pipeline_bound's terms; encode(huff) 1024 count more).
 * stats (may be NULL): n (all input bytes), out_len (bytes used), pipe_stages, pipe_len[i] = the bytes behind stage i summed over the
 * accepted texts, pipe_ms[i] (option pipe_log: one synchronisation per stage; the stage of encode(huff) includes the host's table build,
 * which the log prints on a line of its own), arena_bytes, ms_h2d, ms_d2h, ms_total, and for a leading bwt the fields
 * tdc_gpu_bwt_compress_batch fills.  Option pipe_batch_threads (not enumerated by tdc_gpu_option_name): host threads of that table build,
 * 0 = min(16, hardware threads); the same bytes on any number.
 * The streams are ordinary pipeline streams: tdc_gpu_pipeline_decompress, the host decoders below and tdc_gpu_bwt_decompress_batch decode
 * them.  A batch decoder of the chain and encode(sle) over a batch are not built. */
int tdc_gpu_pipeline_compress_batch(tdc_gpu_ctx* ctx, const tdc_gpu_stage* stages, int nstages,
                                    const uint8_t* in, const uint64_t* in_off /* count + 1 */, size_t count,
                                    uint8_t* out, size_t out_cap, uint64_t* out_off /* count + 1 */, uint64_t* out_len /* count */,
                                    int32_t* status /* count */, tdc_gpu_stats* stats);
/* what `out` of tdc_gpu_pipeline_compress_batch needs at most: the sum of tdc_gpu_pipeline_bound of every text, each rounded up to 8; a
 * text above the cap contributes 0.  0 for what the call refuses from its arguments (an encode(sle) stage and more than 2^32 - 2 bytes in
 * all among them). */
size_t tdc_gpu_pipeline_batch_bound(const tdc_gpu_stage* stages, int nstages, const uint64_t* in_off, size_t count);
/* Inverse, stage by stage from the last one, on the device: one upload of the stream, the decoders of rle, mtf, encode(huff) and encode(sle)
 * (csrc/bytestages_decode.hip) and the inverse of a leading bwt work from buffer to buffer in the arena, one download (*out then holds the
 * escaped, 0-terminated text if the pipeline starts with bwt).  Option dec_parse picks the path once per call from the stream's length:
 * 1 (default) = the device for streams of 1 MiB and more, 2 = the device for every stream, 0 = the host loops below, which are the
 * specification of the device decoders (same bytes, same refusals) and also take the call when the device cannot hold the arena.
 * Malformed input, or a stage that decodes to more than 2^32 - 2 bytes: TDC_GPU_ERR_ARG. */
int tdc_gpu_pipeline_decompress(tdc_gpu_ctx* ctx, const tdc_gpu_stage* stages, int nstages, const uint8_t* in, size_t len, uint8_t** out,
                                size_t* out_len);
int tdc_gpu_pipeline_decompress_into(tdc_gpu_ctx* ctx, const tdc_gpu_stage* stages, int nstages, const uint8_t* in, size_t len,
                                     uint8_t* out, size_t out_cap, size_t* out_len);
/* _into with stats (not NULL): n (the stream's length), out_len, pipe_stages, pipe_len[i] = the length behind stage i as in the stats of
 * the compress call (what stage i's decoder read), pipe_ms[] (option pipe_log), pipe_dev, ms_total, arena_bytes. */
int tdc_gpu_pipeline_decompress_stats(tdc_gpu_ctx* ctx, const tdc_gpu_stage* stages, int nstages, const uint8_t* in, size_t len,
                                      uint8_t* out, size_t out_cap, size_t* out_len, tdc_gpu_stats* stats);
/* The host decoders (no context, no GPU): rle_decode (RunLengthEncoder.hpp:36-50), MTFCompressor::decompress (MTFCompressor.hpp:35-43,
 * 60-68), LiteralEncoder::decompress (LiteralEncoder.hpp:34-41 with HuffmanCoder::Decoder).  out == NULL: nothing is written and *out_len
 * receives the decoded length.  Otherwise at most out_cap bytes are written; a text that does not fit is refused like malformed input
 * (*out_len still receives its length).  TDC_GPU_ERR_ARG for: a vbyte that runs off the end of the input or is longer than ten bytes, a
 * vbyte below `offset`, a Huffman header that is cut off or inconsistent, a code outside the table. */
int tdc_rle_decode(const uint8_t* in, size_t len, uint64_t offset, uint8_t* out, size_t out_cap, size_t* out_len);
int tdc_mtf_decode(const uint8_t* in, size_t len, uint8_t* out, size_t out_cap, size_t* out_len);
int tdc_huff_decode_literals(const uint8_t* in, size_t len, uint8_t* out, size_t out_cap, size_t* out_len);
/* The same contract for LiteralEncoder::decompress with SLECoder::Decoder (coders/SLECoder.hpp:311-416), kmer as TDC_GPU_STAGE_SLE's
 * param: the specification of the device decoder of encode(sle), the host path of the pipeline calls and the path for small streams.
 * TDC_GPU_ERR_ARG for: a kmer above 7, an empty stream, a ranking that does not end inside the stream, a ranking of more than 1024
 * symbols, a ranking entry that is neither a byte nor a k-mer of this kmer (marker byte 0xFF, zero bytes between the marker and the k
 * bytes), a rank outside the ranking (the reference reads out of bounds there), a code cut off by the end of the stream (the reference
 * reads zeros there).  TDC_GPU_ERR_TOO_LARGE for a text of more than 2^32 - 2 bytes. */
int tdc_sle_decode(const uint8_t* in, size_t len, uint32_t kmer, uint8_t* out, size_t out_cap, size_t* out_len);
/* The same contract for LZWCompressor::decompress (lzw::decode_step restated; coder TDC_GPU_CODER_BIT or TDC_GPU_CODER_GAMMA, else
 * TDC_GPU_ERR_UNSUPPORTED): the specification of tdc_gpu_lzw_decompress and its path for small streams.  TDC_GPU_ERR_ARG for what that
 * call refuses, TDC_GPU_ERR_TOO_LARGE for a text of more than 2^32 - 2 bytes. */
int tdc_lzw_decode(const uint8_t* in, size_t len, int coder, uint8_t* out, size_t out_cap, size_t* out_len);
/* The same contract for the lzss token stream (decode_text_internal, LCPCompressor.hpp:23-76) of an lzss_lcp (or lcpcomp) stream written with
 * TDC_GPU_CODER_HUFF, _BIT, _GAMMA, _DELTA or _ASCII (else TDC_GPU_ERR_UNSUPPORTED): the sequential loop, references resolved along their
 * chains.  The specification of tdc_gpu_lzss_lcp_decompress and its path for small streams.  TDC_GPU_ERR_ARG for: a text length the
 * stream cannot hold, more literals or a longer factor than the text has room for, src + len > n, len = 0, a unary prefix that runs
 * into the end of the stream or is longer than 64, a delta width above 64, a length that does not add up to n. */
int tdc_lzss_decode(const uint8_t* in, size_t len, int coder, uint8_t* out, size_t out_cap, size_t* out_len);

/* The same contract for LZSSSlidingWindowCompressor::decompress (:120-143) with the Decoder of TDC_GPU_CODER_ASCII, _BIT, _GAMMA or _DELTA
 * (else TDC_GPU_ERR_UNSUPPORTED): tokens until the stream ends.  window is the compressor's option; only coder=bit reads it (the width of
 * the length field; 0: TDC_GPU_ERR_ARG).  TDC_GPU_ERR_ARG for: a factor of distance 0 or of a distance above the text so far (the
 * reference reads out of bounds), a token cut off by the end of the stream (the reference reads zeros there), a unary prefix that runs
 * into the end of the stream or is longer than 64, a delta width above 64.  TDC_GPU_ERR_TOO_LARGE for a text of more than 2^32 - 2
 * bytes.  A factor of length 0 decodes to nothing, as in the reference. */
int tdc_lzss_sw_decode(const uint8_t* in, size_t len, int coder, uint32_t window, uint8_t* out, size_t out_cap, size_t* out_len);

/* RePairCompressor::decompress (:287-336) on the host with the Decoder of TDC_GPU_CODER_BIT, _ASCII, _GAMMA or _DELTA (else
 * TDC_GPU_ERR_UNSUPPORTED); rules are expanded with an explicit stack, not by recursion.  out == NULL: only *out_len is computed.
 * TDC_GPU_ERR_ARG for: a side of rule i that names a rule >= i (the reference would recurse for ever -- Range(i) holds i itself under
 * BitCoder when i is a power of two), a start symbol that names a rule >= rules, a field cut off by the end of the stream (the reference
 * reads zeros there), more rules than the stream has room for, and what the field readers refuse.  The lengths of the rules are summed
 * in 64 bits with saturation BEFORE any text is written: more than 2^32 - 2 bytes is TDC_GPU_ERR_TOO_LARGE, a buffer of fewer than
 * *out_len bytes TDC_GPU_ERR_OOM with the length in *out_len and `out` untouched. */
int tdc_repair_decode(const uint8_t* in, size_t len, int coder, uint8_t* out, size_t out_cap, size_t* out_len);

/* HuffmanCoder::Encoder + lzss::encode_text on a caller-supplied factor list sorted by pos (LZSSCoding.hpp:18-92) */
int tdc_gpu_encode_huff(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, const uint32_t* pos, const uint32_t* src,
                        const uint32_t* len, size_t z, uint8_t** out, size_t* out_len);

/* the same with ArithmeticCoder::Encoder as the literal coder (coders/ArithmeticCoder.hpp:35-177) */
int tdc_gpu_encode_arith(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, const uint32_t* pos, const uint32_t* src,
                         const uint32_t* len, size_t z, uint8_t** out, size_t* out_len);
/* coder = ASCIICoder (coders/ASCIICoder.hpp:29-50) */
int tdc_gpu_encode_ascii(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, const uint32_t* pos, const uint32_t* src,
                         const uint32_t* len, size_t z, uint8_t** out, size_t* out_len);
/* coder = SLECoder (coders/SLECoder.hpp:42-298), kmer = its option of that name (0 = default 3; 1..7) */
int tdc_gpu_encode_sle(tdc_gpu_ctx* ctx, const uint8_t* text, size_t n, const uint32_t* pos, const uint32_t* src,
                       const uint32_t* len, size_t z, uint32_t kmer, uint8_t** out, size_t* out_len);

/* ---- host-side helpers (no GPU) --------------------------------------------------------------------------- */
/* io/RestrictedBuffer.hpp:43-74 + io/EscapeMap.hpp:39-64 : 0x00 -> FF FE, 0xFF -> FF FF, append 0.
 * out must hold 2*n+1 bytes; returns the escaped length. */
size_t tdc_escape(const uint8_t* in, size_t n, uint8_t* out);
/* io/RestrictedIOStream.hpp:13-89 : inverse (drops the final 0); returns the length. */
size_t tdc_unescape(const uint8_t* in, size_t n, uint8_t* out);
/* coders/HuffmanCoder.hpp:442-474 : canonical code for a literal histogram (for tests of the host table builder) */
int tdc_huffman_table(const uint32_t counts[256], uint32_t* sigma, uint32_t* longest, uint8_t order[256],
                      uint8_t len_of[256], uint64_t code_of[256]);
/* compressors/LZ78Compressor.hpp:97-131 : the LZ78 parse on its own (host; what tdc_gpu_lz78_compress codes on the device).
 * ids[k] = id of the longest dictionary phrase at the start of factor k (0: none; ids count from 1 in insertion order), chars[k] = the byte
 * behind it, a leftover phrase at the end of the text as (parent id, last byte).  *ids / *chars are malloc'd (tdc_gpu_free). */
int tdc_lz78_factors(const uint8_t* in, size_t n, uint32_t** ids, uint8_t** chars, size_t* z);
/* compressors/LZWCompressor.hpp:39-108 : the LZW parse on its own (host; what tdc_gpu_lzw_compress codes on the device).  codes[k] = id of
 * the dictionary node phrase k ends in (0 .. 255: the bytes; 256 + j: phrase j and the byte behind it), the left-over phrase included; no
 * codes for the empty input.  *codes is malloc'd (tdc_gpu_free). */
int tdc_lzw_factors(const uint8_t* in, size_t n, uint32_t** codes, size_t* z);
/* compressors/LZSSSlidingWindowCompressor.hpp:39-118 : the greedy sliding-window parse on its own (host, one core; the specification of
 * tdc_gpu_lzss_sw_factorize), in the closed form stated at tdc_gpu_lzss_sw_compress -- no sliding buffer.  The factors sorted by pos;
 * pos / src / len are malloc'd (tdc_gpu_free).  Any window >= 1 (0: TDC_GPU_ERR_ARG); n above 2^32 - 2: TDC_GPU_ERR_TOO_LARGE. */
int tdc_lzss_sw_factors(const uint8_t* in, size_t n, uint32_t window, uint32_t threshold, uint32_t** pos, uint32_t** src, uint32_t** len,
                        size_t* z);
/* compressors/RePairCompressor.hpp:96-178 : the grammar on its own (host, one core, O(rules * n); the specification of
 * tdc_gpu_repair_grammar).  *rules (l << 32 | r) and *start are malloc'd (tdc_gpu_free).  max_rules 0: unlimited.  n above 2^30:
 * TDC_GPU_ERR_TOO_LARGE. */
int tdc_repair_grammar(const uint8_t* in, size_t n, uint64_t max_rules, uint64_t** rules, size_t* nrules, uint32_t** start, size_t* nstart);
/* The start-up check of tdc_gpu_ctx_create() on its own (no GPU): rebuilds two built-in fixture tables (sigma 40 and 200, many
 * equal counts) and compares them with what the reference build yields; TDC_GPU_ERR_INTERNAL if this build's C++ library
 * orders ties differently (coders/HuffmanCoder.hpp:88-120 heap functions, :455 unstable std::sort) -- every call with
 * coder=huff on a context then fails with the same code (the other coders, lz78 and decompression are not affected). */
int tdc_huffman_selfcheck(void);
/* synthetic corpora of the benchmark configurations */
int tdc_gen_english(uint8_t* out, size_t n, uint64_t seed);
int tdc_gen_dna(uint8_t* out, size_t n, uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif
