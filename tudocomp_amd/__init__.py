"""tudocomp_amd -- MI355X-native lcpcomp hot path behind tudocomp's Compressor surface.

Python face of the C ABI (include/tdc_gpu.h) used by the parity tests and bench.py.  The C++ facade that mirrors
tdc::Compressor / the `tdc` command line lives in tudocomp_amd/host/.  Nothing here computes on the CPU: every
method forwards to the HIP library and raises if it (or a GPU) is unavailable.
"""
import ctypes

import numpy as np

from . import _native
from ._native import Stats, Stage, LIB_PATH, SYMBOLS  # noqa: F401

CODER_HUFF = 0
CODER_GAMMA = 1
CODER_ARITH = 2
CODER_ASCII = 3
CODER_SLE = 4            # coder=sle(kmer=k): CODER_SLE | (k << 8), k = 0 means the reference's default 3
CODER_BIT = 5            # BitCoder: lzw, lzss_lcp, lzss, repair
CODER_DELTA = 6          # EliasDeltaCoder: lzss_lcp, lzss, repair
COMP_ARRAYS = 0
COMP_PLCPPEAKS = 1
COMP_MAXLCP = 2
COMP_HEAP = 3
STAGE_BWT = 0            # stages of a pipeline (tdc_gpu_stage.kind): a stage is a kind or (STAGE_RLE, offset)
STAGE_RLE = 1
STAGE_MTF = 2
STAGE_HUFF = 3
STAGE_SLE = 4            # encode(sle): STAGE_SLE or (STAGE_SLE, kmer), kmer 1 .. 7 (0 = the reference's default 3)


class TdcGpuError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        msg = _native.load().tdc_gpu_strerror(status).decode()
        super().__init__("%s (status %d)%s" % (msg, status, (": " + detail) if detail else ""))


def _u8(b):
    a = np.frombuffer(b, dtype=np.uint8) if isinstance(b, (bytes, bytearray, memoryview)) else np.ascontiguousarray(b, dtype=np.uint8)
    return a


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def escape(data):
    """Input restrictions 'escape {0} + null-terminate' (io/RestrictedBuffer.hpp:43-74): what Input::as_view() yields."""
    L = _native.load()
    a = _u8(data)
    out = np.empty(2 * len(a) + 1, dtype=np.uint8)
    n = L.tdc_escape(_ptr(a), len(a), _ptr(out))
    return out[:n].tobytes()


def unescape(data):
    L = _native.load()
    a = _u8(data)
    out = np.empty(len(a) + 1, dtype=np.uint8)
    n = L.tdc_unescape(_ptr(a), len(a), _ptr(out))
    return out[:n].tobytes()


def _gen_target(n, out):
    """the array a native generator fills: a fresh one, or the caller's -- which must really hold n contiguous bytes"""
    if out is None:
        return np.empty(n, dtype=np.uint8)
    if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.ndim != 1 or not out.flags.c_contiguous or out.size < n:
        raise ValueError("out must be a contiguous one-dimensional uint8 array of at least n bytes")
    return out


def gen_english(n, seed=42, out=None):
    """SURVEY.md 8d English-like generator; `out` (optional): a uint8 array of >= n bytes to fill in place."""
    out = _gen_target(n, out)
    _native.load().tdc_gen_english(_ptr(out), n, seed)
    return out[:n]


def gen_dna(n, seed=7, out=None):
    """SURVEY.md 8d DNA generator; `out` as in gen_english."""
    out = _gen_target(n, out)
    _native.load().tdc_gen_dna(_ptr(out), n, seed)
    return out[:n]


def lz78_factors(data):
    """The LZ78 parse on its own (host; compressors/LZ78Compressor.hpp:97-131): (ids, chars) as numpy arrays."""
    L = _native.load()
    a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    ids, ch, z = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
    rc = L.tdc_lz78_factors(_ptr(a) if len(a) else None, len(a), ctypes.byref(ids), ctypes.byref(ch), ctypes.byref(z))
    if rc:
        raise TdcGpuError(rc)
    try:
        i = np.ctypeslib.as_array(ctypes.cast(ids, ctypes.POINTER(ctypes.c_uint32)), (max(z.value, 1),))[:z.value].copy()
        c = np.ctypeslib.as_array(ctypes.cast(ch, ctypes.POINTER(ctypes.c_uint8)), (max(z.value, 1),))[:z.value].copy()
    finally:
        L.tdc_gpu_free(ids); L.tdc_gpu_free(ch)
    return i, c


def lzw_factors(data):
    """The LZW parse on its own (host; compressors/LZWCompressor.hpp:39-108): the codes as a numpy array."""
    L = _native.load()
    a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    codes, z = ctypes.c_void_p(), ctypes.c_size_t()
    rc = L.tdc_lzw_factors(_ptr(a) if len(a) else None, len(a), ctypes.byref(codes), ctypes.byref(z))
    if rc:
        raise TdcGpuError(rc)
    try:
        return np.ctypeslib.as_array(ctypes.cast(codes, ctypes.POINTER(ctypes.c_uint32)), (max(z.value, 1),))[:z.value].copy()
    finally:
        L.tdc_gpu_free(codes)


def lzss_sw_factors(data, window=16, threshold=3):
    """The sliding-window parse of lzss on its own (host, one core; compressors/LZSSSlidingWindowCompressor.hpp:39-118 in closed form):
    (pos, src, len) as numpy arrays, sorted by pos."""
    L = _native.load()
    a = _u8(data)
    p, s, l, z = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
    rc = L.tdc_lzss_sw_factors(_ptr(a) if len(a) else None, len(a), int(window), int(threshold), ctypes.byref(p), ctypes.byref(s),
                               ctypes.byref(l), ctypes.byref(z))
    if rc:
        raise TdcGpuError(rc, "tdc_lzss_sw_factors")
    try:
        return tuple(np.ctypeslib.as_array(ctypes.cast(x, ctypes.POINTER(ctypes.c_uint32)), (max(z.value, 1),))[:z.value].copy() for x in (p, s, l))
    finally:
        for x in (p, s, l):
            L.tdc_gpu_free(x)


def repair_grammar(data, max_rules=0):
    """The Re-Pair grammar on its own (host, one core, O(rules * n); compressors/RePairCompressor.hpp:96-178): (rules, start) as numpy
    arrays -- rules[k] = l << 32 | r (uint64; rule k is symbol 256 + k), start the sequence that is left (uint32)."""
    L = _native.load()
    a = _u8(data)
    r, s, nr, ns = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t()
    rc = L.tdc_repair_grammar(_ptr(a) if len(a) else None, len(a), int(max_rules), ctypes.byref(r), ctypes.byref(nr), ctypes.byref(s), ctypes.byref(ns))
    if rc:
        raise TdcGpuError(rc, "tdc_repair_grammar")
    try:
        return (np.frombuffer(ctypes.string_at(r, nr.value * 8), dtype=np.uint64).copy(),
                np.frombuffer(ctypes.string_at(s, ns.value * 4), dtype=np.uint32).copy())
    finally:
        L.tdc_gpu_free(r)
        L.tdc_gpu_free(s)


def option_names():
    """Names of the library's options (tdc_gpu_ctx_set_option)."""
    L = _native.load()
    return [L.tdc_gpu_option_name(i).decode() for i in range(L.tdc_gpu_option_count())]


def huffman_table(counts):
    L = _native.load()
    C = np.ascontiguousarray(counts, dtype=np.uint32)
    sigma, longest = ctypes.c_uint32(), ctypes.c_uint32()
    order = np.zeros(256, dtype=np.uint8)
    len_of = np.zeros(256, dtype=np.uint8)
    code_of = np.zeros(256, dtype=np.uint64)
    rc = L.tdc_huffman_table(_ptr(C), ctypes.byref(sigma), ctypes.byref(longest), _ptr(order), _ptr(len_of), _ptr(code_of))
    if rc:
        raise TdcGpuError(rc)
    return {"sigma": sigma.value, "longest": longest.value, "order": order, "len_of": len_of, "code_of": code_of}


def _stages(stages):
    """[kind | (kind, param), ...] -> (tdc_gpu_stage array, count)"""
    items = [(s, 0) if isinstance(s, int) else (int(s[0]), int(s[1])) for s in stages]
    arr = (Stage * max(len(items), 1))()
    for i, (k, p) in enumerate(items):
        arr[i].kind, arr[i].param = k, p
    return arr, len(items)


def pipeline_bound(stages, n):
    """worst-case output length of the pipeline on n bytes (0: invalid pipeline, or a worst case above 2^32 - 2 bytes)"""
    arr, k = _stages(stages)
    return _native.load().tdc_gpu_pipeline_bound(arr, k, n)


def _host_decode(fn, data, *args):
    """measure, then decode (the host decoders of the C ABI; no GPU)"""
    L = _native.load()
    a = _u8(data)
    n = ctypes.c_size_t()
    rc = getattr(L, fn)(_ptr(a) if len(a) else None, len(a), *args, None, 0, ctypes.byref(n))
    if rc:
        raise TdcGpuError(rc, fn)
    out = np.empty(max(n.value, 1), dtype=np.uint8)
    rc = getattr(L, fn)(_ptr(a) if len(a) else None, len(a), *args, _ptr(out), n.value, ctypes.byref(n))
    if rc:
        raise TdcGpuError(rc, fn)
    return out[:n.value].tobytes()


def rle_decode(data, offset=0):
    """rle_decode (compressors/RunLengthEncoder.hpp:36-50) on the host"""
    return _host_decode("tdc_rle_decode", data, ctypes.c_uint64(offset))


def mtf_decode(data):
    """MTFCompressor::decompress (compressors/MTFCompressor.hpp:35-43) on the host"""
    return _host_decode("tdc_mtf_decode", data)


def huff_decode_literals(data):
    """LiteralEncoder<HuffmanCoder>::decompress (compressors/LiteralEncoder.hpp:34-41) on the host"""
    return _host_decode("tdc_huff_decode_literals", data)


def sle_decode_literals(data, kmer=3):
    """LiteralEncoder<SLECoder>::decompress (compressors/LiteralEncoder.hpp:34-41, coders/SLECoder.hpp:311-416) on the host"""
    return _host_decode("tdc_sle_decode", data, ctypes.c_uint32(int(kmer)))


def lzw_decode(data, coder=CODER_BIT):
    """LZWCompressor::decompress (lzw::decode_step restated) on the host"""
    return _host_decode("tdc_lzw_decode", data, int(coder))


def lzss_decode(data, coder=CODER_HUFF):
    """decode_text_internal (LCPCompressor.hpp:23-76) on an lzss_lcp / lcpcomp stream of coder huff, bit, gamma, delta or ascii, on the
    host: the escaped, 0-terminated text"""
    return _host_decode("tdc_lzss_decode", data, int(coder))


def lzss_sw_decode(data, coder=CODER_BIT, window=16):
    """LZSSSlidingWindowCompressor::decompress (:120-143) on the host; only coder=bit reads `window`"""
    return _host_decode("tdc_lzss_sw_decode", data, int(coder), ctypes.c_uint32(int(window)))


def lzss_sw_bound(n, window=16, coder=CODER_BIT):
    """worst-case length of an lzss stream for n input bytes (0: a coder or a window lzss does not take)"""
    return _native.load().tdc_gpu_lzss_sw_bound(n, int(window), int(coder))


def _offsets(lengths):
    """in_off of a batch: count + 1 ascending uint64, the first one 0"""
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    if len(lengths):
        np.cumsum(np.asarray(lengths, dtype=np.uint64), out=off[1:])
    return off


def lzss_sw_batch_bound(lengths, window=16, coder=CODER_BIT):
    """what the output of lzss_sw_compress_batch needs at most for texts of these lengths: the single bounds, each rounded up to 8,
    summed (0: a coder or a window lzss does not take, or more than 2^32 - 2 bytes in all)"""
    off = _offsets(lengths)
    return _native.load().tdc_gpu_lzss_sw_batch_bound(_ptr(off), len(lengths), int(window), int(coder))


def pipeline_batch_bound(stages, lengths):
    """what the output of pipeline_compress_batch needs at most for texts of these lengths: pipeline_bound of every text, each rounded
    up to 8, summed; a text above 2^20 bytes contributes 0 (0: an invalid pipeline, an encode(sle) stage, more than 2^32 - 2 bytes in all)"""
    arr, k = _stages(stages)
    off = _offsets(lengths)
    return _native.load().tdc_gpu_pipeline_batch_bound(arr, k, _ptr(off), len(lengths))


def lzw_batch_bound(lengths, coder=CODER_BIT):
    """what the output of lzw_compress_batch needs at most for texts of these lengths (0: a coder lzw does not take, or more than
    2^32 - 2 bytes in all)"""
    off = _offsets(lengths)
    return _native.load().tdc_gpu_lzw_batch_bound(_ptr(off), len(lengths), int(coder))


def lz78_batch_bound(lengths, coder=CODER_GAMMA):
    """what the output of lz78_compress_batch needs at most for texts of these lengths (0: a coder lz78 does not take, or more than
    2^32 - 2 bytes in all)"""
    off = _offsets(lengths)
    return _native.load().tdc_gpu_lz78_batch_bound(_ptr(off), len(lengths), int(coder))


def repair_decode(data, coder=CODER_BIT):
    """RePairCompressor::decompress (:287-336) on the host, rules expanded with an explicit stack"""
    return _host_decode("tdc_repair_decode", data, int(coder))


def repair_bound(n, coder=CODER_BIT):
    """worst-case length of a repair stream for n input bytes (0: a coder or a length repair does not take)"""
    return _native.load().tdc_gpu_repair_bound(n, int(coder))


def repair_batch_bound(lengths, coder=CODER_BIT):
    """what the output of repair_compress_batch needs at most for texts of these lengths: the single bounds, each rounded up to 8,
    summed (0: a coder repair does not take, or more than 2^32 - 2 bytes in all)"""
    off = _offsets(lengths)
    return _native.load().tdc_gpu_repair_batch_bound(_ptr(off), len(lengths), int(coder))


def lzss_lcp_bound(n, coder=CODER_HUFF):
    """worst-case length of an lzss_lcp stream for a text of n bytes (0: a coder lzss_lcp does not take)"""
    return _native.load().tdc_gpu_lzss_lcp_bound(n, int(coder))


def device_count():
    return _native.load().tdc_gpu_device_count()


def blocks_compress(data, block_size, threshold=5, flatten=1, coder=CODER_HUFF, devices=None):
    """Block mode (tdc_gpu_blocks_compress): `data` (unrestricted bytes) is cut into blocks of block_size bytes, the blocks are
    spread over `devices` (default: all visible ones), every block becomes a complete lcpcomp stream.  Returns (container bytes,
    list of per-block stats dicts)."""
    L = _native.load()
    a = _u8(data)
    if devices is None:
        devices = list(range(max(1, device_count())))
    devs = (ctypes.c_int * len(devices))(*devices)
    G = L.tdc_gpu_blocks_count(len(a), block_size)
    st = (Stats * max(G, 1))()
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    rc = L.tdc_gpu_blocks_compress(devs, len(devices), _ptr(a), len(a), block_size, threshold, int(flatten), coder,
                                   ctypes.byref(out), ctypes.byref(n), st)
    if rc:
        raise TdcGpuError(rc, "tdc_gpu_blocks_compress")
    blob = ctypes.string_at(out, n.value)
    L.tdc_gpu_free(out)
    return blob, [st[i].as_dict() for i in range(G)]


class PinnedBuffer:
    """Page-locked host memory (tdc_gpu_host_alloc) as a numpy uint8 array `.a`; the buffers of the end-to-end entry point."""

    def __init__(self, nbytes):
        self._L = _native.load()
        self.nbytes = int(nbytes)
        self.ptr = self._L.tdc_gpu_host_alloc(self.nbytes)
        if not self.ptr:
            raise TdcGpuError(-5, "tdc_gpu_host_alloc(%d)" % self.nbytes)
        self.a = np.ctypeslib.as_array(ctypes.cast(self.ptr, ctypes.POINTER(ctypes.c_uint8)), shape=(max(self.nbytes, 1),))[:self.nbytes]

    def free(self):
        if getattr(self, "ptr", None):
            self.a = None
            self._L.tdc_gpu_host_free(self.ptr)
            self.ptr = None

    __del__ = free


def host_register(a):
    """page-lock the memory of a numpy array the caller allocated itself (e.g. a memory-mapped shared segment): True on success"""
    if not (isinstance(a, np.ndarray) and a.flags.c_contiguous):
        raise ValueError("host_register: a C-contiguous numpy array is needed")
    return _native.load().tdc_gpu_host_register(ctypes.c_void_p(a.ctypes.data), a.nbytes) == 0


def host_unregister(a):
    return _native.load().tdc_gpu_host_unregister(ctypes.c_void_p(a.ctypes.data)) == 0


class Context:
    """One GPU, three HIP streams, one device arena (tdc_gpu_ctx)."""

    def __init__(self, device=0, options=None):
        """options: {name: value} applied through tdc_gpu_ctx_set_option ("wsort_min" or "TDC_GPU_WSORT_MIN": the same option) --
        the way tests and A/B runs reach the library's switches; the environment is not read (include/tdc_gpu.h)."""
        self._L = _native.load()
        h = ctypes.c_void_p()
        rc = self._L.tdc_gpu_ctx_create(device, ctypes.byref(h))
        if rc:
            raise TdcGpuError(rc, "tdc_gpu_ctx_create(device=%d)" % device)
        self._h = h
        self.device = device
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def set_option(self, name, value):
        rc = self._L.tdc_gpu_ctx_set_option(self._h, str(name).encode(), int(value))
        if rc:
            raise TdcGpuError(rc, "unknown option %r" % (name,))

    def close(self):
        if getattr(self, "_h", None):
            self._L.tdc_gpu_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc:
            raise TdcGpuError(rc, self._L.tdc_gpu_last_error(self._h).decode())

    def _take(self, ptr, nbytes):
        out = ctypes.string_at(ptr, nbytes) if nbytes else b""
        self._L.tdc_gpu_free(ptr)
        return out

    def set_profiling(self, enabled=True):
        self._check(self._L.tdc_gpu_ctx_set_profiling(self._h, int(enabled)))

    def reset_profile(self):
        self._L.tdc_gpu_ctx_reset_profile(self._h)

    def kernel_profile(self):
        """{kernel name: {"ms", "launches", "bytes"}} since the last reset (only while profiling is enabled)."""
        out, i = {}, 0
        while True:
            ms, ln, by = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64()
            name = self._L.tdc_gpu_ctx_kernel_profile(self._h, i, ctypes.byref(ms), ctypes.byref(ln), ctypes.byref(by))
            if name is None:
                return out
            out[name.decode()] = {"ms": ms.value, "launches": ln.value, "bytes": by.value}
            i += 1

    def reserve(self, n):
        self._check(self._L.tdc_gpu_ctx_reserve(self._h, n))

    # ---- hot path --------------------------------------------------------------------------------------
    def lcpcomp_compress(self, text, threshold=5, flatten=1, coder=CODER_HUFF, comp=COMP_ARRAYS):
        """text: escaped + 0-terminated view.  Returns (compressed bytes, stats dict)."""
        a = _u8(text)
        out, n, st = ctypes.c_void_p(), ctypes.c_size_t(), Stats()
        if comp == COMP_ARRAYS:
            rc = self._L.tdc_gpu_lcpcomp_compress(self._h, _ptr(a), len(a), threshold, int(flatten), coder,
                                                  ctypes.byref(out), ctypes.byref(n), ctypes.byref(st))
        else:
            rc = self._L.tdc_gpu_lcpcomp_compress_comp(self._h, _ptr(a), len(a), threshold, int(flatten), coder, comp,
                                                       ctypes.byref(out), ctypes.byref(n), ctypes.byref(st))
        self._check(rc)
        return self._take(out, n.value), st.as_dict()

    def lcpcomp_compress_into(self, text, n, out, threshold=5, flatten=1, coder=CODER_HUFF, comp=COMP_ARRAYS):
        """End-to-end entry point: text (n bytes incl. sentinel) and out are host buffers (PinnedBuffer or numpy uint8 arrays);
        the stream is written into out.  Returns (out_len, stats)."""
        ta = text.a if isinstance(text, PinnedBuffer) else _u8(text)
        oa = out.a if isinstance(out, PinnedBuffer) else out
        ol, st = ctypes.c_size_t(), Stats()
        self._check(self._L.tdc_gpu_lcpcomp_compress_into(self._h, _ptr(ta), n, threshold, int(flatten), coder, comp, _ptr(oa), len(oa),
                                                          ctypes.byref(ol), ctypes.byref(st)))
        return ol.value, st.as_dict()

    def lcpcomp_compress_keep(self, text, n, threshold=5, flatten=1, coder=CODER_HUFF, comp=COMP_ARRAYS):
        """lcpcomp_compress_into without the download: the stream stays on the device until the next call on this context
        (stream_fetch copies it out).  Returns (out_len, stats)."""
        ta = text.a if isinstance(text, PinnedBuffer) else _u8(text)
        ol, st = ctypes.c_size_t(), Stats()
        self._check(self._L.tdc_gpu_lcpcomp_compress_keep(self._h, _ptr(ta), n, threshold, int(flatten), coder, comp, ctypes.byref(ol), ctypes.byref(st)))
        return ol.value, st.as_dict()

    def stream_fetch(self, out):
        """copy the stream kept by lcpcomp_compress_keep into the host buffer `out` (a writable, contiguous numpy uint8 array or a
        PinnedBuffer -- e.g. this rank's slice of a container in shared memory).  Returns the stream length."""
        oa = out.a if isinstance(out, PinnedBuffer) else out
        if not (isinstance(oa, np.ndarray) and oa.dtype == np.uint8 and oa.flags.c_contiguous and oa.flags.writeable):
            raise ValueError("stream_fetch: `out` must be a writable, C-contiguous uint8 array")
        ln = ctypes.c_size_t()
        self._check(self._L.tdc_gpu_stream_fetch(self._h, _ptr(oa), oa.size, ctypes.byref(ln)))
        return ln.value

    def stream_fetch_dev(self, d_dst, cap):
        """copy the kept stream to device memory of this context's GPU (`d_dst`: raw device pointer, `cap` bytes).  Returns its length."""
        ln = ctypes.c_size_t()
        self._check(self._L.tdc_gpu_stream_fetch_dev(self._h, ctypes.c_void_p(d_dst), cap, ctypes.byref(ln)))
        return ln.value

    def lcpcomp_compress_raw(self, data, threshold=5, flatten=1, coder=CODER_HUFF):
        """data: unrestricted input; escaping + sentinel happen on the device.  Returns (compressed bytes, stats dict)."""
        a = _u8(data)
        out, n, st = ctypes.c_void_p(), ctypes.c_size_t(), Stats()
        self._check(self._L.tdc_gpu_lcpcomp_compress_raw(self._h, _ptr(a), len(a), threshold, int(flatten), coder,
                                                         ctypes.byref(out), ctypes.byref(n), ctypes.byref(st)))
        return self._take(out, n.value), st.as_dict()

    def lcpcomp_compress_dev(self, d_text, n, d_out, out_cap, threshold=5, flatten=1, coder=CODER_HUFF):
        """Device-resident variant: d_text / d_out are raw device pointers (ints).  Returns (out_len, stats)."""
        ol, st = ctypes.c_size_t(), Stats()
        self._check(self._L.tdc_gpu_lcpcomp_compress_dev(self._h, ctypes.c_void_p(d_text), n, threshold, int(flatten),
                                                         coder, ctypes.c_void_p(d_out), out_cap, ctypes.byref(ol),
                                                         ctypes.byref(st)))
        return ol.value, st.as_dict()

    def lzss_lcp_compress(self, text, threshold=3, coder=CODER_HUFF):
        """LZSSLCPCompressor<coder>::compress on an escaped + 0-terminated view; coder: CODER_HUFF, _BIT, _GAMMA, _DELTA or _ASCII.
        Returns (stream, stats)."""
        a = _u8(text)
        out, n, st = ctypes.c_void_p(), ctypes.c_size_t(), Stats()
        self._check(self._L.tdc_gpu_lzss_lcp_compress(self._h, _ptr(a), len(a), threshold, coder, ctypes.byref(out),
                                                      ctypes.byref(n), ctypes.byref(st)))
        return self._take(out, n.value), st.as_dict()

    def lzss_lcp_compress_into(self, text, n, out, threshold=3, coder=CODER_HUFF):
        """lzss_lcp_compress of the first n bytes of `text` into a caller-owned buffer (PinnedBuffer or writable uint8 array; lzss_lcp_bound
        sizes it): returns (out_len, stats).  A buffer that is too small raises TdcGpuError (status -5) whose `required` is the length."""
        ta = text.a if isinstance(text, PinnedBuffer) else _u8(text)
        oa = out.a if isinstance(out, PinnedBuffer) else out
        ol, st = ctypes.c_size_t(), Stats()
        rc = self._L.tdc_gpu_lzss_lcp_compress_into(self._h, _ptr(ta), n, threshold, coder, _ptr(oa), oa.size, ctypes.byref(ol), ctypes.byref(st))
        if rc:
            self._raise_required(rc, ol.value)
        return ol.value, st.as_dict()

    lzss_lcp_bound = staticmethod(lzss_lcp_bound)

    def lzss_lcp_decompress(self, stream, coder=CODER_HUFF):
        """LZSSLCPCompressor::decompress for the five coders: returns the escaped, 0-terminated text and {"factors", "rounds",
        "device_parse"} (options dec_parse, dec_lean, dec_seg pick the path)."""
        a = stream.a if isinstance(stream, PinnedBuffer) else _u8(stream)
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        f, r = ctypes.c_uint64(), ctypes.c_uint32()
        self._check(self._L.tdc_gpu_lzss_lcp_decompress(self._h, _ptr(a) if len(a) else None, len(a), coder, ctypes.byref(p), ctypes.byref(n),
                                                        ctypes.byref(f), ctypes.byref(r)))
        return self._take(p, n.value), {"factors": f.value, "rounds": r.value,
                                        "device_parse": int(self._L.tdc_gpu_ctx_last_decode_on_device(self._h))}

    def lzss_lcp_decompress_into(self, stream, out, coder=CODER_HUFF):
        """lzss_lcp_decompress into a caller-owned buffer (a PinnedBuffer or a writable uint8 array): returns (text length, stats)."""
        a = stream.a if isinstance(stream, PinnedBuffer) else _u8(stream)
        oa = out.a if isinstance(out, PinnedBuffer) else out
        n = ctypes.c_size_t()
        f, r = ctypes.c_uint64(), ctypes.c_uint32()
        rc = self._L.tdc_gpu_lzss_lcp_decompress_into(self._h, _ptr(a) if len(a) else None, len(a), coder, _ptr(oa), oa.size, ctypes.byref(n),
                                                      ctypes.byref(f), ctypes.byref(r))
        if rc:
            self._raise_required(rc, n.value)
        return n.value, {"factors": f.value, "rounds": r.value, "device_parse": int(self._L.tdc_gpu_ctx_last_decode_on_device(self._h))}

    def lzss_lcp_factorize(self, text, threshold=3):
        a = _u8(text)
        p, s, l, z = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self._L.tdc_gpu_lzss_lcp_factorize(self._h, _ptr(a), len(a), threshold, ctypes.byref(p), ctypes.byref(s),
                                                       ctypes.byref(l), ctypes.byref(z)))
        out = [np.frombuffer(self._take(x, z.value * 4), dtype=np.uint32).copy() for x in (p, s, l)]
        return out[0], out[1], out[2]

    def lzss_sw_compress(self, data, window=16, threshold=3, coder=CODER_BIT):
        """LZSSSlidingWindowCompressor<coder>::compress on raw bytes (no escaping), factorized on the device; coder: CODER_ASCII, _BIT,
        _GAMMA or _DELTA.  Returns (stream, stats)."""
        a = data.a if isinstance(data, PinnedBuffer) else _u8(data)
        out, n, st = ctypes.c_void_p(), ctypes.c_size_t(), Stats()
        self._check(self._L.tdc_gpu_lzss_sw_compress(self._h, _ptr(a) if len(a) else None, len(a), int(window), int(threshold), coder,
                                                     ctypes.byref(out), ctypes.byref(n), ctypes.byref(st)))
        return self._take(out, n.value), st.as_dict()

    def lzss_sw_compress_into(self, data, n, out, window=16, threshold=3, coder=CODER_BIT):
        """lzss_sw_compress of the first n bytes of `data` into a caller-owned buffer (PinnedBuffer or writable uint8 array; lzss_sw_bound
        sizes it): returns (out_len, stats).  A buffer that is too small raises TdcGpuError (status -5) whose `required` is the length."""
        ta = data.a if isinstance(data, PinnedBuffer) else _u8(data)
        oa = out.a if isinstance(out, PinnedBuffer) else out
        ol, st = ctypes.c_size_t(), Stats()
        rc = self._L.tdc_gpu_lzss_sw_compress_into(self._h, _ptr(ta) if n else None, n, int(window), int(threshold), coder, _ptr(oa), oa.size,
                                                   ctypes.byref(ol), ctypes.byref(st))
        if rc:
            self._raise_required(rc, ol.value)
        return ol.value, st.as_dict()

    lzss_sw_bound = staticmethod(lzss_sw_bound)

    def lzss_sw_factorize(self, data, window=16, threshold=3):
        """the factors of the lzss parse from the device: (pos, src, len), sorted by pos"""
        a = _u8(data)
        p, s, l, z = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self._L.tdc_gpu_lzss_sw_factorize(self._h, _ptr(a) if len(a) else None, len(a), int(window), int(threshold), ctypes.byref(p),
                                                      ctypes.byref(s), ctypes.byref(l), ctypes.byref(z)))
        out = [np.frombuffer(self._take(x, z.value * 4), dtype=np.uint32).copy() for x in (p, s, l)]
        return out[0], out[1], out[2]

    def lzss_sw_decompress(self, stream, window=16, coder=CODER_BIT):
        """LZSSSlidingWindowCompressor::decompress: returns the text and {"factors", "rounds", "device_parse"}.  bit, gamma and delta
        streams of 1 MiB and more are parsed on the device (option dec_parse: 2 = every stream, 0 = never); ascii streams and smaller
        ones go through the host loop (lzss_sw_decode).  Only coder=bit reads `window`."""
        a = stream.a if isinstance(stream, PinnedBuffer) else _u8(stream)
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        f, r = ctypes.c_uint64(), ctypes.c_uint32()
        self._check(self._L.tdc_gpu_lzss_sw_decompress(self._h, _ptr(a) if len(a) else None, len(a), int(coder), int(window), ctypes.byref(p),
                                                       ctypes.byref(n), ctypes.byref(f), ctypes.byref(r)))
        return self._take(p, n.value), {"factors": f.value, "rounds": r.value,
                                        "device_parse": int(self._L.tdc_gpu_ctx_last_decode_on_device(self._h))}

    def lzss_sw_decompress_into(self, stream, out, window=16, coder=CODER_BIT):
        """lzss_sw_decompress into a caller-owned buffer (a PinnedBuffer or a writable uint8 array; `stream` may be a PinnedBuffer too):
        returns (text length, stats).  A buffer that is too small raises TdcGpuError (status -5) whose `required` is the text length."""
        a = stream.a if isinstance(stream, PinnedBuffer) else _u8(stream)
        oa = out.a if isinstance(out, PinnedBuffer) else out
        n = ctypes.c_size_t()
        f, r = ctypes.c_uint64(), ctypes.c_uint32()
        rc = self._L.tdc_gpu_lzss_sw_decompress_into(self._h, _ptr(a) if len(a) else None, len(a), int(coder), int(window), _ptr(oa), oa.size,
                                                     ctypes.byref(n), ctypes.byref(f), ctypes.byref(r))
        if rc:
            self._raise_required(rc, n.value)
        return n.value, {"factors": f.value, "rounds": r.value, "device_parse": int(self._L.tdc_gpu_ctx_last_decode_on_device(self._h))}

    def lzss_sw_compress_batch_into(self, data, in_off, out, window=16, threshold=3, coder=CODER_BIT):
        """tdc_gpu_lzss_sw_compress_batch on caller-owned buffers: text k = data[in_off[k]:in_off[k + 1]] (in_off: count + 1 uint64), the
        streams into `out` (PinnedBuffer or writable uint8 array; lzss_sw_batch_bound sizes it).  Returns (out_off, out_len, status,
        stats): stream k = out[out_off[k]:out_off[k] + out_len[k]], status[k] -6 for a text coder=bit would truncate.  A buffer that is
        too small raises TdcGpuError (status -5) whose `required` is the size."""
        ta = data.a if isinstance(data, PinnedBuffer) else _u8(data)
        oa = out.a if isinstance(out, PinnedBuffer) else out
        off = np.ascontiguousarray(in_off, dtype=np.uint64)
        count = len(off) - 1
        out_off, out_len = np.zeros(count + 1, dtype=np.uint64), np.zeros(max(count, 1), dtype=np.uint64)
        status, st = np.zeros(max(count, 1), dtype=np.int32), Stats()
        rc = self._L.tdc_gpu_lzss_sw_compress_batch(self._h, _ptr(ta) if len(ta) else None, _ptr(off), count, int(window), int(threshold),
                                                    int(coder), _ptr(oa), oa.size, _ptr(out_off), _ptr(out_len), _ptr(status), ctypes.byref(st))
        if rc:
            self._raise_required(rc, int(out_off[count]))
        return out_off, out_len[:count], status[:count], st.as_dict()

    def lzss_sw_compress_batch(self, texts, window=16, threshold=3, coder=CODER_BIT):
        """lzss over many independent texts in one call: returns (list of streams, statuses, stats).  Stream k is what lzss_sw_compress
        returns for texts[k] alone; where coder=bit would truncate a length of text k, statuses[k] is -6 and the stream is b""."""
        parts = [_u8(t) for t in texts]
        lengths = [len(a) for a in parts]
        off = _offsets(lengths)
        data = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
        cap = lzss_sw_batch_bound(lengths, window, coder)
        out = np.empty(max(cap, 8), dtype=np.uint8)
        out_off, out_len, status, st = self.lzss_sw_compress_batch_into(data, off, out, window, threshold, coder)
        streams = [out[int(o):int(o) + int(l)].tobytes() for o, l in zip(out_off[:-1], out_len)]
        return streams, status.tolist(), st

    def _lz_compress_batch_into(self, name, data, in_off, out, coder):
        ta = data.a if isinstance(data, PinnedBuffer) else _u8(data)
        oa = out.a if isinstance(out, PinnedBuffer) else out
        off = np.ascontiguousarray(in_off, dtype=np.uint64)
        count = len(off) - 1
        out_off, out_len = np.zeros(count + 1, dtype=np.uint64), np.zeros(max(count, 1), dtype=np.uint64)
        status, st = np.zeros(max(count, 1), dtype=np.int32), Stats()
        rc = getattr(self._L, "tdc_gpu_%s_compress_batch" % name)(self._h, _ptr(ta) if len(ta) else None, _ptr(off), count, int(coder), _ptr(oa),
                                                                  oa.size, _ptr(out_off), _ptr(out_len), _ptr(status), ctypes.byref(st))
        if rc:
            self._raise_required(rc, int(out_off[count]))
        return out_off, out_len[:count], status[:count], st.as_dict()

    def _lz_compress_batch(self, name, bound, texts, coder):
        parts = [_u8(t) for t in texts]
        lengths = [len(a) for a in parts]
        data = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
        out = np.empty(max(bound(lengths, coder), 8), dtype=np.uint8)
        out_off, out_len, status, st = self._lz_compress_batch_into(name, data, _offsets(lengths), out, coder)
        streams = [out[int(o):int(o) + int(l)].tobytes() for o, l in zip(out_off[:-1], out_len)]
        return streams, status.tolist(), st

    def lzw_compress_batch_into(self, data, in_off, out, coder=CODER_BIT):
        """tdc_gpu_lzw_compress_batch on caller-owned buffers: text k = data[in_off[k]:in_off[k + 1]] (in_off: count + 1 uint64), the
        streams into `out` (PinnedBuffer or writable uint8 array; lzw_batch_bound sizes it).  The texts are parsed on the device, one wave
        per text.  Returns (out_off, out_len, status, stats): stream k = out[out_off[k]:out_off[k] + out_len[k]], status[k] -4 for a text
        beyond the cap of one text (2^25 - 256 bytes).  A buffer that is too small raises TdcGpuError (status -5) whose `required` is the
        size."""
        return self._lz_compress_batch_into("lzw", data, in_off, out, coder)

    def lzw_compress_batch(self, texts, coder=CODER_BIT):
        """lzw over many independent texts in one call: returns (list of streams, statuses, stats).  Stream k is what lzw_compress returns
        for texts[k] alone; a refused text (statuses[k] != 0) yields b""."""
        return self._lz_compress_batch("lzw", lzw_batch_bound, texts, coder)

    def lz78_compress_batch_into(self, data, in_off, out, coder=CODER_GAMMA):
        """tdc_gpu_lz78_compress_batch on caller-owned buffers, as lzw_compress_batch_into; status[k] is also -6 for a text whose
        left-over phrase ends in a byte >= 0x80, the single call's refusal"""
        return self._lz_compress_batch_into("lz78", data, in_off, out, coder)

    def lz78_compress_batch(self, texts, coder=CODER_GAMMA):
        """lz78 over many independent texts in one call: returns (list of streams, statuses, stats).  Stream k is what lz78_compress
        returns for texts[k] alone; a refused text (statuses[k] -6 or -4) yields b""."""
        return self._lz_compress_batch("lz78", lz78_batch_bound, texts, coder)

    def lz_parse_batch(self, texts, lzw):
        """the device parse of a batch alone: returns (items, chars, statuses) -- items[k]: the uint32 codes (lzw) or phrase ids (lz78)
        of texts[k], what lzw_factors / lz78_factors compute on the host; chars[k]: the bytes of the lz78 pairs (None for lzw)"""
        parts = [_u8(t) for t in texts]
        lengths = [len(a) for a in parts]
        off = _offsets(lengths)
        data = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
        n, count = len(data), len(parts)
        items, chars = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint8)
        item_off, status = np.zeros(count + 1, dtype=np.uint64), np.zeros(max(count, 1), dtype=np.int32)
        self._check(self._L.tdc_gpu_lz_parse_batch(self._h, _ptr(data) if n else None, _ptr(off), count, 1 if lzw else 0, _ptr(items),
                                                   None if lzw else _ptr(chars), _ptr(item_off), _ptr(status)))
        cut = [(int(a), int(b)) for a, b in zip(item_off[:-1], item_off[1:])]
        return ([items[a:b].copy() for a, b in cut], None if lzw else [chars[a:b].tobytes() for a, b in cut], status[:count].tolist())

    def lzss_sw_decompress_batch_into(self, blob, s_off, s_len, out, coder, window=16):
        """tdc_gpu_lzss_sw_decompress_batch on caller-owned buffers: stream k = blob[s_off[k]:s_off[k] + s_len[k]], coder bit, gamma or
        delta, always on the device.  out: PinnedBuffer, writable uint8 array, or None for the sizes pass alone.  Returns (out_off,
        status, stats): text k = out[out_off[k]:out_off[k + 1]], status[k] what lzss_sw_decode says of stream k alone (0, -2, -4).
        out None or too small raises TdcGpuError (status -5) with `required`, `out_off` and `statuses` filled."""
        ba = blob.a if isinstance(blob, PinnedBuffer) else _u8(blob)
        oa = None if out is None else (out.a if isinstance(out, PinnedBuffer) else out)
        so, sl = np.ascontiguousarray(s_off, dtype=np.uint64), np.ascontiguousarray(s_len, dtype=np.uint64)
        count = len(so)
        out_off, status, st = np.zeros(count + 1, dtype=np.uint64), np.zeros(max(count, 1), dtype=np.int32), Stats()
        rc = self._L.tdc_gpu_lzss_sw_decompress_batch(self._h, _ptr(ba) if len(ba) else None, _ptr(so), _ptr(sl), count, int(coder), int(window),
                                                      None if oa is None else _ptr(oa), 0 if oa is None else oa.size, _ptr(out_off),
                                                      _ptr(status), ctypes.byref(st))
        if rc:
            err = TdcGpuError(rc, self._L.tdc_gpu_last_error(self._h).decode())
            err.required = int(out_off[count]) if rc == -5 else None
            err.out_off, err.statuses = out_off, status[:count]
            raise err
        return out_off, status[:count], st.as_dict()

    def lzss_sw_decompress_batch(self, streams, coder, window=16):
        """the decoder of lzss_sw_compress_batch, or of any list of lzss streams: returns (list of texts, statuses, stats); a refused
        stream (status -2 or -4, as lzss_sw_decode on it alone) yields b"" and disturbs no neighbour"""
        parts = [_u8(x) for x in streams]
        s_len = np.array([len(a) for a in parts], dtype=np.uint64)
        s_off = np.zeros(len(parts), dtype=np.uint64)
        pos = 0
        for k, a in enumerate(parts):                                 # every stream at a multiple of 8, as the compressor leaves them
            s_off[k] = pos
            pos += (len(a) + 7) & ~7
        blob = np.zeros(pos, dtype=np.uint8)
        for o, a in zip(s_off, parts):
            blob[int(o):int(o) + len(a)] = a
        try:
            self.lzss_sw_decompress_batch_into(blob, s_off, s_len, None, coder, window)
            need = 0
        except TdcGpuError as e:
            if e.status != -5:
                raise
            need = e.required
        out = np.empty(max(need, 1), dtype=np.uint8)
        out_off, status, st = self.lzss_sw_decompress_batch_into(blob, s_off, s_len, out, coder, window)
        texts = [out[int(a):int(b)].tobytes() for a, b in zip(out_off[:-1], out_off[1:])]
        return texts, status.tolist(), st

    lzss_sw_batch_bound = staticmethod(lzss_sw_batch_bound)

    def _lz_decompress_batch_into(self, name, blob, s_off, s_len, out, coder):
        ba = blob.a if isinstance(blob, PinnedBuffer) else _u8(blob)
        oa = None if out is None else (out.a if isinstance(out, PinnedBuffer) else out)
        so, sl = np.ascontiguousarray(s_off, dtype=np.uint64), np.ascontiguousarray(s_len, dtype=np.uint64)
        count = len(so)
        out_off, status, st = np.zeros(count + 1, dtype=np.uint64), np.zeros(max(count, 1), dtype=np.int32), Stats()
        rc = getattr(self._L, "tdc_gpu_%s_decompress_batch" % name)(self._h, _ptr(ba) if len(ba) else None, _ptr(so), _ptr(sl), count, int(coder),
                                                                    None if oa is None else _ptr(oa), 0 if oa is None else oa.size,
                                                                    _ptr(out_off), _ptr(status), ctypes.byref(st))
        if rc:
            err = TdcGpuError(rc, self._L.tdc_gpu_last_error(self._h).decode())
            err.required = int(out_off[count]) if rc == -5 else None
            err.out_off, err.statuses = out_off, status[:count]
            raise err
        return out_off, status[:count], st.as_dict()

    def _lz_decompress_batch(self, name, streams, coder):
        parts = [_u8(x) for x in streams]
        s_len = np.array([len(a) for a in parts], dtype=np.uint64)
        s_off = np.zeros(len(parts), dtype=np.uint64)
        pos = 0
        for k, a in enumerate(parts):                                 # every stream at a multiple of 8, as the compressor leaves them
            s_off[k] = pos
            pos += (len(a) + 7) & ~7
        blob = np.zeros(pos, dtype=np.uint8)
        for o, a in zip(s_off, parts):
            blob[int(o):int(o) + len(a)] = a
        try:
            self._lz_decompress_batch_into(name, blob, s_off, s_len, None, coder)
            need = 0
        except TdcGpuError as e:
            if e.status != -5:
                raise
            need = e.required
        out = np.empty(max(need, 1), dtype=np.uint8)
        out_off, status, st = self._lz_decompress_batch_into(name, blob, s_off, s_len, out, coder)
        texts = [out[int(a):int(b)].tobytes() for a, b in zip(out_off[:-1], out_off[1:])]
        return texts, status.tolist(), st

    def lzw_decompress_batch_into(self, blob, s_off, s_len, out, coder=CODER_BIT):
        """tdc_gpu_lzw_decompress_batch on caller-owned buffers: stream k = blob[s_off[k]:s_off[k] + s_len[k]], coder bit or gamma, always
        on the device, all streams in one pass.  out: PinnedBuffer, writable uint8 array, or None for the sizes alone.  Returns (out_off,
        status, stats): text k = out[out_off[k]:out_off[k + 1]], status[k] what lzw_decode says of stream k alone (0, -2, -4).  out None
        or too small raises TdcGpuError (status -5) with `required`, `out_off` and `statuses` filled."""
        return self._lz_decompress_batch_into("lzw", blob, s_off, s_len, out, coder)

    def lzw_decompress_batch(self, streams, coder=CODER_BIT):
        """the decoder of lzw_compress_batch, or of any list of lzw streams: returns (list of texts, statuses, stats); a refused stream
        (status -2 or -4, as lzw_decode on it alone) yields b"" and disturbs no neighbour"""
        return self._lz_decompress_batch("lzw", streams, coder)

    def lz78_decompress_batch_into(self, blob, s_off, s_len, out, coder=CODER_GAMMA):
        """tdc_gpu_lz78_decompress_batch on caller-owned buffers, as lzw_decompress_batch_into; status[k] is what lz78_decompress returns
        for stream k alone"""
        return self._lz_decompress_batch_into("lz78", blob, s_off, s_len, out, coder)

    def lz78_decompress_batch(self, streams):
        """the decoder of lz78_compress_batch, or of any list of lz78 streams: returns (list of texts, statuses, stats); a refused stream
        yields b"" and disturbs no neighbour"""
        return self._lz_decompress_batch("lz78", streams, CODER_GAMMA)

    def repair_compress(self, data, max_rules=0, coder=CODER_BIT):
        """RePairCompressor<coder>::compress on raw bytes (no escaping), the grammar built on the device; coder: CODER_BIT, _ASCII, _GAMMA
        or _DELTA.  Returns (stream, stats)."""
        a = data.a if isinstance(data, PinnedBuffer) else _u8(data)
        out, n, st = ctypes.c_void_p(), ctypes.c_size_t(), Stats()
        self._check(self._L.tdc_gpu_repair_compress(self._h, _ptr(a) if len(a) else None, len(a), int(max_rules), coder,
                                                    ctypes.byref(out), ctypes.byref(n), ctypes.byref(st)))
        return self._take(out, n.value), st.as_dict()

    def repair_compress_into(self, data, n, out, max_rules=0, coder=CODER_BIT):
        """repair_compress of the first n bytes of `data` into a caller-owned buffer (PinnedBuffer or writable uint8 array; repair_bound
        sizes it): returns (out_len, stats).  A buffer that is too small raises TdcGpuError (status -5) whose `required` is the length."""
        ta = data.a if isinstance(data, PinnedBuffer) else _u8(data)
        oa = out.a if isinstance(out, PinnedBuffer) else out
        ol, st = ctypes.c_size_t(), Stats()
        rc = self._L.tdc_gpu_repair_compress_into(self._h, _ptr(ta) if n else None, n, int(max_rules), coder, _ptr(oa), oa.size,
                                                  ctypes.byref(ol), ctypes.byref(st))
        if rc:
            self._raise_required(rc, ol.value)
        return ol.value, st.as_dict()

    repair_bound = staticmethod(repair_bound)

    def repair_compress_batch_into(self, data, in_off, out, max_rules=0, coder=CODER_BIT):
        """tdc_gpu_repair_compress_batch on caller-owned buffers: text k = data[in_off[k]:in_off[k + 1]] (in_off: count + 1 uint64), the
        streams into `out` (PinnedBuffer or writable uint8 array; repair_batch_bound sizes it).  The grammars are built on the device, one
        workgroup per text.  Returns (out_off, out_len, status, stats): stream k = out[out_off[k]:out_off[k] + out_len[k]], status[k] -4
        for a text beyond the cap of one text (2^24 bytes); stats["len_rounds"] counts the launches.  A buffer that is too small raises
        TdcGpuError (status -5) whose `required` is the size."""
        ta = data.a if isinstance(data, PinnedBuffer) else _u8(data)
        oa = out.a if isinstance(out, PinnedBuffer) else out
        off = np.ascontiguousarray(in_off, dtype=np.uint64)
        count = len(off) - 1
        out_off, out_len = np.zeros(count + 1, dtype=np.uint64), np.zeros(max(count, 1), dtype=np.uint64)
        status, st = np.zeros(max(count, 1), dtype=np.int32), Stats()
        rc = self._L.tdc_gpu_repair_compress_batch(self._h, _ptr(ta) if len(ta) else None, _ptr(off), count, int(max_rules), int(coder),
                                                   _ptr(oa), oa.size, _ptr(out_off), _ptr(out_len), _ptr(status), ctypes.byref(st))
        if rc:
            self._raise_required(rc, int(out_off[count]))
        return out_off, out_len[:count], status[:count], st.as_dict()

    def repair_compress_batch(self, texts, max_rules=0, coder=CODER_BIT):
        """repair over many independent texts in one call: returns (list of streams, statuses, stats).  Stream k is what repair_compress
        returns for texts[k] alone; a refused text (statuses[k] -4) yields b""."""
        parts = [_u8(t) for t in texts]
        lengths = [len(a) for a in parts]
        data = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
        out = np.empty(max(repair_batch_bound(lengths, coder), 8), dtype=np.uint8)
        out_off, out_len, status, st = self.repair_compress_batch_into(data, _offsets(lengths), out, max_rules, coder)
        streams = [out[int(o):int(o) + int(l)].tobytes() for o, l in zip(out_off[:-1], out_len)]
        return streams, status.tolist(), st

    repair_batch_bound = staticmethod(repair_batch_bound)

    def repair_decompress_batch_into(self, blob, s_off, s_len, out, coder=CODER_BIT):
        """tdc_gpu_repair_decompress_batch on caller-owned buffers, as lzw_decompress_batch_into: coder bit, gamma or delta, always on the
        device, the grammars of all streams as one forest.  status[k] is what repair_decode says of stream k alone (0, -2, -4), -2 for a
        gamma / delta field beyond the device's caps, or -6 for a grammar higher than option repair_dec_rounds."""
        return self._lz_decompress_batch_into("repair", blob, s_off, s_len, out, coder)

    def repair_decompress_batch(self, streams, coder=CODER_BIT):
        """the decoder of repair_compress_batch, or of any list of repair streams: returns (list of texts, statuses, stats); a refused
        stream yields b"" and disturbs no neighbour"""
        return self._lz_decompress_batch("repair", streams, coder)

    def repair_grammar_batch(self, texts, max_rules=0):
        """the grammars of a batch alone: returns (rules, start, statuses) -- rules[k] (uint64, l << 32 | r) and start[k] (uint32) are
        what repair_grammar computes for texts[k] on the host"""
        parts = [_u8(t) for t in texts]
        lengths = [len(a) for a in parts]
        off = _offsets(lengths)
        data = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
        n, count = len(data), len(parts)
        rules, start = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint32)
        rule_off, start_off = np.zeros(count + 1, dtype=np.uint64), np.zeros(count + 1, dtype=np.uint64)
        status = np.zeros(max(count, 1), dtype=np.int32)
        self._check(self._L.tdc_gpu_repair_grammar_batch(self._h, _ptr(data) if n else None, _ptr(off), count, int(max_rules), _ptr(rules),
                                                         _ptr(rule_off), _ptr(start), _ptr(start_off), _ptr(status)))
        return ([rules[int(a):int(b)].copy() for a, b in zip(rule_off[:-1], rule_off[1:])],
                [start[int(a):int(b)].copy() for a, b in zip(start_off[:-1], start_off[1:])], status[:count].tolist())

    def repair_grammar(self, data, max_rules=0):
        """the grammar from the device: (rules, start, stats) -- rules[k] = l << 32 | r (uint64), start the sequence that is left (uint32)"""
        a = data.a if isinstance(data, PinnedBuffer) else _u8(data)
        r, s, nr, ns, st = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t(), Stats()
        self._check(self._L.tdc_gpu_repair_grammar(self._h, _ptr(a) if len(a) else None, len(a), int(max_rules), ctypes.byref(r), ctypes.byref(nr),
                                                   ctypes.byref(s), ctypes.byref(ns), ctypes.byref(st)))
        return (np.frombuffer(self._take(r, nr.value * 8), dtype=np.uint64).copy(), np.frombuffer(self._take(s, ns.value * 4), dtype=np.uint32).copy(),
                st.as_dict())

    def repair_decompress_stats(self, stream, coder=CODER_BIT):
        """RePairCompressor::decompress with what the call did: returns (text, stats).  stats: the fields of
        tdc_gpu_repair_decompress_stats and "device_parse".  bit, gamma and delta streams of 1 MiB and more are decoded on the device
        (option dec_parse: 2 = every stream, 0 = never); ascii streams, smaller ones and grammars deeper than option repair_dec_rounds
        go through the host loop (repair_decode)."""
        a = stream.a if isinstance(stream, PinnedBuffer) else _u8(stream)
        n, st = ctypes.c_size_t(), Stats()
        probe = np.empty(1, dtype=np.uint8)      # the length first: no bytes are "too small" for every text but the empty one (the _into form decodes once)
        rc = self._L.tdc_gpu_repair_decompress_stats(self._h, _ptr(a) if len(a) else None, len(a), int(coder), _ptr(probe), 0, ctypes.byref(n),
                                                     ctypes.byref(st))
        if rc == 0:
            return b"", self._repair_dec_stats(st)
        if rc != -5:
            self._check(rc)
        out = np.empty(n.value, dtype=np.uint8)
        self._check(self._L.tdc_gpu_repair_decompress_stats(self._h, _ptr(a) if len(a) else None, len(a), int(coder), _ptr(out), out.size,
                                                            ctypes.byref(n), ctypes.byref(st)))
        return out[:n.value].tobytes(), self._repair_dec_stats(st)

    def repair_decompress_stats_into(self, stream, out, coder=CODER_BIT):
        """repair_decompress_stats into a caller-owned buffer (a PinnedBuffer or a writable uint8 array; `stream` may be a PinnedBuffer
        too): returns (text length, stats).  A buffer that is too small raises TdcGpuError (status -5) whose `required` is the length."""
        a = stream.a if isinstance(stream, PinnedBuffer) else _u8(stream)
        oa = out.a if isinstance(out, PinnedBuffer) else out
        n, st = ctypes.c_size_t(), Stats()
        rc = self._L.tdc_gpu_repair_decompress_stats(self._h, _ptr(a) if len(a) else None, len(a), int(coder), _ptr(oa), oa.size, ctypes.byref(n),
                                                     ctypes.byref(st))
        if rc:
            self._raise_required(rc, n.value)
        return n.value, self._repair_dec_stats(st)

    def _repair_dec_stats(self, st):
        d = st.as_dict()
        d["device_parse"] = int(self._L.tdc_gpu_ctx_last_decode_on_device(self._h))
        return d

    def repair_decompress(self, stream, coder=CODER_BIT):
        """tdc_gpu_repair_decompress: the text.  The path is repair_decompress_stats's."""
        a = _u8(stream)
        out, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self._L.tdc_gpu_repair_decompress(self._h, _ptr(a) if len(a) else None, len(a), coder, ctypes.byref(out), ctypes.byref(n)))
        return self._take(out, n.value)

    def repair_decompress_into(self, stream, out, coder=CODER_BIT):
        """the same into a caller-owned buffer: returns the length; too small raises TdcGpuError (status -5) with `required`"""
        a = _u8(stream)
        oa = out.a if isinstance(out, PinnedBuffer) else out
        n = ctypes.c_size_t()
        rc = self._L.tdc_gpu_repair_decompress_into(self._h, _ptr(a) if len(a) else None, len(a), coder, _ptr(oa), oa.size, ctypes.byref(n))
        if rc:
            self._raise_required(rc, n.value)
        return n.value

    def lz78_compress(self, data, coder=CODER_GAMMA):
        """LZ78Compressor<EliasGammaCoder>::compress on raw bytes (no escaping).  Returns (stream, stats)."""
        a = _u8(data)
        out, n, st = ctypes.c_void_p(), ctypes.c_size_t(), Stats()
        self._check(self._L.tdc_gpu_lz78_compress(self._h, _ptr(a), len(a), coder, ctypes.byref(out), ctypes.byref(n),
                                                  ctypes.byref(st)))
        return self._take(out, n.value), st.as_dict()

    def lzw_compress(self, data, coder=CODER_BIT):
        """LZWCompressor<BitCoder | EliasGammaCoder>::compress on raw bytes (no escaping).  Returns (stream, stats)."""
        a = _u8(data)
        out, n, st = ctypes.c_void_p(), ctypes.c_size_t(), Stats()
        self._check(self._L.tdc_gpu_lzw_compress(self._h, _ptr(a) if len(a) else None, len(a), coder, ctypes.byref(out), ctypes.byref(n),
                                                 ctypes.byref(st)))
        return self._take(out, n.value), st.as_dict()

    def bound(self, n, coder=None):
        return self._L.tdc_gpu_lcpcomp_bound(n) if coder is None else self._L.tdc_gpu_lcpcomp_bound_coder(n, coder)

    # ---- stages ----------------------------------------------------------------------------------------
    def sort_pairs_u64(self, keys, vals, algo=1):
        """The device sorts behind the suffix array (algo 0: LSD radix, 1: splitter partition); returns sorted copies."""
        k = np.ascontiguousarray(keys, dtype=np.uint64).copy()
        v = np.ascontiguousarray(vals, dtype=np.uint32).copy()
        self._check(self._L.tdc_gpu_sort_pairs_u64(self._h, _ptr(k), _ptr(v), len(k), int(algo)))
        return k, v

    # ---- the shared device primitives one by one (csrc/api_prims.hip; tests/test_gpu_prims.py) ------------
    _SCAN_OPS = {"sum_u32": (0, np.uint32), "sum_u64": (1, np.uint64), "max_u32": (2, np.uint32)}
    _SORT_KINDS = {"u32": (0, np.uint32), "u64": (1, np.uint64), "distinct": (2, np.uint64)}

    def prim_scan(self, op, data, in_place=False, want_total=True):
        """exclusive_sum_u32 / exclusive_sum_u64 / inclusive_max_u32 (op "sum_u32" | "sum_u64" | "max_u32"); returns (scan, total or None)."""
        code, dt = self._SCAN_OPS[op]
        a = np.ascontiguousarray(data, dtype=dt).copy()
        tot = np.zeros(1, dtype=dt) if want_total and code != 2 else None
        self._check(self._L.tdc_gpu_prim_scan(self._h, code, _ptr(a), len(a), int(bool(in_place)), _ptr(tot) if tot is not None else None))
        return a, (int(tot[0]) if tot is not None else None)

    def prim_sort_pairs(self, kind, keys, vals, begin_bit, end_bit):
        """radix_sort_pairs_u32 / radix_sort_pairs_u64 / sort_pairs_u64_distinct (kind "u32" | "u64" | "distinct") on bits
        [begin_bit, end_bit); returns the (keys, vals) of the buffer pair the primitive names."""
        code, dt = self._SORT_KINDS[kind]
        k = np.ascontiguousarray(keys, dtype=dt).copy()
        v = np.ascontiguousarray(vals, dtype=np.uint32).copy()
        if len(k) != len(v):
            raise ValueError("keys and vals differ in length")
        self._check(self._L.tdc_gpu_prim_sort_pairs(self._h, code, _ptr(k), _ptr(v), len(k), int(begin_bit), int(end_bit)))
        return k, v

    def prim_bucketed_scatter(self, idx, val, n_dst, fill=0xFFFFFFFF, permutation=False, second_tmp=True, offset=0):
        """bucketed_scatter_u32 into n_dst words that all hold `fill` beforehand; returns dst."""
        i = np.ascontiguousarray(idx, dtype=np.uint32)
        v = np.ascontiguousarray(val, dtype=np.uint32)
        if len(i) != len(v):
            raise ValueError("idx and val differ in length")
        dst = np.empty(int(n_dst), dtype=np.uint32)
        self._check(self._L.tdc_gpu_prim_bucketed_scatter(self._h, _ptr(i), _ptr(v), len(i), _ptr(dst), int(n_dst), int(fill),
                                                          int(bool(permutation)), int(bool(second_tmp)), int(offset)))
        return dst

    def prim_msd_partition(self, idx, val, bits, db):
        """msd_partition_pairs_u32; returns (out_idx, out_val)."""
        i = np.ascontiguousarray(idx, dtype=np.uint32).copy()
        v = np.ascontiguousarray(val, dtype=np.uint32).copy()
        if len(i) != len(v):
            raise ValueError("idx and val differ in length")
        self._check(self._L.tdc_gpu_prim_msd_partition(self._h, _ptr(i), _ptr(v), len(i), int(bits), int(db)))
        return i, v

    def prim_select(self, cls, want, src_a=None, src_b=None, fill_a=0xFFFFFFFF, fill_b=0xFFFFFFFFFFFFFFFF):
        """select_by_class; returns (outA, outB or None, count): all m output words, `fill` where the primitive wrote nothing."""
        c = np.ascontiguousarray(cls, dtype=np.uint8)
        m = len(c)
        a = None if src_a is None else np.ascontiguousarray(src_a, dtype=np.uint32)
        b = None if src_b is None else np.ascontiguousarray(src_b, dtype=np.uint64)
        if (a is not None and len(a) != m) or (b is not None and len(b) != m):
            raise ValueError("cls, src_a and src_b differ in length")
        oa = np.empty(m, dtype=np.uint32)
        ob = None if b is None else np.empty(m, dtype=np.uint64)
        cnt = ctypes.c_uint32(0)
        self._check(self._L.tdc_gpu_prim_select(self._h, _ptr(c), int(want), m, None if a is None else _ptr(a), None if b is None else _ptr(b),
                                                int(fill_a), int(fill_b), _ptr(oa), None if ob is None else _ptr(ob), ctypes.byref(cnt)))
        return oa, ob, cnt.value

    def prim_select_counts(self, cls, want, tile_counts, src_a=None, fill_a=0xFFFFFFFF):
        """select_by_class with the per-tile counts (2 048 classes per tile) handed in; returns (outA, count)."""
        c = np.ascontiguousarray(cls, dtype=np.uint8)
        m = len(c)
        t = np.ascontiguousarray(tile_counts, dtype=np.uint32)
        if len(t) != (m + 2047) // 2048:
            raise ValueError("one count per tile of 2048 classes")
        a = None if src_a is None else np.ascontiguousarray(src_a, dtype=np.uint32)
        if a is not None and len(a) != m:
            raise ValueError("cls and src_a differ in length")
        oa = np.empty(m, dtype=np.uint32)
        cnt = ctypes.c_uint32(0)
        self._check(self._L.tdc_gpu_prim_select_counts(self._h, _ptr(c), int(want), m, None if a is None else _ptr(a), _ptr(t),
                                                       int(fill_a), _ptr(oa), ctypes.byref(cnt)))
        return oa, cnt.value

    def prim_mark_orbit(self, nxt):
        """mark_orbit_u32; returns mark (u8)."""
        a = np.ascontiguousarray(nxt, dtype=np.uint32)
        mark = np.empty(len(a), dtype=np.uint8)
        self._check(self._L.tdc_gpu_prim_mark_orbit(self._h, _ptr(a), len(a), _ptr(mark)))
        return mark

    def prim_tile_entries(self, exits):
        """dx_entries on a (ntiles, states) table of u16 exits (0xFFFF: the chain ends in the tile); returns the entries (u16)."""
        a = np.ascontiguousarray(exits, dtype=np.uint16)
        ntiles, states = a.shape
        entry = np.empty(ntiles, dtype=np.uint16)
        self._check(self._L.tdc_gpu_prim_tile_entries(self._h, _ptr(a), ntiles, states, _ptr(entry)))
        return entry

    def prim_arena_fill(self, byte=None):
        """fill the whole scratch arena with `byte` (0 .. 255; None: fill nothing); returns (base, size), size 0 before the first
        allocation.  For the tests: what a call finds in its scratch is the leftovers of the calls before it."""
        base, size = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._L.tdc_gpu_prim_arena_fill(self._h, -1 if byte is None else int(byte), ctypes.byref(base), ctypes.byref(size)))
        return base.value, size.value

    def suffix_array(self, text):
        a = _u8(text)
        sa = np.empty(len(a), dtype=np.uint32)
        isa = np.empty(len(a), dtype=np.uint32)
        self._check(self._L.tdc_gpu_suffix_array(self._h, _ptr(a), len(a), _ptr(sa), _ptr(isa)))
        return sa, isa

    def textds(self, text):
        a = _u8(text)
        n = len(a)
        arrs = {k: np.empty(n, dtype=np.uint32) for k in ("sa", "isa", "phi", "plcp", "lcp")}
        m = ctypes.c_uint32()
        self._check(self._L.tdc_gpu_textds(self._h, _ptr(a), n, _ptr(arrs["sa"]), _ptr(arrs["isa"]), _ptr(arrs["phi"]),
                                           _ptr(arrs["plcp"]), _ptr(arrs["lcp"]), ctypes.byref(m)))
        arrs["maxlcp"] = m.value
        return arrs

    def lcpcomp_decompress(self, stream, coder=CODER_HUFF):
        """LCPCompressor::decompress on a lcpcomp / lzss_lcp stream written with coder huff, ascii or sle (CODER_SLE | kmer << 8):
        returns the escaped, 0-terminated text and {"factors", "rounds"}."""
        a = _u8(stream)
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        f, r = ctypes.c_uint64(), ctypes.c_uint32()
        self._check(self._L.tdc_gpu_lcpcomp_decompress_coder(self._h, _ptr(a), len(a), coder, ctypes.byref(p), ctypes.byref(n),
                                                             ctypes.byref(f), ctypes.byref(r)))
        return self._take(p, n.value), {"factors": f.value, "rounds": r.value,
                                        "device_parse": int(self._L.tdc_gpu_ctx_last_decode_on_device(self._h))}

    def lcpcomp_decompress_into(self, stream, out, coder=CODER_HUFF):
        """lcpcomp_decompress into a caller-owned buffer (a PinnedBuffer or a writable uint8 array; `stream` may be a PinnedBuffer too):
        returns (text length, {"factors", "rounds", "device_parse"})."""
        a = stream.a if isinstance(stream, PinnedBuffer) else _u8(stream)
        oa = out.a if isinstance(out, PinnedBuffer) else out
        n = ctypes.c_size_t()
        f, r = ctypes.c_uint64(), ctypes.c_uint32()
        self._check(self._L.tdc_gpu_lcpcomp_decompress_into(self._h, _ptr(a), len(a), coder, _ptr(oa), oa.size, ctypes.byref(n),
                                                            ctypes.byref(f), ctypes.byref(r)))
        return n.value, {"factors": f.value, "rounds": r.value, "device_parse": int(self._L.tdc_gpu_ctx_last_decode_on_device(self._h))}

    def lz78_decompress(self, stream, coder=CODER_GAMMA):
        """LZ78Compressor<EliasGammaCoder>::decompress, parsed on the device: returns the text and {"phrases", "rounds"}."""
        a = stream.a if isinstance(stream, PinnedBuffer) else _u8(stream)
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        f, r = ctypes.c_uint64(), ctypes.c_uint32()
        self._check(self._L.tdc_gpu_lz78_decompress(self._h, _ptr(a), len(a), coder, ctypes.byref(p), ctypes.byref(n),
                                                    ctypes.byref(f), ctypes.byref(r)))
        return self._take(p, n.value), {"phrases": f.value, "rounds": r.value}

    def lz78_decompress_into(self, stream, out, coder=CODER_GAMMA):
        """lz78_decompress into a caller-owned buffer (a PinnedBuffer or a writable uint8 array; `stream` may be a PinnedBuffer too):
        returns (text length, {"phrases", "rounds"}).  A buffer that is too small raises TdcGpuError (status -5) whose `required`
        is the text length."""
        a = stream.a if isinstance(stream, PinnedBuffer) else _u8(stream)
        oa = out.a if isinstance(out, PinnedBuffer) else out
        n = ctypes.c_size_t()
        f, r = ctypes.c_uint64(), ctypes.c_uint32()
        rc = self._L.tdc_gpu_lz78_decompress_into(self._h, _ptr(a), len(a), coder, _ptr(oa), oa.size, ctypes.byref(n),
                                                  ctypes.byref(f), ctypes.byref(r))
        if rc:
            err = TdcGpuError(rc, self._L.tdc_gpu_last_error(self._h).decode())
            err.required = n.value if rc == -5 else None
            raise err
        return n.value, {"phrases": f.value, "rounds": r.value}

    def lzw_decompress(self, stream, coder=CODER_BIT):
        """LZWCompressor::decompress: returns the text and {"codes", "rounds", "device_parse"} (option dec_parse picks the path)."""
        a = stream.a if isinstance(stream, PinnedBuffer) else _u8(stream)
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        f, r = ctypes.c_uint64(), ctypes.c_uint32()
        self._check(self._L.tdc_gpu_lzw_decompress(self._h, _ptr(a) if len(a) else None, len(a), coder, ctypes.byref(p), ctypes.byref(n),
                                                   ctypes.byref(f), ctypes.byref(r)))
        return self._take(p, n.value), {"codes": f.value, "rounds": r.value,
                                        "device_parse": int(self._L.tdc_gpu_ctx_last_decode_on_device(self._h))}

    def lzw_decompress_into(self, stream, out, coder=CODER_BIT):
        """lzw_decompress into a caller-owned buffer (a PinnedBuffer or a writable uint8 array; `stream` may be a PinnedBuffer too):
        returns (text length, stats).  A buffer that is too small raises TdcGpuError (status -5) whose `required` is the text length."""
        a = stream.a if isinstance(stream, PinnedBuffer) else _u8(stream)
        oa = out.a if isinstance(out, PinnedBuffer) else out
        n = ctypes.c_size_t()
        f, r = ctypes.c_uint64(), ctypes.c_uint32()
        rc = self._L.tdc_gpu_lzw_decompress_into(self._h, _ptr(a) if len(a) else None, len(a), coder, _ptr(oa), oa.size, ctypes.byref(n),
                                                 ctypes.byref(f), ctypes.byref(r))
        if rc:
            self._raise_required(rc, n.value)
        return n.value, {"codes": f.value, "rounds": r.value, "device_parse": int(self._L.tdc_gpu_ctx_last_decode_on_device(self._h))}

    # ---- bwt ---------------------------------------------------------------------------------------------
    def _raise_required(self, rc, n):
        err = TdcGpuError(rc, self._L.tdc_gpu_last_error(self._h).decode())
        err.required = n if rc == -5 else None
        raise err

    def bwt_compress(self, text):
        """BWTCompressor::compress: text is the escaped + 0-terminated view.  Returns (the transform, stats dict)."""
        a = text.a if isinstance(text, PinnedBuffer) else _u8(text)
        out, n, st = ctypes.c_void_p(), ctypes.c_size_t(), Stats()
        self._check(self._L.tdc_gpu_bwt_compress(self._h, _ptr(a), len(a), ctypes.byref(out), ctypes.byref(n), ctypes.byref(st)))
        return self._take(out, n.value), st.as_dict()

    def bwt_compress_into(self, text, n, out):
        """bwt_compress of the first n bytes of `text` into a caller-owned buffer (PinnedBuffer or writable uint8 array): returns
        (length, stats).  A buffer that is too small raises TdcGpuError (status -5) whose `required` is n."""
        ta = text.a if isinstance(text, PinnedBuffer) else _u8(text)
        oa = out.a if isinstance(out, PinnedBuffer) else out
        ol, st = ctypes.c_size_t(), Stats()
        rc = self._L.tdc_gpu_bwt_compress_into(self._h, _ptr(ta), n, _ptr(oa), oa.size, ctypes.byref(ol), ctypes.byref(st))
        if rc:
            self._raise_required(rc, ol.value)
        return ol.value, st.as_dict()

    def bwt_decompress(self, bwt):
        """BWTCompressor::decompress on the device: returns the escaped, 0-terminated text and {"rounds"}."""
        a = bwt.a if isinstance(bwt, PinnedBuffer) else _u8(bwt)
        p, n, r = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_uint32()
        self._check(self._L.tdc_gpu_bwt_decompress(self._h, _ptr(a), len(a), ctypes.byref(p), ctypes.byref(n), ctypes.byref(r)))
        return self._take(p, n.value), {"rounds": r.value}

    def bwt_decompress_into(self, bwt, out, n=None):
        """bwt_decompress of the first n bytes of `bwt` (default: all of it) into a caller-owned buffer: returns (text length, {"rounds"}).
        A buffer that is too small raises TdcGpuError (status -5) whose `required` is the text length."""
        a = bwt.a if isinstance(bwt, PinnedBuffer) else _u8(bwt)
        oa = out.a if isinstance(out, PinnedBuffer) else out
        ol, r = ctypes.c_size_t(), ctypes.c_uint32()
        rc = self._L.tdc_gpu_bwt_decompress_into(self._h, _ptr(a), len(a) if n is None else n, _ptr(oa), oa.size, ctypes.byref(ol), ctypes.byref(r))
        if rc:
            self._raise_required(rc, ol.value)
        return ol.value, {"rounds": r.value}

    def bwt_inverse_stage(self, bwt, sample=0, max_steps=0, want_lf=True):
        """the inverse with its parameters exposed (0 = the library's choice): sample = expected rows between two list heads, max_steps =
        most steps of a walk per launch.  Returns (text, {"lf", "heads", "launches"})."""
        a = _u8(bwt)
        out = np.empty(len(a), dtype=np.uint8)
        lf = np.empty(len(a), dtype=np.uint32) if want_lf else None
        h, ln = ctypes.c_uint64(), ctypes.c_uint32()
        self._check(self._L.tdc_gpu_bwt_inverse_stage(self._h, _ptr(a), len(a), int(sample), int(max_steps), _ptr(out),
                                                      _ptr(lf) if want_lf else None, ctypes.byref(h), ctypes.byref(ln)))
        return (out.tobytes() if len(a) > 1 else b""), {"lf": lf, "heads": h.value, "launches": ln.value}

    def _bwt_batch_into(self, fn, data, off, out):
        ta = data.a if isinstance(data, PinnedBuffer) else _u8(data)
        oa = out.a if isinstance(out, PinnedBuffer) else out
        if oa is not None and not (isinstance(oa, np.ndarray) and oa.dtype == np.uint8 and oa.flags.c_contiguous and oa.flags.writeable):
            raise TypeError("out must be a PinnedBuffer or a writable, contiguous uint8 array")      # (the call writes oa.size bytes from its first one)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        count = len(off) - 1
        status, st = np.zeros(max(count, 1), dtype=np.int32), Stats()
        rc = fn(self._h, _ptr(ta) if len(ta) else None, _ptr(off), count, _ptr(oa) if oa is not None and oa.size else None,
                oa.size if oa is not None else 0, _ptr(status), ctypes.byref(st))
        if rc:
            self._raise_required(rc, int(off[count]))
        return status[:count], st.as_dict()

    def bwt_compress_batch_into(self, data, off, out):
        """tdc_gpu_bwt_compress_batch on caller-owned buffers: text k = data[off[k]:off[k + 1]] (off: count + 1 uint64, the escaped,
        0-terminated views back to back), its transform into the same range of `out` (PinnedBuffer or writable uint8 array of off[count]
        bytes).  Returns (status, stats): status[k] is what bwt_compress says of text k alone (0, -3, -2), or -4 for a text beyond the
        cap of one text (BWT_BATCH_TEXT_CAP = 2^20 bytes); the range of a refused text is left untouched.  A buffer that is too small
        raises TdcGpuError (status -5) whose `required` is off[count]."""
        return self._bwt_batch_into(self._L.tdc_gpu_bwt_compress_batch, data, off, out)

    def bwt_decompress_batch_into(self, data, off, out):
        """tdc_gpu_bwt_decompress_batch on caller-owned buffers, laid out as for bwt_compress_batch_into: returns (status, stats);
        status[k] is the verdict of bwt_decompress on buffer k alone (0, or -2 for what is no transform).  A buffer of 0 or 1 bytes is
        accepted and writes nothing."""
        return self._bwt_batch_into(self._L.tdc_gpu_bwt_decompress_batch, data, off, out)

    def _bwt_batch(self, into, items, short):
        parts = [_u8(t) for t in items]
        lengths = [len(a) for a in parts]
        off = _offsets(lengths)
        data = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
        out = np.zeros(max(len(data), 1), dtype=np.uint8)
        status, st = into(data, off, out)
        res = [out[int(a):int(b)].tobytes() if s == 0 and int(b) - int(a) > short else b"" for a, b, s in zip(off[:-1], off[1:], status)]
        return res, status.tolist(), st

    def bwt_compress_batch(self, texts):
        """bwt over many independent texts in one call: returns (list of transforms, statuses, stats).  Transform k is what bwt_compress
        returns for texts[k] alone; a refused text yields b\"\"."""
        return self._bwt_batch(self.bwt_compress_batch_into, texts, 0)

    def bwt_decompress_batch(self, bwts):
        """the inverse of bwt_compress_batch, or of any list of transforms: returns (list of texts, statuses, stats); a refused buffer
        and a buffer of at most one byte yield b\"\", and none disturbs a neighbour"""
        return self._bwt_batch(self.bwt_decompress_batch_into, bwts, 1)

    def suffix_array_batch(self, texts):
        """the suffix arrays of many independent texts in one call: returns (list of uint32 arrays, statuses, stats); array k holds
        positions counted from the start of texts[k], a refused text yields an empty array.  The C call keeps no statistics: stats
        holds n, the bytes of all texts, and zeros."""
        parts = [_u8(t) for t in texts]
        lengths = [len(a) for a in parts]
        off = _offsets(lengths)
        data = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
        sa = np.zeros(max(len(data), 1), dtype=np.uint32)
        status = np.zeros(max(len(parts), 1), dtype=np.int32)
        self._check(self._L.tdc_gpu_suffix_array_batch(self._h, _ptr(data) if len(data) else None, _ptr(off), len(parts), _ptr(sa), _ptr(status)))
        status = status[:len(parts)]
        res = [sa[int(a):int(b)].copy() if s == 0 else np.zeros(0, dtype=np.uint32) for a, b, s in zip(off[:-1], off[1:], status)]
        st = Stats()
        st.n = len(data)
        return res, status.tolist(), st.as_dict()

    # ---- rle, mtf, encode(huff) and chains ------------------------------------------------------------------
    def pipeline_compress(self, stages, data):
        """stages: [STAGE_* | (STAGE_RLE, offset), ...], intermediates stay on the device.  A leading STAGE_BWT takes the escaped +
        0-terminated view.  Returns (stream, stats dict with pipe_len / pipe_ms per stage)."""
        arr, k = _stages(stages)
        a = data.a if isinstance(data, PinnedBuffer) else _u8(data)
        out, n, st = ctypes.c_void_p(), ctypes.c_size_t(), Stats()
        self._check(self._L.tdc_gpu_pipeline_compress(self._h, arr, k, _ptr(a) if len(a) else None, len(a), ctypes.byref(out), ctypes.byref(n), ctypes.byref(st)))
        return self._take(out, n.value), st.as_dict()

    def pipeline_compress_into(self, stages, data, n, out):
        """pipeline_compress of the first n bytes of `data` into a caller-owned buffer (PinnedBuffer or writable uint8 array): returns
        (length, stats).  A buffer that is too small raises TdcGpuError (status -5) whose `required` is the stream length."""
        arr, k = _stages(stages)
        a = data.a if isinstance(data, PinnedBuffer) else _u8(data)
        oa = out.a if isinstance(out, PinnedBuffer) else out
        ol, st = ctypes.c_size_t(), Stats()
        rc = self._L.tdc_gpu_pipeline_compress_into(self._h, arr, k, _ptr(a), n, _ptr(oa), oa.size, ctypes.byref(ol), ctypes.byref(st))
        if rc:
            self._raise_required(rc, ol.value)
        return ol.value, st.as_dict()

    def pipeline_compress_batch_into(self, stages, data, in_off, out):
        """tdc_gpu_pipeline_compress_batch on caller-owned buffers: text k = data[in_off[k]:in_off[k + 1]] (in_off: count + 1 uint64), any
        chain of bwt (first only), rle, mtf and encode(huff); the streams into `out` (PinnedBuffer, writable uint8 array, or None for
        the sizes alone).  Returns (out_off, out_len, status, stats): stream k = out[out_off[k]:out_off[k] + out_len[k]] is what
        pipeline_compress returns for text k alone, status[k] that call's code (-4 for a text above 2^20 bytes).  A buffer that is
        missing or too small raises TdcGpuError (status -5) whose `required` is the size and whose `sizes` is (out_off, out_len,
        status), complete."""
        arr, k = _stages(stages)
        ta = data.a if isinstance(data, PinnedBuffer) else _u8(data)
        oa = out.a if isinstance(out, PinnedBuffer) else out
        off = np.ascontiguousarray(in_off, dtype=np.uint64)
        count = len(off) - 1
        out_off, out_len = np.zeros(count + 1, dtype=np.uint64), np.zeros(max(count, 1), dtype=np.uint64)
        status, st = np.zeros(max(count, 1), dtype=np.int32), Stats()
        rc = self._L.tdc_gpu_pipeline_compress_batch(self._h, arr, k, _ptr(ta) if len(ta) else None, _ptr(off), count,
                                                     _ptr(oa) if oa is not None else None, oa.size if oa is not None else 0,
                                                     _ptr(out_off), _ptr(out_len), _ptr(status), ctypes.byref(st))
        if rc:
            try:
                self._raise_required(rc, int(out_off[count]))
            except TdcGpuError as e:
                e.sizes = (out_off, out_len[:count], status[:count])
                raise
        return out_off, out_len[:count], status[:count], st.as_dict()

    def pipeline_compress_batch(self, stages, texts):
        """a chain over many independent texts in one call: returns (list of streams, statuses, stats).  Stream k is what
        pipeline_compress returns for texts[k] alone, b"" where statuses[k] is not 0.  The buffer is sized by the call's sizes pass,
        not by pipeline_batch_bound (encode(huff) is bounded by 8 n + 1024 per text)."""
        parts = [_u8(t) for t in texts]
        off = _offsets([len(a) for a in parts])
        data = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
        required = 0
        try:
            self.pipeline_compress_batch_into(stages, data, off, None)
        except TdcGpuError as e:
            if e.status != -5 or getattr(e, "required", None) is None:
                raise
            required = int(e.required)
        out = np.empty(max(required, 8), dtype=np.uint8)
        out_off, out_len, status, st = self.pipeline_compress_batch_into(stages, data, off, out)
        streams = [out[int(o):int(o) + int(l)].tobytes() for o, l in zip(out_off[:-1], out_len)]
        return streams, status.tolist(), st

    pipeline_batch_bound = staticmethod(pipeline_batch_bound)

    def pipeline_decompress(self, stages, stream):
        """inverse of pipeline_compress, stage by stage on the device (option dec_parse: 1 = streams of 1 MiB and more, 2 = every stream,
        0 = the host loops for rle, mtf and encode(huff))"""
        arr, k = _stages(stages)
        a = stream.a if isinstance(stream, PinnedBuffer) else _u8(stream)
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self._L.tdc_gpu_pipeline_decompress(self._h, arr, k, _ptr(a) if len(a) else None, len(a), ctypes.byref(p), ctypes.byref(n)))
        return self._take(p, n.value)

    def pipeline_decompress_into(self, stages, stream, out, n=None):
        """pipeline_decompress of the first n bytes of `stream` (default: all) into a caller-owned buffer: returns the text length"""
        arr, k = _stages(stages)
        a = stream.a if isinstance(stream, PinnedBuffer) else _u8(stream)
        oa = out.a if isinstance(out, PinnedBuffer) else out
        ol = ctypes.c_size_t()
        rc = self._L.tdc_gpu_pipeline_decompress_into(self._h, arr, k, _ptr(a), len(a) if n is None else n, _ptr(oa), oa.size, ctypes.byref(ol))
        if rc:
            self._raise_required(rc, ol.value)
        return ol.value

    def pipeline_decompress_stats(self, stages, stream, out, n=None):
        """pipeline_decompress_into with stats: returns (text length, stats dict).  pipe_len[i] = the length behind stage i as in the stats
        of pipeline_compress, pipe_ms per stage with option pipe_log, pipe_dev: bit i = stage i ran on the device."""
        arr, k = _stages(stages)
        a = stream.a if isinstance(stream, PinnedBuffer) else _u8(stream)
        oa = out.a if isinstance(out, PinnedBuffer) else out
        ol, st = ctypes.c_size_t(), Stats()
        rc = self._L.tdc_gpu_pipeline_decompress_stats(self._h, arr, k, _ptr(a) if len(a) else None, len(a) if n is None else n, _ptr(oa), oa.size, ctypes.byref(ol), ctypes.byref(st))
        if rc:
            self._raise_required(rc, ol.value)
        return ol.value, st.as_dict()

    def blocks_decompress(self, blob, coder=CODER_HUFF):
        """inverse of blocks_compress on this context's device: the concatenated raw bytes"""
        a = _u8(blob)
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self._L.tdc_gpu_blocks_decompress(self._h, _ptr(a), len(a), coder, ctypes.byref(p), ctypes.byref(n)))
        return self._take(p, n.value)

    def factorize(self, text, threshold=5, flatten=0):
        """Returns (pos, src, len) sorted by pos and the stats dict."""
        a = _u8(text)
        p, s, l = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        z, st = ctypes.c_size_t(), Stats()
        self._check(self._L.tdc_gpu_lcpcomp_factorize(self._h, _ptr(a), len(a), threshold, int(flatten), ctypes.byref(p),
                                                      ctypes.byref(s), ctypes.byref(l), ctypes.byref(z), ctypes.byref(st)))
        out = [np.frombuffer(self._take(x, z.value * 4), dtype=np.uint32).copy() for x in (p, s, l)]
        return out[0], out[1], out[2], st.as_dict()

    def flatten(self, n, pos, src, length):
        pos = np.ascontiguousarray(pos, dtype=np.uint32)
        src = np.ascontiguousarray(src, dtype=np.uint32).copy()
        length = np.ascontiguousarray(length, dtype=np.uint32)
        nf, md = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._L.tdc_gpu_flatten(self._h, n, _ptr(pos), _ptr(src), _ptr(length), len(pos), ctypes.byref(nf),
                                            ctypes.byref(md)))
        return src, nf.value, md.value

    def encode_sle(self, text, pos, src, length, kmer=3):
        """SLECoder::Encoder (coders/SLECoder.hpp:42-298) + lzss::encode_text on a given factor list"""
        a = _u8(text)
        pos = np.ascontiguousarray(pos, dtype=np.uint32)
        src = np.ascontiguousarray(src, dtype=np.uint32)
        length = np.ascontiguousarray(length, dtype=np.uint32)
        out, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self._L.tdc_gpu_encode_sle(self._h, _ptr(a), len(a), _ptr(pos), _ptr(src), _ptr(length), len(pos), int(kmer),
                                               ctypes.byref(out), ctypes.byref(n)))
        return self._take(out, n.value)

    def encode_ascii(self, text, pos, src, length):
        return self.encode_huff(text, pos, src, length, _fn="tdc_gpu_encode_ascii")

    def encode_arith(self, text, pos, src, length):
        return self.encode_huff(text, pos, src, length, _fn="tdc_gpu_encode_arith")

    def encode_huff(self, text, pos, src, length, _fn="tdc_gpu_encode_huff"):
        a = _u8(text)
        pos = np.ascontiguousarray(pos, dtype=np.uint32)
        src = np.ascontiguousarray(src, dtype=np.uint32)
        length = np.ascontiguousarray(length, dtype=np.uint32)
        out, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(getattr(self._L, _fn)(self._h, _ptr(a), len(a), _ptr(pos), _ptr(src), _ptr(length), len(pos),
                                                ctypes.byref(out), ctypes.byref(n)))
        return self._take(out, n.value)


class LCPCompressor:
    """Mirror of tdc::LCPCompressor<coder, ArraysComp, ...> (compressors/LCPCompressor.hpp:79-151) as the
    reference's test harness drives it (test/test/util.hpp:442-463): the input is wrapped with the compressor's
    input restrictions (escape {0}, null-terminate) and handed to compress()."""

    def __init__(self, ctx, coder="huff", threshold=5, flatten=1, comp="arrays", kmer=3):
        if coder not in ("huff", "arithmetic", "ascii", "sle") or comp not in ("arrays", "plcppeaks", "max_lcp", "heap"):
            # same wording as Registry.hpp:214
            raise RuntimeError("No implementation found for compressor lcpcomp(coder=%s,comp=%s)" % (coder, comp))
        self.ctx, self.threshold, self.flatten = ctx, int(threshold), int(flatten)
        self.coder = {"huff": CODER_HUFF, "arithmetic": CODER_ARITH, "ascii": CODER_ASCII, "sle": CODER_SLE | (int(kmer) << 8)}[coder]
        self.comp = {"arrays": COMP_ARRAYS, "plcppeaks": COMP_PLCPPEAKS, "max_lcp": COMP_MAXLCP, "heap": COMP_HEAP}[comp]
        self.last_stats = None

    def compress(self, data):
        out, st = self.ctx.lcpcomp_compress(escape(data), self.threshold, self.flatten, self.coder, self.comp)
        self.last_stats = st
        return out

    def decompress(self, stream):
        """LCPCompressor::decompress (coder huff / ascii / sle): references resolved on the device; the harness then removes
        the input restrictions again (unescape, drop the sentinel)."""
        if self.coder == CODER_ARITH:
            raise RuntimeError("lcpcomp(coder=arithmetic) streams cannot be decoded (neither can the reference)")
        text, _ = self.ctx.lcpcomp_decompress(stream, self.coder)
        return unescape(text)


class BWTCompressor:
    """Mirror of tdc::BWTCompressor (compressors/BWTCompressor.hpp:14-67): the Burrows-Wheeler transform of the input wrapped with the
    compressor's input restrictions (escape {0}, null-terminate); decompress() inverts it on the device and removes them again."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.last_stats = None

    def compress(self, data):
        out, st = self.ctx.bwt_compress(escape(data))
        self.last_stats = st
        return out

    def decompress(self, stream):
        text, _ = self.ctx.bwt_decompress(stream)
        return unescape(text) if text else b""

    def compress_batch(self, datas):
        """every input on its own in one device call: (list of transforms, statuses); transform k is compress(datas[k]), b"" where
        the text is refused (status -4: its escaped view is longer than BWT_BATCH_TEXT_CAP)"""
        out, status, st = self.ctx.bwt_compress_batch([escape(d) for d in datas])
        self.last_stats = st
        return out, status

    def decompress_batch(self, streams):
        """(list of inputs, statuses), all transforms inverted in one pass: entry k is decompress(streams[k]), None where the buffer
        is refused (status -2: no transform)"""
        texts, status, st = self.ctx.bwt_decompress_batch(streams)
        self.last_stats = st
        return [None if s else (unescape(t) if t else b"") for t, s in zip(texts, status)], status


def parse_chain(spec):
    """`a:b:c` (util/algorithm_parser/AlgorithmAST.hpp:119-129: chain(chain(a, b), c)) -> stage list; a, b, c out of bwt, rle,
    rle(offset=N), mtf, encode(huff), encode(sle), encode(sle(kmer=K)), encode(coder=sle(kmer=K))"""
    import re
    stages = []
    for part in str(spec).replace(" ", "").split(":"):
        m = re.fullmatch(r"rle(?:\((?:offset=(\d+))?\))?", part)
        sle = re.fullmatch(r"encode\((?:coder=)?sle(?:\((?:kmer=(-?\d+))?\))?\)", part)
        if m:
            stages.append((STAGE_RLE, int(m.group(1) or 0)))
        elif part in ("bwt", "bwt()"):
            stages.append((STAGE_BWT, 0))
        elif part in ("mtf", "mtf()"):
            stages.append((STAGE_MTF, 0))
        elif part in ("encode(huff)", "encode(coder=huff)", "encode"):
            stages.append((STAGE_HUFF, 0))
        elif sle:
            kmer = sle.group(1)
            if kmer is not None and not 1 <= int(kmer) <= 7:
                raise RuntimeError("sle: kmer must be in 1..7, not %s" % kmer)
            stages.append((STAGE_SLE, int(kmer or 3)))
        else:
            raise RuntimeError("No implementation found for compressor %s" % part)
    return stages


class ChainCompressor:
    """Mirror of tdc::ChainCompressor (tudocomp_driver/ChainCompressor.hpp) for chains of bwt, rle, mtf, encode(huff) and encode(sle), e.g. the
    reference's bwtzip = "bwt:rle:mtf:encode(huff)": every stage's whole output is the next stage's input, on the device.  Only a
    leading bwt has input restrictions: its input is escaped + 0-terminated, and unescaped again on the way back."""

    def __init__(self, ctx, spec):
        self.ctx, self.stages = ctx, parse_chain(spec)
        self.last_stats = None

    def compress(self, data):
        lead = self.stages[0][0] == STAGE_BWT
        out, st = self.ctx.pipeline_compress(self.stages, escape(data) if lead else data)
        self.last_stats = st
        return out

    def decompress(self, stream):
        text = self.ctx.pipeline_decompress(self.stages, stream)
        if self.stages[0][0] == STAGE_BWT:
            return unescape(text) if text else b""
        return text

    def compress_batch(self, datas):
        """every input on its own in one device call: (list of streams, statuses); stream k is compress(datas[k]), b"" where the text
        is refused (status -4: it -- under a leading bwt its escaped view -- is longer than 2^20 bytes).  A chain with encode(sle)
        raises TdcGpuError with status -6: it has no batch form.  The streams are decompress()'s; a batch decoder is not built."""
        lead = self.stages[0][0] == STAGE_BWT
        out, status, st = self.ctx.pipeline_compress_batch(self.stages, [escape(d) for d in datas] if lead else datas)
        self.last_stats = st
        return out, status


class RunLengthEncoder(ChainCompressor):
    """Mirror of tdc::RunLengthEncoder (compressors/RunLengthEncoder.hpp:52-74), option offset"""

    def __init__(self, ctx, offset=0):
        ChainCompressor.__init__(self, ctx, "rle(offset=%d)" % int(offset))


class MTFCompressor(ChainCompressor):
    """Mirror of tdc::MTFCompressor (compressors/MTFCompressor.hpp:45-69)"""

    def __init__(self, ctx):
        ChainCompressor.__init__(self, ctx, "mtf")


class LiteralEncoder(ChainCompressor):
    """Mirror of tdc::LiteralEncoder<coder> (compressors/LiteralEncoder.hpp:11-42), the algorithm `encode(coder)`; coder huff, or sle
    with its option kmer (1 .. 7).  dec="gpu": decompress() through the pipeline (the device for streams of 1 MiB and more, option
    dec_parse); dec="host": the host loop, which needs no context."""

    def __init__(self, ctx, coder="huff", kmer=3, dec="gpu"):
        if coder not in ("huff", "sle") or dec not in ("gpu", "host"):
            raise RuntimeError("No implementation found for compressor encode(coder=%s, dec=%s)" % (coder, dec))
        self.coder, self.kmer, self.dec = coder, int(kmer), dec
        ChainCompressor.__init__(self, ctx, "encode(huff)" if coder == "huff" else "encode(sle(kmer=%d))" % int(kmer))

    def decompress(self, stream):
        if self.dec == "host":
            return huff_decode_literals(stream) if self.coder == "huff" else sle_decode_literals(stream, self.kmer)
        return ChainCompressor.decompress(self, stream)


class LZ78Compressor:
    """Mirror of tdc::LZ78Compressor<coder, trie> (compressors/LZ78Compressor.hpp:45-161); no input restrictions."""

    def __init__(self, ctx, coder="gamma", lz78trie="ternary"):
        if coder != "gamma":
            raise RuntimeError("No implementation found for compressor lz78(coder=%s,lz78trie=%s)" % (coder, lz78trie))
        self.ctx = ctx
        self.last_stats = None

    def compress(self, data):
        out, st = self.ctx.lz78_compress(data)
        self.last_stats = st
        return out

    def decompress(self, stream):
        """LZ78Compressor::decompress (:142-160): the stream is parsed and the phrases are expanded on the device."""
        text, _ = self.ctx.lz78_decompress(stream)
        return text

    def compress_batch(self, texts):
        """every text on its own in one device call, parsed there: (list of streams, statuses); stream k is compress(texts[k])"""
        out, status, st = self.ctx.lz78_compress_batch(texts, CODER_GAMMA)
        self.last_stats = st
        return out, status

    def decompress_batch(self, streams):
        """(list of texts, statuses) on the device, all streams in one pass; text k is decompress(streams[k]), b"" where it is refused"""
        out, status, st = self.ctx.lz78_decompress_batch(streams)
        self.last_stats = st
        return out, status


class LZWCompressor:
    """Mirror of tdc::LZWCompressor<coder, trie> (compressors/LZWCompressor.hpp:19-135); no input restrictions.  coder: bit (the
    reference's default) or gamma; lz78trie is accepted and ignored (every back-end yields the same ids); dict_size must be 0.
    dec="host": the host loop that restates lzw::decode_step; dec="gpu": the device decoder (tdc_gpu_lzw_decompress)."""

    _CODERS = {"bit": CODER_BIT, "gamma": CODER_GAMMA}

    def __init__(self, ctx, coder="bit", lz78trie="ternary", dec="host", dict_size=0):
        if coder not in self._CODERS:
            raise RuntimeError("No implementation found for compressor lzw(coder=%s,lz78trie=%s)" % (coder, lz78trie))
        if int(dict_size) != 0:
            raise RuntimeError("lzw: dict_size=%s is not available (only 0, the unlimited dictionary)" % (dict_size,))
        if dec not in ("host", "gpu"):
            raise RuntimeError("lzw: dec must be host or gpu")
        self.ctx, self.coder, self.dec = ctx, self._CODERS[coder], dec
        self.last_stats = None

    def compress(self, data):
        out, st = self.ctx.lzw_compress(data, self.coder)
        self.last_stats = st
        return out

    def decompress(self, stream):
        if self.dec == "gpu":
            return self.ctx.lzw_decompress(stream, self.coder)[0]
        return lzw_decode(stream, self.coder)

    def compress_batch(self, texts):
        """every text on its own in one device call, parsed there: (list of streams, statuses); stream k is compress(texts[k])"""
        out, status, st = self.ctx.lzw_compress_batch(texts, self.coder)
        self.last_stats = st
        return out, status

    def decompress_batch(self, streams):
        """(list of texts, statuses) on the device, all streams in one pass, whatever dec says; text k is decompress(streams[k]), b""
        where it is refused"""
        out, status, st = self.ctx.lzw_decompress_batch(streams, self.coder)
        self.last_stats = st
        return out, status


class LZSSSlidingWindowCompressor:
    """Mirror of tdc::LZSSSlidingWindowCompressor<coder> (compressors/LZSSSlidingWindowCompressor.hpp:15-144), the algorithm `lzss`; no
    input restrictions.  coder: ascii, bit, gamma or delta (it has no default in the reference); window 1 .. 4096, threshold.  The parse
    runs on the device.  dec="host": decompress() is the host loop (lzss_sw_decode), which needs no context; dec="gpu" (an addition, as
    for lz78 / lzw): the device decoder (tdc_gpu_lzss_sw_decompress).  The stream is the same either way."""

    _CODERS = {"ascii": CODER_ASCII, "bit": CODER_BIT, "gamma": CODER_GAMMA, "delta": CODER_DELTA}

    def __init__(self, ctx, coder=None, window=16, threshold=3, dec="host"):
        if coder not in self._CODERS:
            raise RuntimeError("No implementation found for compressor lzss(coder=%s)" % coder)
        if not 1 <= int(window) <= 4096:
            raise RuntimeError("lzss: window=%s is not available (1 .. 4096)" % (window,))
        if dec not in ("host", "gpu"):
            raise RuntimeError("lzss: dec must be host or gpu")
        self.ctx, self.coder, self.window, self.threshold, self.dec = ctx, self._CODERS[coder], int(window), int(threshold), dec
        self.last_stats = None

    def compress(self, data):
        out, st = self.ctx.lzss_sw_compress(data, self.window, self.threshold, self.coder)
        self.last_stats = st
        return out

    def decompress(self, stream):
        if self.dec == "gpu":
            if self.ctx is None:
                raise RuntimeError("lzss: dec=gpu needs a context")
            return self.ctx.lzss_sw_decompress(stream, self.window, self.coder)[0]
        return lzss_sw_decode(stream, self.coder, self.window)

    def compress_batch(self, texts):
        """every text on its own in one device call: (list of streams, statuses); stream k is compress(texts[k])"""
        out, status, st = self.ctx.lzss_sw_compress_batch(texts, self.window, self.threshold, self.coder)
        self.last_stats = st
        return out, status

    def decompress_batch(self, streams):
        """(list of texts, statuses) on the device, one wave per stream; coder=ascii loops the host decoder"""
        if self.coder == CODER_ASCII:
            out, status = [], []
            for x in streams:
                try:
                    out.append(lzss_sw_decode(x, self.coder, self.window))
                    status.append(0)
                except TdcGpuError as e:
                    out.append(b"")
                    status.append(e.status)
            return out, status
        if self.ctx is None:
            raise RuntimeError("lzss: decompress_batch needs a context")
        out, status, st = self.ctx.lzss_sw_decompress_batch(streams, self.coder, self.window)
        self.last_stats = st
        return out, status


class RePairCompressor:
    """Mirror of tdc::RePairCompressor<coder> (compressors/RePairCompressor.hpp:14-337), the algorithm `repair`; no input restrictions.
    coder: bit (the reference's default), ascii, gamma or delta; max_rules 0 = unlimited.  The grammar is built on the device.
    dec="host": decompress() is the host loop (repair_decode), which needs no context; dec="gpu" (an addition, as for lzss): the device
    decoder (tdc_gpu_repair_decompress; coder=ascii decodes through the host loop there too).  The stream is the same either way."""

    _CODERS = {"bit": CODER_BIT, "ascii": CODER_ASCII, "gamma": CODER_GAMMA, "delta": CODER_DELTA}

    def __init__(self, ctx, coder="bit", max_rules=0, dec="host"):
        if coder not in self._CODERS:
            raise RuntimeError("No implementation found for compressor repair(coder=%s)" % coder)
        if int(max_rules) < 0:
            raise RuntimeError("repair: max_rules must not be negative")
        if dec not in ("host", "gpu"):
            raise RuntimeError("repair: dec must be host or gpu")
        self.ctx, self.coder, self.max_rules, self.dec = ctx, self._CODERS[coder], int(max_rules), dec
        self.last_stats = None

    def compress(self, data):
        out, st = self.ctx.repair_compress(data, self.max_rules, self.coder)
        self.last_stats = st
        return out

    def compress_batch(self, texts):
        """every text on its own in one device call, one workgroup per grammar: (list of streams, statuses); stream k is
        compress(texts[k])"""
        out, status, st = self.ctx.repair_compress_batch(texts, self.max_rules, self.coder)
        self.last_stats = st
        return out, status

    def decompress(self, stream):
        if self.dec == "gpu":
            if self.ctx is None:
                raise RuntimeError("repair: dec=gpu needs a context")
            return self.ctx.repair_decompress(stream, self.coder)
        return repair_decode(stream, self.coder)

    def decompress_batch(self, streams):
        """(list of texts, statuses) on the device, all streams in one pass, whatever dec says; text k is decompress(streams[k]), b""
        where it is refused.  coder=ascii is refused as the C call refuses it (status -6): loop decompress() over such streams."""
        out, status, st = self.ctx.repair_decompress_batch(streams, self.coder)
        self.last_stats = st
        return out, status


class LZSSLCPCompressor:
    """Mirror of tdc::LZSSLCPCompressor<coder> (compressors/LZSSLCPCompressor.hpp:22-132) with the reference's non-consuming coders
    huff, bit, gamma, delta, ascii; threshold defaults to 3.  dec="host": the sequential loop (lzss_decode); dec="gpu" (an addition,
    as for lz78 / lzw): tdc_gpu_lzss_lcp_decompress."""

    _CODERS = {"huff": CODER_HUFF, "bit": CODER_BIT, "gamma": CODER_GAMMA, "delta": CODER_DELTA, "ascii": CODER_ASCII}

    def __init__(self, ctx, coder="huff", threshold=3, dec="host"):
        if coder not in self._CODERS:
            raise RuntimeError("No implementation found for compressor lzss_lcp(coder=%s)" % coder)
        if dec not in ("host", "gpu"):
            raise RuntimeError("lzss_lcp: dec must be host or gpu")
        self.ctx, self.coder, self.threshold, self.dec = ctx, self._CODERS[coder], int(threshold), dec
        self.last_stats = None

    def compress(self, data):
        out, st = self.ctx.lzss_lcp_compress(escape(data), self.threshold, self.coder)
        self.last_stats = st
        return out

    def decompress(self, stream):
        text = self.ctx.lzss_lcp_decompress(stream, self.coder)[0] if self.dec == "gpu" else lzss_decode(stream, self.coder)
        return unescape(text) if text else b""
