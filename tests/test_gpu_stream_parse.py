"""GPU tests of the parse that the device decoders of lz78, lzw, lzss and repair share (tudocomp_amd/csrc/stream_parse.hpp), through the
public decompress calls: fields at the caps of the gamma / delta reader, a token that starts in the last bits of a 32768-bit tile of
the next() pass, and the terminator residues that decide the payload's bit count.  The streams are tests/stream_parse_cases.py's;
tests/test_stream_parse_model.py holds them against the Python models.  Every stream is parsed on the device (dec_parse=2), with
default segments and with segments of 4096 bit positions.  A segment of 4096 positions is one partial tile, so only the run with
default segments reads a token from the tail of an image; the other one meets the same tokens at the borders of segments.  Where
every token of a format has an even number of bits (lz78 pairs, repair under gamma behind its count field) an odd distance from the
border is out of reach, and the case runs one bit further in front of it (stream_parse_cases.straddle returns the distance used).

What is expected: the status and the text of the host loop that specifies the decoder (for lz78, which has none in Python, of the
model's sequential reading).  lzss refuses a field beyond a device cap that its host loop reads: TDC_GPU_ERR_ARG; repair hands such a
stream to its host loop, and says so in device_parse."""
import functools

import pytest

import tudocomp_amd as T
from tests import stream_parse_cases as C

pytestmark = pytest.mark.gpu

ERR_ARG, CID, host = C.ERR_ARG, C.CID, C.host
PAIRS = [(d, c) for d in C.DECODERS for c in C.CODERS[d]]


@pytest.fixture(scope="module")
def seg_ctx():
    with T.Context(0, options={"dec_parse": 2, "dec_seg": 4096}) as ctx:
        yield ctx


@pytest.fixture(scope="module")
def dev_ctx():
    with T.Context(0, options={"dec_parse": 2}) as ctx:
        yield ctx


@pytest.fixture(params=["seg", "dev"])
def ctx(request, seg_ctx, dev_ctx):
    return seg_ctx if request.param == "seg" else dev_ctx


def device(c, decoder, stream, coder):
    """(status, text, device_parse)"""
    try:
        if decoder == "lzss":
            out, st = c.lzss_sw_decompress(stream, C.WINDOW, CID[coder])
        elif decoder == "repair":
            out, st = c.repair_decompress_stats(stream, CID[coder])
        elif decoder == "lzw":
            out, st = c.lzw_decompress(stream, CID[coder])
        else:
            out, st = c.lz78_decompress(stream)
        return 0, out, st.get("device_parse", 1)
    except T.TdcGpuError as e:
        return e.status, None, None


cap_cases = functools.lru_cache(maxsize=None)(C.cap_cases)
straddle = functools.lru_cache(maxsize=None)(C.straddle)
host = functools.lru_cache(maxsize=None)(host)


@pytest.mark.parametrize("decoder,coder", [p for p in PAIRS if p[1] != "bit"])
def test_fields_at_the_caps(ctx, decoder, coder):
    for name, s, wide in cap_cases(decoder, coder):
        want = host(decoder, s, coder)
        status, out, on_device = device(ctx, decoder, s, coder)
        if decoder == "lzss" and wide:
            assert want[0] == 0 and status == ERR_ARG, name      # the device refuses what the host loop reads
            continue
        assert (status, out) == want, name
        if status == 0:
            assert on_device == (0 if wide else 1), name         # (repair: beyond a cap, the host loop decoded it)


@pytest.mark.parametrize("d", C.STRADDLE_D)
@pytest.mark.parametrize("decoder,coder", PAIRS)
def test_a_token_across_the_border_of_a_tile(ctx, decoder, coder, d):
    s, _ = straddle(decoder, coder, d)
    want = host(decoder, s, coder)
    assert want[0] == 0
    assert device(ctx, decoder, s, coder) == (0, want[1], 1)


@pytest.mark.parametrize("coder", ("bit", "gamma", "delta"))
@pytest.mark.parametrize("decoder", ("lzss", "repair"))
def test_terminator_residues(ctx, decoder, coder):
    for s in C.residue_streams():
        assert device(ctx, decoder, s, coder)[:2] == host(decoder, s, coder), s.hex()
