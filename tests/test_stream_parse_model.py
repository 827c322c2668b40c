"""The hand-built streams of tests/stream_parse_cases.py under the Python models and the host loops: each one is well-formed, or
refused, or beyond a device cap, as the GPU tests of the shared parse (tests/test_gpu_stream_parse.py) take it to be."""
import pytest

from tests import stream_parse_cases as C
from tests.models import lz78_decode as M78
from tests.models import lzss_sw as MSW
from tests.models import lzss_sw_decode as MSD
from tests.models import lzw as MLZW
from tests.models import repair as MR
from tests.models import repair_decode as MRD
from tests.models.lzss_coders import Malformed, payload_bits

ERR_ARG, host = C.ERR_ARG, C.host
PAIRS = [(d, c) for d in C.DECODERS for c in C.CODERS[d]]


def model(decoder, stream, coder):
    try:
        if decoder == "lzss":
            return 0, MSW.decode(stream, coder, C.WINDOW)
        if decoder == "repair":
            return 0, MR.sequential_decode(stream, coder)
        if decoder == "lzw":
            return 0, MLZW.sequential_decode(stream, coder)
        return 0, M78.sequential_decode(stream)
    except (Malformed, M78.Malformed, ValueError):
        return ERR_ARG, None


def beyond_a_cap(decoder, stream, coder):
    """does the device model meet a field beyond a cap?"""
    if decoder == "lzss":                                         # (over_cap() looks at value bits only: delta's width code has a cap too)
        try:
            MSD.decode(stream, coder, C.WINDOW)
        except Malformed:
            return host(decoder, stream, coder)[0] == 0
        return False
    try:
        MRD.parse_device(stream, coder)
    except MRD.ToHost:
        return True
    except Malformed:
        pass
    return False


@pytest.mark.parametrize("decoder,coder", [p for p in PAIRS if p[1] != "bit"])
def test_cap_cases(decoder, coder):
    for name, s, wide in C.cap_cases(decoder, coder):
        want = host(decoder, s, coder)
        assert model(decoder, s, coder) == want, name
        if "value bits" in name or "width code" in name:
            # what the reader's caps are about: the host loops read every one of these fields, except an lz78 / lzw id above 32 bits
            assert (want[0] == 0) == (decoder in ("lzss", "repair") or not wide), name
        elif "ends with the stream" in name:
            assert want[0] == 0 and want[1], name
        else:
            assert want[0] == ERR_ARG, name
        if decoder in ("lzss", "repair") and "zeros" not in name:
            assert beyond_a_cap(decoder, s, coder) == wide, name
        if decoder == "lzss" and not wide and want[0] == 0:
            assert MSD.decode(s, coder, C.WINDOW) == want[1], name


@pytest.mark.parametrize("decoder,coder", PAIRS)
def test_straddling_tokens(decoder, coder):
    for d in C.STRADDLE_D:
        s, dd = C.straddle(decoder, coder, d)
        assert dd in (d, d + 1) and payload_bits(s) > C.TILE
        want = host(decoder, s, coder)
        assert want[0] == 0 and len(want[1]) > 1000, d
        assert model(decoder, s, coder) == want, d
        assert decoder not in ("lzss", "repair") or coder == "bit" or not beyond_a_cap(decoder, s, coder)


@pytest.mark.parametrize("coder", ("bit", "gamma", "delta"))
@pytest.mark.parametrize("decoder", ("lzss", "repair"))
def test_terminator_residues(decoder, coder):
    for s in C.residue_streams():
        assert payload_bits(s) == (s[-1] & 7 if len(s) == 1 else 8 * (len(s) - (2 if s[-1] & 7 >= 6 else 1)) + (s[-1] & 7))
        assert model(decoder, s, coder) == host(decoder, s, coder), s.hex()
