"""Batches with more texts than the batch kernels have workgroups, and what they must yield.

Every batch kernel that gives one workgroup (or one wave) to one text is launched with a capped grid and walks the texts with
`k += gridDim.x`: 2^16 workgroups in lz_batch.hip, lz_batch_decode.hip, lzss_sw_batch.hip and repair_batch.hip's coder kernels, 2048 in
repair's round kernel.  The batches here make a workgroup take a second and a third text.  A batch is an index array into a pool of
about 120 distinct texts; the truth is computed once per pool entry by code that is not under test (tests/repair_batches.py,
tests/lz_batches.py, tests/lzss_sw_batches.py), and text k must yield what pool[index[k]] yields.  tests/test_many_texts_cli.py ties
the counts to the constants in the sources and checks the pool's truth on the CPU; tests/test_gpu_many_texts.py runs the kernels.

Everything per text is kept as a Ragged (one flat array and the borders), so that a whole batch is built and compared with numpy."""
import functools
import hashlib

import numpy as np

import tudocomp_amd as T
from tests import lz_batch_decode_cases as LC
from tests import lz_batches as LB
from tests import lzss_sw_batches as SB
from tests import lzss_sw_damage as SD
from tests import lzw_damage
from tests import repair_batches as RB
from tests.models import lzss_sw_decode as SMD

ERR_ARG, ERR_TOO_LARGE, ERR_UNSUPPORTED = -2, -4, -6
CAP16 = 1 << 16                                  # lzb_text_grid, lzb_walk_grid, swb_decode_grid, rb_encode_as
RB_GRID = 2048                                   # RB_MAX_GRID: the round kernel of repair
TRIPS3 = 2 * CAP16 + 4099                        # workgroups 0 .. 4098 take three texts, all others two
BORDERS16 = (CAP16, CAP16 + 1, 2 * CAP16 + 1)
REPAIR_BORDERS = (RB_GRID, RB_GRID + 1, 2 * RB_GRID + 1, 3 * RB_GRID + 77)
WINDOW, THRESHOLD = 16, 3                        # lzss: the defaults of the calls
LZSS_CODERS = ("bit", "gamma", "delta")
REPAIR_CODERS = ("bit", "ascii", "gamma", "delta")
NATURES = ("run", "nopair", "english", "tie")
NATURE_LENGTHS = (2, 3, 4, 6, 9, 14, 20, 27, 33, 40)
TEXT_MOST = 6000


# ---- the pool ------------------------------------------------------------------------------------------------------------------------------
def nature_text(nature, n):
    """n bytes of one nature: a run, no byte twice (so no pair twice), English, the tie text cut"""
    if nature == "run":
        return b"a" * n
    if nature == "nopair":
        return bytes(range(48, 48 + n))
    if nature == "english":
        return RB.english(700, 31)[:n]
    return RB.tie_text()[:n]


def _refused_long():
    """some hundred bytes that lz78 refuses: the left-over phrase ends on 0x80"""
    head = RB.english(300, 33)
    for j in range(2, 40):
        x = head + b"\x80" * j
        if LB.lz78_status(x) == ERR_UNSUPPORTED:
            return x
    raise AssertionError("no refused text")


@functools.lru_cache(maxsize=None)
def pool():
    """((name, class, text), ...)"""
    rng = np.random.default_rng(65536)
    out = [("empty", "empty", b"")]
    out += [("tiny%d" % j, "tiny", x) for j, x in enumerate((b"a", b"b", b"ab", b"aa", b"abc", b"aba", b"\x00", b"\x7f\x00"))]
    for j, n in enumerate(rng.integers(3, 41, 56)):
        out.append(("bulk%d" % j, "bulk", rng.integers(97, 101, int(n), dtype=np.uint8).tobytes()))
    for nature in NATURES:
        out += [("%s%d" % (nature, n), nature, nature_text(nature, n)) for n in NATURE_LENGTHS]
    out += [("english300", "long", RB.english(300, 34)), ("english700", "long", RB.english(700, 35)), ("english511", "long", RB.english(511, 36)),
            ("dna400", "long", RB.dna(400, 37)), ("dna650", "long", RB.dna(650, 38))]
    out += [("a5000", "a5000", b"a" * 5000), ("tie", "tietext", RB.tie_text()), ("distinct64", "distinct64", bytes(range(100, 164)))]
    out += [("zeros300", "runs", b"\x00" * 300), ("ff300", "runs", b"\xff" * 300), ("zeros17", "runs", b"\x00" * 17), ("ff66", "runs", b"\xff" * 66)]
    out += [("refused80", "refused", b"\x80\x80"), ("refused_ab80", "refused", b"ab\x80ab\x80"), ("refused_ff", "refused", b"ab\xffab\xff"),
            ("refused_ff301", "refused", b"\xff" * 301), ("refused_long", "refused", _refused_long())]
    assert len({name for name, _, _ in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def names():
    return {name: j for j, (name, _, _) in enumerate(pool())}


def texts():
    return [x for _, _, x in pool()]


def of_class(*classes):
    return np.array([j for j, (_, c, _) in enumerate(pool()) if c in classes], dtype=np.int64)


SHORT = ("empty", "tiny", "bulk") + NATURES     # the classes of the border batches: at most 40 bytes


# ---- ragged arrays -------------------------------------------------------------------------------------------------------------------------
class Ragged:
    """sequences back to back: sequence j = flat[off[j]:off[j + 1]]"""

    def __init__(self, seqs, dtype=np.uint8):
        parts = [np.frombuffer(s, dtype=np.uint8) if isinstance(s, (bytes, bytearray)) else np.asarray(s, dtype=dtype) for s in seqs]
        self.len = np.array([len(p) for p in parts], dtype=np.int64)
        self.off = np.zeros(len(parts) + 1, dtype=np.int64)
        np.cumsum(self.len, out=self.off[1:])
        self.flat = np.concatenate(parts).astype(dtype, copy=False) if parts else np.zeros(0, dtype=dtype)

    def __getitem__(self, j):
        return self.flat[self.off[j]:self.off[j + 1]]


def _spread(starts, lens):
    """for sequences of `lens` elements that start at `starts`: the position of every element, sequence after sequence"""
    total = int(lens.sum())
    first = np.cumsum(lens) - lens
    return np.repeat(starts - first, lens) + np.arange(total, dtype=np.int64)


def take(r, index, align=1):
    """the sequences r[index[0]], r[index[1]], ... in one array, each at a multiple of `align` (zeros in between): (flat, off, len)"""
    lens = r.len[index]
    step = -(-lens // align) * align
    off = np.zeros(len(index) + 1, dtype=np.int64)
    np.cumsum(step, out=off[1:])
    flat = np.zeros(max(int(off[-1]), 1), dtype=r.flat.dtype)[:int(off[-1])]
    flat[_spread(off[:-1], lens)] = r.flat[_spread(r.off[index], lens)]
    return flat, off, lens


def differing(flat, starts, lens, want, index):
    """the k at which flat[starts[k], + lens[k]) is not want[index[k]], every element compared"""
    starts, lens = np.asarray(starts).astype(np.int64), np.asarray(lens).astype(np.int64)
    wl = want.len[index]
    bad = lens != wl
    same = np.flatnonzero(~bad)
    ln = wl[same]
    ne = flat[_spread(starts[same], ln)] != want.flat[_spread(want.off[index[same]], ln)]
    bad[np.repeat(same, ln)[ne]] = True
    return np.flatnonzero(bad)


def flatten(seqs, dtype):
    """(flat, starts, lens) of a list of arrays or byte strings, as the list-returning calls give them"""
    lens = np.fromiter((len(s) for s in seqs), dtype=np.int64, count=len(seqs))
    if dtype == np.uint8:
        flat = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    else:
        flat = np.concatenate(seqs) if len(seqs) else np.zeros(0, dtype=dtype)
    return flat, np.cumsum(lens) - lens, lens


# ---- the batches ---------------------------------------------------------------------------------------------------------------------------
# (name, the texts of places k, k + 2^16 and k + 2^17, the k): what one workgroup of an index-order kernel takes on its three trips
SEQUENCES = (
    ("long_empty_long", ("english700", "empty", "a5000"), (0, 1033)),
    ("empty_long_tiny", ("empty", "dna650", "tiny0"), (1, 2047)),
    ("refused_accepted_refused", ("refused_long", "bulk0", "refused80"), (2, 63, 4098)),
    ("accepted_refused_accepted", ("bulk1", "refused_ab80", "english300"), (3, 64, 4097)),
    ("run_nopair_tie", ("a5000", "distinct64", "tie"), (4, 2048)),
    ("ff_one_00", ("ff300", "tiny1", "zeros300"), (7, 255, 3000)),
    ("refused_refused_accepted", ("refused_ff", "refused_long", "english511"), (8,)),
)
# the decoders: a damaged stream between two valid ones on one workgroup's trips, and the other way round
DAMAGE_PLACES = (("valid_damaged_valid", (1, 0, 1), (5, 2000)), ("damaged_valid_damaged", (0, 1, 0), (6, 4000)))
VALID_AROUND_DAMAGE = "english700"


@functools.lru_cache(maxsize=None)
def trips3():
    """index[k] of 2 * 2^16 + 4099 texts: nine in ten short, the others from every class; SEQUENCES at their places"""
    rng = np.random.default_rng(4099)
    short, other = of_class(*SHORT), of_class("long", "a5000", "tietext", "distinct64", "runs", "refused")
    weight = np.array([0.2 if pool()[j][1] == "a5000" else 1.0 for j in other])
    index = np.where(rng.random(TRIPS3) < 0.97, short[rng.integers(0, len(short), TRIPS3)], rng.choice(other, TRIPS3, p=weight / weight.sum()))
    for _, seq, places in SEQUENCES:
        for k in places:
            for trip, name in enumerate(seq):
                index[k + trip * CAP16] = names()[name]
    index.setflags(write=False)
    return index


@functools.lru_cache(maxsize=None)
def border(count):
    """index[k] of `count` short texts (at most 40 bytes) for the 2^16 families"""
    short = of_class(*SHORT)
    index = short[np.random.default_rng(count).integers(0, len(short), count)]
    index[[0, -1]] = names()["empty"], names()["bulk2"]            # (the last text, the one text of its workgroup's last trip, is no empty one)
    index.setflags(write=False)
    return index


@functools.lru_cache(maxsize=None)
def repair_border(count):
    """index[k] of `count` texts of NATURE_LENGTHS bytes, a nature drawn per text: the round kernel takes them longest first, stable, so
    the texts of one length stay in this order and a workgroup's consecutive trips meet different natures three times in four"""
    rng = np.random.default_rng(count)
    nat = np.array([of_class(nature) for nature in NATURES])        # [nature][length]
    index = nat[rng.integers(0, len(NATURES), count), rng.integers(0, len(NATURE_LENGTHS), count)]
    index.setflags(write=False)
    return index


def round_order(index):
    """the order in which repair's round kernel takes the texts (repair_batch.hip: std::stable_sort, longest first)"""
    lens = np.array([len(x) for x in texts()], dtype=np.int64)[index]
    return np.argsort(-lens, kind="stable")


def texts_of(index):
    t = texts()
    return [t[j] for j in index.tolist()]


@functools.lru_cache(maxsize=None)
def text_pool():
    return Ragged(texts())


# ---- the truth, once per pool entry ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lzw_items():
    return Ragged([LB.lzw_codes(x) for x in texts()], np.uint32)


@functools.lru_cache(maxsize=None)
def lzw_streams(coder):
    return Ragged([LB.lzw_stream(x, coder) for x in texts()])


@functools.lru_cache(maxsize=None)
def lz78_ids():
    return Ragged([LB.lz78_pairs(x)[0] for x in texts()], np.uint32)


@functools.lru_cache(maxsize=None)
def lz78_chars():
    return Ragged([LB.lz78_pairs(x)[1] for x in texts()])


@functools.lru_cache(maxsize=None)
def lz78_statuses():
    return np.array([LB.lz78_status(x) for x in texts()], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def lz78_streams():
    return Ragged([LB.lz78_stream(x) for x in texts()])


@functools.lru_cache(maxsize=None)
def lzss_truth(coder):
    """(statuses, streams) at the default window and threshold"""
    status, streams = SB.expected(texts(), WINDOW, THRESHOLD, coder)
    return np.array(status, dtype=np.int32), Ragged(streams)


@functools.lru_cache(maxsize=None)
def repair_rules(max_rules=0):
    return Ragged([RB.host(x, max_rules)[0] for x in texts()], np.uint64)


@functools.lru_cache(maxsize=None)
def repair_starts(max_rules=0):
    return Ragged([RB.host(x, max_rules)[1] for x in texts()], np.uint32)


@functools.lru_cache(maxsize=None)
def repair_streams(coder, max_rules=0):
    return Ragged([RB.stream(x, coder, max_rules) for x in texts()])


# ---- streams for the decoders ------------------------------------------------------------------------------------------------------------------
def _sha(x):
    return hashlib.sha256(x).hexdigest()


@functools.lru_cache(maxsize=None)
def damaged(algo):
    """[(stream, status, text)]: four damaged streams that the project already has, with the single decoder's verdict on each alone --
    some refused, some accepted with another text.  algo: lzw-bit, lzw-gamma, lz78, lzss-bit, lzss-gamma, lzss-delta"""
    if algo.startswith("lzss"):
        coder = algo.split("-")[1]
        out = []
        for _, s in SD.damaged_streams(coder)[:-1]:
            if coder != "bit" and SMD.over_cap(s, coder, WINDOW):     # (a field above a device cap: the documented other verdict)
                continue
            try:
                out.append((s, 0, T.lzss_sw_decode(s, SB.CODER_ID[coder], WINDOW)))
            except T.TdcGpuError as e:
                out.append((s, e.status, b""))
        picked = [v for v in out if v[1] != 0][:3] + [v for v in out if v[1] == 0][:3]
    elif algo == "lz78":
        rec = LC.lz78_damage_verdicts()
        streams = LC.lz78_damaged()
        bad = [j for j, v in enumerate(rec) if v[0] != 0][:3]
        good = [j for j, v in enumerate(rec) if v[0] == 0][:1]
        picked = [(streams[j], rec[j][0], b"") for j in bad]
        for j in good:                                                # the recorded verdict holds the text's hash only
            text = LB.lz78_decode(streams[j])
            assert [0, len(text), _sha(text)] == rec[j]
            picked.append((streams[j], 0, text))
    else:
        streams = lzw_damage.damaged_streams(algo.split("-")[1])
        verdicts = [(s,) + LC.host(s, algo) for s in streams[:40]]
        picked = [v for v in verdicts if v[1] != 0][:3] + [v for v in verdicts if v[1] == 0][:1]
    assert any(v[1] for v in picked) and not all(v[1] for v in picked)
    return tuple(picked)


def valid_streams(algo):
    """(streams, statuses, texts) per pool entry as the decoder must see them: a text the compressor refuses has the stream b"" and
    comes back as b"" """
    if algo == "lz78":
        refused = lz78_statuses() != 0
        streams = lz78_streams()
    elif algo.startswith("lzw"):
        refused = np.zeros(len(pool()), dtype=bool)
        streams = lzw_streams(algo.split("-")[1])
    else:
        status, streams = lzss_truth(algo.split("-")[1])
        refused = status != 0
    return streams, [b"" if r else x for r, x in zip(refused.tolist(), texts())]


@functools.lru_cache(maxsize=None)
def decode_batch(algo):
    """(streams, statuses, texts, index): a Ragged of streams -- the pool's, then the damaged ones --, what the single decoder says of
    each, and trips3 with DAMAGE_PLACES overwritten"""
    streams, want = valid_streams(algo)
    extra = damaged(algo)
    count = len(pool())
    all_streams = Ragged([streams[j].tobytes() for j in range(count)] + [s for s, _, _ in extra])
    status = np.array([0] * count + [rc for _, rc, _ in extra], dtype=np.int32)
    all_texts = Ragged(want + [x for _, _, x in extra])
    index = trips3().copy()
    nth = 0
    for _, pattern, places in DAMAGE_PLACES:
        for k in places:
            for trip, valid in enumerate(pattern):
                if valid:
                    index[k + trip * CAP16] = names()[VALID_AROUND_DAMAGE]
                else:
                    index[k + trip * CAP16] = count + nth % len(extra)
                    nth += 1
    index.setflags(write=False)
    return all_streams, status, all_texts, index
