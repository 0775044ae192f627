"""nvt_snappy_inflate_pages against the truth: real streams against their data, hand-assembled streams
against the Python decoder of snappy_reference, malformed streams against their codes.  All pages of a
test go in ONE launch, and ``dst`` lies between guard bytes that must come back untouched."""
import numpy as np
import pyarrow as pa
import pytest

from inflate_reference import copy1, copy2, copy4, out_len
from kernel_buffers import Guarded, dev
from nvtabular_amd import _lib
from nvtabular_amd import kernels_parquet_inflate as KPI
from snappy_reference import decode_raw, literal_tag, varint

pytestmark = pytest.mark.gpu
TRUNCATED, OFFSET, LENGTH, FAR = 1, 2, 3, 4
RNG = np.random.default_rng(11)
NOISE = RNG.integers(0, 256, 70_000, dtype=np.uint8).tobytes()


def run(streams, flags=None, sizes=None, shift=0):
    """-> (outputs, status words); the pages' outputs lie 64 poisoned bytes apart in a guarded buffer.
    ``shift``: every body starts that many bytes behind a 16-byte boundary."""
    flags = flags or [0] * len(streams)
    table, body = KPI.page_table(streams, flags, sizes, gap=64)
    table[:, 0] += shift
    body = b"\x5a" * shift + body
    out = Guarded(int(sum(sizes)) + 64 * len(streams))
    status = KPI.launch(dev(np.frombuffer(bytearray(body), dtype=np.uint8)), out.ptr, table).cpu().numpy()
    whole = out.read(what="inflate")
    for a, b in zip(table[:, 2], table[:, 3]):   # the gaps between the pages as well
        assert (whole[a + b: a + b + 64] == 0xA5).all()
    return [whole[a: a + b].tobytes() for a, b in zip(table[:, 2], table[:, 3])], status


def stream(*elements, total=None):
    """varint(length) | elements; the length is what the elements produce unless ``total`` says."""
    body = b"".join(elements)
    return varint(out_len(body) if total is None else total) + body


def lit(n, at=0):
    return literal_tag(n) + NOISE[at: at + n]


@pytest.mark.parametrize("shift", [0, 1, 7, 15])
def test_real_streams(shift):
    datas = [NOISE[:n] for n in (0, 1, 63, 64, 65, 4097)]
    datas += [np.minimum(RNG.zipf(1.3, 20_000), 1 << 40).astype(np.int64).tobytes(),
              RNG.normal(size=20_000).astype(np.float32).tobytes(), b"\x07" * 100_000,
              bytes(range(7)) * 10_000]
    streams = [pa.compress(d, codec="snappy", asbytes=True) for d in datas]
    outs, status = run(streams, sizes=[len(d) for d in datas], shift=shift)
    assert status.tolist() == [0] * len(datas)
    for i, (o, d) in enumerate(zip(outs, datas)):
        assert o == d, i
    assert KPI.inflate_pages(streams[1:4]) == datas[1:4]


def _shapes(pad):
    """Element lists whose parse windows and ring refills fall at chosen places; ``pad`` literal bytes
    in front move them (4090: the shapes straddle the first refill of the 4096-byte ring)."""
    head = [lit(pad)] if pad else []
    yield [lit(n) for n in (1, 60, 61, 256, 257, 65_537)]
    yield head + [lit(40), copy1(4, 1), copy1(11, 2047 if pad > 2047 else 40), copy2(1, 1), copy2(64, 40),
                  copy4(1, 40), copy4(64, 33)]
    yield head + [lit(8)] + [copy2(64, k) for k in (1, 2, 3, 7)]
    yield head + [lit(5)] + [copy2(3 + k % 5, 3 + k % 5) for k in range(300)]       # each reads what the last wrote
    yield head + [lit(4)] + [copy1(4, 4)] * 200                                      # 32 elements per parse round
    # a literal that starts at byte 60 of a parse window; tags at byte 63 with their length bytes behind it
    yield head + [lit(59), lit(30), lit(7)]
    yield head + [lit(62), lit(300), lit(7)]
    yield head + [lit(62), lit(66_000), copy2(64, 65_535)]


@pytest.mark.parametrize("pad", [0, 4090])
def test_hand_assembled_streams(pad):
    streams = [stream(*els) for els in _shapes(pad)]
    # offsets 65 535 and 65 536 just behind the point where the window wraps
    streams.append(stream(lit(65_530), lit(20, 7), copy2(64, 65_535), copy4(64, 65_536), copy4(11, 65_536)))
    want = [decode_raw(s) for s in streams]
    outs, status = run(streams, sizes=[len(w) for w in want])
    assert status.tolist() == [0] * len(streams)
    for i, (o, w) in enumerate(zip(outs, want)):
        assert o == w, (i, len(w))


@pytest.mark.parametrize("L", [2, 70])
def test_v1_levels_prefix_is_dropped_but_copied_from(L):
    levels = L.to_bytes(4, "little") + NOISE[100: 100 + L]
    els = [literal_tag(len(levels)) + levels, lit(50), copy2(30, 50 + L), copy2(20, 84 + L), lit(5000, 9)]
    s = stream(*els)
    want = decode_raw(s)[4 + L:]
    outs, status = run([s, s], flags=[_lib.INFLATE_V1_LEVELS, _lib.INFLATE_V1_LEVELS], sizes=[len(want), len(want) + 1])
    assert status.tolist() == [0, LENGTH] and outs[0] == want


BAD = {
    "cut inside a tag": (stream(lit(10), copy2(4, 3))[:-1], 14, TRUNCATED),
    "cut inside a literal": (stream(lit(100))[:-1], 100, TRUNCATED),
    "offset 0": (stream(lit(10), copy2(4, 0), total=14), 14, OFFSET),
    "offset past the output": (stream(lit(10), copy2(4, 11), total=14), 14, OFFSET),
    "one byte more": (stream(lit(10), copy2(5, 3), total=14), 14, LENGTH),
    "one byte fewer": (stream(lit(10), copy2(3, 3), total=14), 14, LENGTH),
    "dst_bytes mismatch": (stream(lit(10), copy2(4, 3)), 15, LENGTH),
    "offset 65537": (stream(lit(65_537), copy4(4, 65_537), total=65_541), 65_541, FAR),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_malformed_pages_get_their_code_and_neighbours_stay_correct(case):
    bad, size, code = BAD[case]
    good = pa.compress(NOISE[:5000] * 3, codec="snappy", asbytes=True)
    outs, status = run([good, bad, good], sizes=[15_000, size, 15_000])
    assert status.tolist() == [0, code, 0]
    assert outs[0] == outs[2] == NOISE[:5000] * 3
    with pytest.raises(_lib.NvtHipError, match=f"page 1 .*{_lib.INFLATE_ERRORS[code]}"):
        KPI.inflate_pages([good, bad], sizes=[15_000, size])
