"""tests/snappy_reference.py against pyarrow's codec, its refusals of hand-made bad streams, and
``parquet_plain.snappy_pays`` on hand-made sizes (no GPU)."""
import numpy as np
import pyarrow as pa
import pytest

import snappy_reference as R


def _fixtures():
    rng = np.random.default_rng(0)
    lab = np.minimum(np.random.default_rng(0).zipf(1.3, 32768), 50000).astype(np.int64)
    srt = np.sort(np.random.default_rng(1).choice(1 << 40, 4096, replace=False)).astype(np.int64)
    out = {"labels": lab[:8192].tobytes(), "labels32": lab[:8192].astype(np.int32).tobytes(), "sorted": srt.tobytes(),
           "zeros": bytes(70000), "random": rng.bytes(5000), "empty": b"", "one": b"x"}
    for k in (1, 3, 5, 7):
        out[f"period{k}"] = (rng.bytes(k) * 3000)[:7001]
    return out


FIXTURES = _fixtures()


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_decoder_agrees_with_pyarrow(name):
    data = FIXTURES[name]
    codec = pa.Codec("snappy")
    raw = codec.compress(data).to_pybytes()
    n, at = R.read_varint(raw)
    assert n == len(data)
    assert R.decode_elements(raw[at:], len(data)) == data
    assert R.decode_raw(raw) == data
    if data:
        assert codec.decompress(raw, decompressed_size=len(data)).to_pybytes() == data


@pytest.mark.parametrize("name", sorted(FIXTURES))
@pytest.mark.parametrize("piece", [None, 1, 60, 61, 256, 257, 70000])
def test_literal_encoder_is_read_by_pyarrow(name, piece):
    data = FIXTURES[name]
    stream = R.encode_literal(data, piece)
    assert R.decode_elements(stream, len(data)) == data
    if data:
        assert pa.Codec("snappy").decompress(R.varint(len(data)) + stream, decompressed_size=len(data)).to_pybytes() == data


def test_varints():
    for x in (0, 1, 127, 128, 300, 16383, 16384, (1 << 32) - 1, 1 << 40):
        b = R.varint(x)
        assert R.read_varint(b + b"\xff") == (x, len(b))
    with pytest.raises(ValueError):
        R.read_varint(b"\x80\x80")


def test_bad_streams_are_refused():
    lit = R.encode_literal(b"abcdefgh")

    def copy2(n, off):
        return bytes([((n - 1) << 2) | 2]) + off.to_bytes(2, "little")

    assert R.decode_elements(lit + copy2(4, 8), 12) == b"abcdefghabcd"
    assert R.decode_elements(lit + copy2(6, 1), 14) == b"abcdefgh" + b"h" * 6          # an overlapping copy
    assert R.decode_elements(lit + bytes([0b00000001, 8]), 12) == b"abcdefghabcd"      # 1-byte offset, 4 bytes
    assert R.decode_elements(lit + bytes([0b00000101, 8]), 13) == b"abcdefghabcde"     # ... 5 bytes
    assert R.decode_elements(lit + bytes([(3 << 2) | 3]) + (8).to_bytes(4, "little"), 12) == b"abcdefghabcd"
    bad = [
        (lit + copy2(4, 0), 12),                    # offset 0
        (lit + copy2(4, 9), 12),                    # in front of the output
        (copy2(4, 1), 4),                           # a copy with nothing to copy from
        (lit + copy2(4, 8)[:2], 12),                # the offset is cut off
        (lit + bytes([0b00000001]), 12),            # the offset byte is missing
        (lit[:-1], 8),                              # the literal runs past the stream
        (bytes([61 << 2, 5]), 6),                   # the literal's length is cut off
        (bytes([63 << 2, 1, 0, 0]), 2),             # ... of a 4-byte length too
        (lit, 9), (lit, 7),                         # another length than expected
    ]
    for stream, n in bad:
        with pytest.raises(ValueError):
            R.decode_elements(stream, n)
    # the floor: a fragment's copies stay inside the fragment
    assert R.decode_elements(copy2(4, 8), 4, floor=0, prefix=b"abcdefgh") == b"abcd"
    with pytest.raises(ValueError):
        R.decode_elements(copy2(4, 8), 4, floor=1, prefix=b"abcdefgh")
    with pytest.raises(ValueError):
        R.decode_elements(lit + copy2(4, 8), 12, floor=1)
    with pytest.raises(ValueError):
        R.literal_tag(0)


def test_snappy_pays_on_hand_made_sizes():
    from nvtabular_amd import parquet_plain as PP

    assert PP.snappy_pays(99, 100) and not PP.snappy_pays(100, 100) and not PP.snappy_pays(101, 100)
    assert not PP.snappy_pays(0, 0)
    # one flat page of 1000 int64 values without nulls: 8000 bytes of values behind 6 bytes of levels
    lv = PP.flat_level_bytes(1000, False)
    assert lv == 4 + 2 + 1
    comp, plain = PP.snappy_chunk_bytes([(1000, lv, 8000, 3000, 0)])
    assert plain == len(PP._page_header(1000, 8007)) + 8007
    body = 2 + (1 + lv) + 3000                       # varint(8007) | tag, levels | elements
    assert comp == len(PP._page_header(1000, 8007, 0, body)) + body and PP.snappy_pays(comp, plain)
    # elements as long as the values: the varint and the tag make the chunk larger, it stays as it is
    comp, plain = PP.snappy_chunk_bytes([(1000, lv, 8000, 8000, 0)])
    assert comp == plain + 3 and not PP.snappy_pays(comp, plain)
    # a page of nulls only has no elements at all and never pays
    lv = PP.flat_level_bytes(1000, True)
    assert lv == 4 + 2 + 125
    comp, plain = PP.snappy_chunk_bytes([(1000, lv, 0, 0, 0)])
    assert comp > plain
    # a dictionary chunk: the dictionary page shrinks, the data pages travel as literals
    comp, plain = PP.snappy_chunk_bytes([(1000, 300, 0, 0, 8)], (500, 4000, 1000))
    assert plain == len(PP._dict_page_header(500, 4000)) + 4000 + len(PP._page_header(1000, 300, 8)) + 300
    # (data page body: varint(300) 2 bytes | tag of a 300-byte literal 3 bytes | the 300 bytes)
    assert comp == len(PP._dict_page_header(500, 4000, 1002)) + 1002 + len(PP._page_header(1000, 300, 8, 305)) + 305
    assert PP.list_level_bytes(20) == (4 + 1 + 3) + (4 + 1 + 6)
