"""The snappy raw format restated in pure Python for the tests of the snappy pages (no test module:
the tests import it).  A raw stream is ``varint(uncompressed length)`` followed by ELEMENTS:

* literal: tag ``(len - 1) << 2`` for 1 .. 60 bytes, or ``(59 + k) << 2`` followed by ``len - 1`` in k
  little-endian bytes (k = 1 .. 4), then the bytes;
* copy, 1-byte offset: tag ``01`` in the low bits, ``(len - 4)`` in bits 2 .. 4 (4 .. 11 bytes), offset
  bits 8 .. 10 in bits 5 .. 7, then the low offset byte;
* copy, 2-byte offset: tag ``((len - 1) << 2) | 2`` (1 .. 64 bytes), then the offset, little endian;
* copy, 4-byte offset: tag ``((len - 1) << 2) | 3``, then the offset, little endian.

A copy repeats ``len`` bytes from ``offset`` bytes back in the output, byte by byte (it may overlap
what it writes)."""


def varint(x: int) -> bytes:
    out = bytearray()
    while x >= 0x80:
        out.append((x & 0x7F) | 0x80)
        x >>= 7
    out.append(x)
    return bytes(out)


def read_varint(buf, at=0):
    """(value, position behind it)."""
    val = shift = 0
    while True:
        if at >= len(buf) or shift > 63:
            raise ValueError("snappy: truncated varint")
        b = buf[at]
        at += 1
        val |= (b & 0x7F) << shift
        if not b & 0x80:
            return val, at
        shift += 7


def literal_tag(n: int) -> bytes:
    """The tag bytes of a literal element of n >= 1 bytes."""
    if n < 1:
        raise ValueError("snappy: an empty literal has no tag")
    if n <= 60:
        return bytes([(n - 1) << 2])
    k = ((n - 1).bit_length() + 7) // 8
    return bytes([(59 + k) << 2]) + (n - 1).to_bytes(k, "little")


def encode_literal(data, piece=None) -> bytes:
    """The literal-only element stream of ``data``: literals of ``piece`` bytes (None: one literal)."""
    data = bytes(data)
    piece = piece or max(len(data), 1)
    return b"".join(literal_tag(len(data[i: i + piece])) + data[i: i + piece] for i in range(0, len(data), piece))


def decode_elements(buf, expect_len, floor=0, prefix=b"") -> bytes:
    """Decode the bare element stream ``buf``.  ``prefix``: bytes that stand in the output already
    (the elements' output follows them); no copy may reach in front of position ``floor`` of the
    whole output.  Raises ValueError on a malformed tag, a zero or out-of-range offset, an overrun
    of ``buf``, a copy reaching before ``floor`` and an output other than ``expect_len`` bytes long
    (``prefix`` not counted).  -> the decoded bytes (without ``prefix``)."""
    buf = bytes(buf)
    out = bytearray(prefix)
    base = len(out)
    at = 0
    while at < len(buf):
        tag = buf[at]
        at += 1
        kind = tag & 3
        if kind == 0:
            n = tag >> 2
            if n >= 60:
                k = n - 59
                if at + k > len(buf):
                    raise ValueError("snappy: literal length runs past the stream")
                n = int.from_bytes(buf[at: at + k], "little")
                at += k
            n += 1
            if at + n > len(buf):
                raise ValueError("snappy: literal runs past the stream")
            out += buf[at: at + n]
            at += n
            continue
        if kind == 1:
            if at + 1 > len(buf):
                raise ValueError("snappy: copy runs past the stream")
            n, off = 4 + ((tag >> 2) & 7), ((tag >> 5) << 8) | buf[at]
            at += 1
        else:
            k = 2 if kind == 2 else 4
            if at + k > len(buf):
                raise ValueError("snappy: copy runs past the stream")
            n, off = (tag >> 2) + 1, int.from_bytes(buf[at: at + k], "little")
            at += k
        if off == 0:
            raise ValueError("snappy: copy with offset 0")
        if off > len(out):
            raise ValueError("snappy: copy reaches in front of the output")
        if len(out) - off < floor:
            raise ValueError(f"snappy: copy reaches to {len(out) - off}, in front of the floor {floor}")
        for _ in range(n):
            out.append(out[-off])
    got = bytes(out[base:])
    if len(got) != expect_len:
        raise ValueError(f"snappy: {len(got)} bytes decoded, {expect_len} expected")
    return got


def decode_raw(buf) -> bytes:
    """A whole raw stream: varint(length) | elements."""
    n, at = read_varint(buf)
    return decode_elements(buf[at:], n)
