"""Plain-Python restatement of parquet's DELTA_BINARY_PACKED encoding, from the format alone (DESIGN.md,
"DELTA_BINARY_PACKED in the parquet reader"): varint block_size | varint miniblocks_per_block | varint
total_count | zigzag first_value | blocks of { zigzag min_delta | a width byte per miniblock | the miniblocks,
LSB first }; value k >= 1 is first_value + sum_{j < k} (min_delta of j's block + delta j) modulo 2^bits.
``encode`` exists for the shapes pyarrow never writes (64-value miniblocks, full-width deltas)."""
import numpy as np


def _varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _zigzag(v, bits=64):
    return _varint(((v << 1) ^ (v >> (bits - 1))) & ((1 << bits) - 1))


def _read_varint(buf, at):
    v = sh = 0
    while True:
        b = buf[at]
        at += 1
        v |= (b & 0x7F) << sh
        sh += 7
        if not b & 0x80:
            return v, at


def _signed(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def decode(page_bytes, bits):
    """The values of one values region (bytes behind the last needed miniblock are not looked at)."""
    buf = bytes(page_bytes)
    block_size, at = _read_varint(buf, 0)
    mpb, at = _read_varint(buf, at)
    total, at = _read_varint(buf, at)
    z, at = _read_varint(buf, at)
    vpm = block_size // mpb
    out = [(z >> 1) ^ -(z & 1)] if total else []
    while len(out) < total:
        z, at = _read_varint(buf, at)
        min_delta = (z >> 1) ^ -(z & 1)
        widths = buf[at: at + mpb]
        at += mpb
        for w in widths:
            if len(out) >= total:
                break
            word = int.from_bytes(buf[at: at + vpm * w // 8], "little")
            at += vpm * w // 8
            for k in range(vpm):
                if len(out) < total:
                    out.append(out[-1] + min_delta + ((word >> (k * w)) & ((1 << w) - 1)))
    return np.array([_signed(v, bits) for v in out], dtype=np.int32 if bits == 32 else np.int64)


def encode(values, bits, block_size=128, miniblocks=4):
    """One values region: the last needed miniblock padded, the absent ones' width bytes arbitrary (0xFF)."""
    vals = [int(v) for v in values]
    vpm = block_size // miniblocks
    out = bytearray(_varint(block_size) + _varint(miniblocks) + _varint(len(vals)) + _zigzag(vals[0] if vals else 0))
    deltas = [_signed(b - a, bits) for a, b in zip(vals[:-1], vals[1:])]
    for b0 in range(0, len(deltas), block_size):
        block = deltas[b0: b0 + block_size]
        min_delta = min(block)
        rel = [(d - min_delta) & ((1 << bits) - 1) for d in block]
        minis = [rel[m: m + vpm] for m in range(0, len(rel), vpm)]
        out += _zigzag(min_delta)
        out += bytes([max(x.bit_length() for x in mb) for mb in minis] + [0xFF] * (miniblocks - len(minis)))
        for mb in minis:
            w = max(x.bit_length() for x in mb)
            word = sum(x << (k * w) for k, x in enumerate(mb))
            out += word.to_bytes(vpm * w // 8, "little")
    return bytes(out)
