"""The thrift compact protocol as far as parquet's PageHeader / FileMetaData need it: a struct
writer (``_Struct``) for the PLAIN writer's pages and footer and a reader (``_TReader``) for the
footers the hand-written reader judges (parquet_plain.py)."""
from __future__ import annotations

import struct
from typing import Sequence

# thrift compact type ids
_CT_BOOL_TRUE, _CT_I32, _CT_I64, _CT_BINARY, _CT_LIST, _CT_STRUCT = 1, 5, 6, 8, 9, 12


def _varint(v: int) -> bytes:
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _zigzag(v: int) -> bytes:
    return _varint((v << 1) ^ (v >> 63))


class _Struct:
    """Minimal thrift compact-protocol struct writer (fields must be added in ascending id)."""

    def __init__(self):
        self.b = bytearray()
        self.last = 0

    def _head(self, fid: int, ctype: int):
        d = fid - self.last
        if 0 < d <= 15:
            self.b.append((d << 4) | ctype)
        else:
            self.b.append(ctype)
            self.b += _zigzag(fid)
        self.last = fid

    def byte(self, fid, v):
        self._head(fid, 3)
        self.b.append(int(v) & 0xFF)
        return self

    def i32(self, fid, v):
        self._head(fid, _CT_I32)
        self.b += _zigzag(int(v))
        return self

    def i64(self, fid, v):
        self._head(fid, _CT_I64)
        self.b += _zigzag(int(v))
        return self

    def bool(self, fid, v):
        self._head(fid, 1 if v else 2)   # (the value of a boolean field is its type id)
        return self

    def binary(self, fid, s):
        s = s.encode() if isinstance(s, str) else bytes(s)
        self._head(fid, _CT_BINARY)
        self.b += _varint(len(s)) + s
        return self

    def struct(self, fid, body: bytes):
        self._head(fid, _CT_STRUCT)
        self.b += body
        return self

    def list(self, fid, etype: int, items: Sequence[bytes]):
        self._head(fid, _CT_LIST)
        n = len(items)
        self.b += bytes([(n << 4) | etype]) if n < 15 else bytes([0xF0 | etype]) + _varint(n)
        for it in items:
            self.b += it
        return self

    def done(self) -> bytes:
        return bytes(self.b) + b"\x00"


class _TReader:
    """Minimal thrift compact-protocol reader: a struct comes back as {field id: value}, nested
    structs as dicts, lists as Python lists, binaries as bytes."""

    def __init__(self, buf, pos=0):
        self.b, self.p = buf, pos

    def varint(self) -> int:
        v = sh = 0
        while True:
            c = self.b[self.p]
            self.p += 1
            v |= (c & 0x7F) << sh
            if not c & 0x80:
                return v
            sh += 7

    def zigzag(self) -> int:
        v = self.varint()
        return (v >> 1) ^ -(v & 1)

    def value(self, t):
        if t == 1:
            return True
        if t == 2:
            return False
        if t == 3:
            self.p += 1
            return self.b[self.p - 1]
        if t in (4, 5, 6):
            return self.zigzag()
        if t == 7:
            self.p += 8
            return struct.unpack("<d", bytes(self.b[self.p - 8:self.p]))[0]
        if t == 8:
            n = self.varint()
            self.p += n
            return bytes(self.b[self.p - n:self.p])
        if t in (9, 10):
            h = self.b[self.p]
            self.p += 1
            n = h >> 4
            if n == 15:
                n = self.varint()
            et = h & 0x0F
            if et in (1, 2):   # list<bool>: one byte per element
                out = [self.b[self.p + i] == 1 for i in range(n)]
                self.p += n
                return out
            return [self.value(et) for _ in range(n)]
        if t == 11:
            n = self.varint()
            if n == 0:
                return {}
            kv = self.b[self.p]
            self.p += 1
            return {self.value(kv >> 4): self.value(kv & 0x0F) for _ in range(n)}
        if t == 12:
            return self.struct()
        raise ValueError(f"thrift compact: unknown type {t}")

    def struct(self) -> dict:
        out, fid = {}, 0
        while True:
            h = self.b[self.p]
            self.p += 1
            if h == 0:
                return out
            d, t = h >> 4, h & 0x0F
            fid = fid + d if d else self.zigzag()
            out[fid] = self.value(t)
