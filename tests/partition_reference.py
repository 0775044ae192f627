"""numpy restatement of the nvt_partition_* entries (include/nvt_hip.h): the finaliser and the
partition id of a key tag, the stable plan, and the segmented gather with packed validity bitmaps.
The GPU tests compare the kernels against these bit for bit; test_partition_reference.py checks the
restatement itself on hand-written cases."""
import numpy as np

M64 = (1 << 64) - 1


def mix(tags) -> np.ndarray:
    """The fixed 64-bit finaliser of nvt_partition_ids (wrapping uint64 arithmetic)."""
    z = np.asarray(tags).astype(np.uint64, copy=True)
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def mix_int(tag: int) -> int:
    """The same on one Python integer (no numpy: checks the numpy form)."""
    z = tag & M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def partition_ids(tags, P: int) -> np.ndarray:
    """pid = (uint32)(((mix(tag) >> 32) * P) >> 32)"""
    hi = mix(tags) >> np.uint64(32)
    return ((hi * np.uint64(P)) >> np.uint64(32)).astype(np.uint32)


def plan(pid, P: int):
    """(perm int64[n], counts uint64[P]): the stable counting sort of the row indices by pid."""
    pid = np.asarray(pid)
    perm = np.argsort(pid, kind="stable").astype(np.int64)
    counts = np.bincount(pid.astype(np.int64), minlength=P).astype(np.uint64)
    return perm, counts


def pack_bits(mask) -> np.ndarray:
    """bool[m] -> LSB-first bitmap of ceil(m / 64) * 8 bytes, padding bits zero."""
    mask = np.asarray(mask, dtype=bool)
    out = np.zeros((len(mask) + 63) // 64 * 8, dtype=np.uint8)
    bits = np.packbits(mask, bitorder="little")
    out[: len(bits)] = bits
    return out


def unpack_bits(bitmap, n: int) -> np.ndarray:
    return np.unpackbits(np.asarray(bitmap, dtype=np.uint8), bitorder="little")[:n].astype(bool)


def gather(segments, with_valid: bool):
    """One output partition.  ``segments``: list of (src values, src bitmap or None, idx); output
    rows are src[idx] segment after segment.  -> (values, bitmap or None); a segment without a
    bitmap counts as all valid."""
    vals = [np.asarray(src)[np.asarray(idx, dtype=np.int64)] for src, _, idx in segments]
    out = np.concatenate(vals) if vals else np.zeros(0)
    if not with_valid:
        return out, None
    masks = []
    for src, bitmap, idx in segments:
        idx = np.asarray(idx, dtype=np.int64)
        masks.append(np.ones(len(idx), dtype=bool) if bitmap is None else unpack_bits(bitmap, len(src))[idx])
    return out, pack_bits(np.concatenate(masks) if masks else np.zeros(0, dtype=bool))
