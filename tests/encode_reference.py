"""Plain numpy references of Categorify's encode step and of the hash-bucket step, for the
kernel-level tests of csrc/nvt_encode.hip, nvt_encode_build.hip and nvt_hash_bucket.hip
(test_gpu_encode_kernels.py).  test_encode_reference.py pins them to the pandas oracle on the CPU.  Nothing here shares code with the device side: the
lookup is ``np.unique`` + ``searchsorted``, the hash is the oracle's murmur3 finaliser (itself
pinned to the documented constants in test_oracle_golden.py).
"""
import numpy as np

import oracle as O


def pack_bits(bits) -> np.ndarray:
    """Arrow validity bitmap (LSB first) of a boolean array: bit i set = row i valid."""
    return np.packbits(np.asarray(bits, dtype=bool), bitorder="little")


def encode_ref(keys, valid_bool, vocab_keys, first_label, null_label, oov_label, num_buckets, out_dtype):
    """Labels of ``keys`` against the ordered vocabulary ``vocab_keys``.

    * a row whose validity bit is clear: ``null_label``, whatever bytes lie under it;
    * a valid key of the vocabulary: ``first_label`` + the position of its FIRST occurrence
      (user-supplied vocabularies may hold a key twice);
    * any other valid key: ``oov_label``, plus ``nvt_hash32(key) % num_buckets`` when
      ``num_buckets > 1``.
    The smallest integer of the key type is a key like any other.  ``valid_bool`` None = all valid.
    """
    keys = np.asarray(keys)
    vocab_keys = np.asarray(vocab_keys)
    n = keys.size
    out = np.full(n, int(oov_label), dtype=np.int64)
    nb = int(num_buckets or 0)
    if nb > 1 and n:
        out += (O.nvt_hash32(keys.astype(np.int64)).astype(np.uint64) % np.uint64(nb)).astype(np.int64)
    if vocab_keys.size and n:
        uniq, first_pos = np.unique(vocab_keys.astype(np.int64), return_index=True)   # first occurrence
        k64 = keys.astype(np.int64)
        at = np.searchsorted(uniq, k64)
        at_c = np.minimum(at, uniq.size - 1)
        found = uniq[at_c] == k64
        out[found] = int(first_label) + first_pos[at_c[found]].astype(np.int64)
    if valid_bool is not None:
        out[~np.asarray(valid_bool, dtype=bool)] = int(null_label)
    return out.astype(out_dtype)


def found_mask(keys, valid_bool, vocab_keys) -> np.ndarray:
    """True where a row is valid and its key is in the vocabulary."""
    m = np.isin(np.asarray(keys).astype(np.int64), np.asarray(vocab_keys).astype(np.int64))
    if valid_bool is not None:
        m &= np.asarray(valid_bool, dtype=bool)
    return m


def hash64_ref(keys, valid_bool=None, xor_in=None) -> np.ndarray:
    """uint64 row hash of the hash-bucket kernel: murmur3 fmix64 of the sign-extended key, a null
    row hashing as key 0; ``xor_in`` (uint64, the hash carried over from the columns in front of a
    hashed cross) is XOR-ed in."""
    k = np.asarray(keys).astype(np.int64).copy()
    if valid_bool is not None:
        k[~np.asarray(valid_bool, dtype=bool)] = 0
    h = O.nvt_hash64(k)
    if xor_in is not None:
        h = h ^ np.asarray(xor_in).view(np.uint64)
    return h


def hash_bucket_ref(keys, valid_bool, num_buckets, xor_in=None) -> np.ndarray:
    """int32 bucket: the high 32 bits of the row hash modulo ``num_buckets``."""
    h = hash64_ref(keys, valid_bool, xor_in)
    return ((h >> np.uint64(32)) % np.uint64(int(num_buckets))).astype(np.int32)


def first_mismatch(got, exp, what: str) -> None:
    """assert_array_equal with a message that names the case, the first mismatching row and
    got / expected there."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype, f"{what}: dtype {got.dtype}, expected {exp.dtype}"
    assert got.shape == exp.shape, f"{what}: shape {got.shape}, expected {exp.shape}"
    bad = np.flatnonzero(got != exp)
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} rows differ, first at row {i}: "
                             f"got {got[i]}, expected {exp[i]}")
    np.testing.assert_array_equal(got, exp)
