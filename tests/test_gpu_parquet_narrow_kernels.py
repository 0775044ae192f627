"""nvt_expand_narrow, nvt_pq_bool_pack and nvt_pq_widen_i32_many against numpy, guard bytes around
every output (kernels_parquet_narrow.py; include/nvt_hip.h)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64


def dev():
    return torch.device("cuda:0")


def t(v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(dev())


def _guards_untouched(out, used=None):
    """The 0xA5 bytes in front of and behind the view of ``out`` (``used``: the bytes of the view
    that are written; what lies behind them inside the view must be untouched too)."""
    raw = out.raw.cpu().numpy()
    nbytes = out.numel() * out.element_size()
    assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + nbytes:] == 0xA5).all()
    if used is not None:
        assert (raw[GUARD + used: GUARD + nbytes] == 0xA5).all()


def _bitmap_words(bits, n, rng):
    """ceil(n / 64) words of an Arrow bitmap of bits[:n] with GARBAGE behind bit n."""
    words = (n + 63) // 64
    full = rng.integers(0, 2, words * 64).astype(bool)
    full[:n] = bits
    return np.packbits(full, bitorder="little")


@pytest.mark.parametrize("sizes", ["4->1", "4->2", "1->1"])
@pytest.mark.parametrize("pattern", ["absent", "all", "none", "last", "random"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4099])
def test_expand_narrow(n, pattern, sizes):
    from nvtabular_amd import kernels_parquet_narrow as KPN

    rng = np.random.default_rng(n * 7 + len(pattern))
    dtype, np_dt = {"4->1": (torch.int8, np.int8), "4->2": (torch.int16, np.int16), "1->1": (torch.bool, np.bool_)}[sizes]
    bits = {"absent": np.ones(n, bool), "all": np.ones(n, bool), "none": np.zeros(n, bool),
            "last": np.arange(n) == n - 1, "random": rng.random(n) < 0.5}[pattern]
    nv = int(bits.sum())
    if sizes == "1->1":
        packed = rng.integers(0, 2, nv).astype(np.uint8)
    else:   # values outside the target range keep their low bits; the type's extremes are among them
        packed = rng.integers(-2**31, 2**31, nv).astype(np.int32)
        packed[: min(nv, 4)] = np.array([-128, 127, -32768, 32767], dtype=np.int32)[: min(nv, 4)]
    bitmap = None if pattern == "absent" else t(_bitmap_words(bits, n, rng))
    out = KPN.expand_narrow(t(packed), dtype, bitmap, n, guard=GUARD)
    torch.cuda.synchronize()
    want = np.zeros(n, dtype=np_dt)
    want[bits] = packed.astype(np_dt)
    assert out.dtype == dtype and out.numel() == n
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    _guards_untouched(out)


def test_bool_pack_pages():
    """One call with pages of 0, 1, 7, 8, 9, 64 and 513 values, an empty page in the middle: every
    page is np.packbits(bitorder="little") of its values at its byte, tail bits 0, and nothing is
    written behind the last page."""
    from nvtabular_amd import kernels_parquet_narrow as KPN

    rng = np.random.default_rng(3)
    sizes = [0, 1, 7, 8, 0, 9, 64, 513]
    page_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    vals = rng.random(int(page_start[-1])) < 0.5
    vals[-1] = True
    out = KPN.bool_pack(t(vals), t(page_start), guard=GUARD)
    torch.cuda.synchronize()
    byte_at = KPN.bool_byte_at(t(page_start)).cpu().numpy()
    np.testing.assert_array_equal(byte_at, np.concatenate([[0], np.cumsum([(s + 7) // 8 for s in sizes])]))
    assert out.numel() == (len(vals) + 7) // 8 + len(sizes)
    got = out.cpu().numpy()
    for p, s in enumerate(sizes):
        want = np.packbits(vals[page_start[p]: page_start[p + 1]], bitorder="little")
        np.testing.assert_array_equal(got[byte_at[p]: byte_at[p + 1]], want, err_msg=f"page {p}")
    _guards_untouched(out, used=int(byte_at[-1]))


def test_bool_pack_without_values_launches_nothing():
    from nvtabular_amd import kernels_parquet_narrow as KPN

    out = KPN.bool_pack(t(np.zeros(0, dtype=bool)), t(np.zeros(2, dtype=np.int64)), guard=GUARD)
    torch.cuda.synchronize()
    _guards_untouched(out, used=0)


@pytest.mark.parametrize("shift", [1, 3])
def test_widen_many(shift):
    """Several descriptors in one call: n in {0, 1, 15, 16, 17, 4099}, int8 and int16 sources that start
    ``shift`` elements behind a 16-byte boundary, the types' extremes among the values."""
    from nvtabular_amd import kernels_parquet_narrow as KPN

    rng = np.random.default_rng(shift)
    srcs, wants = [], []
    for np_dt in (np.int8, np.int16):
        info = np.iinfo(np_dt)
        for n in (0, 1, 15, 16, 17, 4099):
            v = rng.integers(info.min, info.max + 1, n + shift).astype(np_dt)
            v[shift: shift + 2] = np.array([info.min, info.max], dtype=np_dt)[: max(0, min(2, n))]
            base = t(v)
            assert base.data_ptr() % 16 == 0
            srcs.append(base[shift:])
            wants.append(v[shift:].astype(np.int32))
    outs = KPN.widen_many(srcs, guard=GUARD)
    torch.cuda.synchronize()
    assert len(outs) == len(srcs)
    for out, want in zip(outs, wants):
        assert out.dtype == torch.int32
        np.testing.assert_array_equal(out.cpu().numpy(), want)
        _guards_untouched(out)


def test_widen_refuses_other_sources():
    import ctypes as C

    from nvtabular_amd import _lib

    lib = _lib.load()
    d = (_lib.PqWidenCol * 1)()
    buf = t(np.zeros(16, dtype=np.int32))
    d[0].src, d[0].dst, d[0].n, d[0].src_dtype = buf.data_ptr(), buf.data_ptr(), 4, _lib.NVT_I32
    assert lib.nvt_pq_widen_i32_many(d, 1, None) == _lib.NVT_EINVAL and b"src_dtype" in lib.nvt_last_error()
    d[0].src_dtype, d[0].dst = _lib.NVT_I8, buf.data_ptr() + 2
    assert lib.nvt_pq_widen_i32_many(d, 1, None) == _lib.NVT_EINVAL and b"aligned" in lib.nvt_last_error()
    assert lib.nvt_expand_narrow(buf.data_ptr(), 8, 1, None, 4, buf.data_ptr(), None, None) == _lib.NVT_EINVAL
    assert C.c_int(lib.nvt_pq_bool_pack(None, None, None, 0, None, None)).value == 0
