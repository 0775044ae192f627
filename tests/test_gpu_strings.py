"""String columns keyed on the device from Arrow buffers (nvt_str_*, kernels_strings.py) give
exactly what the host path (strings.string_column_to_device: pandas' SipHash per row) gives:
the same int64 surrogates, the same validity and the same {surrogate -> str} dict, in the same
order."""
import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")

INT64_MIN = np.iinfo(np.int64).min


def _dev():
    return torch.device("cuda", 0)


def _expected_keys(values):
    """pandas' surrogates (0 under a null) -- the contract of nvt_str_hash."""
    out = np.zeros(len(values), dtype=np.int64)
    idx = [i for i, v in enumerate(values) if v is not None]
    if idx:
        out[idx] = pd.util.hash_array(np.array([values[i] for i in idx], dtype=object),
                                      categorize=False).view(np.int64)
    return out


def _host(values, dev=None):
    from nvtabular_amd.strings import string_column_to_device

    return string_column_to_device(pd.Series(values, dtype=object), dev or _dev())


def _assert_same(got, exp):
    np.testing.assert_array_equal(got.data.cpu().numpy(), exp.data.cpu().numpy())
    assert got.data.dtype == exp.data.dtype == torch.int64
    assert (got.valid is None) == (exp.valid is None)
    if got.valid is not None:
        np.testing.assert_array_equal(got.valid_mask_host(), exp.valid_mask_host())
    assert type(got.strings) is dict
    assert got.strings == exp.strings
    assert list(got.strings) == list(exp.strings)   # first-appearance order


def _random_strings(rng, n, max_len=300, alphabet="abcXYZ019 _-é€\U0001F600"):
    chars = np.array(list(alphabet), dtype=object)
    lens = rng.integers(0, max_len + 1, n)
    return ["".join(rng.choice(chars, size=int(k))) for k in lens]


# ---- hash entry ------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", ["string", "large_string"])
def test_hash_matches_pandas(typ):
    from nvtabular_amd import kernels_strings as KS

    rng = np.random.default_rng(7)
    vals = [("q" * k) for k in range(0, 301)]                    # every length 0..300
    vals += _random_strings(rng, 2000)                          # multi-byte UTF-8
    vals += _random_strings(rng, 500, alphabet="ab\x00é")       # embedded NUL bytes
    vals += ["".join(rng.choice(list("0123456789abcdef"), size=65536)) for _ in range(3)]
    vals += ["€" * 21845 + "z"]                             # 64 KB of 3-byte code points
    for i in rng.choice(len(vals), 100, replace=False):
        vals[i] = None
    arr = pa.array(vals, type=getattr(pa, typ)())
    got = KS.hash_array(arr, _dev()).cpu().numpy()
    np.testing.assert_array_equal(got, _expected_keys(vals))
    # sliced: the first offset is not 0 and the bitmap does not start on a byte boundary
    for start, stop in ((3, 2000), (8, 1000), (301, 302), (17, 17)):
        sl = arr.slice(start, stop - start)
        got = KS.hash_array(sl, _dev()).cpu().numpy()
        np.testing.assert_array_equal(got, _expected_keys(vals[start:stop]))


def test_hash_every_alignment_and_tail():
    """Each length 0..40 at each start alignment 0..7 of the chars buffer."""
    from nvtabular_amd import kernels_strings as KS

    vals = []
    for pad in range(8):
        for k in range(41):
            vals += ["p" * pad, "".join(chr(0x41 + (i * 7 + k) % 26) for i in range(k))]
    got = KS.hash_array(pa.array(vals, type=pa.string()), _dev()).cpu().numpy()
    np.testing.assert_array_equal(got, _expected_keys(vals))


# ---- dedup + verify ---------------------------------------------------------------------------
def _buffers(vals, typ=None):
    from nvtabular_amd import kernels_strings as KS

    return KS.upload(pa.array(vals, type=typ or pa.string()), _dev())


def test_dedup_first_appearance():
    from nvtabular_amd import kernels_strings as KS

    rng = np.random.default_rng(1)
    pool = _random_strings(rng, 500, max_len=20)
    vals = [pool[i] for i in rng.zipf(1.3, 50_000) % 500]
    for i in rng.choice(len(vals), 2000, replace=False):
        vals[i] = None
    b = _buffers(vals)
    keys = KS.hash_buffers(b)
    m, bad, rep_keys, rep_strs = KS.dedup(keys, b.valid, b)
    s = pd.Series(vals, dtype=object)
    uniq = pd.unique(s.dropna())
    first = [vals.index(u) for u in uniq]
    assert bad == 0 and m == len(uniq)
    np.testing.assert_array_equal(rep_strs.cpu().numpy(), first)
    np.testing.assert_array_equal(rep_keys.cpu().numpy(), _expected_keys(list(uniq)))


def test_dedup_reports_forged_collisions():
    from nvtabular_amd import kernels_strings as KS

    vals = ["apple", "pear", "apple", "fig", "pear!", "apple"]
    b = _buffers(vals, pa.large_string())
    keys = torch.tensor([5, 9, 5, 5, 9, 5], dtype=torch.int64, device=_dev())   # fig / pear! collide
    m, bad, rep_keys, rep_strs = KS.dedup(keys, None, b)
    assert (m, bad) == (2, 2)
    assert rep_keys.cpu().tolist() == [5, 9] and rep_strs.cpu().tolist() == [0, 1]
    with pytest.raises(ValueError, match="64-bit surrogate collision between distinct strings"):
        KS.lookup_dict(keys, None, b)
    # same length, bytes differ only in the last block
    b2 = _buffers(["abcdefghijk", "abcdefghijx"])
    keys2 = torch.tensor([1, 1], dtype=torch.int64, device=_dev())
    assert KS.dedup(keys2, None, b2)[:2] == (1, 1)


def test_dedup_sentinel_and_all_equal_keys():
    from nvtabular_amd import kernels_strings as KS

    vals = ["x", "y", "x", "y", "z"] * 1000
    b = _buffers(vals)
    keys = torch.tensor([INT64_MIN, 3, INT64_MIN, 3, 0] * 1000, dtype=torch.int64, device=_dev())
    m, bad, rep_keys, rep_strs = KS.dedup(keys, None, b)
    assert (m, bad) == (3, 0)
    assert rep_keys.cpu().tolist() == [INT64_MIN, 3, 0] and rep_strs.cpu().tolist() == [0, 1, 4]
    assert KS.lookup_dict(keys, None, b) == {INT64_MIN: "x", 3: "y", 0: "z"}
    # one key for every row: equal strings are no collision, the others are
    same = torch.full((5000,), 42, dtype=torch.int64, device=_dev())
    assert KS.dedup(same, None, _buffers(["w"] * 5000))[:2] == (1, 0)
    assert KS.dedup(same, None, b)[:2] == (1, 3000)
    assert KS.dedup(torch.full((5000,), INT64_MIN, dtype=torch.int64, device=_dev()), None, b)[:2] == (1, 3000)


def test_embedded_nul_strings_keep_every_value():
    """pd.unique compares object strings only up to their first NUL, so the host path's dict
    drops every string that differs from an earlier one after a NUL; the keys agree, and the
    device dict holds every distinct string."""
    from nvtabular_amd.device import DeviceColumn

    vals = ["a\x00b", "a\x00c", None, "a\x00b", "\x00", "", "x\x00\x00y"] * 100
    got = DeviceColumn.from_arrow(pa.array(vals, type=pa.string()), _dev())
    exp = _host(vals)
    np.testing.assert_array_equal(got.data.cpu().numpy(), exp.data.cpu().numpy())
    np.testing.assert_array_equal(got.valid_mask_host(), exp.valid_mask_host())
    distinct = list(dict.fromkeys(v for v in vals if v is not None))
    assert got.strings == dict(zip(_expected_keys(distinct).tolist(), distinct))
    assert list(got.strings.values()) == distinct


# ---- column construction ----------------------------------------------------------------------
def _arrow_cases():
    rng = np.random.default_rng(3)
    pool = _random_strings(rng, 300, max_len=24)
    vals = [pool[i] for i in rng.zipf(1.2, 20_000) % 300]
    for i in rng.choice(len(vals), 500, replace=False):
        vals[i] = None
    nonull = [v if v is not None else "" for v in vals]
    s = pa.array(vals, type=pa.string())
    return {
        "string": (s, vals),
        "large_string": (pa.array(vals, type=pa.large_string()), vals),
        "no_nulls": (pa.array(nonull, type=pa.string()), nonull),
        "chunked": (pa.chunked_array([s.slice(0, 7001), s.slice(7001)]), vals),
        "sliced": (s.slice(13, 9000), vals[13:9013]),
        "sliced_by_8": (s.slice(16, 9000), vals[16:9016]),
        "empty": (pa.array([], type=pa.string()), []),
        "all_null": (pa.array([None] * 37, type=pa.string()), [None] * 37),
        "empty_strings": (pa.array([""] * 5 + [None], type=pa.large_string()), [""] * 5 + [None]),
    }


@pytest.mark.parametrize("case", list(_arrow_cases()))
def test_from_arrow_equals_host_path(case):
    from nvtabular_amd.device import DeviceColumn

    arr, vals = _arrow_cases()[case]
    _assert_same(DeviceColumn.from_arrow(arr, _dev()), _host(vals))


def test_from_arrow_list_of_strings():
    from nvtabular_amd.device import DeviceColumn

    rows = [["a", "bb"], [], None, ["bb", None, "ccc€"], ["a"]] * 200
    got = DeviceColumn.from_arrow(pa.array(rows, type=pa.list_(pa.string())), _dev())
    leaves = [v for r in rows if r is not None for v in r]
    _assert_same(got, _host(leaves))
    off = np.cumsum([0] + [len(r) if r is not None else 0 for r in rows])
    np.testing.assert_array_equal(got.offsets.cpu().numpy(), off)


def test_dictionary_array_equals_host_path_on_decoded():
    from nvtabular_amd.device import DeviceColumn

    dictionary = pa.array(["red", "green", "blue€", "", "red"])   # (a repeated entry)
    for itype in (pa.int8(), pa.int32(), pa.int64()):
        idx = pa.array([0, 1, None, 2, 4, 3, None, 1, 0, 2] * 300, type=itype)
        arr = pa.DictionaryArray.from_arrays(idx, dictionary)
        for a in (arr, arr.slice(3, 2000)):
            got = DeviceColumn.from_arrow(a, _dev())
            _assert_same(got, _host(a.dictionary_decode().to_pylist()))


@pytest.mark.parametrize("dtype", [object, "string[pyarrow]", "string[python]"])
def test_from_pandas_equals_host_path(dtype):
    from nvtabular_amd.device import DeviceColumn

    rng = np.random.default_rng(5)
    pool = _random_strings(rng, 100, max_len=12)
    vals = [pool[i] for i in rng.integers(0, 100, 10_000)]
    vals[::17] = [None] * len(vals[::17])
    s = pd.Series(vals, dtype=dtype)
    _assert_same(DeviceColumn.from_pandas(s, _dev()), _host(vals))
    if dtype is object:
        s2 = s.copy()
        s2[::19] = np.nan     # NaN is missing as well
        _assert_same(DeviceColumn.from_pandas(s2, _dev()), _host(list(s2)))


@pytest.mark.parametrize("vals", [
    [b"ab", b"cd", None, b"ab"],          # bytes -> binary
    ["ab", 1, None, "ab"],                # mixed types
    ["ab", b"cd", "ef"],                  # str and bytes -> binary
    [None, None],                         # all missing -> null
    [],                                   # empty
])
def test_fallback_inputs_keep_the_host_path(monkeypatch, vals):
    from nvtabular_amd import kernels_strings as KS
    from nvtabular_amd.device import DeviceColumn
    from nvtabular_amd.strings import string_column_to_device

    exp = string_column_to_device(pd.Series(vals, dtype=object), _dev())

    def no_device(*a, **k):
        raise AssertionError("device path taken")

    monkeypatch.setattr(KS, "column_from_string_array", no_device)
    _assert_same(DeviceColumn.from_pandas(pd.Series(vals, dtype=object), _dev()), exp)


def test_large_zipf_column():
    from nvtabular_amd.device import DeviceColumn

    rng = np.random.default_rng(11)
    n, card = 20_000_000, 1_000_000
    vocab = pa.array([f"{x:016x}" for x in rng.integers(0, 2**63, card)])
    idx = pa.array((rng.zipf(1.1, n) % card).astype(np.int32))
    arr = pa.DictionaryArray.from_arrays(idx, vocab).dictionary_decode()
    got = DeviceColumn.from_arrow(arr, _dev())
    _assert_same(got, _host(arr.to_pandas()))


# ---- whole workflows without a host SipHash ---------------------------------------------------
def _string_frame(n=40_000):
    rng = np.random.default_rng(21)
    pool_a = [f"user_{x:08x}" for x in rng.integers(0, 2**32, 800)]
    pool_b = ["en", "fr", "de", "pté", "日本"]
    a = np.array(pool_a, dtype=object)[rng.zipf(1.2, n) % 800]
    b = np.array(pool_b, dtype=object)[rng.integers(0, 5, n)]
    a[rng.random(n) < 0.05] = None
    b[rng.random(n) < 0.02] = None
    return pd.DataFrame({
        "sa": a, "sb": b,
        "x": rng.normal(size=n),
        "y": (rng.random(n) < 0.3).astype("float32"),
    })


def _workflows(tmp, tag):
    from nvtabular_amd import ops

    return {
        "categorify": ["sa", "sb"] >> ops.Categorify(out_path=f"{tmp}/{tag}_c"),
        "categorify_freq": ["sa"] >> ops.Categorify(out_path=f"{tmp}/{tag}_f", freq_threshold=5),
        "categorify_combo": [["sa", "sb"]] >> ops.Categorify(out_path=f"{tmp}/{tag}_k", encode_type="combo"),
        "join_groupby": ["sa", ["sa", "sb"]] >> ops.JoinGroupby(out_path=f"{tmp}/{tag}_j", stats=["count", "sum"],
                                                                cont_cols=["x"]),
        "target_encoding": ["sa", ["sa", "sb"]] >> ops.TargetEncoding("y", out_path=f"{tmp}/{tag}_t", kfold=1,
                                                                      p_smooth=20),
        "hash_bucket": ["sa", "sb"] >> ops.HashBucket(97),
        "groupby": ["sa", "x"] >> ops.Groupby(groupby_cols=["sa"], aggs={"x": ["sum", "count"]}),
    }


def _run(name, tmp, tag, source):
    import nvtabular_amd as nvt

    wf = nvt.Workflow(_workflows(tmp, tag)[name])
    wf.fit(nvt.Dataset(source))
    return wf.transform(nvt.Dataset(source)).to_ddf().compute().reset_index(drop=True)


@pytest.mark.parametrize("name", ["categorify", "categorify_freq", "categorify_combo", "join_groupby",
                                  "target_encoding", "hash_bucket", "groupby"])
def test_workflow_without_host_hashing(tmp_path, monkeypatch, name):
    import pyarrow.parquet as pq

    import oracle as O
    from nvtabular_amd import strings

    df = _string_frame()
    path = str(tmp_path / "in.parquet")
    pq.write_table(pa.Table.from_pandas(df, preserve_index=False), path)
    odf = pd.read_parquet(path)
    # expected: the same workflow on host-path columns (pandas' SipHash per row)
    with monkeypatch.context() as m:
        m.setattr(strings, "as_string_array", lambda s: None)
        exp = _run(name, str(tmp_path), "host", odf.copy())

    def no_host_hash(values):
        raise AssertionError("host SipHash called")

    monkeypatch.setattr(strings, "string_key64", no_host_hash)
    got = _run(name, str(tmp_path), "dev", path)
    pd.testing.assert_frame_equal(got, exp, check_exact=False, rtol=1e-12)
    # and against the CPU oracle where it restates the operator
    if name == "categorify":
        paths = O.categorify_fit([odf], ["sa", "sb"], str(tmp_path / "o"), tie_break="stable")
        ref = O.categorify_transform(odf, ["sa", "sb"], paths)
        for c in ("sa", "sb"):
            np.testing.assert_array_equal(got[c].to_numpy(), ref[c].to_numpy())
    elif name == "categorify_freq":
        paths = O.categorify_fit([odf], ["sa"], str(tmp_path / "o"), tie_break="stable", freq_threshold=5)
        ref = O.categorify_transform(odf, ["sa"], paths)
        np.testing.assert_array_equal(got["sa"].to_numpy(), ref["sa"].to_numpy())
    elif name == "join_groupby":
        groups = ["sa", ["sa", "sb"]]
        cats = O.join_groupby_fit([odf.copy()], groups, ["x"], ["count", "sum"], str(tmp_path / "o"))
        ref = O.join_groupby_transform(odf.copy(), groups, cats)
        for c in ref.columns:
            np.testing.assert_allclose(got[c].to_numpy().astype("float64"), ref[c].to_numpy().astype("float64"),
                                       rtol=2e-5, atol=1e-6, err_msg=c)
    elif name == "target_encoding":
        groups = ["sa", ["sa", "sb"]]
        o = odf[["sa", "sb", "y"]].copy()
        st, means = O.target_encoding_fit([o], groups, ["y"], str(tmp_path / "o"), kfold=1)
        ref = O.target_encoding_transform(odf[["sa", "sb", "y"]].copy(), groups, ["y"], st, means, kfold=1,
                                          p_smooth=20)
        for c in ref.columns:
            np.testing.assert_allclose(got[c].to_numpy(), ref[c].to_numpy(), rtol=1e-5, atol=1e-6, err_msg=c)
