"""Host-side logic that needs neither the GPU nor the shared library."""
import numpy as np


def test_estimate_distinct_model():
    from nvtabular_amd.kernels import _estimate_distinct as est

    m, n = 1 << 18, 45_000_000
    assert est(2, m, n) < 100
    assert 3 * 3500 <= est(3500, m, n) < 12_000            # stays on the LDS-table path
    assert est(20_000, m, n) > 11_000                       # partitioned path
    assert est(m - 10, m, n) == n                           # (almost) all unique
    for D in (50_000, 1_000_000, 20_000_000):               # uniform model, within the 3x margin
        d = int(D * (1 - np.exp(-m / D)))
        assert D <= est(d, m, n) <= min(n, 3.5 * D + 100)


def test_rank_sharding_semantics(tmp_path):
    """Under torch.distributed a parquet dataset is a global list (rank r takes every world-th
    partition); frames handed over in memory are the rank's own shard and are all kept --
    bench.py builds one frame per rank, which an index filter would silently drop on ranks > 0."""
    import pandas as pd

    from nvtabular_amd.io import Dataset

    parts = [pd.DataFrame({"a": np.arange(4) + 10 * i}) for i in range(5)]
    mem = Dataset(parts)
    assert len(list(mem._host_parts(None, None))) == 5
    assert len(list(mem._host_parts(None, (1, 2)))) == 5      # rank-local: nothing is skipped
    one = Dataset(parts[0])
    assert len(list(one._host_parts(None, (3, 8)))) == 1       # the bench.py case
    path = tmp_path / "d.parquet"
    pd.concat(parts).to_parquet(path, row_group_size=4)
    pq = Dataset(str(path), engine="parquet", row_groups_per_part=1)
    assert pq.npartitions == 5

    def first(t):   # (a pyarrow table, or the hand-written reader's staged partition)
        return int(t.columns["a"].values[0]) if hasattr(t, "to_device") else t.column("a")[0].as_py()

    firsts = lambda shard: [first(t) for t in pq._host_parts(None, shard)]
    assert firsts(None) == [0, 10, 20, 30, 40]
    assert firsts((0, 2)) == [0, 20, 40] and firsts((1, 2)) == [10, 30]


def test_path_selection_thresholds():
    """kernels._path_for: the C-ABI path id for an expected distinct count (include/nvt_hip.h)."""
    from nvtabular_amd import kernels as K

    assert K._path_for(0) == 0                      # unknown: start on the plain LDS-table path
    assert K._path_for(3) == 6 and K._path_for(64) == 6
    assert K._path_for(65) == 0 and K._path_for(K.PATH_S_MAX_DISTINCT) == 0
    # 11-21 k int32 keys: two key classes (path 7) only without the hot-key filter
    # int32 keys without weights: the range path (9) from the end of the LDS-table path up to
    # ~6.5 M distinct keys, hash partitions beyond
    rng_on = K.USE_RANGE and K.HOT_FILTER
    assert K._path_for(K.PATH_S_MAX_DISTINCT + 1) == (9 if rng_on else 1 if K.HOT_FILTER else 7)
    assert K._path_for(int(K.PATH_S2_FACTOR * K.PATH_S_MAX_DISTINCT) + 1) == (9 if rng_on else 1)
    assert K._path_for(K.PATH_P1_MAX_DISTINCT + 1) == (9 if rng_on else 2)
    # beyond the range path: the sort path (int32 keys without weights), hash partitions otherwise
    assert K._path_for(K.PATH_RANGE_MAX_DISTINCT + 1) == (K.PATH_SORT if K.USE_SORT else 2)
    assert K._path_for(K.PATH_P2_MAX_DISTINCT + 1) == (K.PATH_SORT if K.USE_SORT else 3)
    assert K._path_for(K.PATH_P2_MAX_DISTINCT + 1, small_tables=True) == 3
    j = K.DenseCountJob.__new__(K.DenseCountJob)
    j.min_range_bits = 8
    # (round 6: 10000 keys per bucket -- 256 buckets up to 2.56 M keys, 512 up to 5.12 M)
    kpb = K.RANGE_KEYS_PER_BUCKET
    for hint, bits in ((12_000, 8), (256 * kpb, 8), (256 * kpb + 1, 9), (512 * kpb, 9), (512 * kpb + 1, 10),
                       (6_400_000, 10 if 6_400_000 > 512 * kpb else 9)):
        j.hint = hint
        assert j.range_bits() == bits, (hint, j.range_bits())
    # (int32 keys without weights never reach the global-table fallback: the sort path has no
    # capacity limit below 2^30 rows)
    assert K._path_for(K.PATH_P3_MAX_DISTINCT + 1) == (K.PATH_SORT if K.USE_SORT else -1)
    assert K._path_for(K.PATH_P3_MAX_DISTINCT + 1, small_tables=True) == -1   # global-table fallback
    # int64 keys / weighted merges use the smaller tables
    assert K._path_for(K.PATH_S_MAX_WEIGHTED + 1, small_tables=True) == 7
    assert K._path_for(int(K.PATH_S2_FACTOR * K.PATH_S_MAX_WEIGHTED) + 1, small_tables=True) == 1
    assert K._path_for(K.PATH_P1_MAX_SMALL + 1, small_tables=True) == 2
    assert K._path_for(K.PATH_P2_MAX_DISTINCT + 1, small_tables=True) == 3
    # escalation order covers every automatic path exactly once
    assert sorted(K.PATH_ORDER) == [0, 1, 2, 3, 6, 7] and set(K._PATH_MAX) >= set(K.PATH_ORDER)


def test_shuffle_option_coercion():
    from nvtabular_amd.io import Shuffle

    assert Shuffle.coerce(None) is None and Shuffle.coerce(False) is None
    assert Shuffle.coerce(True) == Shuffle.PER_WORKER
    assert Shuffle.coerce(Shuffle.PER_PARTITION) == Shuffle.PER_PARTITION
    assert Shuffle.coerce(Shuffle.FULL) == Shuffle.PER_WORKER
    import pytest

    with pytest.raises(ValueError):
        Shuffle.coerce("sideways")


def test_graph_json_dtype_and_tag_records():
    """The merlin DType / Tags records of graph_serializer.py:106-153 as this engine writes
    and reads them."""
    from nvtabular_amd import Tags
    from nvtabular_amd import graph_json as G

    d = G._dtype_to_dict(np.dtype("int32"), with_shape=True)
    assert d == {"name": "int32", "element_type": "int", "element_size": 32, "signed": True,
                 "shape": [{"min": None, "max": None}]}
    assert G._dtype_to_dict(np.float64)["element_type"] == "float"
    lst = G._dtype_to_dict(np.int64, is_list=True, is_ragged=True, with_shape=True)
    assert len(lst["shape"]) == 2 and lst["shape"][1] == {"min": 0, "max": None}
    assert G._dtype_from_dict({"name": "int64"}) == np.dtype("int64")
    assert G._dtype_from_dict("float32") == np.dtype("float32")
    assert G._dtype_from_dict({"name": "str"}) == np.dtype("O")
    assert G._dtype_from_dict({"name": "weird", "element_type": "uint", "element_size": 8}) == np.dtype("uint8")
    assert G._tags_to_list([Tags.CATEGORICAL, Tags.LIST]) == ["Tags.CATEGORICAL", "Tags.LIST"]
    assert G._tags_from_list(["Tags.CONTINUOUS", "categorical", "Tags.NOT_A_TAG"]) == [
        Tags.CONTINUOUS, Tags.CATEGORICAL]
    assert G._paths_from_json(G._paths_to_json({("a", "b"): "/x/art/categories/u.parquet"}, "/x/art"),
                              "/y") == {("a", "b"): "/y/categories/u.parquet"}


def test_one_pass_class_order_equals_count_desc_key_asc():
    """The rule behind nvt_vocab_order.hip's cls_scatter_kernel, emulated in numpy: for a KEY-SORTED
    (key, count) list, "count descending, key ascending" (categorify.py:1300,1316 with the stable
    tie rule) == class 255 (count >= 255) sorted on its own, followed by classes 254 .. 1, each in
    the key order the list already has.  (The GPU tests compare the kernel with the oracle; this
    pins the algebra the kernel relies on.)"""
    import numpy as np

    rng = np.random.default_rng(0)
    keys = np.unique(rng.integers(-2**31, 2**31 - 1, 50_000).astype(np.int64))  # sorted, distinct
    counts = np.minimum(rng.zipf(1.3, keys.size), 10**6).astype(np.int64)
    want = np.lexsort((keys, -counts))                       # count desc, key asc
    cls = np.minimum(counts, 255)
    digit = 255 - cls                                        # class 255 first
    order = np.argsort(digit, kind="stable")                 # ONE stable counting pass
    n_big = int((cls == 255).sum())
    head = order[:n_big]
    head = head[np.lexsort((keys[head], -counts[head]))]     # the small sort of class 255
    got = np.concatenate([head, order[n_big:]])
    np.testing.assert_array_equal(got, want)
    # and the flat range table: positions of the sorted keys under a monotone slot function with
    # linear probing are a prefix maximum, p_i = i + max_{j <= i}(h_j - j)
    slots = 1 << 17
    span = int(keys[-1] - keys[0])
    h = ((keys - keys[0]).astype(np.float64) * (slots / (span + 1))).astype(np.int64)
    p = np.arange(keys.size) + np.maximum.accumulate(h - np.arange(keys.size))
    ref = np.empty(keys.size, dtype=np.int64)
    last = -1
    for i, hi in enumerate(h.tolist()):                      # sequential linear probing
        last = max(hi, last + 1)
        ref[i] = last
    np.testing.assert_array_equal(p, ref)


def test_fold_sparse_and_sorted_groupby_eligibility():
    """Host logic of the groupby sort path: dense per-(group, fold) statistics -> the compacted
    [fold, key] groups of the reference's second aggregate (only pairs that have rows), and
    which inputs may take the sort path at all."""
    import torch

    from nvtabular_amd import kernels as K
    from nvtabular_amd.ops._groupby import fold_sparse

    kfold = 3
    keys = torch.tensor([-7, 2, 40], dtype=torch.int64)
    fsize = torch.tensor([1, 0, 2, 0, 0, 5, 3, 3, 0], dtype=torch.int64)  # [g * kfold + f]
    fsum = torch.arange(9, dtype=torch.float64) * 1.5
    comp = dict(keys=[keys], n=3, fold=dict(kfold=kfold, size=fsize, sum=[fsum]))
    sp = fold_sparse(comp)
    assert sp["n"] == 5
    assert sp["keys"][0].tolist() == [0, 2, 2, 0, 1]          # fold ids
    assert sp["keys"][1].tolist() == [-7, -7, 2, 40, 40]      # keys
    assert sp["size"].tolist() == [1, 2, 5, 3, 3] and sp["count"].tolist() == sp["size"].tolist()
    assert sp["sum"][0].tolist() == [0.0, 3.0, 7.5, 9.0, 10.5]
    assert sp["null_mask"].tolist() == [0] * 5 and sp["sumsq"] == [] and sp["min"] == []
    n = K.SORTED_GROUPBY_MIN_ROWS
    k32, k64 = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int64)
    assert K.sorted_groupby_eligible(k32, None, n) and K.sorted_groupby_eligible(k64, None, n, 5)
    assert not K.sorted_groupby_eligible(k32, None, n - 1)                 # launch latency
    assert not K.sorted_groupby_eligible(k32, torch.zeros(1, dtype=torch.uint8), n)  # null keys
    assert not K.sorted_groupby_eligible(torch.zeros(4, dtype=torch.uint8), None, n)
    assert not K.sorted_groupby_eligible(k32, None, n, K.SORTED_GROUPBY_MAX_KFOLD + 1)
    assert not K.sorted_groupby_eligible(k32, None, (1 << 29) + 1, 5)      # row index + 3 fold bits > 32
    assert K.sorted_groupby_eligible(k32, None, (1 << 29), 5)


def test_harness_rehearsals_collect_last():
    """Tests that shell out to bench.py / torchrun live in test_zz_rehearsals.py only: under
    `pytest -x` a harness assertion must not be able to mask the kernel-parity tests collected
    behind it (Weak #1)."""
    import glob
    import os
    import re

    here = os.path.dirname(os.path.abspath(__file__))
    files = sorted(glob.glob(os.path.join(here, "test_*.py")))
    assert os.path.basename(files[-1]) == "test_zz_rehearsals.py"
    for f in files[:-1]:
        if os.path.basename(f).startswith("test_gpu_"):
            src = open(f).read()
            assert not re.search(r"subprocess|torch\.distributed\.run", src), f


def test_bench_parity_verdicts_cover_every_leg():
    """bench.parity_verdicts: a failed nested leg, an extra that died and an extra without a parity leg
    all make the line's top-level verdict false; only oracle legs count into parity_rows."""
    import bench

    line = {"parity": {"parity_checked_rows": 100, "parity_ok": True, "full_frame_ok": True},
            "extra_configs": {"a": {"parity": {"method": "oracle ...", "parity_checked_rows": 5, "parity_ok": True}},
                              "b": {"parity": {"method": "files ...", "files_equal_in_memory_transform": True}},
                              "c": {"parity": {"method": "properties ...", "parity_ok": True, "rows": 10 ** 9}}}}
    assert bench.parity_verdicts(line) == (True, 105, [])
    line["parity"]["full_frame_ok"] = False
    line["extra_configs"]["a"]["parity"]["parity_ok"] = False
    line["extra_configs"]["d"] = {"error": "RuntimeError('x')"}
    line["extra_configs"]["e"] = {"ms_per_step": 1.0}
    ok, rows, failed = bench.parity_verdicts(line)
    assert not ok and failed == ["headline.full_frame", "a", "d:error", "e:no parity leg"]
