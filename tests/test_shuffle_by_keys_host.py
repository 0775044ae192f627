"""Dataset.shuffle_by_keys refuses bad arguments before any GPU work (no GPU needed), and exists
under both package names."""
import pandas as pd
import pytest


def _dataset():
    import nvtabular_amd as nvt

    df = pd.DataFrame({"a": [1, 2, 3, 4], "b": [1.0, 2.0, 3.0, 4.0], "c": [5, 6, 7, 8], "d": [0, 1, 0, 1],
                       "e": [9, 9, 9, 9], "l": [[1], [2, 3], [], [4]]})
    return nvt.Dataset(df, npartitions=2)


def test_unknown_key_lists_the_missing_names():
    with pytest.raises(ValueError, match=r"unknown key columns \['nope', 'zzz'\]"):
        _dataset().shuffle_by_keys(["a", "nope", "zzz"])
    with pytest.raises(ValueError, match="nope"):
        _dataset().shuffle_by_keys("nope")
    with pytest.raises(ValueError, match="at least one"):
        _dataset().shuffle_by_keys([])


def test_list_key_is_a_type_error():
    with pytest.raises(TypeError, match="list columns cannot be keys"):
        _dataset().shuffle_by_keys(["a", "l"])


def test_more_than_four_keys():
    with pytest.raises(NotImplementedError, match="at most 4"):
        _dataset().shuffle_by_keys(["a", "b", "c", "d", "e"])


@pytest.mark.parametrize("npartitions", [0, -1, 4097])
def test_npartitions_out_of_range(npartitions):
    with pytest.raises(ValueError, match="npartitions must be 1 to 4096"):
        _dataset().shuffle_by_keys("a", npartitions=npartitions)


def test_hive_data_is_not_supported():
    with pytest.raises(NotImplementedError, match="hive-partitioned directories are not tracked by this Dataset"):
        _dataset().shuffle_by_keys("a", hive_data=True)


def test_more_than_one_rank_is_refused(monkeypatch):
    from nvtabular_amd import dist

    monkeypatch.setattr(dist, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="across ranks"):
        _dataset().shuffle_by_keys("a")


def test_same_method_through_the_nvtabular_name():
    import nvtabular

    import nvtabular_amd

    assert nvtabular.Dataset is nvtabular_amd.Dataset
    assert callable(nvtabular.Dataset.shuffle_by_keys)

