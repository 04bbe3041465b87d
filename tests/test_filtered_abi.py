"""Filtered search at the C ABI and in the host mirrors, without a GPU: the entry points are exported and declared on every
layer, bad filters are refused before any device is touched, and the ids-to-runs helper is right."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mx_index_search_filtered", "mx_index_search_filtered_device")


def test_filtered_entry_points_are_exported_and_declared(lib_built):
    from memex_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "memex_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib_built, name)
        assert name in _lib.EXPORTS
        assert f"int {name}(mx_index *idx," in hdr
    assert "const uint64_t *ranges, uint64_t n_ranges" in hdr
    # the stats struct grew at the end by the two counters, and the binding tracks it
    assert [f[0] for f in _lib.IndexStats._fields_][-2:] == ["filtered_queries", "subset_queries"]
    assert lib_built.mx_index_stats_size() == ctypes.sizeof(_lib.IndexStats)
    assert "uint64_t filtered_queries;" in hdr and "uint64_t subset_queries;" in hdr


def _call(lib, name, idx, ranges, n_ranges, B=1, k=10):
    q = (ctypes.c_float * 4)()
    ids = (ctypes.c_uint64 * k)()
    sc = (ctypes.c_float * k)()
    nf = (ctypes.c_int32 * B)()
    return getattr(lib, name)(idx, q, B, k, ranges, n_ranges, ids, sc, None, nf)


def test_filtered_argument_validation_without_device(lib_built):
    from memex_amd import _lib
    good = (ctypes.c_uint64 * 4)(1, 5, 9, 9)
    bad = (ctypes.c_uint64 * 4)(1, 5, 9, 8)
    for name in NAMES:
        # a null index with a valid filter: the code mx_index_search gives
        assert _call(lib_built, name, None, good, 2) == _lib.MX_ESEARCH
        assert _call(lib_built, name, None, None, 0) == _lib.MX_ESEARCH       # the empty filter is valid
        # the filter is checked first: null ranges with n_ranges > 0, and lo > hi in any pair
        assert _call(lib_built, name, None, None, 3) == _lib.MX_EINVAL
        assert b"null ranges" in lib_built.mx_last_error()
        assert _call(lib_built, name, None, bad, 2) == _lib.MX_EINVAL
        assert b"lo > hi" in lib_built.mx_last_error()
    ref = lib_built.mx_index_search(None, (ctypes.c_float * 4)(), 1, 10, None, None, None, None)
    assert ref == _lib.MX_ESEARCH


def test_host_mirrors_have_filtered_search():
    from memex_amd.index import FlatIndex
    from memex_amd.storage import HipFlatStore
    assert callable(FlatIndex.search_filtered) and callable(FlatIndex.search_filtered_device)
    assert callable(HipFlatStore.search_within)
    hpp = open(os.path.join(ROOT, "include", "memex_hip.hpp")).read()
    assert "std::vector<VectorSearchResult> search_within(const std::vector<float> &vec, size_t limit," in hpp
    assert "mx_index_search_filtered(" in hpp
    assert "mx_index_search_filtered(" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_exactly_one_filter_argument():
    from memex_amd.index import _filter_ranges
    for kw in ({}, {"ranges": [[1, 2]], "ids": [1]}):
        try:
            _filter_ranges(kw.get("ranges"), kw.get("ids"))
        except ValueError:
            pass
        else:
            raise AssertionError(kw)
    np.testing.assert_array_equal(_filter_ranges([[3, 9], [1, 2]], None), np.array([[3, 9], [1, 2]], dtype=np.uint64))


def test_ids_to_runs_on_random_id_sets():
    from memex_amd.index import ids_to_ranges
    rng = np.random.default_rng(5)
    assert ids_to_ranges([]).shape == (0, 2)
    np.testing.assert_array_equal(ids_to_ranges([5, 3, 4, 4, 9, 10, 1]), [[1, 2], [3, 6], [9, 11]])
    np.testing.assert_array_equal(ids_to_ranges(iter([7, 7, 8])), [[7, 9]])
    for trial in range(200):
        n = int(rng.integers(1, 400))
        ids = rng.integers(1, int(rng.integers(2, 600)), n).astype(np.uint64)   # duplicates, unsorted, adjacent runs
        r = ids_to_ranges(ids.tolist() if trial % 2 else ids)
        assert r.dtype == np.uint64 and r.shape[1] == 2
        assert (r[:, 0] < r[:, 1]).all()
        assert (r[1:, 0] > r[:-1, 1]).all()                      # sorted, disjoint, never adjacent (maximal runs)
        cover = np.concatenate([np.arange(a, b, dtype=np.uint64) for a, b in r])
        np.testing.assert_array_equal(cover, np.unique(ids))


def test_search_within_on_an_empty_store_touches_no_device(tmp_path):
    from memex_amd.storage import HipFlatStore
    st = HipFlatStore(storage_path=str(tmp_path / "c"))          # nothing inserted: no index, no device
    assert st.search_within([0.0, 1.0], 5, ["a", "b"]) == []
    assert st.search_within([0.0, 1.0], 5, "a") == []
    assert st._index is None
