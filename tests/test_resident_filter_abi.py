"""Resident filters (mx_filter) at the C ABI and in the host mirrors, without a GPU: every entry point is exported and declared on
every layer, and the argument checks that come before the device is looked at return the stated codes."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_NAMES = ("mx_filter_create", "mx_filter_set_ranges", "mx_filter_set_ids", "mx_filter_count", "mx_filter_get_ranges",
             "mx_index_search_with_filter", "mx_index_search_with_filter_device")


def test_filter_entry_points_are_exported_and_declared(lib_built):
    from memex_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "memex_hip.h")).read()
    assert "typedef struct mx_filter mx_filter;" in hdr
    for name in INT_NAMES:
        assert hasattr(lib_built, name)
        assert name in _lib.EXPORTS
        assert f"int {name}(" in hdr
    assert hasattr(lib_built, "mx_filter_destroy") and "mx_filter_destroy" in _lib.EXPORTS
    assert "void mx_filter_destroy(mx_filter *f);" in hdr
    # the stats struct did not grow: a resident filter moves the counters a per-call one moves
    assert [f[0] for f in _lib.IndexStats._fields_][-2:] == ["filtered_queries", "subset_queries"]
    assert lib_built.mx_index_stats_size() == ctypes.sizeof(_lib.IndexStats)


def test_null_arguments_are_refused_before_anything_else(lib_built):
    from memex_amd import _lib
    L = lib_built
    out = ctypes.c_void_p(123)
    assert L.mx_filter_create(None, ctypes.byref(out)) == _lib.MX_EINVAL
    assert out.value is None                                              # nothing handed out
    assert L.mx_filter_create(None, None) == _lib.MX_EINVAL
    L.mx_filter_destroy(None)                                             # a no-op
    pairs = (ctypes.c_uint64 * 4)(1, 5, 9, 9)
    n = ctypes.c_uint64(7)
    assert L.mx_filter_set_ranges(None, pairs, 2, 1) == _lib.MX_EINVAL
    assert b"null filter" in L.mx_last_error()
    assert L.mx_filter_set_ids(None, pairs, 4, 0) == _lib.MX_EINVAL
    assert L.mx_filter_count(None, ctypes.byref(n), ctypes.byref(n)) == _lib.MX_EINVAL
    assert L.mx_filter_get_ranges(None, pairs, 2, ctypes.byref(n)) == _lib.MX_EINVAL
    assert n.value == 7


def _search(lib, name, idx, flt, B=1, k=10):
    q = (ctypes.c_float * 4)()
    ids = (ctypes.c_uint64 * k)()
    sc = (ctypes.c_float * k)()
    nf = (ctypes.c_int32 * B)()
    return getattr(lib, name)(idx, flt, q, B, k, ids, sc, None, nf)


def test_search_argument_validation_without_device(lib_built):
    from memex_amd import _lib
    # a filter handle that is never looked at: the index is checked first once the filter is not null
    fake = ctypes.cast((ctypes.c_uint64 * 64)(), ctypes.c_void_p)
    for name in ("mx_index_search_with_filter", "mx_index_search_with_filter_device"):
        assert _search(lib_built, name, None, None) == _lib.MX_EINVAL       # a null filter, before anything else
        assert b"null filter" in lib_built.mx_last_error()
        assert _search(lib_built, name, None, fake) == _lib.MX_ESEARCH      # a null index: the code mx_index_search gives
    assert lib_built.mx_index_search(None, (ctypes.c_float * 4)(), 1, 10, None, None, None, None) == _lib.MX_ESEARCH


def test_host_mirrors_have_resident_filters():
    from memex_amd.index import FlatIndex, IndexFilter
    from memex_amd.storage import HipFlatStore, StoreFilter
    assert callable(FlatIndex.make_filter) and callable(FlatIndex.search_with) and callable(FlatIndex.search_with_device)
    for m in ("allow", "deny", "count", "ranges", "close", "__enter__", "__exit__"):
        assert callable(getattr(IndexFilter, m))
    assert callable(HipFlatStore.make_filter) and callable(HipFlatStore.search_in)
    assert callable(StoreFilter.allow) and callable(StoreFilter.deny)
    hpp = open(os.path.join(ROOT, "include", "memex_hip.hpp")).read()
    assert "class Filter" in hpp and "mx_index_search_with_filter(" in hpp and "mx_filter_destroy(" in hpp
    assert "mx_index_search_with_filter(" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_make_filter_on_an_empty_store_touches_no_device(tmp_path):
    import pytest
    from memex_amd.storage import HipFlatStore, VectorStoreError
    st = HipFlatStore(storage_path=str(tmp_path / "c"))                   # nothing inserted: no index, no device
    with pytest.raises(VectorStoreError):
        st.make_filter(["a"])
    assert st._index is None
