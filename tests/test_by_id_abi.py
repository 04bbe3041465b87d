"""Search by stored row at the C ABI and in the host mirrors, without a GPU: the four entry points are exported and declared on every
layer, bad arguments are refused before any index or device is looked at, and an empty store answers without opening one."""
import ctypes
import math
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPK = ("mx_index_search_by_id", "mx_index_search_by_id_device")
RANGE = ("mx_index_search_range_by_id", "mx_index_search_range_by_id_device")


def test_by_id_entry_points_are_exported_and_declared(lib_built):
    from memex_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "memex_hip.h")).read()
    for name in TOPK + RANGE:
        assert hasattr(lib_built, name)
        assert name in _lib.EXPORTS
        assert f"int {name}(mx_index *idx, const uint64_t *query_ids, int B," in hdr
    assert "int B, int k, int exclude_self, uint64_t *ids, float *scores" in hdr
    assert "int B, const float *min_scores, int cap, int exclude_self" in hdr
    assert "k + 1 or more exact copies with smaller ids" in hdr       # the header says what happens to the own row among ties
    assert "NOT combined" in hdr                                       # ... and how concurrent callers are served


def _topk(lib, name, idx, k, e, B=1):
    n = max(k, 1) * max(B, 1)
    q = (ctypes.c_uint64 * max(B, 1))(*([1] * max(B, 1)))
    ids = (ctypes.c_uint64 * n)()
    sc = (ctypes.c_float * n)()
    nf = (ctypes.c_int32 * max(B, 1))()
    return getattr(lib, name)(idx, q, B, k, e, ids, sc, None, nf)


def _range(lib, name, idx, thr, cap, e, B=1):
    n = max(cap, 1) * max(B, 1)
    q = (ctypes.c_uint64 * max(B, 1))(*([1] * max(B, 1)))
    t = (ctypes.c_float * max(B, 1))(*([thr] * max(B, 1)))
    ids = (ctypes.c_uint64 * n)()
    sc = (ctypes.c_float * n)()
    nf = (ctypes.c_int32 * max(B, 1))()
    nr = (ctypes.c_uint64 * max(B, 1))()
    return getattr(lib, name)(idx, q, B, t, cap, e, ids, sc, None, nf, nr)


def test_top_k_argument_validation_without_device(lib_built):
    from memex_amd import _lib
    for name in TOPK:
        # valid arguments, null index: the code mx_index_search gives
        for k, e in ((10, 1), (10, 0), (1, 1), (4095, 1), (4096, 0)):
            assert _topk(lib_built, name, None, k, e) == _lib.MX_ESEARCH
        assert _topk(lib_built, name, None, 10, 1, B=0) == _lib.MX_ESEARCH
        # the arguments are checked first
        assert _topk(lib_built, name, None, 10, 1, B=-1) == _lib.MX_EINVAL
        assert _topk(lib_built, name, None, 0, 1) == _lib.MX_EINVAL
        assert _topk(lib_built, name, None, -3, 0) == _lib.MX_EINVAL
        assert _topk(lib_built, name, None, 10, 2) == _lib.MX_EINVAL
        assert b"exclude_self" in lib_built.mx_last_error()
        assert _topk(lib_built, name, None, 10, -1) == _lib.MX_EINVAL
        assert _topk(lib_built, name, None, 4096, 1) == _lib.MX_EUNSUPPORTED        # k + 1 is what mx_index_search would be asked
        assert _topk(lib_built, name, None, 4097, 0) == _lib.MX_EUNSUPPORTED


def test_range_argument_validation_without_device(lib_built):
    from memex_amd import _lib
    for name in RANGE:
        for thr, cap, e in ((0.5, 10, 1), (-2.0, 1, 0), (2.0, 4095, 1), (0.9, 4096, 0), (math.inf, 8, 1)):
            assert _range(lib_built, name, None, thr, cap, e) == _lib.MX_ESEARCH
        assert _range(lib_built, name, None, 0.5, 10, 1, B=0) == _lib.MX_ESEARCH
        assert _range(lib_built, name, None, 0.5, 10, 1, B=-1) == _lib.MX_EINVAL
        assert _range(lib_built, name, None, 0.5, 0, 1) == _lib.MX_EINVAL
        assert _range(lib_built, name, None, 0.5, -1, 0) == _lib.MX_EINVAL
        assert _range(lib_built, name, None, 0.5, 10, 2) == _lib.MX_EINVAL
        assert b"exclude_self" in lib_built.mx_last_error()
        assert _range(lib_built, name, None, math.nan, 10, 1) == _lib.MX_EINVAL
        assert b"NaN" in lib_built.mx_last_error()
        assert _range(lib_built, name, None, 0.5, 4096, 1) == _lib.MX_EUNSUPPORTED   # cap + 1 > 4096
        assert _range(lib_built, name, None, 0.5, 4097, 0) == _lib.MX_EUNSUPPORTED
        # null thresholds with a batch
        fn = getattr(lib_built, name)
        q = (ctypes.c_uint64 * 1)(1)
        ids, sc, nf, nr = (ctypes.c_uint64 * 4)(), (ctypes.c_float * 4)(), (ctypes.c_int32 * 1)(), (ctypes.c_uint64 * 1)()
        assert fn(None, q, 1, None, 4, 1, ids, sc, None, nf, nr) == _lib.MX_EINVAL


def test_host_mirrors_have_search_by_stored_row():
    from memex_amd.index import FlatIndex
    from memex_amd.storage import HipFlatStore
    for m in ("search_by_id", "search_by_id_device", "search_range_by_id", "search_range_by_id_device", "near_duplicates"):
        assert callable(getattr(FlatIndex, m)), m
    assert callable(HipFlatStore.more_like) and callable(HipFlatStore.find_duplicates)
    assert "lost only when BOTH" in FlatIndex.near_duplicates.__doc__   # the guarantee is documented where the caller reads it
    hpp = open(os.path.join(ROOT, "include", "memex_hip.hpp")).read()
    assert "std::vector<VectorSearchResult> more_like(const std::string &_id, size_t limit)" in hpp
    assert "std::vector<DuplicatePair> find_duplicates(float min_score, size_t per_row = 64" in hpp
    assert "mx_index_search_by_id(" in hpp and "mx_index_search_range_by_id(" in hpp
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fn mx_index_search_by_id(" in integ and "fn mx_index_search_range_by_id(" in integ
    assert "pub fn more_like(" in integ and "pub fn find_duplicates(" in integ


def test_more_like_and_find_duplicates_on_an_empty_store_touch_no_device(tmp_path):
    from memex_amd.storage import HipFlatStore
    st = HipFlatStore(storage_path=str(tmp_path / "c"))          # nothing inserted: no index, no device
    assert st.more_like("s1", 5) == []
    assert st.more_like("s1", 0) == []
    assert st.find_duplicates(0.98) == ([], [])
    assert st.find_duplicates(0.5, per_row=4) == ([], [])
    assert st._index is None
