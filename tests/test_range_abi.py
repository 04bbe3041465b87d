"""Range search at the C ABI and in the host mirrors, without a GPU: the entry points are exported and declared on every layer,
and bad arguments are refused before any index or device is looked at."""
import ctypes
import math
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mx_index_search_range", "mx_index_search_range_device")


def test_range_entry_points_are_exported_and_declared(lib_built):
    from memex_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "memex_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib_built, name)
        assert name in _lib.EXPORTS
        assert f"int {name}(mx_index *idx," in hdr
    assert "const float *min_scores, int cap" in hdr
    assert "uint64_t *n_in_range);" in hdr and "uint64_t *d_n_in_range);" in hdr


def _call(lib, name, idx, thresholds, cap, B=1):
    q = (ctypes.c_float * (4 * B))()
    t = (ctypes.c_float * B)(*thresholds) if thresholds is not None else None
    n = max(cap, 1) * B
    ids = (ctypes.c_uint64 * n)()
    sc = (ctypes.c_float * n)()
    nf = (ctypes.c_int32 * B)()
    nr = (ctypes.c_uint64 * B)()
    return getattr(lib, name)(idx, q, B, t, cap, ids, sc, None, nf, nr)


def test_range_argument_validation_without_device(lib_built):
    from memex_amd import _lib
    for name in NAMES:
        # valid arguments, null index: the code mx_index_search gives
        assert _call(lib_built, name, None, [0.5], 10) == _lib.MX_ESEARCH
        assert _call(lib_built, name, None, [-5.0, 2.0], 4096, B=2) == _lib.MX_ESEARCH   # any non-NaN threshold is valid
        # the arguments are checked first
        assert _call(lib_built, name, None, [math.nan], 10) == _lib.MX_EINVAL
        assert b"NaN" in lib_built.mx_last_error()
        assert _call(lib_built, name, None, [0.5, math.nan], 10, B=2) == _lib.MX_EINVAL
        assert _call(lib_built, name, None, [0.5], 0) == _lib.MX_EINVAL
        assert _call(lib_built, name, None, [0.5], -3) == _lib.MX_EINVAL
        assert _call(lib_built, name, None, [0.5], 4097) == _lib.MX_EUNSUPPORTED
        assert _call(lib_built, name, None, None, 10) == _lib.MX_EINVAL                 # null min_scores with B > 0
        assert _call(lib_built, name, None, None, 10, B=0) == _lib.MX_ESEARCH           # B = 0 needs no thresholds


def test_host_mirrors_have_range_search():
    from memex_amd.index import FlatIndex
    from memex_amd.storage import HipFlatStore
    assert callable(FlatIndex.search_range) and callable(FlatIndex.search_range_device)
    assert callable(HipFlatStore.search_above)
    hpp = open(os.path.join(ROOT, "include", "memex_hip.hpp")).read()
    assert "std::vector<VectorSearchResult> search_above(const std::vector<float> &vec, float min_score, size_t limit)" in hpp
    assert "mx_index_search_range(" in hpp
    assert "mx_index_search_range(" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_search_above_on_an_empty_store_touches_no_device(tmp_path):
    from memex_amd.storage import HipFlatStore
    st = HipFlatStore(storage_path=str(tmp_path / "c"))          # nothing inserted: no index, no device
    assert st.search_above([0.0, 1.0], 0.5, 5) == []
    assert st.search_above([0.0, 1.0], 0.5, 0) == []
    assert st._index is None
