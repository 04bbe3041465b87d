"""Diversified search at the C ABI and in the host mirrors, without a GPU: the entry points are exported and declared on every
layer, and bad arguments are refused before any index or device is looked at."""
import ctypes
import math
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mx_index_search_mmr", "mx_index_search_mmr_device")


def test_mmr_entry_points_are_exported_and_declared(lib_built):
    from memex_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "memex_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib_built, name)
        assert name in _lib.EXPORTS
        assert f"int {name}(mx_index *idx," in hdr
    assert "int B, int k, int fetch, float lambda, uint64_t *ids, float *scores" in hdr
    assert "int B, int k, int fetch, float lambda, uint64_t *d_ids" in hdr
    assert "O(k * fetch * dim)" in hdr                                  # the header says what the selection costs
    assert "NOT combined" in hdr                                        # ... and how concurrent callers are served


def _call(lib, name, idx, k, fetch, lam, B=1):
    q = (ctypes.c_float * (4 * max(B, 1)))()
    n = max(k, 1) * max(B, 1)
    ids = (ctypes.c_uint64 * n)()
    sc = (ctypes.c_float * n)()
    nf = (ctypes.c_int32 * max(B, 1))()
    return getattr(lib, name)(idx, q, B, k, fetch, lam, ids, sc, None, nf)


def test_mmr_argument_validation_without_device(lib_built):
    from memex_amd import _lib
    for name in NAMES:
        # valid arguments, null index: the code mx_index_search gives
        for k, fetch, lam in ((10, 64, 0.5), (1, 1, 0.0), (1024, 1024, 1.0), (10, 10, 0.3)):
            assert _call(lib_built, name, None, k, fetch, lam) == _lib.MX_ESEARCH
        assert _call(lib_built, name, None, 10, 64, 0.5, B=0) == _lib.MX_ESEARCH
        # the arguments are checked first
        assert _call(lib_built, name, None, 10, 64, 0.5, B=-1) == _lib.MX_EINVAL
        assert _call(lib_built, name, None, 0, 64, 0.5) == _lib.MX_EINVAL
        assert _call(lib_built, name, None, -2, 64, 0.5) == _lib.MX_EINVAL
        assert _call(lib_built, name, None, 10, 9, 0.5) == _lib.MX_EINVAL           # fetch < k
        assert b"fetch" in lib_built.mx_last_error()
        assert _call(lib_built, name, None, 2000, 1500, 0.5) == _lib.MX_EINVAL      # fetch < k, whatever their size
        assert _call(lib_built, name, None, 10, 64, math.nan) == _lib.MX_EINVAL
        assert b"lambda" in lib_built.mx_last_error()
        assert _call(lib_built, name, None, 10, 64, -0.01) == _lib.MX_EINVAL
        assert _call(lib_built, name, None, 10, 64, 1.01) == _lib.MX_EINVAL
        assert _call(lib_built, name, None, 10, 64, math.inf) == _lib.MX_EINVAL
        assert _call(lib_built, name, None, 10, 1025, 0.5) == _lib.MX_EUNSUPPORTED
        assert _call(lib_built, name, None, 1025, 1025, 0.5) == _lib.MX_EUNSUPPORTED


def test_host_mirrors_have_diversified_search():
    from memex_amd.index import FlatIndex
    from memex_amd.storage import HipFlatStore
    assert callable(FlatIndex.search_mmr) and callable(FlatIndex.search_mmr_device)
    assert callable(HipFlatStore.search_diverse)
    assert FlatIndex._mmr_fetch(10, None) == 40 and FlatIndex._mmr_fetch(2, None) == 32 and FlatIndex._mmr_fetch(400, None) == 1024
    assert FlatIndex._mmr_fetch(10, 77) == 77
    hpp = open(os.path.join(ROOT, "include", "memex_hip.hpp")).read()
    assert "std::vector<VectorSearchResult> search_diverse(const std::vector<float> &vec, size_t limit, size_t fetch = 0, float lambda = 0.5f)" in hpp
    assert "mx_index_search_mmr(" in hpp
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fn mx_index_search_mmr(" in integ and "pub fn search_diverse(" in integ


def test_search_diverse_on_an_empty_store_touches_no_device(tmp_path):
    from memex_amd.storage import HipFlatStore
    st = HipFlatStore(storage_path=str(tmp_path / "c"))          # nothing inserted: no index, no device
    assert st.search_diverse([0.0, 1.0], 5) == []
    assert st.search_diverse([0.0, 1.0], 0) == []
    assert st.search_diverse([0.0, 1.0], 5, fetch=64, lam=0.2) == []
    assert st._index is None
