"""Boosted search at the C ABI and in the host mirrors, without a GPU: the entry points are exported and declared on every layer, and bad
arguments are refused before any index or device is looked at, in the documented order.  What needs a handle -- overlapping ranges, an
id with two values, values that are not finite, stale and foreign priors -- cannot be checked here: tests/test_boosted_gpu.py does."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIOR = ("mx_prior_create", "mx_prior_destroy", "mx_prior_set_ranges", "mx_prior_set_ids", "mx_prior_get", "mx_prior_bound")
SEARCH = ("mx_index_search_boosted", "mx_index_search_boosted_device")


def test_boosted_entry_points_are_exported_and_declared(lib_built):
    from memex_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "memex_hip.h")).read()
    for name in PRIOR + SEARCH:
        assert hasattr(lib_built, name)
        assert name in _lib.EXPORTS
        assert f" {name}(" in hdr
    assert "typedef struct mx_prior mx_prior;" in hdr
    for name in SEARCH:
        assert f"int {name}(mx_index *idx, mx_prior *p, mx_filter *f," in hdr
    assert "const float *weights, int B, int k, int fetch" in hdr
    assert "int mx_prior_set_ranges(mx_prior *p, const uint64_t *ranges, const float *values, uint64_t n_ranges);" in hdr
    assert "int mx_prior_bound(mx_prior *p, int refresh, float *hi);" in hdr
    section = hdr[hdr.index("Boosted search:"):hdr.index("typedef struct mx_prior")]
    assert "complete = 1 promises the EXACT top-k of ALL live rows" in section
    assert "(double)score_j + (double)w * (double)prior_j" in section
    assert "sufficient, not necessary" in section and "NOT combined" in section


def _call(lib, name, idx, p=1, B=1, k=10, fetch=10, null=None, weights=None):
    n = max(B, 1)
    q = (ctypes.c_float * (4 * n))()
    ids = (ctypes.c_uint64 * (n * max(k, 1)))()
    sc = (ctypes.c_float * (n * max(k, 1)))()
    nf = (ctypes.c_int32 * n)()
    args = {"q": q, "ids": ids, "scores": sc, "nf": nf}
    if null:
        args[null] = None
    w = (ctypes.c_float * n)(*weights) if weights is not None else None
    # p: any non-null pointer stands for a prior; it is not looked at before the index is
    return getattr(lib, name)(idx, ctypes.c_void_p(p) if p else None, None, args["q"], w, B, k, fetch, args["ids"], args["scores"], None,
                              None, None, args["nf"], None)


def test_boosted_argument_validation_without_device(lib_built):
    from memex_amd import _lib
    L = lib_built
    nan, inf = float("nan"), float("inf")
    for name in SEARCH:
        # valid arguments, null index: the code mx_index_search gives
        for kw in (dict(), dict(k=1, fetch=1), dict(k=10, fetch=4096), dict(k=4096, fetch=4096), dict(B=0), dict(B=0, null="ids"),
                   dict(B=0, null="q"), dict(B=600, k=2, fetch=2), dict(weights=[0.0]), dict(weights=[2.5]),
                   dict(B=3, weights=[0.0, 1.0, 3e38]), dict(weights=[-0.0])):
            assert _call(L, name, None, **kw) == _lib.MX_ESEARCH, kw
        # the arguments are checked first
        bad = [dict(B=-1), dict(k=0), dict(k=-2), dict(k=10, fetch=9), dict(k=300, fetch=290), dict(p=0), dict(B=0, p=0), dict(null="q"),
               dict(null="ids"), dict(null="scores"), dict(null="nf"), dict(weights=[nan]), dict(weights=[inf]), dict(weights=[-inf]),
               dict(weights=[-1.0]), dict(weights=[-1e-30]), dict(B=3, weights=[1.0, 1.0, -0.5]), dict(B=3, weights=[1.0, nan, 1.0])]
        for kw in bad:
            assert _call(L, name, None, **kw) == _lib.MX_EINVAL, kw
        assert _call(L, name, None, k=10, fetch=9) == _lib.MX_EINVAL and b"fetch" in L.mx_last_error()
        assert _call(L, name, None, p=0) == _lib.MX_EINVAL and b"prior" in L.mx_last_error()
        assert _call(L, name, None, B=2, weights=[1.0, -2.0]) == _lib.MX_EINVAL and b"weights[1]" in L.mx_last_error()
        for kw in (dict(fetch=4097), dict(fetch=5000), dict(k=4097, fetch=4097)):
            assert _call(L, name, None, **kw) == _lib.MX_EUNSUPPORTED, kw
        assert _call(L, name, None, fetch=5000) == _lib.MX_EUNSUPPORTED and b"fetch" in L.mx_last_error()
        # an invalid argument before an unsupported one
        assert _call(L, name, None, k=5001, fetch=5000) == _lib.MX_EINVAL
        assert _call(L, name, None, p=0, fetch=5000) == _lib.MX_EINVAL
        assert _call(L, name, None, null="nf", fetch=5000) == _lib.MX_EINVAL
        assert _call(L, name, None, weights=[nan], fetch=5000) == _lib.MX_EINVAL
        assert _call(L, name, None, weights=[-1.0], fetch=5000) == _lib.MX_EINVAL
        # ... and in the order of the list: k before fetch before the prior before the pointers before the weights
        assert _call(L, name, None, B=-1, k=0) == _lib.MX_EINVAL and b"batch" in L.mx_last_error()
        assert _call(L, name, None, k=0, fetch=-1, p=0) == _lib.MX_EINVAL and b"k = 0" in L.mx_last_error()
        assert _call(L, name, None, k=3, fetch=2, p=0) == _lib.MX_EINVAL and b"fetch" in L.mx_last_error()
        assert _call(L, name, None, p=0, null="q", weights=[nan]) == _lib.MX_EINVAL and b"prior" in L.mx_last_error()
        assert _call(L, name, None, null="q", weights=[nan]) == _lib.MX_EINVAL and b"null argument" in L.mx_last_error()


def test_prior_calls_refuse_null_handles(lib_built):
    from memex_amd import _lib
    L = lib_built
    h = ctypes.c_void_p(7)
    assert L.mx_prior_create(None, ctypes.byref(h)) == _lib.MX_EINVAL and h.value is None       # *out is cleared
    assert L.mx_prior_create(None, None) == _lib.MX_EINVAL
    assert L.mx_prior_set_ranges(None, None, None, 0) == _lib.MX_EINVAL and b"prior" in L.mx_last_error()
    assert L.mx_prior_set_ids(None, None, None, 0) == _lib.MX_EINVAL
    assert L.mx_prior_get(None, None, 0, None) == _lib.MX_EINVAL
    assert L.mx_prior_bound(None, 0, None) == _lib.MX_EINVAL
    L.mx_prior_destroy(None)                                             # a no-op


def test_host_mirrors_have_boosted_search():
    import inspect
    from memex_amd import tasks
    from memex_amd.index import FlatIndex, IndexPrior
    from memex_amd.storage import HipFlatStore, StorePrior, VectorStorage
    sig = inspect.signature(FlatIndex.search_boosted)
    assert list(sig.parameters)[1:] == ["prior", "queries", "k", "weight", "fetch", "flt"]
    assert sig.parameters["weight"].default == 1.0 and sig.parameters["fetch"].default is None
    assert list(inspect.signature(FlatIndex.search_boosted_device).parameters)[1:4] == ["prior", "q", "k"]
    assert callable(FlatIndex.make_prior)
    for m in ("set_ranges", "set_ids", "values_of", "bound", "close", "__enter__", "__exit__"):
        assert callable(getattr(IndexPrior, m)), m
    assert list(inspect.signature(IndexPrior.set_ranges).parameters)[1:] == ["ranges", "values"]
    assert list(inspect.signature(IndexPrior.set_ids).parameters)[1:] == ["ids", "values"]
    assert inspect.signature(IndexPrior.bound).parameters["refresh"].default is False
    assert list(inspect.signature(HipFlatStore.make_prior).parameters) == ["self"]
    assert list(inspect.signature(HipFlatStore.search_boosted).parameters)[1:] == ["vec", "limit", "prior", "weight", "fetch", "flt"]
    assert list(inspect.signature(StorePrior.set).parameters)[1:] == ["ids", "values"]
    assert list(inspect.signature(StorePrior.set_document).parameters)[1:] == ["document_ids", "value"]
    assert callable(VectorStorage.search_boosted)
    assert list(inspect.signature(tasks.search_docs_recent).parameters) == ["client", "embedder", "prior", "query", "limit", "now", "half_life",
                                                                            "t0", "weight"]
    assert list(inspect.signature(tasks.stamp_document).parameters) == ["prior", "vectors", "t", "half_life", "t0"]
    hpp = open(os.path.join(ROOT, "include", "memex_hip.hpp")).read()
    assert "mx_index_search_boosted(" in hpp and "mx_prior_create(" in hpp and "mx_prior_destroy(" in hpp and "mx_prior_set_ids(" in hpp
    assert "class Prior {" in hpp and "struct BoostedHit" in hpp and "search_boosted(" in hpp and "make_prior(" in hpp
    assert hpp.count("search_boosted(const std::vector<float> &") == 2, "the store's method and the VectorStorage forward"
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fn mx_index_search_boosted(" in integ and "fn mx_index_search_boosted_device(" in integ
    for name in PRIOR:
        assert f"fn {name}(" in integ, name
    assert "pub fn search_boosted(" in integ


def test_the_mirrors_refuse_bad_weights_without_a_device(lib_built):
    """FlatIndex.search_boosted hands its arguments to the ABI, whose checks come before the (null) handle is looked at"""
    import pytest
    from memex_amd import _lib
    from memex_amd.index import FlatIndex

    class Handle:
        _h = ctypes.c_void_p(1)                                          # never looked at: the arguments fail first

    idx = FlatIndex.__new__(FlatIndex)
    idx._h, idx.dim = None, 4
    try:
        q = np.zeros((2, 4), np.float32)
        for w in (-1.0, float("nan"), float("inf"), [1.0, -0.5], [float("nan"), 0.0]):
            with pytest.raises(_lib.MemexHipError) as e:
                idx.search_boosted(Handle, q, 3, weight=w)
            assert e.value.code == _lib.MX_EINVAL and "weights[" in str(e.value), w
        with pytest.raises(_lib.MemexHipError) as e:
            idx.search_boosted(Handle, q, 3, weight=[1.0, 1.0, 1.0])
        assert e.value.code == _lib.MX_EINVAL and "weights" in str(e.value)
        with pytest.raises(_lib.MemexHipError) as e:
            idx.search_boosted(Handle, q, 3, fetch=2)
        assert e.value.code == _lib.MX_EINVAL
        with pytest.raises(_lib.MemexHipError) as e:
            idx.search_boosted(Handle, q, 3, fetch=5000)
        assert e.value.code == _lib.MX_EUNSUPPORTED
        with pytest.raises(_lib.MemexHipError) as e:
            idx.search_boosted(Handle, q, 3, weight=0.5)                 # valid arguments: the null index is reported
        assert e.value.code == _lib.MX_ESEARCH
        with pytest.raises(_lib.MemexHipError):
            idx.search_boosted(Handle, np.zeros((2, 5), np.float32), 3)
    finally:
        idx._h = None                                                    # (nothing to close)


def test_search_boosted_on_an_empty_store_touches_no_device(tmp_path):
    import pytest
    from memex_amd.storage import HipFlatStore, SearchError, VectorStorage
    st = HipFlatStore(storage_path=str(tmp_path / "c"))                  # nothing inserted: no index, no device
    assert st.search_boosted([0.0, 1.0], 5, None) == ([], True)
    assert st.search_boosted([0.0, 1.0], 0, None, 0.5, fetch=64) == ([], True)
    assert VectorStorage(st).search_boosted([0.0, 1.0], 3, None) == ([], True)
    with pytest.raises(SearchError, match="insert first"):
        st.make_prior()
    assert st._index is None


def test_tasks_recency_statement():
    import pytest
    from memex_amd import tasks
    from memex_amd.storage import VectorData

    class Hit:
        def __init__(self, v):
            self.vector = v

    class Embedder:
        def encode_single(self, text):
            return Hit([float(len(text)), 1.0]) if text else None

    class Client:
        def search_boosted(self, vec, limit, prior, weight):
            self.seen = (vec, limit, prior, weight)
            return [("seg", 0.5, 0.25, 0.625)], True

    class Prior:
        def __init__(self):
            self.calls = []

        def set_document(self, ids, value):
            self.calls.append((list(ids), value))

    c, p = Client(), Prior()
    out = tasks.search_docs_recent(c, Embedder(), p, "abc", limit=3, now=130.0, half_life=10.0, t0=100.0, weight=0.5)
    assert out == ([("seg", 0.5, 0.25, 0.625)], True)
    assert c.seen[:3] == ([3.0, 1.0], 3, p) and c.seen[3] == float(np.float32(0.5 * 2.0 ** -3.0)) == 0.0625
    with pytest.raises(ValueError, match="Invalid query"):
        tasks.search_docs_recent(c, Embedder(), p, "", limit=3, now=0.0, half_life=1.0, t0=0.0, weight=1.0)
    vs = [VectorData(_id=f"s{i}", document_id="d", text="", vector=[0.0]) for i in range(3)]
    tasks.stamp_document(p, vs, 120.0, 10.0, 100.0)
    assert p.calls == [(["s0", "s1", "s2"], 4.0)]
    tasks.stamp_document(p, [], 120.0, 10.0, 100.0)
    assert len(p.calls) == 1
    # the folded weight times the stored value is the decayed boost: weight * 2^-((now - t) / half_life), here 0.5 * 2^-1
    assert c.seen[3] * p.calls[0][1] == 0.25
    # an f32 holds about 127 half-lives either way; past that the stamp is refused, not stored as inf
    tasks.stamp_document(p, vs, 100.0 + 120 * 10.0, 10.0, 100.0)
    assert p.calls[-1][1] == 2.0 ** 120
    with pytest.raises(ValueError, match="move t0"):
        tasks.stamp_document(p, vs, 100.0 + 129 * 10.0, 10.0, 100.0)
    assert tasks.recency_weight(1.0, 100.0 + 120 * 10.0, 10.0, 100.0) == 2.0 ** -120
