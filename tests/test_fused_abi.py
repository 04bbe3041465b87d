"""Fused search at the C ABI and in the host mirrors, without a GPU: the entry points are exported and declared on every layer, and
bad arguments are refused before any index or device is looked at."""
import ctypes
import math
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mx_index_search_fused", "mx_index_search_fused_device")
MAX, RRF = 0, 1


def test_fused_entry_points_are_exported_and_declared(lib_built):
    from memex_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "memex_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib_built, name)
        assert name in _lib.EXPORTS
        assert f"int {name}(mx_index *idx," in hdr
    assert "enum { MX_FUSE_MAX = 0, MX_FUSE_RRF = 1 };" in hdr
    assert (_lib.MX_FUSE_MAX, _lib.MX_FUSE_RRF) == (MAX, RRF)
    assert "int R, int m, const float *weights, int mode, int k, int fetch" in hdr
    assert "EXACT global top-k by min_i dist_i(row) over ALL live rows" in hdr      # the header states what MAX computes
    assert "ASCENDING i" in hdr                                                     # ... the order of the RRF sum
    assert "NOT combined" in hdr                                                    # ... and how concurrent callers are served


def _call(lib, name, idx, R=1, m=2, weights=None, mode=MAX, k=10, fetch=10, c=60.0, null=None):
    n = max(R, 1)
    q = (ctypes.c_float * (4 * n * max(m, 1)))()
    w = (ctypes.c_float * len(weights))(*weights) if weights is not None else None
    ids = (ctypes.c_uint64 * (n * max(k, 1)))()
    sc = (ctypes.c_float * (n * max(k, 1)))()
    nf = (ctypes.c_int32 * n)()
    args = {"q": q, "ids": ids, "scores": sc, "nf": nf}
    if null:
        args[null] = None
    return getattr(lib, name)(idx, args["q"], R, m, w, mode, k, fetch, c, args["ids"], args["scores"], None, None, None, args["nf"])


def test_fused_argument_validation_without_device(lib_built):
    from memex_amd import _lib
    L = lib_built
    for name in NAMES:
        # valid arguments, null index: the code mx_index_search gives
        for kw in (dict(), dict(m=1, k=1, fetch=1), dict(m=16, k=256, fetch=256, mode=RRF), dict(mode=RRF, c=0.0, fetch=64),
                   dict(weights=[0.0, 2.5]), dict(R=2, m=3, weights=[1, 0, 0, 0, 0, 0]), dict(R=0), dict(c=math.nan),  # (MAX ignores rrf_c)
                   dict(R=0, null="ids")):
            assert _call(L, name, None, **kw) == _lib.MX_ESEARCH, kw
        # the arguments are checked first
        bad = [dict(R=-1), dict(m=0), dict(m=-3), dict(k=0), dict(k=-2), dict(k=10, fetch=9), dict(k=300, fetch=290), dict(mode=2),
               dict(mode=-1), dict(weights=[1.0, math.nan]), dict(weights=[math.inf, 1.0]), dict(weights=[1.0, -0.5]),
               dict(R=2, m=2, weights=[1.0, 1.0, 1.0, -1.0]), dict(mode=RRF, c=math.nan), dict(mode=RRF, c=math.inf),
               dict(mode=RRF, c=-1.0), dict(null="q"), dict(null="ids"), dict(null="scores"), dict(null="nf")]
        for kw in bad:
            assert _call(L, name, None, **kw) == _lib.MX_EINVAL, kw
        assert _call(L, name, None, k=10, fetch=9) == _lib.MX_EINVAL and b"fetch" in L.mx_last_error()
        assert _call(L, name, None, weights=[1.0, -0.5]) == _lib.MX_EINVAL and b"weights[1]" in L.mx_last_error()
        assert _call(L, name, None, mode=RRF, c=-1.0) == _lib.MX_EINVAL and b"rrf_c" in L.mx_last_error()
        for kw in (dict(m=17), dict(fetch=257), dict(k=257, fetch=257), dict(m=17, fetch=1000)):
            assert _call(L, name, None, **kw) == _lib.MX_EUNSUPPORTED, kw
        assert _call(L, name, None, m=17, k=10, fetch=9) == _lib.MX_EINVAL           # an invalid argument before an unsupported one


def test_default_fetch_helper():
    from memex_amd.index import FlatIndex
    f = FlatIndex._fused_fetch
    assert f(10, "max", None) == 10 and f(300, "max", None) == 300
    assert f(10, "rrf", None) == 40 and f(2, "rrf", None) == 32 and f(100, "rrf", None) == 256
    assert f(10, "max", 77) == 77 and f(10, "rrf", 77) == 77


def test_host_mirrors_have_fused_search():
    import inspect
    from memex_amd import tasks
    from memex_amd.index import FlatIndex
    from memex_amd.storage import HipFlatStore, VectorStorage
    assert callable(FlatIndex.search_fused) and callable(FlatIndex.search_fused_device)
    assert list(inspect.signature(FlatIndex.search_fused).parameters)[1:] == ["queries", "k", "mode", "fetch", "weights", "rrf_c"]
    assert inspect.signature(FlatIndex.search_fused).parameters["rrf_c"].default == 60.0
    assert list(inspect.signature(HipFlatStore.search_fused).parameters)[1:] == ["vecs", "limit", "mode", "fetch", "weights"]
    assert callable(VectorStorage.search_fused)
    assert list(inspect.signature(tasks.search_docs_multi).parameters) == ["client", "embedder", "queries", "limit", "mode"]
    hpp = open(os.path.join(ROOT, "include", "memex_hip.hpp")).read()
    assert "std::vector<VectorSearchResult> search_fused(const std::vector<std::vector<float>> &vecs, size_t limit" in hpp
    assert "mx_index_search_fused(" in hpp and "search_docs_multi(" in hpp
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fn mx_index_search_fused(" in integ and "fn mx_index_search_fused_device(" in integ and "pub fn search_fused(" in integ


def test_search_fused_on_an_empty_store_touches_no_device(tmp_path):
    from memex_amd.storage import HipFlatStore, VectorStorage
    st = HipFlatStore(storage_path=str(tmp_path / "c"))          # nothing inserted: no index, no device
    assert st.search_fused([[0.0, 1.0], [1.0, 0.0]], 5) == []
    assert st.search_fused([[0.0, 1.0]], 0) == []
    assert st.search_fused([[0.0, 1.0], [1.0, 0.0]], 5, mode="rrf", fetch=64, weights=[1.0, 0.5]) == []
    assert VectorStorage(st).search_fused([[0.0, 1.0]], 3) == []
    assert st._index is None


def test_search_docs_multi_embeds_every_text_and_rejects_an_empty_one():
    import pytest
    from memex_amd import tasks

    class Hit:
        def __init__(self, v):
            self.vector = v

    class Embedder:
        def encode_single(self, text):
            return Hit([float(len(text)), 1.0]) if text else None

    class Client:
        def search_fused(self, vecs, limit, mode):
            self.seen = (vecs, limit, mode)
            return [("a", 0.5)]

    c = Client()
    assert tasks.search_docs_multi(c, Embedder(), ["ab", "abcd"], limit=3, mode="rrf") == [("a", 0.5)]
    assert c.seen == ([[2.0, 1.0], [4.0, 1.0]], 3, "rrf")
    with pytest.raises(ValueError, match="Invalid query"):
        tasks.search_docs_multi(c, Embedder(), ["ab", ""])
    with pytest.raises(ValueError, match="Invalid query"):
        tasks.search_docs_multi(c, Embedder(), [])
