"""Search by examples at the C ABI and in the host mirrors, without a GPU: the two entry points are exported and declared on every
layer, bad arguments are refused before any index or device is looked at (invalid ones before unsupported ones), and an empty store
answers without opening one."""
import ctypes
import inspect
import math
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mx_index_search_like", "mx_index_search_like_device")


def test_like_entry_points_are_exported_and_declared(lib_built):
    from memex_amd import _lib
    hdr = " ".join(open(os.path.join(ROOT, "include", "memex_hip.h")).read().replace("\n *", " ").split())   # comments as running text
    for name, d in zip(NAMES, ("", "d_")):
        assert hasattr(lib_built, name)
        assert name in _lib.EXPORTS
        assert (f"int {name}(mx_index *idx, const float *{d}queries, const float *query_weights, const uint64_t *example_ids, "
                f"const float *example_weights, int R, int m, int k, int exclude_examples, uint64_t *{d}ids, float *{d}scores, "
                f"float *{d}dists, int32_t *{d}n_found, int32_t *{d}n_used, float *{d}combined);") in hdr
        assert len(getattr(lib_built, name).argtypes) == 15
    assert "ASCENDING i" in hdr and "round to nearest even" in hdr           # the header states the arithmetic of the blend
    assert "k + E > 256" in hdr and "EXACT path" in hdr                      # ... the path a wide list takes
    assert "below f32's normal range are unspecified" in hdr
    assert "HOST memory on both variants" in hdr and "NOT combined" in hdr


def _call(lib, name, idx, R=1, m=2, k=10, e=1, w=None, qw=None, q=False, null=None):
    n = max(R, 1)
    ex = (ctypes.c_uint64 * (n * max(m, 1)))(*([1] * (n * max(m, 1))))
    wa = (ctypes.c_float * len(w))(*w) if w is not None else None
    qa = (ctypes.c_float * (4 * n))() if q else None
    qwa = (ctypes.c_float * len(qw))(*qw) if qw is not None else None
    ids = (ctypes.c_uint64 * (n * max(k, 1)))()
    sc = (ctypes.c_float * (n * max(k, 1)))()
    nf = (ctypes.c_int32 * n)()
    args = {"ex": ex, "ids": ids, "scores": sc, "nf": nf}
    if null:
        args[null] = None
    return getattr(lib, name)(idx, qa, qwa, args["ex"], wa, R, m, k, e, args["ids"], args["scores"], None, args["nf"], None, None)


def test_like_argument_validation_without_device(lib_built):
    from memex_amd import _lib
    L = lib_built
    for name in NAMES:
        # valid arguments, null index: the code mx_index_search gives
        for kw in (dict(), dict(m=1, k=1), dict(m=16, k=4080), dict(m=16, k=4096, e=0), dict(e=0), dict(w=[0.0, -2.5]),
                   dict(w=[1e-6, -1e6]), dict(R=2, m=3, w=[1, 0, 0, 0, 0, 0]), dict(q=True), dict(q=True, qw=[0.5]),
                   dict(q=True, qw=[0.0]), dict(R=0), dict(R=0, null="ids"), dict(R=0, null="ex")):
            assert _call(L, name, None, **kw) == _lib.MX_ESEARCH, kw
        # the arguments are checked first
        bad = [dict(R=-1), dict(m=0), dict(m=-3), dict(k=0), dict(k=-2), dict(e=2), dict(e=-1), dict(w=[1.0, math.nan]),
               dict(w=[math.inf, 1.0]), dict(w=[1.0, -math.inf]), dict(w=[1.0, 1e-7]), dict(w=[-2e6, 1.0]), dict(w=[1.0, -1e-30]),
               dict(R=2, m=2, w=[1.0, 1.0, 1.0, 1e7]), dict(q=True, qw=[math.nan]), dict(q=True, qw=[1e7]), dict(q=True, qw=[-1e-9]),
               dict(qw=[1.0]), dict(null="ex"), dict(null="ids"), dict(null="scores"), dict(null="nf")]
        for kw in bad:
            assert _call(L, name, None, **kw) == _lib.MX_EINVAL, kw
        assert _call(L, name, None, e=2) == _lib.MX_EINVAL and b"exclude_examples" in L.mx_last_error()
        assert _call(L, name, None, R=2, m=2, w=[1.0, 1.0, 1.0, 1e7]) == _lib.MX_EINVAL and b"example_weights[3]" in L.mx_last_error()
        assert _call(L, name, None, R=2, q=True, qw=[1.0, math.nan]) == _lib.MX_EINVAL and b"query_weights[1]" in L.mx_last_error()
        assert _call(L, name, None, qw=[1.0]) == _lib.MX_EINVAL and b"query_weights without queries" in L.mx_last_error()
        for kw in (dict(m=17), dict(m=16, k=4081), dict(m=1, k=4096), dict(k=4097, e=0), dict(m=17, k=5000), dict(k=2 ** 31 - 1)):
            assert _call(L, name, None, **kw) == _lib.MX_EUNSUPPORTED, kw
        # an invalid argument before an unsupported one
        assert _call(L, name, None, m=17, e=2) == _lib.MX_EINVAL
        assert _call(L, name, None, m=17, w=[1.0] * 16 + [math.nan]) == _lib.MX_EINVAL
        assert _call(L, name, None, k=5000, null="nf") == _lib.MX_EINVAL


def test_host_mirrors_have_search_like():
    from memex_amd import tasks
    from memex_amd.index import FlatIndex
    from memex_amd.storage import HipFlatStore, VectorStorage
    sig = inspect.signature(FlatIndex.search_like)
    assert list(sig.parameters)[1:] == ["example_ids", "k", "weights", "queries", "query_weights", "exclude_examples"]
    assert sig.parameters["exclude_examples"].default is True and sig.parameters["weights"].default is None
    assert callable(FlatIndex.search_like_device)
    for cls in (HipFlatStore, VectorStorage):
        sig = inspect.signature(cls.search_like)
        assert list(sig.parameters)[1:] == ["positive", "negative", "limit", "vec", "alpha", "beta", "gamma"]
        assert [sig.parameters[p].default for p in ("negative", "limit", "vec", "alpha", "beta", "gamma")] == [(), 10, None, 1.0, 0.75, 0.15]
    sig = inspect.signature(tasks.search_docs_feedback)
    assert list(sig.parameters) == ["client", "embedder", "query", "relevant", "irrelevant", "limit"]
    assert sig.parameters["irrelevant"].default == () and sig.parameters["limit"].default == 10
    hpp = open(os.path.join(ROOT, "include", "memex_hip.hpp")).read()
    assert hpp.count("std::vector<VectorSearchResult> search_like(const std::vector<std::string> &positive") == 2   # store and storage
    assert "mx_index_search_like(" in hpp
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fn mx_index_search_like(" in integ and "fn mx_index_search_like_device(" in integ and "pub fn search_like(" in integ


def test_search_like_on_an_empty_store_touches_no_device(tmp_path):
    from memex_amd.storage import HipFlatStore, VectorStorage
    st = HipFlatStore(storage_path=str(tmp_path / "c"))          # nothing inserted: no index, no device
    assert st.search_like(["s1", "s2"], ["s3"], 5) == []
    assert st.search_like(["s1"], limit=0) == []
    assert st.search_like([], [], 5, vec=[0.0, 1.0]) == []
    assert VectorStorage(st).search_like(["s1"], ["s2"], 3, [1.0, 0.0], 1.0, 0.5, 0.25) == []
    assert st._index is None


def test_search_docs_feedback_embeds_the_query_and_passes_the_marks():
    from memex_amd import tasks

    class Hit:
        def __init__(self, v):
            self.vector = v

    class Embedder:
        def encode_single(self, text):
            return Hit([float(len(text)), 1.0]) if text else None

    class Client:
        def search_like(self, positive, negative, limit, vec):
            self.seen = (positive, negative, limit, vec)
            return [("a", 0.5)]

    c = Client()
    assert tasks.search_docs_feedback(c, Embedder(), "abc", ["s1", "s2"], ("s9",), limit=3) == [("a", 0.5)]
    assert c.seen == (["s1", "s2"], ["s9"], 3, [3.0, 1.0])
    assert tasks.search_docs_feedback(c, Embedder(), None, ["s1"]) == [("a", 0.5)]      # no query: the marks alone
    assert c.seen == (["s1"], [], 10, None)
    with pytest.raises(ValueError, match="Invalid query"):
        tasks.search_docs_feedback(c, Embedder(), "", ["s1"])
