"""Scoring of named rows at the C ABI and in the host mirrors, without a GPU: the two entry points are exported and declared on every
layer, bad arguments are refused before any index or device is looked at (invalid ones before unsupported ones), and an empty store
answers without opening one."""
import ctypes
import inspect
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mx_index_score_ids", "mx_index_score_ids_device")


def test_score_ids_entry_points_are_exported_and_declared(lib_built):
    from memex_amd import _lib
    hdr = " ".join(open(os.path.join(ROOT, "include", "memex_hip.h")).read().replace("\n *", " ").split())   # comments as running text
    for name, d in zip(NAMES, ("", "d_")):
        assert hasattr(lib_built, name)
        assert name in _lib.EXPORTS
        assert (f"int {name}(mx_index *idx, const float *{d}queries, int B, const uint64_t *cand_ids, int m, float *{d}scores, "
                f"float *{d}dists, int32_t *{d}order, int32_t *{d}n_found);") in hdr
        assert len(getattr(lib_built, name).argtypes) == 9
    assert "(dist ascending, id ascending, position j ascending)" in hdr     # the header states the order of the ranking
    assert "holds score 0 and dist +inf" in hdr                              # ... and the blank pattern
    assert "slots from n_found[b] on hold -1" in hdr
    assert "HOST memory on both variants" in hdr and "NOT combined" in hdr
    assert "An id named twice in a list is scored twice" in hdr


def _call(lib, name, idx, B=1, m=4, null=None, outs=True):
    n, w = max(B, 1), max(m, 1)
    args = {"q": (ctypes.c_float * (4 * n))(), "cand": (ctypes.c_uint64 * (n * w))(*([1] * (n * w))), "scores": (ctypes.c_float * (n * w))()}
    if null:
        for nm in null.split(","):
            args[nm] = None
    di = (ctypes.c_float * (n * w))() if outs else None
    od = (ctypes.c_int32 * (n * w))() if outs else None
    nf = (ctypes.c_int32 * n)() if outs else None
    return getattr(lib, name)(idx, args["q"], B, args["cand"], m, args["scores"], di, od, nf)


def test_score_ids_argument_validation_without_device(lib_built):
    from memex_amd import _lib
    L = lib_built
    for name in NAMES:
        # valid arguments, null index: the code mx_index_search gives
        for kw in (dict(), dict(m=1), dict(m=4096), dict(B=513, m=8), dict(outs=False), dict(B=0), dict(B=0, null="q,cand,scores"),
                   dict(B=0, m=4096, null="scores")):
            assert _call(L, name, None, **kw) == _lib.MX_ESEARCH, kw
        # the arguments are checked first
        for kw in (dict(B=-1), dict(m=0), dict(m=-3), dict(null="q"), dict(null="cand"), dict(null="scores"), dict(B=0, m=0)):
            assert _call(L, name, None, **kw) == _lib.MX_EINVAL, kw
        assert _call(L, name, None, m=0) == _lib.MX_EINVAL and b"m = 0" in L.mx_last_error()
        for kw in (dict(m=4097), dict(m=70000, B=0), dict(B=0, m=5000, null="q,cand,scores")):
            assert _call(L, name, None, **kw) == _lib.MX_EUNSUPPORTED, kw
        # an invalid argument before an unsupported one
        assert _call(L, name, None, m=4097, null="scores") == _lib.MX_EINVAL
        assert _call(L, name, None, B=-1, m=4097) == _lib.MX_EINVAL


def test_host_mirrors_have_score_ids_and_rerank():
    from memex_amd import tasks
    from memex_amd.index import FlatIndex
    from memex_amd.storage import HipFlatStore, VectorStorage
    assert list(inspect.signature(FlatIndex.score_ids).parameters)[1:] == ["queries", "ids"]
    sig = inspect.signature(FlatIndex.score_ids_device)
    assert list(sig.parameters)[1:] == ["q", "ids", "scores", "dists", "order", "n_found"]
    assert [sig.parameters[p].default for p in ("dists", "order", "n_found")] == [None, None, None]
    for cls in (HipFlatStore, VectorStorage):
        sig = inspect.signature(cls.rerank)
        assert list(sig.parameters)[1:] == ["vec", "ids", "limit"] and sig.parameters["limit"].default is None
    sig = inspect.signature(tasks.rerank_docs)
    assert list(sig.parameters) == ["client", "embedder", "query", "candidates", "limit"] and sig.parameters["limit"].default == 10
    assert "rerank_docs" in tasks.__doc__
    hpp = open(os.path.join(ROOT, "include", "memex_hip.hpp")).read()
    assert hpp.count("std::vector<VectorSearchResult> rerank(const std::vector<float> &vec, const std::vector<std::string> &ids") == 2
    assert "mx_index_score_ids(" in hpp
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fn mx_index_score_ids(" in integ and "fn mx_index_score_ids_device(" in integ and "pub fn rerank(" in integ


def test_candidate_lists_are_padded_with_zero():
    import numpy as np
    from memex_amd.index import FlatIndex
    a = FlatIndex._cand_ids([[5, 6, 7], [], [9]], 3)
    assert a.dtype == np.uint64 and a.tolist() == [[5, 6, 7], [0, 0, 0], [9, 0, 0]]
    assert FlatIndex._cand_ids([3, 4], 1).tolist() == [[3, 4]]
    assert FlatIndex._cand_ids(np.arange(6).reshape(2, 3), 2).shape == (2, 3)
    assert FlatIndex._cand_ids([], 0).shape == (0, 1)


def test_rerank_on_an_empty_store_touches_no_device(tmp_path):
    from memex_amd.storage import HipFlatStore, VectorStorage
    st = HipFlatStore(storage_path=str(tmp_path / "c"))          # nothing inserted: no index, no device
    assert st.rerank([0.0, 1.0], ["s1", "s2"]) == []
    assert st.rerank([0.0, 1.0], ["s1"], 5) == [] and st.rerank([0.0, 1.0], [], 0) == []
    assert VectorStorage(st).rerank([1.0, 0.0], ["s1", "s2"], 3) == []
    assert st._index is None


def test_rerank_docs_embeds_the_query_and_passes_the_candidates():
    from memex_amd import tasks

    class Hit:
        def __init__(self, v):
            self.vector = v

    class Embedder:
        def encode_single(self, text):
            return Hit([float(len(text)), 1.0]) if text else None

    class Client:
        def rerank(self, vec, ids, limit):
            self.seen = (vec, ids, limit)
            return [("a", 0.5)]

    c = Client()
    assert tasks.rerank_docs(c, Embedder(), "abc", ("s1", "s2"), limit=3) == [("a", 0.5)]
    assert c.seen == ([3.0, 1.0], ["s1", "s2"], 3)
    assert tasks.rerank_docs(c, Embedder(), "abcd", ["s9"]) == [("a", 0.5)] and c.seen == ([4.0, 1.0], ["s9"], 10)
    with pytest.raises(ValueError, match="Invalid query"):
        tasks.rerank_docs(c, Embedder(), "", ["s1"])
