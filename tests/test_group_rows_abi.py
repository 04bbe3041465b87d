"""Grouped search with members at the C ABI and in the host mirrors, without a GPU: the entry points are exported and declared on every
layer, and bad arguments are refused, in the documented order, before any index or device is looked at.  What needs a handle -- stale
and foreign groupings -- cannot be checked here: tests/test_group_rows_gpu.py does."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = ("mx_index_search_group_rows", "mx_index_search_group_rows_device")
CAPPED = ("mx_index_search_capped", "mx_index_search_capped_device")
COUNTS = ("mx_grouping_key_counts",)


def test_entry_points_are_exported_and_declared(lib_built):
    from memex_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "memex_hip.h")).read()
    for name in ROWS + CAPPED + COUNTS:
        assert hasattr(lib_built, name), name
        assert name in _lib.EXPORTS
        assert f"int {name}(" in hdr
    for name in ROWS:
        assert f"int {name}(mx_index *idx, mx_grouping *g, mx_filter *f," in hdr
    assert "int B, int k, int n, int fetch" in hdr and "int B, int k, int per_key, int fetch" in hdr
    assert "int mx_grouping_key_counts(mx_grouping *g, const uint32_t *keys, uint64_t n_keys, uint64_t *n_rows, uint64_t *n_live);" in hdr
    section = hdr[hdr.index("Grouped search with members:"):hdr.index("int mx_index_search_group_rows(")]
    assert "members_complete   [j] = 1 iff n_members[j] == n, or L holds fewer than fetch entries, or the key is 0" in section
    assert "ALWAYS its exact best n_members live" in section
    assert "complete[b] = 1 iff n_found[b] == k or L holds fewer than fetch" in section
    assert "NOT combined" in section and "n > 16 or k * n > 4096: MX_EUNSUPPORTED" in section


def _call(lib, name, idx, g=1, B=1, k=10, per=2, fetch=40, null=None):
    nq = max(B, 1)
    width = nq * max(k, 1) * max(min(per, 16), 1)
    args = {"q": (ctypes.c_float * (4 * nq))(), "ids": (ctypes.c_uint64 * width)(), "scores": (ctypes.c_float * width)(),
            "nf": (ctypes.c_int32 * nq)()}
    if null:
        args[null] = None
    # g: any non-null pointer stands for a grouping; it is not looked at before the index is
    head = (idx, ctypes.c_void_p(g) if g else None, None, args["q"], B, k, per, fetch, args["ids"], args["scores"], None, None)
    if name in ROWS:
        return getattr(lib, name)(*head, None, None, None, args["nf"], None)
    return getattr(lib, name)(*head, args["nf"], None)


def test_argument_validation_without_device(lib_built):
    from memex_amd import _lib
    L = lib_built
    for name in ROWS + CAPPED:
        rows = name in ROWS
        # valid arguments, null index: the code mx_index_search gives
        for kw in (dict(), dict(k=1, per=1, fetch=1), dict(k=10, fetch=4096), dict(k=4096, per=1, fetch=4096), dict(B=0),
                   dict(B=0, null="ids"), dict(B=0, null="q"), dict(B=600, k=2, fetch=2), dict(k=256, per=16, fetch=4096)):
            assert _call(L, name, None, **kw) == _lib.MX_ESEARCH, (name, kw)
        # the arguments are checked first
        bad = [dict(B=-1), dict(k=0), dict(k=-2), dict(per=0), dict(per=-3), dict(k=10, fetch=9), dict(k=300, fetch=290), dict(g=0),
               dict(B=0, g=0), dict(null="q"), dict(null="ids"), dict(null="scores"), dict(null="nf")]
        for kw in bad:
            assert _call(L, name, None, **kw) == _lib.MX_EINVAL, (name, kw)
        assert _call(L, name, None, per=0) == _lib.MX_EINVAL and (b"n = 0" if rows else b"per_key = 0") in L.mx_last_error()
        assert _call(L, name, None, k=10, fetch=9) == _lib.MX_EINVAL and b"fetch" in L.mx_last_error()
        assert _call(L, name, None, g=0) == _lib.MX_EINVAL and b"grouping" in L.mx_last_error()
        for kw in (dict(fetch=4097), dict(fetch=5000), dict(k=4097, per=1, fetch=4097)):
            assert _call(L, name, None, **kw) == _lib.MX_EUNSUPPORTED, (name, kw)
        # n > 16 and k * n > 4096 are the group-rows form's; per_key has no cap
        for kw in (dict(per=17, fetch=400), dict(k=257, per=16, fetch=4096), dict(k=4096, per=2, fetch=4096)):
            assert _call(L, name, None, **kw) == (_lib.MX_EUNSUPPORTED if rows else _lib.MX_ESEARCH), (name, kw)
        if rows:
            assert _call(L, name, None, per=17, fetch=400) == _lib.MX_EUNSUPPORTED and b"n = 17" in L.mx_last_error()
            assert _call(L, name, None, k=257, per=16, fetch=4096) == _lib.MX_EUNSUPPORTED and b"k * n" in L.mx_last_error()
        else:
            assert _call(L, name, None, per=2 ** 31 - 1) == _lib.MX_ESEARCH
        # an invalid argument before an unsupported one
        assert _call(L, name, None, k=5001, fetch=5000) == _lib.MX_EINVAL
        assert _call(L, name, None, g=0, fetch=5000) == _lib.MX_EINVAL
        assert _call(L, name, None, null="nf", fetch=5000) == _lib.MX_EINVAL
        assert _call(L, name, None, per=0, fetch=5000) == _lib.MX_EINVAL
        assert _call(L, name, None, k=0, per=17) == _lib.MX_EINVAL
        assert _call(L, name, None, g=0, per=17, fetch=400) == _lib.MX_EINVAL


def test_key_counts_refuses_bad_arguments(lib_built):
    from memex_amd import _lib
    L = lib_built
    one = (ctypes.c_uint32 * 1)()
    assert L.mx_grouping_key_counts(None, one, 1, None, None) == _lib.MX_EINVAL and b"grouping" in L.mx_last_error()
    assert L.mx_grouping_key_counts(ctypes.c_void_p(1), None, 1, None, None) == _lib.MX_EINVAL and b"keys" in L.mx_last_error()
    assert L.mx_grouping_key_counts(ctypes.c_void_p(1), one, 2 ** 20 + 1, None, None) == _lib.MX_EUNSUPPORTED
    assert L.mx_grouping_key_counts(None, one, 2 ** 20 + 1, None, None) == _lib.MX_EINVAL


def test_default_fetch_helper():
    from group_rows_model import default_fetch_rows
    from memex_amd.index import FlatIndex
    f = FlatIndex._group_rows_fetch
    assert f(10, 3, None) == 120 and f(1, 1, None) == 32 and f(10, 16, None) == 256 and f(300, 2, None) == 300
    assert f(5000, 1, None) == 4096 and f(10, 3, 77) == 77
    assert all(f(k, n, None) == default_fetch_rows(k, n) for k in range(1, 4097, 37) for n in (1, 2, 5, 16))


def test_host_mirrors_have_the_new_searches():
    import inspect
    from memex_amd.index import FlatIndex, IndexGrouping
    sig = lambda f: list(inspect.signature(f).parameters)[1:]  # noqa: E731
    assert sig(FlatIndex.search_group_rows) == ["grouping", "queries", "k", "n", "fetch", "flt", "settle"]
    assert inspect.signature(FlatIndex.search_group_rows).parameters["settle"].default is False
    assert sig(FlatIndex.search_capped) == ["grouping", "queries", "k", "per_key", "fetch", "flt"]
    assert sig(FlatIndex.search_group_rows_device)[:4] == ["grouping", "q", "k", "n"]
    assert sig(FlatIndex.search_capped_device)[:4] == ["grouping", "q", "k", "per_key"]
    assert sig(IndexGrouping.key_counts) == ["keys"]
    from memex_amd import tasks
    from memex_amd.storage import HipFlatStore, VectorStorage
    assert sig(HipFlatStore.search_document_passages) == ["vec", "limit", "grouping", "passages", "fetch", "flt"]
    assert inspect.signature(HipFlatStore.search_document_passages).parameters["passages"].default == 3
    assert sig(HipFlatStore.search_spread) == ["vec", "limit", "grouping", "per_document", "fetch", "flt"]
    assert inspect.signature(HipFlatStore.search_spread).parameters["per_document"].default == 2
    assert callable(VectorStorage.search_document_passages) and callable(VectorStorage.search_spread)
    assert list(inspect.signature(tasks.search_document_passages).parameters) == ["client", "embedder", "grouping", "query", "limit", "passages"]
    assert list(inspect.signature(tasks.search_docs_spread).parameters) == ["client", "embedder", "grouping", "query", "limit", "per_document"]
    hpp = open(os.path.join(ROOT, "include", "memex_hip.hpp")).read()
    assert "mx_index_search_group_rows(" in hpp and "mx_index_search_capped(" in hpp
    assert "struct DocumentPassages" in hpp and "search_document_passages(" in hpp and "struct SpreadHit" in hpp and "search_spread(" in hpp
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ROWS + CAPPED + COUNTS:
        assert f"fn {name}(" in integ, name
    assert "pub fn search_document_passages(" in integ


def test_store_searches_on_an_empty_store_touch_no_device(tmp_path):
    from memex_amd.storage import HipFlatStore, VectorStorage
    st = HipFlatStore(storage_path=str(tmp_path / "c"))                  # nothing inserted: no index, no device
    assert st.search_document_passages([0.0, 1.0], 5, None) == ([], True)
    assert st.search_spread([0.0, 1.0], 5, None, fetch=64) == ([], True)
    assert VectorStorage(st).search_document_passages([0.0, 1.0], 3, None) == ([], True)
    assert VectorStorage(st).search_spread([0.0, 1.0], 3, None) == ([], True)
    assert st._index is None


def test_tasks_forward_to_the_client():
    import pytest
    from memex_amd import tasks

    class Hit:
        def __init__(self, v):
            self.vector = v

    class Embedder:
        def encode_single(self, text):
            return Hit([float(len(text)), 1.0]) if text else None

    class Client:
        def search_document_passages(self, vec, limit, grouping, passages):
            self.seen = ("passages", vec, limit, grouping, passages)
            return [("doc", [("seg", 0.5)], True)], True

        def search_spread(self, vec, limit, grouping, per_document):
            self.seen = ("spread", vec, limit, grouping, per_document)
            return [("doc", "seg", 0.5)], True

    c, g = Client(), object()
    assert tasks.search_document_passages(c, Embedder(), g, "abc", limit=3, passages=4) == ([("doc", [("seg", 0.5)], True)], True)
    assert c.seen == ("passages", [3.0, 1.0], 3, g, 4)
    tasks.search_document_passages(c, Embedder(), g, "abcd")
    assert c.seen[2:] == (10, g, 3)
    assert tasks.search_docs_spread(c, Embedder(), g, "ab", limit=7, per_document=1) == ([("doc", "seg", 0.5)], True)
    assert c.seen == ("spread", [2.0, 1.0], 7, g, 1)
    tasks.search_docs_spread(c, Embedder(), g, "abcd")
    assert c.seen[2:] == (10, g, 2)
    for call in (tasks.search_document_passages, tasks.search_docs_spread):
        with pytest.raises(ValueError, match="Invalid query"):
            call(c, Embedder(), g, "")
