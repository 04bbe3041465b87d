"""Grouped search at the C ABI and in the host mirrors, without a GPU: the entry points are exported and declared on every layer, and
bad arguments are refused before any index or device is looked at.  What needs a handle -- overlapping ranges, an id with two keys,
stale and foreign groupings -- cannot be checked here: tests/test_grouped_gpu.py does."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPING = ("mx_grouping_create", "mx_grouping_destroy", "mx_grouping_set_ranges", "mx_grouping_set_ids", "mx_grouping_get_keys",
            "mx_grouping_count")
SEARCH = ("mx_index_search_grouped", "mx_index_search_grouped_device")


def test_grouped_entry_points_are_exported_and_declared(lib_built):
    from memex_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "memex_hip.h")).read()
    for name in GROUPING + SEARCH:
        assert hasattr(lib_built, name)
        assert name in _lib.EXPORTS
        assert f" {name}(" in hdr
    assert "typedef struct mx_grouping mx_grouping;" in hdr
    for name in SEARCH:
        assert f"int {name}(mx_index *idx, mx_grouping *g, mx_filter *f," in hdr
    assert "int B, int k, int fetch" in hdr
    assert "int mx_grouping_set_ranges(mx_grouping *g, const uint64_t *ranges, const uint32_t *keys, uint64_t n_ranges);" in hdr
    assert "int mx_grouping_count(mx_grouping *g, uint64_t *n_keyed, uint64_t *n_live_keyed);" in hdr
    # the header states what `complete` promises, what key 0 means, and how concurrent callers are served
    assert "complete = 1 promises the EXACT top-k groups over ALL live rows" in hdr
    assert "complete[b] = 1 iff n_found[b] == k or L holds fewer than fetch entries" in hdr
    assert 'Key 0 means "ungrouped"' in hdr
    section = hdr[hdr.index("Grouped search:"):hdr.index("typedef struct mx_grouping")]
    assert "NOT combined" in section


def _call(lib, name, idx, g=1, B=1, k=10, fetch=10, null=None):
    n = max(B, 1)
    q = (ctypes.c_float * (4 * n))()
    ids = (ctypes.c_uint64 * (n * max(k, 1)))()
    sc = (ctypes.c_float * (n * max(k, 1)))()
    nf = (ctypes.c_int32 * n)()
    args = {"q": q, "ids": ids, "scores": sc, "nf": nf}
    if null:
        args[null] = None
    # g: any non-null pointer stands for a grouping; it is not looked at before the index is
    return getattr(lib, name)(idx, ctypes.c_void_p(g) if g else None, None, args["q"], B, k, fetch, args["ids"], args["scores"], None,
                              None, None, args["nf"], None)


def test_grouped_argument_validation_without_device(lib_built):
    from memex_amd import _lib
    L = lib_built
    for name in SEARCH:
        # valid arguments, null index: the code mx_index_search gives
        for kw in (dict(), dict(k=1, fetch=1), dict(k=10, fetch=4096), dict(k=4096, fetch=4096), dict(B=0), dict(B=0, null="ids"),
                   dict(B=0, null="q"), dict(B=600, k=2, fetch=2)):
            assert _call(L, name, None, **kw) == _lib.MX_ESEARCH, kw
        # the arguments are checked first
        bad = [dict(B=-1), dict(k=0), dict(k=-2), dict(k=10, fetch=9), dict(k=300, fetch=290), dict(g=0), dict(B=0, g=0), dict(null="q"),
               dict(null="ids"), dict(null="scores"), dict(null="nf")]
        for kw in bad:
            assert _call(L, name, None, **kw) == _lib.MX_EINVAL, kw
        assert _call(L, name, None, k=10, fetch=9) == _lib.MX_EINVAL and b"fetch" in L.mx_last_error()
        assert _call(L, name, None, g=0) == _lib.MX_EINVAL and b"grouping" in L.mx_last_error()
        for kw in (dict(fetch=4097), dict(fetch=5000), dict(k=4097, fetch=4097)):
            assert _call(L, name, None, **kw) == _lib.MX_EUNSUPPORTED, kw
        assert _call(L, name, None, fetch=5000) == _lib.MX_EUNSUPPORTED and b"fetch" in L.mx_last_error()
        # an invalid argument before an unsupported one: fetch < k also when k itself is past the cap
        assert _call(L, name, None, k=5001, fetch=5000) == _lib.MX_EINVAL
        assert _call(L, name, None, k=10, fetch=9) == _lib.MX_EINVAL
        assert _call(L, name, None, g=0, fetch=5000) == _lib.MX_EINVAL
        assert _call(L, name, None, null="nf", fetch=5000) == _lib.MX_EINVAL


def test_grouping_calls_refuse_null_handles(lib_built):
    from memex_amd import _lib
    L = lib_built
    h = ctypes.c_void_p(7)
    assert L.mx_grouping_create(None, ctypes.byref(h)) == _lib.MX_EINVAL and h.value is None     # *out is cleared
    assert L.mx_grouping_create(None, None) == _lib.MX_EINVAL
    assert L.mx_grouping_set_ranges(None, None, None, 0) == _lib.MX_EINVAL and b"grouping" in L.mx_last_error()
    assert L.mx_grouping_set_ids(None, None, None, 0) == _lib.MX_EINVAL
    assert L.mx_grouping_get_keys(None, None, 0, None) == _lib.MX_EINVAL
    assert L.mx_grouping_count(None, None, None) == _lib.MX_EINVAL
    L.mx_grouping_destroy(None)                                          # a no-op


def test_default_fetch_helper():
    from memex_amd.index import FlatIndex
    f = FlatIndex._grouped_fetch
    assert f(10, None) == 40 and f(1, None) == 32 and f(8, None) == 32 and f(64, None) == 256 and f(100, None) == 256
    assert f(256, None) == 256 and f(300, None) == 300 and f(4096, None) == 4096 and f(5000, None) == 4096
    assert f(10, 77) == 77 and f(10, 4096) == 4096
    from grouped_model import default_fetch
    assert all(f(k, None) == default_fetch(k) for k in range(1, 4097, 7))


def test_host_mirrors_have_grouped_search():
    import inspect
    from memex_amd import tasks
    from memex_amd.index import FlatIndex, IndexGrouping
    from memex_amd.storage import HipFlatStore, StoreGrouping, VectorStorage
    assert list(inspect.signature(FlatIndex.search_grouped).parameters)[1:] == ["grouping", "queries", "k", "fetch", "flt"]
    assert inspect.signature(FlatIndex.search_grouped).parameters["fetch"].default is None
    assert list(inspect.signature(FlatIndex.search_grouped_device).parameters)[1:4] == ["grouping", "q", "k"]
    assert callable(FlatIndex.make_grouping)
    for m in ("set_ranges", "set_ids", "keys_of", "count", "close", "__enter__", "__exit__"):
        assert callable(getattr(IndexGrouping, m)), m
    assert list(inspect.signature(IndexGrouping.set_ranges).parameters)[1:] == ["ranges", "keys"]
    assert list(inspect.signature(IndexGrouping.set_ids).parameters)[1:] == ["ids", "keys"]
    assert list(inspect.signature(HipFlatStore.make_grouping).parameters)[1:] == ["documents"]
    assert list(inspect.signature(HipFlatStore.search_documents).parameters)[1:] == ["vec", "limit", "grouping", "fetch", "flt"]
    for m in ("assign", "release", "count", "close"):
        assert callable(getattr(StoreGrouping, m)), m
    assert callable(VectorStorage.search_documents)
    assert list(inspect.signature(tasks.search_documents).parameters) == ["client", "embedder", "grouping", "query", "limit"]
    assert inspect.signature(tasks.search_documents).parameters["limit"].default == 10
    assert list(inspect.signature(tasks.group_document).parameters) == ["grouping", "vectors"]
    assert list(inspect.signature(tasks.search_docs).parameters) == ["client", "embedder", "query", "limit"]   # unchanged
    hpp = open(os.path.join(ROOT, "include", "memex_hip.hpp")).read()
    assert "mx_index_search_grouped(" in hpp and "mx_grouping_create(" in hpp and "mx_grouping_destroy(" in hpp
    assert "class Grouping {" in hpp and "struct DocumentHit" in hpp and "search_documents(" in hpp and "make_grouping(" in hpp
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fn mx_index_search_grouped(" in integ and "fn mx_index_search_grouped_device(" in integ
    for name in GROUPING:
        assert f"fn {name}(" in integ, name
    assert "pub fn search_documents(" in integ


def test_search_documents_on_an_empty_store_touches_no_device(tmp_path):
    import pytest
    from memex_amd.storage import HipFlatStore, SearchError, VectorStorage
    st = HipFlatStore(storage_path=str(tmp_path / "c"))                  # nothing inserted: no index, no device
    assert st.search_documents([0.0, 1.0], 5, None) == ([], True)
    assert st.search_documents([0.0, 1.0], 0, None, fetch=64) == ([], True)
    assert VectorStorage(st).search_documents([0.0, 1.0], 3, None) == ([], True)
    with pytest.raises(SearchError, match="insert first"):
        st.make_grouping()
    assert st._index is None


def test_tasks_search_documents_and_group_document():
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
        def search_documents(self, vec, limit, grouping):
            self.seen = (vec, limit, grouping)
            return [("doc", "seg", 0.5, 3)], True

    class Grouping:
        def __init__(self):
            self.calls = []

        def assign(self, document, ids):
            self.calls.append((document, list(ids)))

    c, g = Client(), Grouping()
    assert tasks.search_documents(c, Embedder(), g, "abc", limit=3) == ([("doc", "seg", 0.5, 3)], True)
    assert c.seen == ([3.0, 1.0], 3, g)
    tasks.search_documents(c, Embedder(), g, "abcd")
    assert c.seen[1] == 10
    with pytest.raises(ValueError, match="Invalid query"):
        tasks.search_documents(c, Embedder(), g, "")
    vs = [VectorData(_id=f"s{i}", document_id=f"d{i // 2}", text="", vector=[0.0]) for i in range(5)]
    tasks.group_document(g, vs)
    assert g.calls == [("d0", ["s0", "s1"]), ("d1", ["s2", "s3"]), ("d2", ["s4"])]
    tasks.group_document(g, [])
    assert len(g.calls) == 3
