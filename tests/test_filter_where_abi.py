"""Filters from row attributes (mx_filter_set_where / set_keys / combine / invert) at the C ABI and in the host
mirrors, without a GPU: the four entry points are exported and declared on every layer with the documented signatures, NULL handles
are refused before any index or device is looked at, and the NumPy model the GPU tests use obeys the laws of set algebra.  What
needs a handle -- NaN bounds, stale and foreign objects, the key limit -- cannot be checked here: tests/test_filter_where_gpu.py does."""
import ctypes
import inspect
import os

import numpy as np

import where_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mx_filter_set_where", "mx_filter_set_keys", "mx_filter_combine", "mx_filter_invert")
DECLS = (
    "enum { MX_FILTER_AND = 0, MX_FILTER_OR = 1, MX_FILTER_ANDNOT = 2, MX_FILTER_XOR = 3 };",
    "int mx_filter_set_where(mx_filter *f, mx_prior *p, float lo, float hi, int allow, uint64_t *n_selected);",
    "int mx_filter_set_keys(mx_filter *f, mx_grouping *g, const uint32_t *keys, uint64_t n_keys, int allow, uint64_t *n_selected);",
    "int mx_filter_combine(mx_filter *dst, mx_filter *a, mx_filter *b, int op);",
    "int mx_filter_invert(mx_filter *f);",
)


def test_entry_points_are_exported_and_declared(lib_built):
    from memex_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "memex_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib_built, name), name
        assert name in _lib.EXPORTS, name
    for decl in DECLS:
        assert decl in hdr, decl
    # declared after the three handle types they take
    at = hdr.index(DECLS[1])
    for t in ("mx_filter", "mx_grouping", "mx_prior"):
        assert hdr.index(f"typedef struct {t} {t};") < at, t
    section = hdr[hdr.index("Filters from row attributes:"):at]
    for phrase in ("lo <= v_r && v_r <= hi", "-0.0 matches [0, 0]", "lo > hi selects nothing", "a NaN bound is MX_EINVAL",
                   "it receives |S|, not the change of the set", "Key 0 may be listed", "n_keys > 2^20: MX_EUNSUPPORTED",
                   "dst may be a or b, and a may be b", "the complement within [0, size)", "A failing call changes nothing",
                   '"null filter", "null prior", "null grouping"', '"stale" in the message'):
        assert phrase in section, phrase
    assert (_lib.MX_FILTER_AND, _lib.MX_FILTER_OR, _lib.MX_FILTER_ANDNOT, _lib.MX_FILTER_XOR) == (0, 1, 2, 3)
    assert (wm.AND, wm.OR, wm.ANDNOT, wm.XOR) == (0, 1, 2, 3)


def test_null_handles_are_refused_before_any_device(lib_built):
    from memex_amd import _lib
    L = lib_built
    h = ctypes.c_void_p(1)                                               # stands for a handle; never looked at
    n = ctypes.c_uint64(77)
    keys = (ctypes.c_uint32 * 2)(1, 2)
    assert L.mx_filter_set_where(None, h, 0.0, 1.0, 1, ctypes.byref(n)) == _lib.MX_EINVAL and L.mx_last_error() == b"null filter"
    assert L.mx_filter_set_where(None, None, 0.0, 1.0, 1, None) == _lib.MX_EINVAL and L.mx_last_error() == b"null filter"
    assert L.mx_filter_set_where(h, None, 0.0, 1.0, 1, None) == _lib.MX_EINVAL and L.mx_last_error() == b"null prior"
    assert L.mx_filter_set_where(h, None, float("nan"), 1.0, 5, None) == _lib.MX_EINVAL and L.mx_last_error() == b"null prior"
    assert L.mx_filter_set_keys(None, h, keys, 2, 1, ctypes.byref(n)) == _lib.MX_EINVAL and L.mx_last_error() == b"null filter"
    assert L.mx_filter_set_keys(h, None, keys, 2, 1, None) == _lib.MX_EINVAL and L.mx_last_error() == b"null grouping"
    assert L.mx_filter_set_keys(h, None, None, 0, 1, None) == _lib.MX_EINVAL and L.mx_last_error() == b"null grouping"
    for args in ((None, h, h), (h, None, h), (h, h, None), (None, None, None)):
        for op in (0, 3, 9):
            assert L.mx_filter_combine(*args, op) == _lib.MX_EINVAL and L.mx_last_error() == b"null filter", (args, op)
    assert L.mx_filter_invert(None) == _lib.MX_EINVAL and L.mx_last_error() == b"null filter"
    assert n.value == 77                                                 # a failing call writes nothing


def test_the_stats_struct_did_not_grow(lib_built):
    from memex_amd import _lib
    assert lib_built.mx_index_stats_size() == ctypes.sizeof(_lib.IndexStats) == 160


def test_host_mirrors_have_the_methods():
    from memex_amd import tasks
    from memex_amd.index import FlatIndex, IndexFilter
    from memex_amd.storage import HipFlatStore, StoreFilter
    for m in ("allow_where", "deny_where"):
        p = inspect.signature(getattr(IndexFilter, m)).parameters
        assert list(p)[1:] == ["prior", "lo", "hi"] and p["lo"].default == -np.inf and p["hi"].default == np.inf, m
        assert list(inspect.signature(getattr(StoreFilter, m)).parameters)[1:] == ["prior", "lo", "hi"], m
    for m in ("allow_keys", "deny_keys"):
        assert list(inspect.signature(getattr(IndexFilter, m)).parameters)[1:] == ["grouping", "keys"], m
    for m in ("allow_documents", "deny_documents"):
        assert list(inspect.signature(getattr(StoreFilter, m)).parameters)[1:] == ["grouping", "documents"], m
    for cls in (IndexFilter, StoreFilter):
        assert list(inspect.signature(cls.invert).parameters) == ["self"]
    for m in ("__and__", "__or__", "__sub__", "__xor__"):
        assert m in vars(IndexFilter), m
    for cls in (FlatIndex, HipFlatStore):
        p = inspect.signature(cls.combine_filters).parameters
        assert list(p)[1:] == ["a", "b", "op", "out"] and p["out"].default is None
    p = inspect.signature(tasks.search_docs_since).parameters
    assert list(p) == ["client", "embedder", "prior", "flt", "query", "limit", "t_min", "half_life", "t0", "now", "weight"]
    hpp = open(os.path.join(ROOT, "include", "memex_hip.hpp")).read()
    for call in ("mx_filter_set_where(", "mx_filter_set_keys(", "mx_filter_combine(", "mx_filter_invert("):
        assert call in hpp, call
    for m in ("uint64_t allow_where(", "uint64_t deny_where(", "uint64_t allow_documents(", "uint64_t deny_documents(", "void invert()",
              "Filter combine_filters(", "void combine_filters("):
        assert m in hpp, m
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert f"fn {name}(" in integ, name


def test_the_mirrors_hand_null_handles_to_the_abi(lib_built):
    """IndexFilter's new methods pass their handles through; the ABI refuses the null ones by name, without a device"""
    import pytest
    from memex_amd import _lib
    from memex_amd.index import FlatIndex, IndexFilter

    class Null:
        _h = None

    flt = IndexFilter.__new__(IndexFilter)
    flt._h = None
    idx = FlatIndex.__new__(FlatIndex)
    idx._h = None
    try:
        for call, msg in ((lambda: flt.allow_where(Null), "null filter"), (lambda: flt.deny_where(Null, 0.0, 1.0), "null filter"),
                          (lambda: flt.allow_keys(Null, [1, 2, 2]), "null filter"), (lambda: flt.deny_keys(Null, np.zeros(0)), "null filter"),
                          (flt.invert, "null filter"), (lambda: idx.combine_filters(flt, flt, "xor", out=flt), "null filter")):
            with pytest.raises(_lib.MemexHipError) as e:
                call()
            assert e.value.code == _lib.MX_EINVAL and msg in str(e.value)
        with pytest.raises(_lib.MemexHipError, match="unknown filter op"):
            idx.combine_filters(flt, flt, "nand", out=flt)
    finally:
        flt._h = idx._h = None                                           # (nothing to close)


def test_tasks_since_statement():
    import pytest
    from memex_amd import tasks

    class Hit:
        def __init__(self, v):
            self.vector = v

    class Embedder:
        def encode_single(self, text):
            return Hit([float(len(text)), 1.0]) if text else None

    class Client:
        def search_boosted(self, vec, limit, prior, weight, fetch, flt):
            self.seen = (vec, limit, prior, weight, fetch, flt)
            return [("seg", 0.5, 4.0, 0.5)], True

    class Filter:
        def __init__(self):
            self.calls = []

        def allow_where(self, prior, lo=-np.inf, hi=np.inf):
            self.calls.append((prior, lo, hi))
            return 3

    c, f, p = Client(), Filter(), object()
    out = tasks.search_docs_since(c, Embedder(), p, f, "abc", limit=3, t_min=120.0, half_life=10.0, t0=100.0)
    assert out == ([("seg", 0.5, 4.0, 0.5)], True)
    assert f.calls == [(p, 4.0, np.inf)]                                 # the value stamp_document stores for t = 120
    assert c.seen == ([3.0, 1.0], 3, p, 0.0, None, f)
    tasks.search_docs_since(c, Embedder(), p, f, "abc", t_min=110.0, half_life=10.0, t0=100.0, now=130.0, weight=0.5)
    assert f.calls[-1] == (p, 2.0, np.inf) and c.seen[3] == 0.0625
    with pytest.raises(ValueError, match="Invalid query"):
        tasks.search_docs_since(c, Embedder(), p, f, "")
    assert len(f.calls) == 2                                             # nothing edited for a query that is refused
    with pytest.raises(ValueError, match="move t0"):
        tasks.search_docs_since(c, Embedder(), p, f, "abc", t_min=100.0 + 129 * 10.0, half_life=10.0, t0=100.0)


def test_host_bit_helpers(tmp_path):
    """copy_bits (the dealing of a selection to the shards), rows_below_word and combine_word of mx_filter_bits.h against a boolean
    model, under the host sanitizers (tests/cpp/test_where_bits.cpp)"""
    import subprocess
    exe = str(tmp_path / "test_where_bits")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_where_bits.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK where bits" in r.stdout, r.stdout + r.stderr


def test_where_model_laws():
    rng = np.random.default_rng(5)
    n = 1000
    a, b, c = (rng.random(n) < p for p in (0.5, 0.3, 0.05))
    # De Morgan
    np.testing.assert_array_equal(wm.invert(wm.combine(a, b, "and")), wm.combine(wm.invert(a), wm.invert(b), "or"))
    np.testing.assert_array_equal(wm.invert(wm.combine(a, b, "or")), wm.combine(wm.invert(a), wm.invert(b), "and"))
    np.testing.assert_array_equal(wm.invert(wm.invert(a)), a)
    np.testing.assert_array_equal(wm.combine(a, b, "andnot"), wm.combine(a, wm.invert(b), "and"))
    np.testing.assert_array_equal(wm.combine(a, b, "xor"), wm.combine(wm.combine(a, b, "or"), wm.combine(a, b, "and"), "andnot"))
    np.testing.assert_array_equal(wm.combine(a, a, "xor"), np.zeros(n, bool))
    np.testing.assert_array_equal(wm.combine(a, a, wm.ANDNOT), np.zeros(n, bool))
    for op in ("and", "or"):
        np.testing.assert_array_equal(wm.combine(a, a, op), a)
        np.testing.assert_array_equal(wm.combine(wm.combine(a, b, op), c, op), wm.combine(a, wm.combine(b, c, op), op))
    # edits: allow then deny of the same selection leaves a - s; n_selected is |S|, not the change
    m, k = wm.edit(a, b, 1)
    assert k == int(b.sum())
    m, k = wm.edit(m, b, 0)
    np.testing.assert_array_equal(m, a & ~b)
    assert k == int(b.sum())
    # predicates: a column shorter than the rows reads 0 behind its end; -0.0 matches [0, 0]; lo > hi selects nothing
    v = np.array([1.0, -0.0, 0.5, 3.0], np.float32)
    np.testing.assert_array_equal(wm.select_where(v, 6, 0.0, 0.0), [False, True, False, False, True, True])
    np.testing.assert_array_equal(wm.select_where(v, 6, 0.5, 1.0), [True, False, True, False, False, False])
    np.testing.assert_array_equal(wm.select_where(v, 6, -np.inf, np.inf), np.ones(6, bool))
    assert not wm.select_where(v, 6, 1.0, 0.5).any()
    assert wm.select_where(v, 3, 3.0, 3.0).sum() == 0                    # a column longer than the rows is cut
    ks = np.array([5, 0, 0xFFFFFFFF, 5], np.uint32)
    np.testing.assert_array_equal(wm.select_keys(ks, 6, [5, 5]), [True, False, False, True, False, False])
    np.testing.assert_array_equal(wm.select_keys(ks, 6, [0]), [False, True, False, False, True, True])
    np.testing.assert_array_equal(wm.select_keys(ks, 6, [0xFFFFFFFF, 7]), [False, False, True, False, False, False])
    assert not wm.select_keys(ks, 6, []).any()
    np.testing.assert_array_equal(wm.grown(np.array([True, False]), 4), [True, False, False, False])
