"""Row removal at the C ABI and in the host mirrors, without a GPU: the entry points are exported and declared on every
layer, and bad arguments get the usual error codes before any device is touched."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_remove_entry_points_are_exported(lib_built):
    from memex_amd import _lib
    for name in ("mx_index_remove", "mx_index_removed"):
        assert hasattr(lib_built, name)
        assert name in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "memex_hip.h")).read()
    assert "int mx_index_remove(mx_index *idx, const uint64_t *ids, uint64_t n, uint64_t *n_removed);" in hdr
    assert "int mx_index_removed(mx_index *idx, uint64_t *n_removed);" in hdr


def test_remove_argument_validation_without_device(lib_built):
    from memex_amd import _lib
    n = ctypes.c_uint64(7)
    assert lib_built.mx_index_remove(None, None, 0, ctypes.byref(n)) == _lib.MX_EINVAL
    assert n.value == 0                                          # *n_removed is cleared even on failure
    ids = (ctypes.c_uint64 * 2)(1, 2)
    assert lib_built.mx_index_remove(None, ids, 2, None) == _lib.MX_EINVAL
    assert lib_built.mx_index_removed(None, ctypes.byref(n)) == _lib.MX_EINVAL
    assert lib_built.mx_index_removed(None, None) == _lib.MX_EINVAL
    assert b"null" in lib_built.mx_last_error()


def test_host_mirrors_have_remove():
    from memex_amd.index import FlatIndex
    from memex_amd.storage import HipFlatStore
    assert callable(FlatIndex.remove) and isinstance(FlatIndex.removed, property)
    assert callable(HipFlatStore.remove)
    hpp = open(os.path.join(ROOT, "include", "memex_hip.hpp")).read()
    assert "size_t remove(const std::vector<std::string> &ids)" in hpp and "mx_index_remove(" in hpp


def test_store_remove_on_an_empty_store_is_a_noop(tmp_path):
    from memex_amd.storage import HipFlatStore
    st = HipFlatStore(storage_path=str(tmp_path / "c"))         # nothing inserted: no index, no device
    assert st.remove("anything") == 0
    assert st.remove(["a", "b"]) == 0
    try:
        st.delete("a")                                           # delete keeps the reference's unimplemented!() contract
    except NotImplementedError:
        pass
    else:
        raise AssertionError("delete must still raise")
