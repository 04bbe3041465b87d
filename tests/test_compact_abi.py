"""Compaction at the C ABI and in the host mirrors, without a GPU: the entry point is exported and declared on every layer, bad
arguments get the usual error codes, and both vector-file header versions are read by mx_index_store_info / has_store."""
import ctypes
import os
import struct

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_compact_entry_point_is_exported(lib_built):
    from memex_amd import _lib
    assert hasattr(lib_built, "mx_index_compact")
    assert "mx_index_compact" in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "memex_hip.h")).read()
    assert "int mx_index_compact(mx_index *idx, uint64_t *kept_ids, uint64_t kept_cap, uint64_t *n_live);" in hdr


def test_compact_argument_validation_without_device(lib_built):
    from memex_amd import _lib
    n = ctypes.c_uint64(7)
    assert lib_built.mx_index_compact(None, None, 0, ctypes.byref(n)) == _lib.MX_EINVAL
    assert n.value == 0                                          # *n_live is cleared even on failure
    kept = (ctypes.c_uint64 * 4)()
    assert lib_built.mx_index_compact(None, kept, 4, None) == _lib.MX_EINVAL
    assert b"null" in lib_built.mx_last_error()


def test_host_mirrors_have_compact():
    from memex_amd.index import FlatIndex
    from memex_amd.storage import HipFlatStore
    assert callable(FlatIndex.compact)
    assert callable(HipFlatStore.compact)
    hpp = open(os.path.join(ROOT, "include", "memex_hip.hpp")).read()
    assert "size_t compact()" in hpp and "mx_index_compact(" in hpp


def test_store_compact_on_an_empty_store_is_a_noop(tmp_path):
    from memex_amd.storage import HipFlatStore
    st = HipFlatStore(storage_path=str(tmp_path / "c"))         # nothing inserted: no index, no device
    kept = st.compact()
    assert kept.dtype.name == "uint64" and kept.size == 0
    assert not os.path.exists(tmp_path / "c")                    # nothing written either


def _write_store(path, magic, dim, n, gen=None, rows=True):
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "vectors.mxflat"), "wb") as f:
        f.write(magic + struct.pack("<IIQ", dim, 0, n))
        if gen is not None:
            f.write(struct.pack("<Q", gen))
        if rows:
            f.write(b"\0" * (4 * dim * n))


def _info(lib, path):
    d, n = ctypes.c_int(0), ctypes.c_uint64(0)
    rc = lib.mx_index_store_info(str(path).encode(), ctypes.byref(d), ctypes.byref(n))
    return rc, d.value, n.value


@pytest.mark.parametrize("magic,gen,ok", [
    (b"MXFLAT01", None, True),                                   # a never-compacted store
    (b"MXFLAT02", 3, True),                                      # a compacted one: generation 3
    (b"MXFLAT02", 0, False),                                     # generation 0 is MXFLAT01's: a damaged header
    (b"MXFLAT02", None, False),                                  # the generation word is missing
    (b"MXFLAT03", 1, False),                                     # an unknown version
])
def test_store_header_versions(lib_built, tmp_path, magic, gen, ok):
    from memex_amd import _lib
    p = tmp_path / "s"
    _write_store(str(p), magic, 5, 2, gen, rows=gen is not None or magic == b"MXFLAT01")
    if magic == b"MXFLAT02" and gen is None:                     # the file ends right after the row count
        with open(p / "vectors.mxflat", "wb") as f:
            f.write(magic + struct.pack("<IIQ", 5, 0, 2))
    e = ctypes.c_int(0)
    assert lib_built.mx_index_has_store(str(p).encode(), ctypes.byref(e)) == _lib.MX_OK and e.value == 1
    rc, d, n = _info(lib_built, p)
    if ok:
        assert (rc, d, n) == (_lib.MX_OK, 5, 2)
    else:
        assert rc == _lib.MX_EIO and b"bad header" in lib_built.mx_last_error()
