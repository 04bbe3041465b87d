"""memex::HipFlatStore::compact, the C++ host mirror of compaction (include/memex_hip.hpp): renumbers, saves and reloads
with the right _ids (tests/cpp/test_compact_store.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "test_compact_store")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_compact_store.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "memex_amd"), "-lmemex_hip", "-lpthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "memex_amd")])
    return exe


def test_cpp_compact_compiles_and_links(tmp_path, lib_built):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_cpp_compact_store(tmp_path, lib_built):
    exe = _build(tmp_path)
    r = subprocess.run([exe, str(tmp_path / "work")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK compact store" in r.stdout
