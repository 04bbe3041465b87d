"""The host mirror of a resident filter (memex_amd/csrc/mx_filter_bits.h: range edits, run export) against a boolean model, as a
stand-alone program built with the host sanitizers.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_filter_bit_bookkeeping_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "test_filter_bits")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_filter_bits.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK filter bits" in r.stdout, r.stdout + r.stderr
