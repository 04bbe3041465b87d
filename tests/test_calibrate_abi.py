"""The calibrated encoder open (include/memex_hip.h: mx_encoder_open_calibrated), the part that needs no GPU: the ABI, the
default probe, argument validation, the host weight-image routines against a NumPy statement of the layouts, and the
loaders' "auto"."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from calibrate_cases import FORMS, edge_matrix, edge_values, library_image, numpy_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = ctypes.c_void_p


def _cfg(**kw):
    from memex_amd._lib import EncoderCfg
    d = dict(layers=2, hidden=384, heads=12, ffn=768, vocab=3000, max_pos=512, type_vocab=2, ln_eps=1e-12, pooling=0, normalize=1,
             pos_offset=0, precision=0)
    d.update(kw)
    return EncoderCfg(**d)


def _probe(lib, cfg):
    B, S = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.mx_encoder_default_probe(ctypes.byref(cfg), None, None, ctypes.byref(B), ctypes.byref(S)) == 0
    ids = np.full((B.value, S.value), -1, dtype=np.int32)
    lens = np.zeros(B.value, dtype=np.int32)
    assert lib.mx_encoder_default_probe(ctypes.byref(cfg), ids.ctypes.data_as(vp), lens.ctypes.data_as(vp), ctypes.byref(B), ctypes.byref(S)) == 0
    assert ids.shape == (B.value, S.value)
    return ids, lens


def test_struct_size_and_constants(lib_built):
    from memex_amd import _lib
    assert lib_built.mx_encoder_calibration_size() == ctypes.sizeof(_lib.EncoderCalibration) == 96
    header = open(os.path.join(ROOT, "include", "memex_hip.h")).read()
    assert "#define MX_CALIBRATE_BAR 4e-4" in header and _lib.MX_CALIBRATE_BAR == 4e-4
    assert "enum { MX_CALIBRATE_ALL = 1 }" in header and _lib.MX_CALIBRATE_ALL == 1
    for name in ("mx_encoder_open_calibrated", "mx_encoder_calibrate", "mx_encoder_default_probe", "mx_encoder_get_cfg",
                 "mx_encoder_weight_image", "mx_embeddings_deviation_device", "mx_encoder_calibration_size"):
        assert name in _lib.EXPORTS and hasattr(lib_built, name)


def test_default_probe(lib_built):
    cfg = _cfg()
    ids, lens = _probe(lib_built, cfg)
    ids2, lens2 = _probe(lib_built, cfg)
    assert np.array_equal(ids, ids2) and np.array_equal(lens, lens2)          # deterministic
    assert ids.shape == (16, 200)
    assert ids.min() >= 0 and ids.max() < 3000 and len(np.unique(ids)) > 1000
    assert lens.min() == 100 and lens.max() == 200 and (np.diff(lens) >= 0).all()
    assert np.abs(np.diff(lens) - 100 / 15).max() < 1.0                        # spread evenly
    rows = int(((lens + 7) // 8 * 8).sum())
    assert rows > 2048, rows                                                   # above the small-pass limit of the hidden-384 models
    # the ids are a counter hash (splitmix64) modulo vocab
    def splitmix64(x):
        m = (1 << 64) - 1
        x = (x + 0x9e3779b97f4a7c15) & m
        x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & m
        x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & m
        return x ^ (x >> 31)
    assert [int(v) for v in ids.reshape(-1)[:50]] == [splitmix64(i) % 3000 for i in range(50)]
    short = _cfg(max_pos=64, pos_offset=2)
    ids, lens = _probe(lib_built, short)
    assert ids.shape == (16, 62) and lens.min() == 31 and lens.max() == 62
    one = _cfg(max_pos=1, vocab=7)
    ids, lens = _probe(lib_built, one)
    assert ids.shape == (16, 1) and (lens == 1).all() and ids.max() < 7


def test_argument_validation_without_a_device(lib_built):
    from memex_amd import _lib
    L = lib_built
    cfg = _cfg()
    blob = np.zeros(L.mx_encoder_weight_bytes(ctypes.byref(cfg)) // 4, dtype=np.float32)
    rep = _lib.EncoderCalibration()
    ids = np.zeros((4, 16), dtype=np.int32)
    lens = np.full(4, 16, dtype=np.int32)

    def cal(out=ctypes.byref(rep), bar=4e-4, ids=ids, lens=lens, B=4, S=16, flags=0, cfg=cfg, nbytes=blob.nbytes):
        return L.mx_encoder_calibrate(ctypes.byref(cfg), blob.ctypes.data_as(vp), nbytes, 0,
                                      None if ids is None else ids.ctypes.data_as(vp), None if lens is None else lens.ctypes.data_as(vp),
                                      B, S, bar, flags, out)
    assert cal(out=None) == _lib.MX_EINVAL
    for bar in (0.0, -1e-3, math.nan, math.inf, -math.inf):
        assert cal(bar=bar) == _lib.MX_EINVAL, bar
    assert cal(B=1) == _lib.MX_EINVAL
    big_ids, big_lens = np.zeros((65, 16), dtype=np.int32), np.full(65, 16, dtype=np.int32)
    assert cal(ids=big_ids, lens=big_lens, B=65) == _lib.MX_EINVAL
    for bad in (0, 17, -3):
        ln = lens.copy()
        ln[2] = bad
        assert cal(lens=ln) == _lib.MX_EINVAL, bad
    assert cal(S=0) == _lib.MX_EINVAL and cal(S=513) == _lib.MX_EINVAL
    assert cal(lens=None) == _lib.MX_EINVAL and cal(flags=2) == _lib.MX_EINVAL and cal(nbytes=blob.nbytes - 4) == _lib.MX_EINVAL
    assert cal(cfg=_cfg(hidden=512)) == _lib.MX_EUNSUPPORTED                   # check_cfg's refusals stay
    h = vp()
    assert L.mx_encoder_open_calibrated(None, ctypes.byref(cfg), blob.ctypes.data_as(vp), blob.nbytes, 0, None, None, 0, 0, 4e-4, 0,
                                        None, ctypes.byref(rep)) == _lib.MX_EINVAL
    assert L.mx_encoder_open_calibrated(b"k", ctypes.byref(cfg), blob.ctypes.data_as(vp), blob.nbytes, 0, None, None, 0, 0, 0.0, 0,
                                        ctypes.byref(h), ctypes.byref(rep)) == _lib.MX_EINVAL
    assert L.mx_encoder_get_cfg(None, ctypes.byref(cfg)) == _lib.MX_EINVAL
    # an unknown precision is still refused by mx_encoder_create; the calibrated open ignores the field
    assert L.mx_encoder_create(ctypes.byref(_cfg(precision=7)), blob.ctypes.data_as(vp), blob.nbytes, 0, ctypes.byref(h)) == _lib.MX_EINVAL
    if _lib.device_count() > 0:
        return
    # valid arguments, no GPU: MX_EDEVICE -- never a host computation
    for kw in (dict(), dict(ids=None, lens=None, B=0, S=0), dict(cfg=_cfg(precision=7))):
        assert cal(**kw) == _lib.MX_EDEVICE, kw
    assert L.mx_encoder_open_calibrated(None, ctypes.byref(cfg), blob.ctypes.data_as(vp), blob.nbytes, 0, None, None, 0, 0, 4e-4, 0,
                                        ctypes.byref(h), ctypes.byref(rep)) == _lib.MX_EDEVICE
    w = np.zeros((32, 32), dtype=np.float32)
    out = np.zeros(32 * 32 * 3, dtype=np.uint16)
    assert L.mx_encoder_weight_image(w.ctypes.data_as(vp), 32, 32, 1, 1, 0, out.ctypes.data_as(vp)) == _lib.MX_EDEVICE
    from memex_amd.encoder import Encoder
    from memex_amd.weights import EncoderConfig, synthetic_weights
    ec = EncoderConfig(layers=1, hidden=384, heads=12, ffn=384, vocab=100, precision="auto")
    with pytest.raises(_lib.MemexHipError) as ei:
        Encoder(ec, synthetic_weights(ec))
    assert ei.value.code == _lib.MX_EDEVICE


@pytest.mark.parametrize("form", list(FORMS))
def test_host_weight_images_equal_the_numpy_statement(lib_built, form):
    """Pins the host routines (what mx_encoder_create uploads) before the kernel is compared with them."""
    from memex_amd import _lib
    w = edge_matrix(96, 64)
    e = edge_values()
    assert all((w.view(np.uint32) == b).sum() >= 2 for b in e.view(np.uint32))    # the edge values are in
    got = library_image(lib_built, w, form, 0)
    want = numpy_image(w, form)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (form, bad[:8], got[bad[:8]], want[bad[:8]])
    out = np.zeros(8, dtype=np.uint16)
    for rows, k, f in ((0, 32, 0), (4, 48, 0), (4, 0, 0), (4, 32, 4), (4, 32, -1)):
        assert lib_built.mx_encoder_weight_image(w.ctypes.data_as(vp), rows, k, f, 0, 0, out.ctypes.data_as(vp)) == _lib.MX_EINVAL


def test_the_named_edge_cases_of_the_images():
    """The NumPy statement itself gives what the issue's list says at the values that are easy to get wrong."""
    def one(bits, form):
        w = np.zeros((1, 32), dtype=np.float32)
        w.view(np.uint32)[0, 0] = bits
        return numpy_image(w, form).reshape(-1, 32)[:, 0]
    assert list(one(0x7fc12345, "bf16")) == [0x7fc1 | 0x40]                         # NaN rule: (u >> 16) | 0x40
    assert list(one(0x7f7fffff, "bf16x3")) == [0x7f80, 0x7f80, 0xff80]               # carry into infinity; lo = bf16(w - inf)
    assert list(one(0x3f808000, "bf16")) == [0x3f80] and list(one(0x3f818000, "bf16")) == [0x3f82]   # ties to even
    assert list(one(np.float32(65520.0).view(np.uint32), "mixed1")) == [0x7bff]      # saturation, not infinity
    assert list(one(np.float32(-1e6).view(np.uint32), "mixed")) == [0xfbff, 0xfbff]
    assert list(one(0xff800000, "mixed1")) == [0xfbff]
    assert list(one(0x33800000, "mixed1")) == [0x0001]                               # 2^-24: the smallest fp16 subnormal is kept
    assert list(one(0x33000000, "mixed1")) == [0x0000] and list(one(0x33c00000, "mixed1")) == [0x0002]   # ties to even
    x = np.float32(0.1)
    hi, _, lo = one(x.view(np.uint32), "bf16x3")
    f = lambda b: np.array([int(b) << 16], dtype=np.uint32).view(np.float32)[0]
    assert abs(float(f(hi)) + float(f(lo)) - float(x)) <= 2.0 ** -17 * float(x)       # hi + lo carries 16 significant bits


def test_device_conversions_as_host_code_equal_the_host_routines(tmp_path, lib_built):
    """memex_amd/csrc/mx_weight_forms.h -- the text the kernel compiles -- run on the host over a stride of ALL f32 bit patterns."""
    exe = str(tmp_path / "test_weight_forms")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_weight_forms.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "memex_amd"), "-lmemex_hip", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "memex_amd")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK weight forms" in r.stdout, r.stdout + r.stderr


def test_loaders_pass_auto_through(tmp_path):
    from test_pretrained import make_st_dir
    from memex_amd.pretrained import default_precision, load_pretrained_dir
    d = str(tmp_path / "st")
    make_st_dir(d, hidden=384, layers=1, ffn=384)
    assert load_pretrained_dir(d, "auto")[0].precision == "auto"
    assert load_pretrained_dir(d)[0].precision == "bf16" and load_pretrained_dir(d, None)[0].precision == "bf16"
    # default_precision is unchanged
    assert default_precision(768, "cls") == "bf16x3" and default_precision(768, "mean") == "bf16"
    assert default_precision(384, "cls") == "bf16" and default_precision(384, "mean") == "bf16"


def test_cpp_loader_carries_calibrate_through(tmp_path, lib_built):
    """include/memex_pretrained.hpp: kPrecisionCalibrated stays in the returned configuration, distinct from the `< 0` loader's choice."""
    from test_pretrained import make_st_dir
    exe = str(tmp_path / "test_pretrained_calibrated")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_pretrained_calibrated.cpp"), "-o", exe, "-L", os.path.join(ROOT, "memex_amd"),
                           "-lmemex_hip", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "memex_amd")])
    d = str(tmp_path / "st")
    make_st_dir(d, hidden=384, layers=1, ffn=384)
    r = subprocess.run([exe, d, "load"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["OK", "loaded", "-2"], r.stdout + r.stderr


def test_calibration_report_by_name():
    from memex_amd import _lib
    from memex_amd.encoder import Calibration
    r = _lib.EncoderCalibration(chosen=3, tried=0b1011, probe_seqs=16, probe_tokens=2400, bar=4e-4, ms=12.5)
    nan = math.nan
    r.pair_dev[:] = [2e-3, 0.0, nan, 1e-4]
    r.row_dev[:] = [1e-5, 0.0, nan, 1e-8]
    c = Calibration.from_struct(r)
    assert c.chosen == "mixed1" and c.tried == ("bf16", "bf16x3", "mixed1") and c.probe_seqs == 16 and c.probe_tokens == 2400
    assert c.pair_dev == {"bf16": 2e-3, "bf16x3": 0.0, "mixed1": 1e-4} and c.row_dev["mixed1"] == 1e-8 and c.bar == 4e-4 and c.ms == 12.5
