"""The calibrated encoder open on the GPU (include/memex_hip.h: mx_encoder_open_calibrated): the weight-image kernel against the
host routines bit for bit, whole encoders built on the device against mx_encoder_create's, the deviation kernel against NumPy
f64, the rule, what the caller gets against the f64 oracle, keyed handles and HBM accounting, Python against the C++ mirror."""
import ctypes
import dataclasses
import math
import os
import subprocess

import numpy as np
import pytest

from calibrate_cases import FORMS, edge_matrix, edge_values, library_image

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = ctypes.c_void_p
MODES = ("bf16", "bf16x3", "mixed", "mixed1")
ORDER = ("bf16", "mixed1", "mixed")          # the candidates by cost
BAR = 4e-4


def minilm(**kw):
    from memex_amd.weights import EncoderConfig
    return EncoderConfig(**{**dict(layers=6, hidden=384, heads=12, ffn=1536, vocab=3000), **kw})


def sample(seed=52, B=8, S=200, lo=100):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 3000, (B, S)).astype(np.int32)
    lens = rng.integers(lo, S + 1, B).astype(np.int32)
    return ids, lens


def unit(e):
    e = np.asarray(e, dtype=np.float64)
    return e / np.linalg.norm(e, axis=1, keepdims=True)


def deviations(a, b):
    """(pair, row) of two embedding sets in NumPy f64, as mx_encoder_calibration defines them."""
    a, b = unit(a), unit(b)
    iu = np.triu_indices(a.shape[0], 1)
    return float(np.abs((a @ a.T)[iu] - (b @ b.T)[iu]).max()), float((1.0 - (a * b).sum(1)).max())


def default_probe(lib, cfg):
    from memex_amd.encoder import _cfg_struct
    c = _cfg_struct(dataclasses.replace(cfg, precision="bf16"))
    B, S = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.mx_encoder_default_probe(ctypes.byref(c), None, None, ctypes.byref(B), ctypes.byref(S)) == 0
    ids, lens = np.zeros((B.value, S.value), dtype=np.int32), np.zeros(B.value, dtype=np.int32)
    assert lib.mx_encoder_default_probe(ctypes.byref(c), ids.ctypes.data_as(vp), lens.ctypes.data_as(vp), ctypes.byref(B), ctypes.byref(S)) == 0
    return ids, lens


def first_passing(dev, bar):
    return next((m for m in ORDER if dev[m] <= bar), "bf16x3")


# ---- 1. weight images

@pytest.mark.parametrize("rows,k", [(96, 64), (1152, 384), (384, 1920)])
@pytest.mark.parametrize("form", list(FORMS))
def test_weight_image_kernel_equals_the_host_routine(lib_built, rows, k, form):
    w = edge_matrix(rows, k, seed=rows + k)
    assert all((w.view(np.uint32) == b).sum() >= 2 for b in edge_values().view(np.uint32))
    host = library_image(lib_built, w, form, 0)
    dev = library_image(lib_built, w, form, 1)
    bad = np.flatnonzero(host != dev)
    assert bad.size == 0, (form, bad.size, bad[:8], host[bad[:8]], dev[bad[:8]])


# ---- 2. whole encoders

@pytest.mark.parametrize("hidden,heads,ffn", [(384, 12, 768), (384, 12, 1920), (768, 12, 768)])
def test_encoders_built_on_the_device_equal_the_host_built_ones(lib_built, hidden, heads, ffn):
    """Every mode, forced by the bar: the handle mx_encoder_open_calibrated returns (device blob, device conversion) and
    Encoder(cfg(precision=mode)) (mx_encoder_create: host conversion) give the same bits."""
    from memex_amd.encoder import Encoder
    from memex_amd.weights import EncoderConfig, checkpoint_like_weights, pack_weights
    base = EncoderConfig(layers=2, hidden=hidden, heads=heads, ffn=ffn, vocab=3000)
    blob = pack_weights(checkpoint_like_weights(base, 7), base)
    auto = dataclasses.replace(base, precision="auto")
    dev = Encoder.calibrate(auto, blob, measure_all=True).pair_dev
    print(f"{hidden}/{ffn}: pair_dev " + "  ".join(f"{m} {dev[m]:.3e}" for m in ORDER))
    assert dev["bf16"] > dev["mixed1"] > dev["mixed"] > 1e-12, dev         # what lets a bar single out each mode
    bars = {"bf16": 1.0, "bf16x3": 1e-12, "mixed1": math.sqrt(dev["bf16"] * dev["mixed1"]), "mixed": math.sqrt(dev["mixed1"] * dev["mixed"])}
    rng = np.random.default_rng(3)
    calls = [(rng.integers(0, 3000, (4, 40)).astype(np.int32), np.array([40, 17, 1, 33], dtype=np.int32))]
    if hidden == 384:  # more than 2048 packed rows: past the small pass
        calls.append((rng.integers(0, 3000, (24, 100)).astype(np.int32), np.full(24, 100, dtype=np.int32)))
    for mode in MODES:
        with Encoder(auto, blob, bar=bars[mode]) as got, Encoder(dataclasses.replace(base, precision=mode), blob) as want:
            assert got.cfg.precision == mode and got.calibration.chosen == mode, (mode, got.calibration)
            for ids, lens in calls:
                a, b = got.encode(ids, lens), want.encode(ids, lens)
                assert np.isfinite(b).all() and np.array_equal(a, b), (mode, ids.shape, np.abs(a - b).max())


# ---- 3. the deviation kernel

@pytest.mark.parametrize("H", [384, 768])
@pytest.mark.parametrize("B", [2, 8, 64])
def test_deviation_kernel_against_numpy_f64(lib_built, B, H):
    import torch
    rng = np.random.default_rng(B * 1000 + H)
    a = (rng.standard_normal((B, H)) * rng.uniform(0.1, 30.0, (B, 1))).astype(np.float32)       # unnormalised rows
    b = (a + 1e-3 * rng.standard_normal((B, H))).astype(np.float32)

    def run(x, y):
        dx, dy = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        torch.cuda.synchronize()
        p, r = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
        rc = lib_built.mx_embeddings_deviation_device(vp(dx.data_ptr()), vp(dy.data_ptr()), B, H, ctypes.byref(p), ctypes.byref(r))
        assert rc == 0, lib_built.mx_last_error()
        return p.value, r.value
    pair, row = run(a, b)
    want_pair, want_row = deviations(a, b)
    print(f"B={B} H={H}: pair {pair:.6e} (numpy {want_pair:.6e})  row {row:.6e} (numpy {want_row:.6e})")
    assert want_pair > 1e-9 and want_row > 1e-9
    assert abs(pair - want_pair) <= 1e-12 and abs(row - want_row) <= 1e-12
    assert run(a, a) == (0.0, run(a, a)[1]) and abs(run(a, a)[1]) <= 1e-15
    inf = (math.inf, math.inf)
    for bad in (math.nan, math.inf):
        c = b.copy()
        c[B - 1, H - 1] = bad
        assert run(a, c) == inf and run(c, a) == inf, bad
    z = b.copy()
    z[B // 2] = 0.0
    assert run(a, z) == inf and run(z, a) == inf
    p, r = ctypes.c_double(), ctypes.c_double()
    for nb, nh in ((1, H), (65, H), (B, 512)):
        assert lib_built.mx_embeddings_deviation_device(vp(8), vp(8), nb, nh, ctypes.byref(p), ctypes.byref(r)) == -1


# ---- 4. the rule

@pytest.fixture(scope="module")
def seed52(lib_built):
    """MiniLM-L6 shape, checkpoint-like weights seed 52, the 8-sequence sample: the four plain encoders' embeddings."""
    from memex_amd.encoder import Encoder
    from memex_amd.weights import checkpoint_like_weights, pack_weights
    cfg = minilm()
    w = checkpoint_like_weights(cfg, 52)
    blob = pack_weights(w, cfg)
    ids, lens = sample(52)
    emb = {}
    for mode in MODES:
        with Encoder(minilm(precision=mode), blob) as enc:
            emb[mode] = enc.encode(ids, lens)
    pair = {m: deviations(emb[m], emb["bf16x3"])[0] for m in ORDER}
    row = {m: deviations(emb[m], emb["bf16x3"])[1] for m in ORDER}
    return dict(cfg=cfg, w=w, blob=blob, ids=ids, lens=lens, emb=emb, pair=pair, row=row)


def test_the_rule(lib_built, seed52):
    from memex_amd.encoder import Encoder
    s = seed52
    pair, row, probe, auto = s["pair"], s["row"], (s["ids"], s["lens"]), minilm(precision="auto")
    print("numpy pair_dev " + "  ".join(f"{m} {pair[m]:.3e}" for m in ORDER) + " | row_dev " + "  ".join(f"{m} {row[m]:.3e}" for m in ORDER))
    full = Encoder.calibrate(auto, s["blob"], probe=probe, measure_all=True)
    print(full)
    assert set(full.tried) == set(MODES) and full.probe_seqs == 8 and full.probe_tokens == int(s["lens"].sum()) and full.bar == BAR
    assert full.pair_dev["bf16x3"] == 0.0 and full.row_dev["bf16x3"] == 0.0 and full.ms > 0.0
    for m in ORDER:
        assert abs(full.pair_dev[m] - pair[m]) <= 1e-12 and abs(full.row_dev[m] - row[m]) <= 1e-12, m
    # the recorded ordering (profiles/r6_precision_modes_over_seeds.txt: 2.66e-3, 2.58e-4, 1.11e-4 against the oracle)
    assert pair["bf16"] > pair["mixed1"] > pair["mixed"], pair
    bars = [1.0, 1e-12, BAR, math.sqrt(pair["bf16"] * pair["mixed1"]), math.sqrt(pair["mixed1"] * pair["mixed"])]
    want = [first_passing(pair, b) for b in bars]
    assert want[0] == "bf16" and want[1] == "bf16x3" and want[3] == "mixed1" and want[4] == "mixed", want
    for bar, w in zip(bars, want):
        r = Encoder.calibrate(auto, s["blob"], probe=probe, bar=bar, measure_all=True)
        assert r.chosen == w and set(r.tried) == set(MODES) and r.bar == bar, (bar, w, r)
        assert r.pair_dev == full.pair_dev and r.row_dev == full.row_dev                # bit-reproducible
        # without MX_CALIBRATE_ALL the measurement stops at the chosen mode; the rest reads NaN in the struct = absent here
        r = Encoder.calibrate(auto, s["blob"], probe=probe, bar=bar)
        upto = ORDER[:ORDER.index(w) + 1] if w != "bf16x3" else ORDER
        assert r.chosen == w and set(r.tried) == {"bf16x3", *upto}, (bar, w, r)
        assert all(r.pair_dev[m] == full.pair_dev[m] for m in upto)
    # ... in the struct itself
    from memex_amd import _lib
    from memex_amd.encoder import _cfg_struct
    rep, c = _lib.EncoderCalibration(), _cfg_struct(auto)
    assert lib_built.mx_encoder_calibrate(ctypes.byref(c), s["blob"].ctypes.data_as(vp), s["blob"].nbytes, 0, s["ids"].ctypes.data_as(vp),
                                          s["lens"].ctypes.data_as(vp), 8, 200, 1.0, 0, ctypes.byref(rep)) == 0
    assert rep.chosen == _lib.MX_PREC_BF16 and rep.tried == (1 << _lib.MX_PREC_BF16) | (1 << _lib.MX_PREC_BF16X3)
    assert math.isnan(rep.pair_dev[_lib.MX_PREC_MIXED]) and math.isnan(rep.row_dev[_lib.MX_PREC_MIXED1]) and rep.pair_dev[_lib.MX_PREC_BF16X3] == 0.0
    # an unknown precision on entry is ignored, not refused
    c.precision = 9
    assert lib_built.mx_encoder_calibrate(ctypes.byref(c), s["blob"].ctypes.data_as(vp), s["blob"].nbytes, 0, None, None, 0, 0, 1.0, 0,
                                          ctypes.byref(rep)) == 0 and rep.probe_seqs == 16


def test_a_reference_that_is_not_finite_is_an_error(lib_built):
    from memex_amd import _lib
    from memex_amd.encoder import Encoder
    from memex_amd.weights import EncoderConfig, pack_weights, synthetic_weights
    cfg = EncoderConfig(layers=1, hidden=384, heads=12, ffn=384, vocab=3000, precision="auto")
    w = synthetic_weights(cfg, 1)
    w["embeddings.LayerNorm.weight"][:] = np.nan
    with pytest.raises(_lib.MemexHipError) as ei:
        Encoder(cfg, pack_weights(w, cfg))
    assert "reference" in ei.value.msg and "finite" in ei.value.msg, ei.value.msg


# ---- 5. what the caller gets

@pytest.mark.parametrize("seed", [52, 5, 6])
def test_calibrated_minilm_holds_the_bar_against_the_oracle(lib_built, seed52, seed):
    from memex_amd.encoder import Encoder
    from memex_amd.weights import checkpoint_like_weights, pack_weights
    from oracle import bert_oracle
    cfg = minilm()
    w = seed52["w"] if seed == 52 else checkpoint_like_weights(cfg, seed)
    blob = pack_weights(w, cfg)
    p_ids, p_lens = default_probe(lib_built, cfg)
    own = {}
    for mode in ("bf16", "bf16x3"):
        with Encoder(minilm(precision=mode), blob) as enc:
            own[mode] = enc.encode(p_ids, p_lens)
    bf16_dev = deviations(own["bf16"], own["bf16x3"])[0]
    ids, lens = sample(52)
    with Encoder(minilm(precision="auto"), blob) as enc:
        rep = enc.calibration
        got = unit(enc.encode(ids, lens))
    assert abs(rep.pair_dev["bf16"] - bf16_dev) <= 1e-12 and rep.probe_seqs == 16 and rep.bar == BAR
    if bf16_dev > BAR:
        assert rep.chosen != "bf16", rep
    ref = unit(bert_oracle.encode_many(w, cfg.as_dict(), ids, lens))
    err = float(np.abs(got @ got.T - ref @ ref.T).max())
    print(f"MiniLM-L6 seed {seed}: bf16 pair_dev on the default probe {bf16_dev:.3e}, chosen {rep.chosen} "
          f"({'  '.join(f'{m} {v:.3e}' for m, v in rep.pair_dev.items())}), {rep.ms:.0f} ms; scores against the oracle {err:.3e}")
    assert err <= 1e-3, (rep, err)


def test_calibrated_bge_holds_the_bar_against_the_oracle(lib_built):
    """bge-base shape, seed 4 -- where the margin to 1e-3 is thinnest (mixed reads 1.5e-3 on the record): the probe is the inputs
    of test_encoder_gpu.py::test_precision_modes_over_weight_seeds, on which bf16x3 is known to meet the bar."""
    from memex_amd.encoder import Encoder
    from memex_amd.weights import EncoderConfig, checkpoint_like_weights, pack_weights
    from oracle import bert_oracle
    kw = dict(layers=12, hidden=768, heads=12, ffn=3072, vocab=3000, pooling="cls")
    base = EncoderConfig(**kw)
    w = checkpoint_like_weights(base, 4)
    B, S = 6, 200
    rng = np.random.default_rng(4)
    ids = rng.integers(0, base.vocab, (B, S)).astype(np.int32)
    lens = rng.integers(S // 2, S + 1, B).astype(np.int32)
    lens[0] = S
    with Encoder(EncoderConfig(**kw, precision="auto"), pack_weights(w, base), probe=(ids, lens)) as enc:
        rep = enc.calibration
        got = unit(enc.encode(ids, lens))
    ref = unit(bert_oracle.encode_many(w, base.as_dict(), ids, lens))
    err = float(np.abs(got @ got.T - ref @ ref.T).max())
    print(f"bge-base seed 4: chosen {rep.chosen} ({'  '.join(f'{m} {v:.3e}' for m, v in rep.pair_dev.items())}), {rep.ms:.0f} ms; "
          f"scores against the oracle {err:.3e}")
    assert rep.probe_seqs == 6 and err <= 1e-3, (rep, err)


def test_calibrated_open_on_mild_weights_reports_its_choice(lib_built):
    from memex_amd.encoder import Encoder
    from memex_amd.weights import pack_weights, synthetic_weights
    cfg = minilm(precision="auto")
    with Encoder(cfg, pack_weights(synthetic_weights(cfg, 0), cfg), measure_all=True) as enc:
        rep = enc.calibration
        print(f"synthetic_weights MiniLM-L6: chosen {rep.chosen} ({'  '.join(f'{m} {v:.3e}' for m, v in rep.pair_dev.items())})")
        assert rep.chosen == enc.cfg.precision == first_passing(rep.pair_dev, BAR)
        assert np.isfinite(enc.encode(*sample(1, B=2, S=16, lo=4))).all()


# ---- 6. keyed handles and accounting

def test_keyed_handles_and_accounting(lib_built, seed52):
    import torch
    from memex_amd import _lib
    from memex_amd.encoder import Encoder
    s = seed52
    auto, probe = minilm(precision="auto"), (s["ids"], s["lens"])
    bar = math.sqrt(s["pair"]["bf16"] * s["pair"]["mixed1"])                    # -> mixed1, as in test_the_rule
    with Encoder(auto, s["blob"], probe=probe, bar=bar):
        pass                                                                     # (kernels loaded, the runtime's pools warm)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    with Encoder(minilm(precision="mixed1"), s["blob"]) as plain:
        plain.encode(*probe)
        plain_used = free0 - torch.cuda.mem_get_info()[0]
    assert abs(torch.cuda.mem_get_info()[0] - free0) <= 2 << 20
    a = Encoder(auto, s["blob"], key="k", probe=probe, bar=bar)
    used = free0 - torch.cuda.mem_get_info()[0]
    print(f"HBM held by the calibrated handle {used / 2**20:.1f} MiB, by a plain mixed1 encoder after the same call {plain_used / 2**20:.1f} MiB; "
          f"blob {s['blob'].nbytes / 2**20:.1f} MiB")
    assert used <= plain_used + (8 << 20), (used, plain_used)                    # the f32 blob, the reference and the probe buffers are gone
    assert a.cfg.precision == a.calibration.chosen == "mixed1"
    assert a.stats().calls == 0 and a.stats().sequences == 0 and a.stats().tokens == 0
    b = Encoder(auto, None, key="k", bar=0.5)                                    # attaches in O(1): nothing is measured again
    assert b._h.value == a._h.value and b.calibration == a.calibration and b.calibration.ms == a.calibration.ms and b.cfg.precision == "mixed1"
    c = Encoder(auto, s["blob"], key="k")
    assert c._h.value == a._h.value and c.calibration == a.calibration
    got = _lib.EncoderCfg()
    assert lib_built.mx_encoder_get_cfg(a._h, ctypes.byref(got)) == 0
    assert got.precision == _lib.MX_PREC_MIXED1 and (got.layers, got.hidden, got.ffn, got.vocab) == (6, 384, 1536, 3000)
    d = Encoder(minilm(precision="mixed1"), None, key="k")                       # mx_encoder_open with the chosen precision attaches
    assert d._h.value == a._h.value and d.calibration is None
    for other in ("bf16", "bf16x3", "mixed"):                                    # ... with another one: the strict comparison
        with pytest.raises(_lib.MemexHipError) as ei:
            Encoder(minilm(precision=other), None, key="k")
        assert ei.value.code == _lib.MX_EINVAL
    with pytest.raises(_lib.MemexHipError) as ei:                                # every field but the precision is compared
        Encoder(minilm(precision="auto", pooling="cls"), None, key="k")
    assert ei.value.code == _lib.MX_EINVAL
    assert np.array_equal(a.encode(*probe), s["emb"]["mixed1"]) and a.stats().calls == 1
    for h in (a, b, c):
        h.close()
    assert np.array_equal(d.encode(*probe), s["emb"]["mixed1"])                  # the last reference keeps it alive
    d.close()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert abs(free1 - free0) <= 2 << 20, (free0, free1)
    # a handle that mx_encoder_open registered: the calibrated open attaches and says that nothing was measured
    with Encoder(minilm(precision="mixed"), s["blob"], key="plain") as p, Encoder(auto, None, key="plain") as q:
        assert q._h.value == p._h.value and q.cfg.precision == "mixed" and q.calibration.tried == () and q.calibration.chosen == "mixed"


# ---- 7. Python and C++ agree

def test_python_and_cpp_embedders_agree(tmp_path, lib_built):
    from test_pretrained import make_st_dir
    from memex_amd import embedding as E
    d = str(tmp_path / "st")
    make_st_dir(d, hidden=384, layers=2, ffn=768, max_seq_length=64, seed=3)
    th, emb = E.SentenceEmbedder.from_pretrained_dir(d, precision="auto")
    rep = emb.calibration
    v = emb.encode_single("the state of the union").vector
    emb.shutdown()
    assert rep is not None and rep.probe_seqs == 16 and len(v) == 384 and rep.chosen in MODES
    exe = str(tmp_path / "test_pretrained_calibrated")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_pretrained_calibrated.cpp"), "-o", exe, "-L", os.path.join(ROOT, "memex_amd"),
                           "-lmemex_hip", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "memex_amd")])
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK "), r.stdout + r.stderr
    f = r.stdout.split()
    from memex_amd import _lib
    assert _lib.PRECISION_NAMES[int(f[1])] == rep.chosen and int(f[3]) == 16 and int(f[4]) == rep.probe_tokens and float(f[5]) == BAR
    assert int(f[6]) == 384
    by_name = {name: m for m, name in _lib.PRECISION_NAMES.items()}
    for name, m in by_name.items():
        got = float(f[7 + m])
        assert (got == rep.pair_dev[name]) if name in rep.tried else math.isnan(got), (name, got, rep)
    # the caller's own texts as the probe
    texts = ["What does Biden say about taxes?", "The STATE of the Union 2023 -- unbelievable, isn't it?!", "hello world " * 60,
             "tokenizing long words", "they've said: we'll do it"]
    th, emb = E.SentenceEmbedder.from_pretrained_dir(d, precision="auto", calibration_texts=texts)
    rep5 = emb.calibration
    emb.shutdown()
    assert rep5.probe_seqs == 5 and 5 * 3 <= rep5.probe_tokens <= 5 * 64
    th, emb = E.SentenceEmbedder.from_pretrained_dir(d, precision="auto", calibration_texts=[f"text number {i}" for i in range(70)])
    assert emb.calibration.probe_seqs == 64
    emb.shutdown()
    with pytest.raises(E.SetupError):
        E.SentenceEmbedder.from_pretrained_dir(d, precision="auto", calibration_texts=["one"])
