"""Shared by tests/test_calibrate_abi.py and tests/test_calibrate_gpu.py: the edge-value weight matrix and a NumPy statement of
the four K-blocked weight images (include/memex_hip.h: mx_encoder_weight_image)."""
import numpy as np

FORMS = {"bf16": 0, "bf16x3": 1, "mixed": 2, "mixed1": 3}     # MX_PREC_*
COPIES = {"bf16": 1, "bf16x3": 3, "mixed": 2, "mixed1": 1}


def edge_values() -> np.ndarray:
    """f32 values at which a rounding, a saturation or a NaN rule of the conversions changes."""
    bits = [0x00000000, 0x80000000,                         # +-0
            0x7fc12345, 0xffc54321,                         # NaN with a payload
            0x7f800000, 0xff800000,                         # +-inf
            0x7f7fffff, 0xff7fffff,                         # carries to bf16 inf
            0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000,  # exact bf16 ties: even below (down), odd below (up)
            0x3f801000, 0x3f803000, 0xbf801000, 0xbf803000,  # exact fp16 ties, both parities
            0x33000000, 0x33000001, 0x33800000, 0x33c00000,  # 2^-25 (fp16 tie to zero), just above, 2^-24, the tie 1.5 x 2^-24
            0x387fc000, 0x387fe000, 0x38800000]             # the largest fp16 subnormal, the tie above it, the smallest normal
    v = [np.array(bits, dtype=np.uint32).view(np.float32)]
    sat = np.array([65504.0, 65520.0, 1e6, 65519.996, 65503.0], dtype=np.float32)
    v += [sat, -sat]
    sub = np.geomspace(6e-8, 6e-5, 48).astype(np.float32)    # the fp16 subnormal range
    v += [sub, -sub, np.array([1e-38, -1e-38, 1e-30, 3e-39], dtype=np.float32)]
    return np.concatenate(v)


def edge_matrix(rows: int, k: int, seed: int = 0) -> np.ndarray:
    """[rows, k] f32: ordinary N(0, 0.05) weights with the edge values scattered through it (every one at least twice)."""
    rng = np.random.default_rng(seed)
    w = (0.05 * rng.standard_normal((rows, k))).astype(np.float32)
    e = edge_values()
    flat = w.reshape(-1)
    where = rng.choice(flat.size, size=3 * e.size, replace=False)
    flat[where] = np.tile(e, 3)
    return w


def _bf16_bits(w: np.ndarray) -> np.ndarray:
    u = w.view(np.uint32).astype(np.uint64)
    nan = (u & 0x7fffffff) > 0x7f800000
    r = (u + 0x7fff + ((u >> 16) & 1)) >> 16                  # round to nearest even (a carry may run into infinity)
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def numpy_image(w: np.ndarray, form: str) -> np.ndarray:
    """The image [k'/32][rows][32] as uint16, flattened: index arithmetic + bit manipulation (bf16) / np.float16 with a clamp (fp16)."""
    rows, k = w.shape
    with np.errstate(invalid="ignore", over="ignore"):
        if form in ("bf16", "bf16x3"):
            hi = _bf16_bits(w)
            if form == "bf16":
                wide = hi
            else:
                hf = (hi.astype(np.uint32) << 16).view(np.float32)
                wide = np.concatenate([hi, hi, _bf16_bits(w - hf)], axis=1)       # lo = bf16(w - hi)
        else:
            h = np.clip(w, np.float32(-65504.0), np.float32(65504.0)).astype(np.float16).view(np.uint16)
            wide = np.concatenate([h, h], axis=1) if form == "mixed" else h
    kk = wide.shape[1]
    return np.ascontiguousarray(wide.reshape(rows, kk // 32, 32).transpose(1, 0, 2)).reshape(-1)


def library_image(lib, w: np.ndarray, form: str, via_device: int) -> np.ndarray:
    import ctypes
    w = np.ascontiguousarray(w, dtype=np.float32)
    rows, k = w.shape
    out = np.zeros(rows * k * COPIES[form], dtype=np.uint16)
    rc = lib.mx_encoder_weight_image(w.ctypes.data_as(ctypes.c_void_p), rows, k, FORMS[form], via_device, 0,
                                     out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, lib.mx_last_error()
    return out
