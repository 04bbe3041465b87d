"""Object wrapper over the ``mx_encoder_*`` C ABI (include/memex_hip.h): the HIP sentence encoder
that replaces the rust-bert model behind ``model.encode(&segments)``
(reference lib/libmemex/src/llm/embedding.rs:99-100,109)."""
from __future__ import annotations

import ctypes
import dataclasses
from typing import Dict, Optional, Tuple

import numpy as np

from . import _lib
from ._lib import EncoderCalibration, EncoderCfg, EncoderStats, check, lib
from .weights import EncoderConfig, pack_weights


def _cfg_struct(cfg: EncoderConfig) -> EncoderCfg:
    # "auto" (the calibrated open) travels as bf16: mx_encoder_open_calibrated ignores the field on entry
    return EncoderCfg(cfg.layers, cfg.hidden, cfg.heads, cfg.ffn, cfg.vocab, cfg.max_pos, cfg.type_vocab,
                      cfg.ln_eps, _lib.MX_POOL_CLS if cfg.pooling == "cls" else _lib.MX_POOL_MEAN,
                      1 if cfg.normalize else 0, cfg.pos_offset,
                      {"bf16": _lib.MX_PREC_BF16, "bf16x3": _lib.MX_PREC_BF16X3, "mixed": _lib.MX_PREC_MIXED,
                       "mixed1": _lib.MX_PREC_MIXED1, "auto": _lib.MX_PREC_BF16}[cfg.precision])


@dataclasses.dataclass(frozen=True)
class Calibration:
    """``mx_encoder_calibration`` with the modes by name.  ``pair_dev`` / ``row_dev``: mode -> deviation from the bf16x3 reference
    on the probe, for the modes in ``tried`` only."""
    chosen: str
    tried: Tuple[str, ...]
    probe_seqs: int
    probe_tokens: int
    bar: float
    pair_dev: Dict[str, float]
    row_dev: Dict[str, float]
    ms: float

    @classmethod
    def from_struct(cls, r: EncoderCalibration) -> "Calibration":
        tried = tuple(name for m, name in _lib.PRECISION_NAMES.items() if r.tried >> m & 1)
        by_name = {name: m for m, name in _lib.PRECISION_NAMES.items()}
        return cls(_lib.PRECISION_NAMES[r.chosen], tried, int(r.probe_seqs), int(r.probe_tokens), float(r.bar),
                   {n: float(r.pair_dev[by_name[n]]) for n in tried}, {n: float(r.row_dev[by_name[n]]) for n in tried}, float(r.ms))


def _blob(weights, cfg: EncoderConfig) -> np.ndarray:
    blob = weights if isinstance(weights, np.ndarray) else pack_weights(weights, cfg)
    return np.ascontiguousarray(blob, dtype=np.float32)


def _probe_args(probe):
    """(ids [B,S], lens [B]) or None -> what the C ABI takes (+ the arrays, to keep them alive through the call)."""
    if probe is None:
        return None, None, 0, 0, ()
    ids = np.ascontiguousarray(probe[0], dtype=np.int32)
    lens = np.ascontiguousarray(probe[1], dtype=np.int32)
    if ids.ndim != 2 or lens.shape != (ids.shape[0],):
        raise ValueError("probe: ids [B, S] and lens [B]")
    return ids.ctypes.data_as(ctypes.c_void_p), lens.ctypes.data_as(ctypes.c_void_p), ids.shape[0], ids.shape[1], (ids, lens)


class Encoder:
    def __init__(self, cfg: EncoderConfig, weights, device: int = 0, key: str | None = None, probe=None,
                 bar: Optional[float] = None, measure_all: bool = False):
        """``weights``: packed f32 blob (np.ndarray) or a mapping of HF tensor names (None = attach to
        the resident encoder ``key``).  ``key``: register / attach under that name: every Encoder opened
        with the same key shares ONE resident set of weights (the reference reloads the checkpoint per
        request, handlers.rs:61-63).

        ``cfg.precision == "auto"``: the calibrated open (mx_encoder_open_calibrated, include/memex_hip.h) -- the cheapest mode
        whose scores on a probe batch stay within ``bar`` (default MX_CALIBRATE_BAR) of the bf16x3 mode's, measured on these
        weights.  ``probe=(ids, lens)``: the caller's probe instead of the library's; ``measure_all``: measure every mode.
        Afterwards ``self.cfg.precision`` names the chosen mode and ``self.calibration`` holds the report."""
        self.cfg = cfg
        self.device = device
        self.calibration: Optional[Calibration] = None
        c = _cfg_struct(cfg)
        h = ctypes.c_void_p()
        if cfg.precision == "auto":
            blob = None if weights is None else _blob(weights, cfg)
            p_ids, p_lens, B, S, _keep = _probe_args(probe)
            rep = EncoderCalibration()
            check(lib().mx_encoder_open_calibrated(key.encode() if key else None, ctypes.byref(c),
                                                   None if blob is None else blob.ctypes.data_as(ctypes.c_void_p),
                                                   0 if blob is None else blob.nbytes, device, p_ids, p_lens, B, S,
                                                   _lib.MX_CALIBRATE_BAR if bar is None else float(bar),
                                                   _lib.MX_CALIBRATE_ALL if measure_all else 0, ctypes.byref(h), ctypes.byref(rep)))
            self.calibration = Calibration.from_struct(rep)
            self.cfg = dataclasses.replace(cfg, precision=self.calibration.chosen)
        elif weights is None:
            check(lib().mx_encoder_open(key.encode() if key else None, ctypes.byref(c), None, 0, device, ctypes.byref(h)))
        else:
            blob = _blob(weights, cfg)
            check(lib().mx_encoder_open(key.encode() if key else None, ctypes.byref(c), blob.ctypes.data_as(ctypes.c_void_p),
                                        blob.nbytes, device, ctypes.byref(h)))
        self._h = h

    @staticmethod
    def weight_bytes(cfg: EncoderConfig) -> int:
        c = _cfg_struct(cfg)
        return int(lib().mx_encoder_weight_bytes(ctypes.byref(c)))

    @staticmethod
    def calibrate(cfg: EncoderConfig, weights, device: int = 0, probe=None, bar: Optional[float] = None,
                  measure_all: bool = False) -> Calibration:
        """The report of the calibrated open alone (mx_encoder_calibrate): nothing stays resident.  ``cfg.precision`` is ignored."""
        c = _cfg_struct(dataclasses.replace(cfg, precision="auto"))
        blob = _blob(weights, cfg)
        p_ids, p_lens, B, S, _keep = _probe_args(probe)
        rep = EncoderCalibration()
        check(lib().mx_encoder_calibrate(ctypes.byref(c), blob.ctypes.data_as(ctypes.c_void_p), blob.nbytes, device, p_ids, p_lens, B, S,
                                         _lib.MX_CALIBRATE_BAR if bar is None else float(bar),
                                         _lib.MX_CALIBRATE_ALL if measure_all else 0, ctypes.byref(rep)))
        return Calibration.from_struct(rep)

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().mx_encoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def encode(self, ids, lens) -> np.ndarray:
        """ids [B,S] int, lens [B] -> [B, hidden] f32 (pooled, L2-normalised per cfg)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        B, S = ids.shape
        out = np.zeros((B, self.cfg.hidden), dtype=np.float32)
        check(lib().mx_encoder_encode(self._h, ids.ctypes.data_as(ctypes.c_void_p),
                                      lens.ctypes.data_as(ctypes.c_void_p), B, S,
                                      out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def encode_device(self, ids, lens, out) -> None:
        """Device tensors: ids int32 [B,S], lens int32 [B], out f32 [B,hidden] (blocks until done)."""
        B, S = int(ids.shape[0]), int(ids.shape[1])
        try:  # inputs were produced on torch's current stream (stream contract, include/memex_hip.h)
            import torch
            check(lib().mx_encoder_wait_stream(self._h, ctypes.c_void_p(torch.cuda.current_stream(ids.device).cuda_stream)))
        except ImportError:
            pass
        check(lib().mx_encoder_encode_device(self._h, ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(lens.data_ptr()),
                                             B, S, ctypes.c_void_p(out.data_ptr())))

    def set_profiling(self, on: bool) -> None:
        check(lib().mx_encoder_set_profiling(self._h, 1 if on else 0))

    def stats(self) -> EncoderStats:
        s = EncoderStats()
        check(lib().mx_encoder_get_stats(self._h, ctypes.byref(s)))
        return s

    def reset_stats(self) -> None:
        check(lib().mx_encoder_reset_stats(self._h))
