"""Thin object wrapper over the ``mx_index_*`` C ABI (include/memex_hip.h).

``FlatIndex`` is the GPU-resident exact cosine index that stands in for memex's ``HnswStore``
(reference lib/libmemex/src/storage/local.rs:21-166).  Host arrays are NumPy; the ``*_device``
methods take torch tensors already in HBM and refuse one of the wrong device, dtype, shape or layout before
the library sees its pointer (``FlatIndex._device_args``).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import IndexStats, check, lib


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def _caller_stream(t) -> ctypes.c_void_p | None:
    """The HIP stream torch is enqueueing work for tensor ``t`` on (None when torch is not in use)."""
    try:
        import torch
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    except ImportError:
        pass
    return None


# what a ``*_device`` tensor may be made of, by the kind the docstrings name
_DEVICE_DTYPES = {"f32": ("float32",), "f64": ("float64",), "i32": ("int32",), "u8": ("uint8",),
                  "id": ("int64", "uint64"), "key": ("int32", "uint32")}


SEARCH_AUTO, SEARCH_EXACT = 0, 1   # mx_index_set_search_mode


class FlatIndex:
    """``devices=None``: one index on ``device``.  ``devices=[...]``: the in-library sharded index
    (``mx_index_open_sharded``): rows dealt to the listed devices in blocks of ``block_rows``, local
    scans in parallel, one exchange of the per-shard top-k, merge on ``devices[0]``."""

    def __init__(self, dim: int, key: str | None = None, device: int = 0, devices=None, block_rows: int = 0):
        h = ctypes.c_void_p()
        if devices is None:
            check(lib().mx_index_open(key.encode() if key else None, int(dim), int(device), ctypes.byref(h)))
        else:
            devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
            check(lib().mx_index_open_sharded(key.encode() if key else None, int(dim), len(devices), devs,
                                              int(block_rows), ctypes.byref(h)))
            device = int(devices[0])
        self._h = h
        self.dim = int(dim)
        self.device = int(device)
        self.key = key
        self._id_offset = 0

    @property
    def n_shards(self) -> int:
        n = ctypes.c_int(0)
        check(lib().mx_index_n_shards(self._h, ctypes.byref(n)))
        return int(n.value)

    @property
    def exchange(self) -> str:
        """How the shards exchange their top-k blocks: "none" (plain index), "p2p" (copies) or "rccl"."""
        kind = ctypes.c_int(0)
        check(lib().mx_index_exchange(self._h, ctypes.byref(kind)))
        return ("none", "p2p", "rccl")[int(kind.value)]

    def wait_stream(self, stream) -> None:
        """Order the next operation on this index after everything enqueued on ``stream`` (a raw
        hipStream_t as int / c_void_p, or None for the default stream).  See the stream contract in
        include/memex_hip.h; the ``*_device`` methods call this with torch's current stream."""
        check(lib().mx_index_wait_stream(self._h, stream))

    def _device_args(self, *specs) -> None:
        """The tensors of a ``*_device`` call, checked before any library call: ``(name, tensor, kind, shape)`` each, ``kind`` a key
        of ``_DEVICE_DTYPES``; a tensor that is None (an optional output) and a ``shape`` that is None are not looked at.  The C ABI
        takes raw pointers, so a tensor on another device, of another dtype, too small or strided would be read or written out of
        bounds: each raises MX_EINVAL naming the argument."""
        for name, t, kind, shape in specs:
            if t is None:
                continue
            dev = getattr(t, "device", None)
            if getattr(dev, "type", None) != "cuda" or dev.index != self.device:
                raise _lib.MemexHipError(_lib.MX_EINVAL, f"{name}: expected a tensor on cuda:{self.device}, got one on {dev}")
            dt = str(t.dtype).rsplit(".", 1)[-1]
            if dt not in _DEVICE_DTYPES[kind]:
                raise _lib.MemexHipError(_lib.MX_EINVAL, f"{name}: expected dtype {' or '.join(_DEVICE_DTYPES[kind])}, got {dt}")
            if shape is not None and tuple(t.shape) != tuple(shape):
                raise _lib.MemexHipError(_lib.MX_EINVAL, f"{name}: expected shape {list(shape)}, got {list(t.shape)}")
            if not t.is_contiguous():
                raise _lib.MemexHipError(_lib.MX_EINVAL, f"{name}: expected a contiguous tensor, got strides {tuple(t.stride())}")

    def _device_queries(self, q, name: str = "q") -> int:
        """-> B of a device block of vectors f32 [B, dim] (queries, or rows to add), checked like every other device tensor"""
        if getattr(q, "ndim", None) != 2:
            raise _lib.MemexHipError(_lib.MX_EINVAL, f"{name}: expected shape [B, {self.dim}], got {list(getattr(q, 'shape', ()))}")
        B = int(q.shape[0])
        self._device_args((name, q, "f32", (B, self.dim)))
        return B

    def _device_lists(self, B: int, width, ids, scores, dists, n_found, *extra) -> None:
        """The outputs every search form has -- ids i64/u64, scores and dists f32 [B, *width], n_found i32 [B] -- and the form's own
        ``(name, tensor, kind, shape)``, ``shape`` a tuple, "B" for [B] or "BW" for [B, *width]"""
        w = tuple(max(int(x), 0) for x in width) if isinstance(width, tuple) else (max(int(width), 0),)
        shapes = {"B": (B,), "BW": (B,) + w}
        self._device_args(("ids", ids, "id", shapes["BW"]), ("scores", scores, "f32", shapes["BW"]), ("dists", dists, "f32", shapes["BW"]),
                          ("n_found", n_found, "i32", shapes["B"]), *((n, t, kd, shapes.get(sh, sh)) for n, t, kd, sh in extra))

    def _device_topk_args(self, q, width, ids, scores, dists, n_found, *extra) -> int:
        """-> B of a form with a device query block [B, dim] and the outputs of ``_device_lists``"""
        B = self._device_queries(q)
        self._device_lists(B, width, ids, scores, dists, n_found, *extra)
        return B

    # -- lifetime -------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().mx_index_close(self._h)
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

    def __len__(self) -> int:
        n = ctypes.c_uint64(0)
        check(lib().mx_index_size(self._h, ctypes.byref(n)))
        return int(n.value)

    # -- configuration -------------------------------------------------------------------
    def reserve(self, n_rows: int) -> None:
        check(lib().mx_index_reserve(self._h, int(n_rows)))

    def set_id_offset(self, off: int) -> None:
        check(lib().mx_index_set_id_offset(self._h, int(off)))
        self._id_offset = int(off)

    def set_search_mode(self, mode: int) -> None:
        check(lib().mx_index_set_search_mode(self._h, int(mode)))

    def set_filter_copy(self, on) -> None:
        """Keep or drop the filter copy the scan streams; results do not change.  ``False`` / ``"none"``: none (the
        scan reads the f32 rows); ``True`` / ``"auto"``: the library chooses (int8 up to 1024 dims, bf16 above, and an
        int8 copy is rebuilt as bf16 if a batch overflows it); ``"i8"``: int8 rows with one quantisation step per 32
        rows; ``"bf16"``: bf16 rows."""
        if isinstance(on, str):
            kind = {"none": 0, "auto": 1, "i8": 2, "int8": 2, "bf16": 3}[on]
        else:
            kind = 1 if on else 0
        check(lib().mx_index_set_filter_copy(self._h, int(kind)))

    def set_corpus_mode(self, mode: str) -> None:
        """``"f32"`` (default) or ``"bf16"``: keep only the bf16 rows (a third of the HBM); searches are
        then exact with respect to the stored rows (``get_rows``).  Only while the index is empty."""
        check(lib().mx_index_set_corpus_mode(self._h, {"f32": _lib.MX_CORPUS_F32, "bf16": _lib.MX_CORPUS_BF16}[mode]))

    def get_rows(self, first_row: int, n: int) -> np.ndarray:
        """Rows as stored (0-based, insertion order) -> f32 [n, dim]."""
        out = np.zeros((int(n), self.dim), dtype=np.float32)
        check(lib().mx_index_get_rows(self._h, int(first_row), int(n), _ptr(out)))
        return out

    def set_profiling(self, on: bool) -> None:
        check(lib().mx_index_set_profiling(self._h, 1 if on else 0))

    def stats(self) -> IndexStats:
        s = IndexStats()
        check(lib().mx_index_get_stats(self._h, ctypes.byref(s)))
        return s

    def reset_stats(self) -> None:
        check(lib().mx_index_reset_stats(self._h))

    # -- mutation ------------------------------------------------------------------------
    def add(self, rows) -> int:
        """Append rows [n, dim]; returns the (1-based) id of the first one."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim == 1:
            rows = rows[None, :]
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            raise _lib.MemexHipError(_lib.MX_EINVAL, f"expected [n, {self.dim}] rows, got {rows.shape}")
        first = ctypes.c_uint64(0)
        check(lib().mx_index_add(self._h, _ptr(rows), rows.shape[0], ctypes.byref(first)))
        return int(first.value)

    def add_device(self, t) -> int:
        """Append rows held in HBM (contiguous f32 [n, dim] tensor on this index's device)."""
        n = self._device_queries(t, "rows")
        first = ctypes.c_uint64(0)
        st = _caller_stream(t)
        if st is not None:
            self.wait_stream(st)
        check(lib().mx_index_add_device(self._h, ctypes.c_void_p(t.data_ptr()), n, ctypes.byref(first)))
        return int(first.value)

    def clear(self) -> None:
        check(lib().mx_index_clear(self._h))

    def remove(self, ids) -> int:
        """Remove rows by the ids search returns (tombstones: ids stay, the rows never appear in a result again).
        Every id is checked first: one that does not name a row raises and nothing is removed.  -> rows newly removed."""
        a = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64).reshape(-1))
        n = ctypes.c_uint64(0)
        check(lib().mx_index_remove(self._h, _ptr(a) if a.size else None, a.size, ctypes.byref(n)))
        return int(n.value)

    @property
    def removed(self) -> int:
        """Rows removed so far (len(self) still counts them)."""
        n = ctypes.c_uint64(0)
        check(lib().mx_index_removed(self._h, ctypes.byref(n)))
        return int(n.value)

    def compact(self) -> np.ndarray:
        """Drop the removed rows for good: the live rows keep their order and get dense ids again (the i-th gets
        id_offset + i + 1).  -> uint64 [len(self) afterwards]: the id each new id had before.  Ids held from before the
        call no longer name the same rows; the next save rewrites the store.  Nothing removed: the identity, a no-op."""
        live = len(self) - self.removed
        kept = np.zeros(max(live, 1), dtype=np.uint64)
        n = ctypes.c_uint64(0)
        check(lib().mx_index_compact(self._h, _ptr(kept), kept.size, ctypes.byref(n)))
        return kept[: int(n.value)]

    # -- search --------------------------------------------------------------------------
    def search(self, queries, k: int):
        """-> (ids u64 [B,k], scores f32 [B,k], dists f32 [B,k], n_found i32 [B])."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise _lib.MemexHipError(_lib.MX_EINVAL, f"expected [B, {self.dim}] queries, got {q.shape}")
        B = q.shape[0]
        ids = np.zeros((B, k), dtype=np.uint64)
        scores = np.zeros((B, k), dtype=np.float32)
        dists = np.zeros((B, k), dtype=np.float32)
        nf = np.zeros(B, dtype=np.int32)
        check(lib().mx_index_search(self._h, _ptr(q), B, int(k), _ptr(ids), _ptr(scores), _ptr(dists), _ptr(nf)))
        return ids, scores, dists, nf

    def search_device(self, q, k: int, ids, scores, dists, n_found) -> None:
        """All arguments are device tensors: q f32 [B,dim]; ids i64/u64 [B,k]; scores, dists f32 [B,k];
        n_found i32 [B].  Blocks until the results are in HBM."""
        B = self._device_topk_args(q, k, ids, scores, dists, n_found)
        st = _caller_stream(q)
        if st is not None:  # q and the (possibly just zero-filled) outputs were produced on torch's stream
            self.wait_stream(st)
        check(lib().mx_index_search_device(self._h, ctypes.c_void_p(q.data_ptr()), B, int(k),
                                           ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(scores.data_ptr()),
                                           ctypes.c_void_p(dists.data_ptr()) if dists is not None else None,
                                           ctypes.c_void_p(n_found.data_ptr())))

    def search_filtered(self, queries, k: int, *, ranges=None, ids=None):
        """The exact top-k among the rows whose ids are allowed -> like ``search``.  Give exactly one of ``ranges`` (an [m, 2]
        array of half-open id ranges [lo, hi), any order, overlaps allowed) or ``ids`` (an iterable of ids, turned into sorted
        runs).  Ids that name no row select nothing; an empty filter finds nothing."""
        r = _filter_ranges(ranges, ids)
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise _lib.MemexHipError(_lib.MX_EINVAL, f"expected [B, {self.dim}] queries, got {q.shape}")
        B = q.shape[0]
        out_ids = np.zeros((B, k), dtype=np.uint64)
        scores = np.zeros((B, k), dtype=np.float32)
        dists = np.zeros((B, k), dtype=np.float32)
        nf = np.zeros(B, dtype=np.int32)
        check(lib().mx_index_search_filtered(self._h, _ptr(q), B, int(k), _ptr(r) if r.size else None, r.shape[0],
                                             _ptr(out_ids), _ptr(scores), _ptr(dists), _ptr(nf)))
        return out_ids, scores, dists, nf

    def search_filtered_device(self, q, k: int, ids, scores, dists, n_found, *, ranges=None, allow_ids=None) -> None:
        """``search_device`` restricted like ``search_filtered``: the queries and outputs are device tensors, the filter
        (``ranges`` or ``allow_ids``) stays on the host."""
        r = _filter_ranges(ranges, allow_ids)
        B = self._device_topk_args(q, k, ids, scores, dists, n_found)
        st = _caller_stream(q)
        if st is not None:
            self.wait_stream(st)
        check(lib().mx_index_search_filtered_device(self._h, ctypes.c_void_p(q.data_ptr()), B, int(k), _ptr(r) if r.size else None,
                                                    r.shape[0], ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(scores.data_ptr()),
                                                    ctypes.c_void_p(dists.data_ptr()) if dists is not None else None,
                                                    ctypes.c_void_p(n_found.data_ptr())))

    def make_filter(self, ranges=None, ids=None) -> "IndexFilter":
        """A resident filter (``mx_filter``): an allow-set of this index's rows kept in HBM and named in ``search_with``.
        It starts empty, or with ``ranges`` and / or ``ids`` allowed (as ``IndexFilter.allow`` takes them)."""
        f = IndexFilter(self)
        try:
            if ranges is not None or ids is not None:
                f.allow(ranges=ranges, ids=ids)
        except Exception:
            f.close()
            raise
        return f

    _FILTER_OPS = {"and": _lib.MX_FILTER_AND, "or": _lib.MX_FILTER_OR, "andnot": _lib.MX_FILTER_ANDNOT, "xor": _lib.MX_FILTER_XOR}

    def combine_filters(self, a: "IndexFilter", b: "IndexFilter", op, out: "IndexFilter | None" = None) -> "IndexFilter":
        """``out = a op b`` over the rows, on the device (``mx_filter_combine``): ``op`` is "and", "or", "andnot" (``a`` and not
        ``b``), "xor" or the ``MX_FILTER_*`` number.  ``out`` may be ``a`` or ``b``; None makes a new filter.  -> ``out``."""
        code = self._FILTER_OPS.get(op, op) if isinstance(op, str) else op
        if isinstance(code, str):
            raise _lib.MemexHipError(_lib.MX_EINVAL, f"unknown filter op {op!r}: and, or, andnot, xor")
        dst = out if out is not None else IndexFilter(self)
        try:
            check(lib().mx_filter_combine(dst._h, a._h, b._h, int(code)))
        except Exception:
            if out is None:
                dst.close()
            raise
        return dst

    def search_with(self, flt: "IndexFilter", queries, k: int):
        """``search`` restricted to the rows of a resident filter: what ``search_filtered(queries, k, ranges=flt.ranges())``
        returns, bit for bit, without the per-call set-up."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise _lib.MemexHipError(_lib.MX_EINVAL, f"expected [B, {self.dim}] queries, got {q.shape}")
        B = q.shape[0]
        out_ids = np.zeros((B, k), dtype=np.uint64)
        scores = np.zeros((B, k), dtype=np.float32)
        dists = np.zeros((B, k), dtype=np.float32)
        nf = np.zeros(B, dtype=np.int32)
        check(lib().mx_index_search_with_filter(self._h, flt._h, _ptr(q), B, int(k), _ptr(out_ids), _ptr(scores), _ptr(dists),
                                                _ptr(nf)))
        return out_ids, scores, dists, nf

    def search_with_device(self, flt: "IndexFilter", q, k: int, ids, scores, dists, n_found) -> None:
        """``search_device`` restricted to the rows of a resident filter."""
        B = self._device_topk_args(q, k, ids, scores, dists, n_found)
        st = _caller_stream(q)
        if st is not None:
            self.wait_stream(st)
        check(lib().mx_index_search_with_filter_device(self._h, flt._h, ctypes.c_void_p(q.data_ptr()), B, int(k),
                                                       ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(scores.data_ptr()),
                                                       ctypes.c_void_p(dists.data_ptr()) if dists is not None else None,
                                                       ctypes.c_void_p(n_found.data_ptr())))

    def _min_scores(self, min_score, B: int) -> np.ndarray:
        t = np.asarray(min_score, dtype=np.float32)
        if t.ndim == 0:
            t = np.full(B, t, dtype=np.float32)
        t = np.ascontiguousarray(t.reshape(-1))
        if t.size != B:
            raise _lib.MemexHipError(_lib.MX_EINVAL, f"expected {B} thresholds, got {t.size}")
        return t

    def search_range(self, queries, min_score, cap: int):
        """Every row whose score reaches ``min_score`` (a scalar, or one threshold per query), exactly.
        -> (ids u64 [B,cap], scores f32 [B,cap], dists f32 [B,cap], n_found i32 [B], n_in_range u64 [B]): per query the in-range
        rows best-first, at most ``cap`` (1 .. 4096) of them; ``n_found`` = min(cap, n_in_range), ``n_in_range`` the exact count."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise _lib.MemexHipError(_lib.MX_EINVAL, f"expected [B, {self.dim}] queries, got {q.shape}")
        B = q.shape[0]
        t = self._min_scores(min_score, B)
        c = max(int(cap), 0)
        ids = np.zeros((B, c), dtype=np.uint64)
        scores = np.zeros((B, c), dtype=np.float32)
        dists = np.zeros((B, c), dtype=np.float32)
        nf = np.zeros(B, dtype=np.int32)
        nr = np.zeros(B, dtype=np.uint64)
        check(lib().mx_index_search_range(self._h, _ptr(q), B, _ptr(t) if t.size else None, int(cap), _ptr(ids) if ids.size else None,
                                          _ptr(scores) if scores.size else None, _ptr(dists) if dists.size else None, _ptr(nf),
                                          _ptr(nr)))
        return ids, scores, dists, nf, nr

    def search_range_device(self, q, min_score, cap: int, ids, scores, dists, n_found, n_in_range) -> None:
        """``search_range`` on device tensors: q f32 [B,dim]; ids i64/u64 [B,cap]; scores, dists f32 [B,cap] (dists may be
        None); n_found i32 [B]; n_in_range i64/u64 [B].  The thresholds stay on the host.  Blocks until the results are in HBM."""
        B = self._device_topk_args(q, max(int(cap), 0), ids, scores, dists, n_found, ("n_in_range", n_in_range, "id", "B"))
        t = self._min_scores(min_score, B)
        st = _caller_stream(q)
        if st is not None:
            self.wait_stream(st)
        check(lib().mx_index_search_range_device(self._h, ctypes.c_void_p(q.data_ptr()), B, _ptr(t) if t.size else None, int(cap),
                                                 ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(scores.data_ptr()),
                                                 ctypes.c_void_p(dists.data_ptr()) if dists is not None else None,
                                                 ctypes.c_void_p(n_found.data_ptr()), ctypes.c_void_p(n_in_range.data_ptr())))

    @staticmethod
    def _mmr_fetch(k: int, fetch) -> int:
        return min(max(4 * int(k), 32), 1024) if fetch is None else int(fetch)

    def search_mmr(self, queries, k: int, fetch=None, lam: float = 0.5):
        """Diversified search: exact maximal-marginal-relevance re-ranking of the top-``fetch`` rows (``mx_index_search_mmr``).
        -> (ids u64 [B,k], scores f32 [B,k], dists f32 [B,k], n_found i32 [B]) in SELECTION order: the best row first, then the
        rows that maximise ``lam * score - (1 - lam) * (largest similarity to a row already picked)``.  ``fetch=None``:
        ``min(max(4 * k, 32), 1024)`` candidates; ``lam = 1`` is the plain top-k, ``lam = 0`` cares for diversity only."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise _lib.MemexHipError(_lib.MX_EINVAL, f"expected [B, {self.dim}] queries, got {q.shape}")
        B = q.shape[0]
        kk = max(int(k), 0)
        ids = np.zeros((B, kk), dtype=np.uint64)
        scores = np.zeros((B, kk), dtype=np.float32)
        dists = np.zeros((B, kk), dtype=np.float32)
        nf = np.zeros(B, dtype=np.int32)
        check(lib().mx_index_search_mmr(self._h, _ptr(q), B, int(k), self._mmr_fetch(k, fetch), float(lam),
                                        _ptr(ids) if ids.size else None, _ptr(scores) if scores.size else None,
                                        _ptr(dists) if dists.size else None, _ptr(nf)))
        return ids, scores, dists, nf

    def search_mmr_device(self, q, k: int, ids, scores, dists, n_found, fetch=None, lam: float = 0.5) -> None:
        """``search_mmr`` on device tensors: q f32 [B,dim]; ids i64/u64 [B,k]; scores, dists f32 [B,k] (dists may be None);
        n_found i32 [B].  Blocks until the results are in HBM."""
        B = self._device_topk_args(q, k, ids, scores, dists, n_found)
        st = _caller_stream(q)
        if st is not None:
            self.wait_stream(st)
        check(lib().mx_index_search_mmr_device(self._h, ctypes.c_void_p(q.data_ptr()), B, int(k), self._mmr_fetch(k, fetch), float(lam),
                                               ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(scores.data_ptr()),
                                               ctypes.c_void_p(dists.data_ptr()) if dists is not None else None,
                                               ctypes.c_void_p(n_found.data_ptr())))

    # -- fused search ----------------------------------------------------------------------
    _FUSE_MODES = {"max": _lib.MX_FUSE_MAX, "rrf": _lib.MX_FUSE_RRF}

    @staticmethod
    def _fused_fetch(k: int, mode: str, fetch) -> int:
        if fetch is not None:
            return int(fetch)
        return int(k) if mode == "max" else min(max(4 * int(k), 32), 256)

    def _fused_args(self, shape, mode, weights):
        """-> (R, m, mode code, weights f32 [R, m] or None) for queries of ``shape`` ([R, m, dim] or [m, dim])"""
        if mode not in self._FUSE_MODES:
            raise _lib.MemexHipError(_lib.MX_EINVAL, f"mode {mode!r} is neither 'max' nor 'rrf'")
        shape = tuple(int(s) for s in shape)
        if len(shape) == 2:
            shape = (1,) + shape
        if len(shape) != 3 or shape[2] != self.dim:
            raise _lib.MemexHipError(_lib.MX_EINVAL, f"expected [R, m, {self.dim}] queries, got {shape}")
        R, m = shape[0], shape[1]
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.ndim == 1 and w.size == m:
                w = np.ascontiguousarray(np.broadcast_to(w, (R, m)))
            if w.shape != (R, m):
                raise _lib.MemexHipError(_lib.MX_EINVAL, f"expected [{R}, {m}] weights, got {w.shape}")
        return R, m, self._FUSE_MODES[mode], w

    def search_fused(self, queries, k: int, mode: str = "max", fetch=None, weights=None, rrf_c: float = 60.0):
        """One ranked list per request from SEVERAL query vectors (``mx_index_search_fused``): queries [R, m, dim], or [m, dim] for
        one request.  -> (ids u64 [R,k], scores f32 [R,k], dists f32 [R,k], n_found i32 [R], best_sub i32 [R,k], fused f64 [R,k]).
        ``mode="max"``: the exact top-k by the best score over the sub-queries ("any of these phrasings"); ``"rrf"``: reciprocal-rank
        fusion of the top-``fetch`` lists, ``sum w_i / (rrf_c + rank_i)``.  Each row appears once, with the score and dist of its
        best sub-query, whose index is ``best_sub``.  ``fetch=None``: ``k`` for "max", ``min(max(4 * k, 32), 256)`` for "rrf".
        ``weights`` [R, m] or [m]: a weight of 0 leaves that sub-query out of the request (padding of ragged requests)."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        R, m, code, w = self._fused_args(q.shape, mode, weights)
        kk = max(int(k), 0)
        ids = np.zeros((R, kk), dtype=np.uint64)
        scores = np.zeros((R, kk), dtype=np.float32)
        dists = np.zeros((R, kk), dtype=np.float32)
        best = np.zeros((R, kk), dtype=np.int32)
        fused = np.zeros((R, kk), dtype=np.float64)
        nf = np.zeros(R, dtype=np.int32)
        check(lib().mx_index_search_fused(self._h, _ptr(q) if q.size else None, R, m, _ptr(w) if w is not None and w.size else None, code,
                                          int(k), self._fused_fetch(k, mode, fetch), float(rrf_c), _ptr(ids) if ids.size else None,
                                          _ptr(scores) if scores.size else None, _ptr(dists) if dists.size else None,
                                          _ptr(best) if best.size else None, _ptr(fused) if fused.size else None, _ptr(nf)))
        return ids, scores, dists, nf, best, fused

    def search_fused_device(self, q, k: int, ids, scores, dists, n_found, best_sub=None, fused=None, mode: str = "max", fetch=None,
                            weights=None, rrf_c: float = 60.0) -> None:
        """``search_fused`` on device tensors: q f32 [R,m,dim]; ids i64/u64 [R,k]; scores, dists f32 [R,k]; best_sub i32 [R,k];
        fused f64 [R,k] (dists, best_sub and fused may be None); n_found i32 [R].  The weights stay on the host.  Blocks until the
        results are in HBM."""
        R, m, code, w = self._fused_args(q.shape, mode, weights)
        self._device_args(("q", q, "f32", None))
        self._device_lists(R, k, ids, scores, dists, n_found, ("best_sub", best_sub, "i32", "BW"), ("fused", fused, "f64", "BW"))
        st = _caller_stream(q)
        if st is not None:
            self.wait_stream(st)
        dp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        check(lib().mx_index_search_fused_device(self._h, dp(q), R, m, _ptr(w) if w is not None and w.size else None, code, int(k),
                                                 self._fused_fetch(k, mode, fetch), float(rrf_c), dp(ids), dp(scores), dp(dists),
                                                 dp(best_sub), dp(fused), dp(n_found)))

    # -- grouped search --------------------------------------------------------------------
    def make_grouping(self) -> "IndexGrouping":
        """A grouping (``mx_grouping``): one u32 key per row of this index, kept in HBM and named in ``search_grouped``.  It starts
        with key 0 (ungrouped) everywhere."""
        return IndexGrouping(self)

    @staticmethod
    def _grouped_fetch(k: int, fetch) -> int:
        if fetch is not None:
            return int(fetch)
        return min(4096, max(int(k), min(256, max(32, 4 * int(k)))))

    def search_grouped(self, grouping: "IndexGrouping", queries, k: int, fetch=None, flt: "IndexFilter | None" = None):
        """The ``k`` best GROUPS (documents), each by its best row (``mx_index_search_grouped``).
        -> (ids u64 [B,k], scores f32 [B,k], dists f32 [B,k], keys u32 [B,k], group_rows i32 [B,k], n_found i32 [B], complete bool [B]).
        Per query the top-``fetch`` list of ``search`` (of ``search_with(flt, ...)`` when ``flt`` is given) is walked in its order; a
        row whose key is 0, or whose key no earlier row of the list has, heads a group, and the first ``k`` heads are reported with
        their key and the number of rows of the list under that key.  ``complete[b]``: the answer is the exact top-k groups over all
        rows; otherwise it is exact for the list only and a larger ``fetch`` may find more.  ``fetch=None``: ``4 * k`` clamped to
        [32, 256] and never below ``k``."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise _lib.MemexHipError(_lib.MX_EINVAL, f"expected [B, {self.dim}] queries, got {q.shape}")
        B = q.shape[0]
        kk = max(int(k), 0)
        ids = np.zeros((B, kk), dtype=np.uint64)
        scores = np.zeros((B, kk), dtype=np.float32)
        dists = np.zeros((B, kk), dtype=np.float32)
        keys = np.zeros((B, kk), dtype=np.uint32)
        rows = np.zeros((B, kk), dtype=np.int32)
        nf = np.zeros(B, dtype=np.int32)
        done = np.zeros(B, dtype=np.uint8)
        p = lambda a: _ptr(a) if a.size else None  # noqa: E731
        check(lib().mx_index_search_grouped(self._h, grouping._h, flt._h if flt is not None else None, p(q), B, int(k),
                                            self._grouped_fetch(k, fetch), p(ids), p(scores), p(dists), p(keys), p(rows), p(nf), p(done)))
        return ids, scores, dists, keys, rows, nf, done.astype(bool)

    def search_grouped_device(self, grouping: "IndexGrouping", q, k: int, ids, scores, dists, keys, group_rows, n_found, complete,
                              fetch=None, flt: "IndexFilter | None" = None) -> None:
        """``search_grouped`` on device tensors: q f32 [B,dim]; ids i64/u64 [B,k]; scores, dists f32 [B,k]; keys i32/u32 [B,k];
        group_rows i32 [B,k]; n_found i32 [B]; complete u8 [B] (dists, keys, group_rows and complete may be None).  Blocks until the
        results are in HBM."""
        B = self._device_topk_args(q, k, ids, scores, dists, n_found, ("keys", keys, "key", "BW"), ("group_rows", group_rows, "i32", "BW"),
                                   ("complete", complete, "u8", "B"))
        st = _caller_stream(q)
        if st is not None:
            self.wait_stream(st)
        dp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        check(lib().mx_index_search_grouped_device(self._h, grouping._h, flt._h if flt is not None else None, dp(q), B, int(k),
                                                   self._grouped_fetch(k, fetch), dp(ids), dp(scores), dp(dists), dp(keys),
                                                   dp(group_rows), dp(n_found), dp(complete)))

    # -- grouped search with members -------------------------------------------------------
    @staticmethod
    def _group_rows_fetch(k: int, n: int, fetch) -> int:
        if fetch is not None:
            return int(fetch)
        return min(4096, max(int(k), min(256, max(32, 4 * int(k) * int(n)))))

    def _grouped_queries(self, queries) -> np.ndarray:
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise _lib.MemexHipError(_lib.MX_EINVAL, f"expected [B, {self.dim}] queries, got {q.shape}")
        return q

    def search_group_rows(self, grouping: "IndexGrouping", queries, k: int, n: int, fetch=None, flt: "IndexFilter | None" = None,
                          settle: bool = False):
        """The ``k`` best GROUPS (documents), each with its ``n`` best rows (``mx_index_search_group_rows``).
        -> (ids u64 [B,k,n], scores f32 [B,k,n], dists f32 [B,k,n], keys u32 [B,k], group_rows i32 [B,k], n_members i32 [B,k],
        members_complete bool [B,k], n_found i32 [B], complete bool [B]).
        The heads are those of ``search_grouped``; slot ``[b, j, r]`` is the r-th row of the top-``fetch`` list under head j's key
        (slot 0 the head itself; a key-0 head has itself only), unused slots id 0 / score 0 / dist +inf.  The listed members are
        always the exact best ``n_members`` rows of their group; ``members_complete[b, j]`` adds that the group has no further row
        that belongs in its first ``n``.  ``settle=True`` asks ``grouping.key_counts`` about the reported keys whose flag is 0 and
        raises it where ``n_members`` equals the key's live rows (one more pass over the keys, only when some flag is 0).
        ``fetch=None``: ``4 * k * n`` clamped to [32, 256] and never below ``k``."""
        q = self._grouped_queries(queries)
        B = q.shape[0]
        kk, nn = max(int(k), 0), max(int(n), 0)
        ids = np.zeros((B, kk, nn), dtype=np.uint64)
        scores = np.zeros((B, kk, nn), dtype=np.float32)
        dists = np.zeros((B, kk, nn), dtype=np.float32)
        keys = np.zeros((B, kk), dtype=np.uint32)
        rows = np.zeros((B, kk), dtype=np.int32)
        members = np.zeros((B, kk), dtype=np.int32)
        mdone = np.zeros((B, kk), dtype=np.uint8)
        nf = np.zeros(B, dtype=np.int32)
        done = np.zeros(B, dtype=np.uint8)
        p = lambda a: _ptr(a) if a.size else None  # noqa: E731
        check(lib().mx_index_search_group_rows(self._h, grouping._h, flt._h if flt is not None else None, p(q), B, int(k), int(n),
                                               self._group_rows_fetch(k, n, fetch), p(ids), p(scores), p(dists), p(keys), p(rows),
                                               p(members), p(mdone), p(nf), p(done)))
        mdone = mdone.astype(bool)
        if settle:
            open_ = ~mdone & (np.arange(kk)[None, :] < nf[:, None])
            if open_.any():
                asked = np.unique(keys[open_])
                live = grouping.key_counts(asked)[1]
                at = np.searchsorted(asked, keys[open_])
                mdone[open_] = members[open_].astype(np.uint64) == live[at]
        return ids, scores, dists, keys, rows, members, mdone, nf, done.astype(bool)

    def search_group_rows_device(self, grouping: "IndexGrouping", q, k: int, n: int, ids, scores, dists, keys, group_rows, n_members,
                                 members_complete, n_found, complete, fetch=None, flt: "IndexFilter | None" = None) -> None:
        """``search_group_rows`` on device tensors: q f32 [B,dim]; ids i64/u64, scores, dists f32 [B,k,n]; keys i32/u32, group_rows
        i32, n_members i32, members_complete u8 [B,k]; n_found i32 [B]; complete u8 [B] (dists, keys, group_rows, n_members,
        members_complete and complete may be None).  Blocks until the results are in HBM."""
        B = self._device_queries(q)
        heads = (B, max(int(k), 0))
        self._device_lists(B, (k, n), ids, scores, dists, n_found, ("keys", keys, "key", heads), ("group_rows", group_rows, "i32", heads),
                           ("n_members", n_members, "i32", heads), ("members_complete", members_complete, "u8", heads),
                           ("complete", complete, "u8", "B"))
        st = _caller_stream(q)
        if st is not None:
            self.wait_stream(st)
        dp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        check(lib().mx_index_search_group_rows_device(self._h, grouping._h, flt._h if flt is not None else None, dp(q), B, int(k), int(n),
                                                      self._group_rows_fetch(k, n, fetch), dp(ids), dp(scores), dp(dists), dp(keys),
                                                      dp(group_rows), dp(n_members), dp(members_complete), dp(n_found), dp(complete)))

    def search_capped(self, grouping: "IndexGrouping", queries, k: int, per_key: int, fetch=None, flt: "IndexFilter | None" = None):
        """The top-``k`` rows with at most ``per_key`` rows of any one group (``mx_index_search_capped``).
        -> (ids u64 [B,k], scores f32 [B,k], dists f32 [B,k], keys u32 [B,k], n_found i32 [B], complete bool [B]).
        The top-``fetch`` list is walked in its order; a row is accepted when its key is 0 or fewer than ``per_key`` earlier rows of
        the list have its key.  ``complete[b]``: the answer is the exact capped top-k over all rows.  ``fetch=None``: as
        ``search_grouped``."""
        q = self._grouped_queries(queries)
        B = q.shape[0]
        kk = max(int(k), 0)
        ids = np.zeros((B, kk), dtype=np.uint64)
        scores = np.zeros((B, kk), dtype=np.float32)
        dists = np.zeros((B, kk), dtype=np.float32)
        keys = np.zeros((B, kk), dtype=np.uint32)
        nf = np.zeros(B, dtype=np.int32)
        done = np.zeros(B, dtype=np.uint8)
        p = lambda a: _ptr(a) if a.size else None  # noqa: E731
        check(lib().mx_index_search_capped(self._h, grouping._h, flt._h if flt is not None else None, p(q), B, int(k), int(per_key),
                                           self._grouped_fetch(k, fetch), p(ids), p(scores), p(dists), p(keys), p(nf), p(done)))
        return ids, scores, dists, keys, nf, done.astype(bool)

    def search_capped_device(self, grouping: "IndexGrouping", q, k: int, per_key: int, ids, scores, dists, keys, n_found, complete,
                             fetch=None, flt: "IndexFilter | None" = None) -> None:
        """``search_capped`` on device tensors: q f32 [B,dim]; ids i64/u64, scores, dists f32, keys i32/u32 [B,k]; n_found i32 [B];
        complete u8 [B] (dists, keys and complete may be None).  Blocks until the results are in HBM."""
        B = self._device_topk_args(q, k, ids, scores, dists, n_found, ("keys", keys, "key", "BW"), ("complete", complete, "u8", "B"))
        st = _caller_stream(q)
        if st is not None:
            self.wait_stream(st)
        dp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        check(lib().mx_index_search_capped_device(self._h, grouping._h, flt._h if flt is not None else None, dp(q), B, int(k),
                                                  int(per_key), self._grouped_fetch(k, fetch), dp(ids), dp(scores), dp(dists), dp(keys),
                                                  dp(n_found), dp(complete)))

    # -- boosted search --------------------------------------------------------------------
    def make_prior(self) -> "IndexPrior":
        """A prior (``mx_prior``): one f32 per row of this index, kept in HBM and named in ``search_boosted``.  It starts at 0
        everywhere."""
        return IndexPrior(self)

    @staticmethod
    def _boost_weights(weight, B: int):
        """-> f32 [B], or None for weight 1.0 everywhere."""
        w = np.asarray(weight, dtype=np.float32)
        if w.ndim == 0:
            if float(w) == 1.0:
                return None
            w = np.full(B, w, dtype=np.float32)
        w = np.ascontiguousarray(w.reshape(-1))
        if w.size != B:
            raise _lib.MemexHipError(_lib.MX_EINVAL, f"expected {B} weights, got {w.size}")
        return w

    def search_boosted(self, prior: "IndexPrior", queries, k: int, weight=1.0, fetch=None, flt: "IndexFilter | None" = None):
        """The ``k`` best rows by ``score + weight * prior`` (``mx_index_search_boosted``).
        -> (ids u64 [B,k], scores f32 [B,k], dists f32 [B,k], priors f32 [B,k], combined f64 [B,k], n_found i32 [B], complete bool [B]).
        Per query the top-``fetch`` list of ``search`` (of ``search_with(flt, ...)`` when ``flt`` is given) is re-ranked by
        ``combined = float64(score) + float64(weight) * float64(prior)``, descending, ties in the list's order.  ``weight`` is a
        scalar or one value per query, finite and not negative.  ``complete[b]``: the answer is the exact top-k over all rows;
        otherwise it is exact for the list only and a larger ``fetch`` may change it.  ``fetch=None``: ``4 * k`` clamped to
        [32, 256] and never below ``k``."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise _lib.MemexHipError(_lib.MX_EINVAL, f"expected [B, {self.dim}] queries, got {q.shape}")
        B = q.shape[0]
        w = self._boost_weights(weight, B)
        kk = max(int(k), 0)
        ids = np.zeros((B, kk), dtype=np.uint64)
        scores = np.zeros((B, kk), dtype=np.float32)
        dists = np.zeros((B, kk), dtype=np.float32)
        priors = np.zeros((B, kk), dtype=np.float32)
        combined = np.zeros((B, kk), dtype=np.float64)
        nf = np.zeros(B, dtype=np.int32)
        done = np.zeros(B, dtype=np.uint8)
        p = lambda a: _ptr(a) if a is not None and a.size else None  # noqa: E731
        check(lib().mx_index_search_boosted(self._h, prior._h, flt._h if flt is not None else None, p(q), p(w), B, int(k),
                                            self._grouped_fetch(k, fetch), p(ids), p(scores), p(dists), p(priors), p(combined), p(nf),
                                            p(done)))
        return ids, scores, dists, priors, combined, nf, done.astype(bool)

    def search_boosted_device(self, prior: "IndexPrior", q, k: int, ids, scores, dists, priors, combined, n_found, complete,
                              weight=1.0, fetch=None, flt: "IndexFilter | None" = None) -> None:
        """``search_boosted`` on device tensors: q f32 [B,dim]; ids i64/u64 [B,k]; scores, dists, priors f32 [B,k]; combined f64
        [B,k]; n_found i32 [B]; complete u8 [B] (dists, priors, combined and complete may be None).  ``weight`` stays on the host.
        Blocks until the results are in HBM."""
        B = self._device_topk_args(q, k, ids, scores, dists, n_found, ("priors", priors, "f32", "BW"), ("combined", combined, "f64", "BW"),
                                   ("complete", complete, "u8", "B"))
        w = self._boost_weights(weight, B)
        st = _caller_stream(q)
        if st is not None:
            self.wait_stream(st)
        dp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        check(lib().mx_index_search_boosted_device(self._h, prior._h, flt._h if flt is not None else None, dp(q),
                                                   _ptr(w) if w is not None and w.size else None, B, int(k),
                                                   self._grouped_fetch(k, fetch), dp(ids), dp(scores), dp(dists), dp(priors),
                                                   dp(combined), dp(n_found), dp(complete)))

    # -- search by stored row --------------------------------------------------------------
    @staticmethod
    def _query_ids(ids) -> np.ndarray:
        return np.ascontiguousarray(np.asarray(ids, dtype=np.uint64).reshape(-1))

    def search_by_id(self, ids, k: int, exclude_self: bool = True):
        """More like these rows: ``search`` with the stored rows named by ``ids`` as queries (``mx_index_search_by_id``); the rows
        never leave HBM.  -> (ids u64 [B,k], scores f32 [B,k], dists f32 [B,k], n_found i32 [B]).  ``exclude_self``: the exact
        top-k of the live rows OTHER than the own row (exact copies of it stay).  An id that names no row, or a removed one,
        finds nothing."""
        a = self._query_ids(ids)
        B, kk = a.size, max(int(k), 0)
        out = np.zeros((B, kk), dtype=np.uint64)
        scores = np.zeros((B, kk), dtype=np.float32)
        dists = np.zeros((B, kk), dtype=np.float32)
        nf = np.zeros(B, dtype=np.int32)
        check(lib().mx_index_search_by_id(self._h, _ptr(a) if B else None, B, int(k), int(exclude_self), _ptr(out) if out.size else None,
                                          _ptr(scores) if scores.size else None, _ptr(dists) if dists.size else None, _ptr(nf)))
        return out, scores, dists, nf

    def search_by_id_device(self, ids, k: int, out_ids, scores, dists, n_found, exclude_self: bool = True) -> None:
        """``search_by_id`` with device tensors for the outputs: out_ids i64/u64 [B,k]; scores, dists f32 [B,k] (dists may be
        None); n_found i32 [B].  The query ids stay on the host.  Blocks until the results are in HBM."""
        a = self._query_ids(ids)
        self._device_lists(a.size, k, out_ids, scores, dists, n_found)
        st = _caller_stream(out_ids)
        if st is not None:
            self.wait_stream(st)
        check(lib().mx_index_search_by_id_device(self._h, _ptr(a) if a.size else None, a.size, int(k), int(exclude_self),
                                                 ctypes.c_void_p(out_ids.data_ptr()), ctypes.c_void_p(scores.data_ptr()),
                                                 ctypes.c_void_p(dists.data_ptr()) if dists is not None else None,
                                                 ctypes.c_void_p(n_found.data_ptr())))

    def search_range_by_id(self, ids, min_score, cap: int, exclude_self: bool = True):
        """``search_range`` with the stored rows named by ``ids`` as queries (``mx_index_search_range_by_id``) -> (ids u64 [B,cap],
        scores f32 [B,cap], dists f32 [B,cap], n_found i32 [B], n_in_range u64 [B]).  ``exclude_self``: the own row is neither
        listed nor counted."""
        a = self._query_ids(ids)
        B = a.size
        t = self._min_scores(min_score, B)
        c = max(int(cap), 0)
        out = np.zeros((B, c), dtype=np.uint64)
        scores = np.zeros((B, c), dtype=np.float32)
        dists = np.zeros((B, c), dtype=np.float32)
        nf = np.zeros(B, dtype=np.int32)
        nr = np.zeros(B, dtype=np.uint64)
        check(lib().mx_index_search_range_by_id(self._h, _ptr(a) if B else None, B, _ptr(t) if t.size else None, int(cap), int(exclude_self),
                                                _ptr(out) if out.size else None, _ptr(scores) if scores.size else None,
                                                _ptr(dists) if dists.size else None, _ptr(nf), _ptr(nr)))
        return out, scores, dists, nf, nr

    def search_range_by_id_device(self, ids, min_score, cap: int, out_ids, scores, dists, n_found, n_in_range,
                                  exclude_self: bool = True) -> None:
        """``search_range_by_id`` with device tensors for the outputs (as ``search_range_device``'s); the query ids and the
        thresholds stay on the host."""
        a = self._query_ids(ids)
        t = self._min_scores(min_score, a.size)
        self._device_lists(a.size, cap, out_ids, scores, dists, n_found, ("n_in_range", n_in_range, "id", "B"))
        st = _caller_stream(out_ids)
        if st is not None:
            self.wait_stream(st)
        check(lib().mx_index_search_range_by_id_device(self._h, _ptr(a) if a.size else None, a.size, _ptr(t) if t.size else None, int(cap),
                                                       int(exclude_self), ctypes.c_void_p(out_ids.data_ptr()),
                                                       ctypes.c_void_p(scores.data_ptr()),
                                                       ctypes.c_void_p(dists.data_ptr()) if dists is not None else None,
                                                       ctypes.c_void_p(n_found.data_ptr()), ctypes.c_void_p(n_in_range.data_ptr())))

    # -- search by examples ----------------------------------------------------------------
    def _like_args(self, example_ids, weights, queries_shape, query_weights):
        """-> (example ids u64 [R, m], weights f32 [R, m] or None, query weights f32 [R] or None)"""
        a = np.asarray(example_ids, dtype=np.uint64)
        if a.ndim == 1:
            a = a[None, :]
        if a.ndim != 2:
            raise _lib.MemexHipError(_lib.MX_EINVAL, f"expected [R, m] example ids, got {a.shape}")
        a = np.ascontiguousarray(a)
        R, m = a.shape
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.ndim == 1 and w.size == m:
                w = np.ascontiguousarray(np.broadcast_to(w, (R, m)))
            if w.shape != (R, m):
                raise _lib.MemexHipError(_lib.MX_EINVAL, f"expected [{R}, {m}] weights, got {w.shape}")
        if queries_shape is not None and tuple(queries_shape) != (R, self.dim):
            raise _lib.MemexHipError(_lib.MX_EINVAL, f"expected [{R}, {self.dim}] queries, got {tuple(queries_shape)}")
        qw = None
        if query_weights is not None:
            if queries_shape is None:
                raise _lib.MemexHipError(_lib.MX_EINVAL, "query_weights without queries")
            qw = np.asarray(query_weights, dtype=np.float32)
            qw = np.ascontiguousarray(np.broadcast_to(qw, (R,)) if qw.ndim == 0 else qw.reshape(-1))
            if qw.shape != (R,):
                raise _lib.MemexHipError(_lib.MX_EINVAL, f"expected {R} query weights, got {qw.shape}")
        return a, w, qw

    def search_like(self, example_ids, k: int, weights=None, queries=None, query_weights=None, exclude_examples: bool = True):
        """More like these rows, less like those (``mx_index_search_like``): per request the exact top-k for the weighted blend of
        the stored rows ``example_ids`` names -- [R, m], or [m] for one request -- each row scaled to unit length, plus
        ``query_weights * queries / |queries|`` when ``queries`` [R, dim] is given.  The rows never leave HBM.
        -> (ids u64 [R,k], scores f32 [R,k], dists f32 [R,k], n_found i32 [R], n_used i32 [R], combined f32 [R,dim]).
        ``weights`` [R, m] or [m]: positive = more like, negative = less like, 0 = the slot is absent (padding of ragged requests).
        Removed rows, ids that name no row and zero rows are skipped; ``n_used`` counts the examples that took part and ``combined``
        is the query that was searched.  ``exclude_examples``: the exact top-k of the live rows OTHER than the used examples (exact
        copies of them stay).  A request without a term, or whose terms cancel, finds nothing."""
        q = None
        if queries is not None:
            q = np.ascontiguousarray(queries, dtype=np.float32)
            if q.ndim == 1:
                q = q[None, :]
        a, w, qw = self._like_args(example_ids, weights, None if q is None else q.shape, query_weights)
        R, m = a.shape
        kk = max(int(k), 0)
        ids = np.zeros((R, kk), dtype=np.uint64)
        scores = np.zeros((R, kk), dtype=np.float32)
        dists = np.zeros((R, kk), dtype=np.float32)
        nf = np.zeros(R, dtype=np.int32)
        nu = np.zeros(R, dtype=np.int32)
        comb = np.zeros((R, self.dim), dtype=np.float32)
        opt = lambda x: _ptr(x) if x is not None and x.size else None  # noqa: E731
        check(lib().mx_index_search_like(self._h, opt(q), opt(qw), opt(a), opt(w), R, m, int(k), int(exclude_examples), opt(ids),
                                         opt(scores), opt(dists), _ptr(nf), _ptr(nu), opt(comb)))
        return ids, scores, dists, nf, nu, comb

    def search_like_device(self, example_ids, k: int, ids, scores, dists, n_found, n_used=None, combined=None, weights=None,
                           queries=None, query_weights=None, exclude_examples: bool = True) -> None:
        """``search_like`` on device tensors: queries f32 [R,dim] (or None); ids i64/u64 [R,k]; scores, dists f32 [R,k]; n_found,
        n_used i32 [R]; combined f32 [R,dim] (dists, n_used and combined may be None).  The example ids and all weights stay on the
        host.  Blocks until the results are in HBM."""
        a, w, qw = self._like_args(example_ids, weights, None if queries is None else queries.shape, query_weights)
        R, m = a.shape
        self._device_lists(R, k, ids, scores, dists, n_found, ("queries", queries, "f32", (R, self.dim)), ("n_used", n_used, "i32", "B"),
                           ("combined", combined, "f32", (R, self.dim)))
        st = _caller_stream(queries if queries is not None else ids)
        if st is not None:
            self.wait_stream(st)
        dp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        opt = lambda x: _ptr(x) if x is not None and x.size else None  # noqa: E731
        check(lib().mx_index_search_like_device(self._h, dp(queries), opt(qw), opt(a), opt(w), R, m, int(k), int(exclude_examples),
                                                dp(ids), dp(scores), dp(dists), dp(n_found), dp(n_used), dp(combined)))

    # -- scoring of named rows -------------------------------------------------------------
    @staticmethod
    def _cand_ids(ids, B: int) -> np.ndarray:
        """-> candidate ids u64 [B, m]; a list of lists is padded with 0 to its longest list"""
        if B == 0:
            return np.zeros((0, 1), dtype=np.uint64)
        if not isinstance(ids, np.ndarray) and len(ids) and all(hasattr(r, "__len__") for r in ids):
            m = max(max((len(r) for r in ids), default=0), 1)
            a = np.zeros((len(ids), m), dtype=np.uint64)
            for b, r in enumerate(ids):
                a[b, :len(r)] = np.asarray(r, dtype=np.uint64)
        else:
            a = np.asarray(ids, dtype=np.uint64)
            if a.ndim == 1:
                a = a[None, :]
        if a.ndim != 2 or a.shape[0] != B:
            raise _lib.MemexHipError(_lib.MX_EINVAL, f"expected [{B}, m] candidate ids, got {a.shape}")
        return np.ascontiguousarray(a)

    def score_ids(self, queries, ids):
        """What do these queries score against THESE rows (``mx_index_score_ids``): ``ids`` is [B, m], or a list of B lists padded
        with 0, of ids as ``search`` returns them.  -> (scores f32 [B,m], dists f32 [B,m], order i32 [B,m], n_found i32 [B]).
        An entry is found when ``search(queries[b], k=len(self))`` would list its id, and then holds that list's score and dist bit
        for bit; every other entry (id 0, an id that names no row, a removed row) is blank: score 0, dist +inf.  ``order[b, r]``,
        r < n_found[b], is the position of the r-th best found entry by (dist, id, position), -1 behind them:
        ``ids[b, order[b, :k]]`` is the exact top-k of the list.  Nothing is scanned and no row leaves HBM."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise _lib.MemexHipError(_lib.MX_EINVAL, f"expected [B, {self.dim}] queries, got {q.shape}")
        B = q.shape[0]
        a = self._cand_ids(ids, B)
        m = a.shape[1]
        scores = np.zeros((B, m), dtype=np.float32)
        dists = np.full((B, m), np.inf, dtype=np.float32)
        order = np.full((B, m), -1, dtype=np.int32)
        nf = np.zeros(B, dtype=np.int32)
        opt = lambda x: _ptr(x) if x.size else None  # noqa: E731
        check(lib().mx_index_score_ids(self._h, opt(q), B, opt(a), m, opt(scores), opt(dists), opt(order), opt(nf)))
        return scores, dists, order, nf

    def score_ids_device(self, q, ids, scores, dists=None, order=None, n_found=None) -> None:
        """``score_ids`` on device tensors: q f32 [B,dim]; scores, dists f32 [B,m]; order i32 [B,m]; n_found i32 [B] (dists, order and
        n_found may be None).  The candidate ids stay on the host.  Blocks until the results are in HBM."""
        B = self._device_queries(q)
        a = self._cand_ids(ids, B)
        cand = (B, a.shape[1])
        self._device_args(("scores", scores, "f32", cand), ("dists", dists, "f32", cand), ("order", order, "i32", cand),
                          ("n_found", n_found, "i32", (B,)))
        st = _caller_stream(q)
        if st is not None:
            self.wait_stream(st)
        dp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        check(lib().mx_index_score_ids_device(self._h, dp(q) if B else None, B, _ptr(a) if a.size else None, a.shape[1], dp(scores),
                                              dp(dists), dp(order), dp(n_found)))

    def near_duplicates(self, min_score: float, per_row: int = 64, block: int = 512):
        """The exact self-join: every pair of live rows whose score reaches ``min_score``.
        -> (pairs u64 [P, 2] with pairs[:, 0] < pairs[:, 1], sorted by (first id, second id), each pair once; scores f32 [P];
        truncated u64 [T]: the ids with more than ``per_row`` rows in range, whose lists were cut).
        Walks the ids id_offset + 1 .. id_offset + len in blocks of ``block`` through ``search_range_by_id(exclude_self=True,
        cap=per_row)``, id_offset being what ``set_id_offset`` was last given on this object.
        Guarantee: the score is symmetric bit for bit -- f32 products commute, the three f64 chains run in element order whichever
        row is the query, and na * nb commutes -- so row j is in row i's range exactly when i is in j's, with the same score.  A
        pair is therefore lost only when BOTH of its rows are listed in ``truncated``; raise ``per_row`` (at most 4095) to get
        those."""
        n = len(self)
        empty = (np.zeros((0, 2), dtype=np.uint64), np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.uint64))
        if n == 0:
            return empty
        first = self._id_offset + 1
        a_parts, b_parts, s_parts, trunc = [], [], [], []
        for lo in range(0, n, max(int(block), 1)):
            q = np.arange(first + lo, first + min(lo + max(int(block), 1), n), dtype=np.uint64)
            ids, scores, _, nf, nr = self.search_range_by_id(q, float(min_score), int(per_row), exclude_self=True)
            listed = np.arange(ids.shape[1])[None, :] < nf[:, None]
            own = np.broadcast_to(q[:, None], ids.shape)[listed]
            other = ids[listed]
            a_parts.append(np.minimum(own, other))
            b_parts.append(np.maximum(own, other))
            s_parts.append(scores[listed])
            trunc.append(q[nr > np.uint64(per_row)])
        a, b, s = np.concatenate(a_parts), np.concatenate(b_parts), np.concatenate(s_parts)
        truncated = np.concatenate(trunc)
        if a.size == 0:
            return empty[0], empty[1], truncated
        order = np.lexsort((b, a))
        a, b, s = a[order], b[order], s[order]
        keep = np.r_[True, (a[1:] != a[:-1]) | (b[1:] != b[:-1])]      # a pair seen from both ends: the same score, kept once
        return np.ascontiguousarray(np.stack([a[keep], b[keep]], axis=1)), s[keep], truncated

    # -- persistence ---------------------------------------------------------------------
    def save(self, directory: str) -> None:
        check(lib().mx_index_save(self._h, str(directory).encode()))

    def load(self, directory: str) -> None:
        check(lib().mx_index_load(self._h, str(directory).encode()))

    @staticmethod
    def has_store(directory: str) -> bool:
        e = ctypes.c_int(0)
        check(lib().mx_index_has_store(str(directory).encode(), ctypes.byref(e)))
        return bool(e.value)

    @staticmethod
    def store_info(directory: str):
        """-> (dim, n_rows) of the persisted vector file."""
        d = ctypes.c_int(0)
        n = ctypes.c_uint64(0)
        check(lib().mx_index_store_info(str(directory).encode(), ctypes.byref(d), ctypes.byref(n)))
        return int(d.value), int(n.value)

    @staticmethod
    def remove_files(directory: str) -> None:
        check(lib().mx_index_remove_files(str(directory).encode()))


def ids_to_ranges(ids) -> np.ndarray:
    """Ids (any order, repeats allowed) -> uint64 [m, 2]: the sorted, maximal runs of consecutive ids as half-open ranges."""
    a = np.unique(np.asarray(list(ids) if not hasattr(ids, "__len__") else ids, dtype=np.uint64).reshape(-1))
    if a.size == 0:
        return np.zeros((0, 2), dtype=np.uint64)
    brk = np.flatnonzero(np.diff(a) != 1) + 1           # where a run ends
    starts = a[np.r_[0, brk]]
    ends = a[np.r_[brk - 1, a.size - 1]] + np.uint64(1)
    return np.ascontiguousarray(np.stack([starts, ends], axis=1), dtype=np.uint64)


def _id_array(ids) -> np.ndarray:
    """Ids (an array or any iterable) -> contiguous uint64 [n]."""
    a = ids if isinstance(ids, np.ndarray) else np.fromiter(ids, dtype=np.uint64)
    return np.ascontiguousarray(a.astype(np.uint64, copy=False).reshape(-1))


def _per_item(x, n: int, dtype, noun: str) -> np.ndarray:
    """One ``x`` per item, or one for all -> contiguous ``dtype`` [n]."""
    v = np.asarray(x, dtype=dtype)
    if v.ndim == 0:
        v = np.full(n, v, dtype=dtype)
    v = np.ascontiguousarray(v.reshape(-1))
    if v.size != n:
        raise _lib.MemexHipError(_lib.MX_EINVAL, f"expected {n} {noun}, got {v.size}")
    return v


class _Handle:
    """A native handle ``_h`` that the library function named ``_destroy`` releases."""
    _destroy = ""

    def close(self) -> None:
        if getattr(self, "_h", None):
            getattr(lib(), self._destroy)(self._h)
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


class IndexFilter(_Handle):
    """A set of rows of one ``FlatIndex``, resident on the device(s) of the index (``mx_filter``).  It holds a
    reference on the index.  After the index's ``clear``, ``load`` or a ``compact`` that dropped rows every method but ``close``
    raises: make a new filter."""
    _destroy = "mx_filter_destroy"

    def __init__(self, index: FlatIndex):
        h = ctypes.c_void_p()
        check(lib().mx_filter_create(index._h, ctypes.byref(h)))
        self._h = h
        self._index = index

    def _edit(self, ranges, ids, allow: int) -> None:
        if ranges is None and ids is None:
            raise ValueError("give ranges and / or ids")
        if ranges is not None:
            r = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint64).reshape(-1, 2))
            check(lib().mx_filter_set_ranges(self._h, _ptr(r) if r.size else None, r.shape[0], allow))
        if ids is not None:
            a = _id_array(ids)
            check(lib().mx_filter_set_ids(self._h, _ptr(a) if a.size else None, a.size, allow))

    def allow(self, ranges=None, ids=None) -> None:
        """Add ids to the set: ``ranges`` ([m, 2] half-open id ranges, any order, overlaps allowed) and / or ``ids`` (any order,
        repeats allowed).  Ids that name no row at this moment are ignored."""
        self._edit(ranges, ids, 1)

    def deny(self, ranges=None, ids=None) -> None:
        """Take ids away from the set."""
        self._edit(ranges, ids, 0)

    def _where(self, prior: "IndexPrior", lo, hi, allow: int) -> int:
        n = ctypes.c_uint64(0)
        check(lib().mx_filter_set_where(self._h, prior._h, float(lo), float(hi), allow, ctypes.byref(n)))
        return int(n.value)

    def allow_where(self, prior: "IndexPrior", lo: float = -np.inf, hi: float = np.inf) -> int:
        """Add the rows whose value in ``prior`` lies in ``[lo, hi]`` (IEEE f32 compares; rows the prior does not reach read 0)
        -- decided on the device, no ids pass through the host (``mx_filter_set_where``).  -> rows selected."""
        return self._where(prior, lo, hi, 1)

    def deny_where(self, prior: "IndexPrior", lo: float = -np.inf, hi: float = np.inf) -> int:
        """Take the rows whose value in ``prior`` lies in ``[lo, hi]`` away from the set.  -> rows selected."""
        return self._where(prior, lo, hi, 0)

    def _keys(self, grouping: "IndexGrouping", keys, allow: int) -> int:
        k = keys if isinstance(keys, np.ndarray) else np.fromiter(keys, dtype=np.uint32)
        k = np.ascontiguousarray(k.astype(np.uint32, copy=False).reshape(-1))
        n = ctypes.c_uint64(0)
        check(lib().mx_filter_set_keys(self._h, grouping._h, _ptr(k) if k.size else None, k.size, allow, ctypes.byref(n)))
        return int(n.value)

    def allow_keys(self, grouping: "IndexGrouping", keys) -> int:
        """Add the rows whose key in ``grouping`` is one of ``keys`` (any order, repeats allowed, at most 2^20; key 0 names the
        ungrouped rows) -- ``mx_filter_set_keys``.  -> rows selected."""
        return self._keys(grouping, keys, 1)

    def deny_keys(self, grouping: "IndexGrouping", keys) -> int:
        """Take the rows whose key in ``grouping`` is one of ``keys`` away from the set.  -> rows selected."""
        return self._keys(grouping, keys, 0)

    def invert(self) -> None:
        """Replace the set by its complement within the rows the index holds at this moment (``mx_filter_invert``)."""
        check(lib().mx_filter_invert(self._h))

    def __and__(self, other: "IndexFilter") -> "IndexFilter":
        return self._index.combine_filters(self, other, "and")

    def __or__(self, other: "IndexFilter") -> "IndexFilter":
        return self._index.combine_filters(self, other, "or")

    def __sub__(self, other: "IndexFilter") -> "IndexFilter":
        return self._index.combine_filters(self, other, "andnot")

    def __xor__(self, other: "IndexFilter") -> "IndexFilter":
        return self._index.combine_filters(self, other, "xor")

    def count(self):
        """-> (rows in the set, those of them that are not removed)."""
        a, l = ctypes.c_uint64(0), ctypes.c_uint64(0)
        check(lib().mx_filter_count(self._h, ctypes.byref(a), ctypes.byref(l)))
        return int(a.value), int(l.value)

    def ranges(self) -> np.ndarray:
        """The set as normalised id ranges -> uint64 [m, 2], sorted and merged, under the index's current id offset."""
        n = ctypes.c_uint64(0)
        check(lib().mx_filter_get_ranges(self._h, None, 0, ctypes.byref(n)))
        out = np.zeros((int(n.value), 2), dtype=np.uint64)
        if out.size:
            check(lib().mx_filter_get_ranges(self._h, _ptr(out), out.shape[0], ctypes.byref(n)))
        return out[: int(n.value)]


class IndexGrouping(_Handle):
    """Which rows of one ``FlatIndex`` belong together: one u32 key per row, resident on the index's first device (``mx_grouping``,
    DESIGN.md 3.16).  Key 0 means ungrouped; rows appended later have key 0 until a call names them.  It holds a reference on the
    index.  After the index's ``clear``, ``load`` or a ``compact`` that dropped rows every method but ``close`` raises: make a new
    grouping."""
    _destroy = "mx_grouping_destroy"

    def __init__(self, index: FlatIndex):
        h = ctypes.c_void_p()
        check(lib().mx_grouping_create(index._h, ctypes.byref(h)))
        self._h = h

    def set_ranges(self, ranges, keys) -> None:
        """Every id of range ``i`` ([m, 2] half-open id ranges, pairwise disjoint, any order) gets ``keys[i]`` (one key per range,
        or one for all); key 0 un-groups.  Ids that name no row at this moment are ignored."""
        r = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint64).reshape(-1, 2))
        k = _per_item(keys, r.shape[0], np.uint32, "keys")
        check(lib().mx_grouping_set_ranges(self._h, _ptr(r) if r.size else None, _ptr(k) if k.size else None, r.shape[0]))

    def set_ids(self, ids, keys) -> None:
        """``ids[i]`` gets ``keys[i]`` (one key per id, or one for all).  Ids may repeat and come in any order, but not with two
        different keys in one call."""
        a = _id_array(ids)
        k = _per_item(keys, a.size, np.uint32, "keys")
        check(lib().mx_grouping_set_ids(self._h, _ptr(a) if a.size else None, _ptr(k) if k.size else None, a.size))

    def keys_of(self, ids) -> np.ndarray:
        """-> uint32 [n]: the key of the row each id names, 0 for an id that names no row."""
        a = _id_array(ids)
        out = np.zeros(a.size, dtype=np.uint32)
        check(lib().mx_grouping_get_keys(self._h, _ptr(a) if a.size else None, a.size, _ptr(out) if out.size else None))
        return out

    def count(self):
        """-> (rows with a non-zero key, those of them that are not removed)."""
        a, l = ctypes.c_uint64(0), ctypes.c_uint64(0)
        check(lib().mx_grouping_count(self._h, ctypes.byref(a), ctypes.byref(l)))
        return int(a.value), int(l.value)

    def key_counts(self, keys):
        """-> (uint64 [n] rows of the index under each key, uint64 [n] those of them that are not removed) -- ``mx_grouping_key_counts``.
        Key 0 counts the ungrouped rows; keys may repeat; at most 2^20."""
        k = np.ascontiguousarray(np.asarray(keys, dtype=np.uint32).reshape(-1))
        rows = np.zeros(k.size, dtype=np.uint64)
        live = np.zeros(k.size, dtype=np.uint64)
        check(lib().mx_grouping_key_counts(self._h, _ptr(k) if k.size else None, k.size, _ptr(rows) if k.size else None,
                                           _ptr(live) if k.size else None))
        return rows, live


class IndexPrior(_Handle):
    """What the vectors do not carry, per row of one ``FlatIndex``: one f32 per row, resident on the index's first device
    (``mx_prior``), added to the score by ``search_boosted``.  Rows nobody set, and rows appended later, read 0.  It
    holds a reference on the index.  After the index's ``clear``, ``load`` or a ``compact`` that dropped rows every method but
    ``close`` raises: make a new prior."""
    _destroy = "mx_prior_destroy"

    def __init__(self, index: FlatIndex):
        h = ctypes.c_void_p()
        check(lib().mx_prior_create(index._h, ctypes.byref(h)))
        self._h = h

    def set_ranges(self, ranges, values) -> None:
        """Every id of range ``i`` ([m, 2] half-open id ranges, pairwise disjoint, any order) gets ``values[i]`` (one value per
        range, or one for all).  Values are finite; a negative one is a penalty.  Ids that name no row at this moment are ignored."""
        r = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint64).reshape(-1, 2))
        v = _per_item(values, r.shape[0], np.float32, "values")
        check(lib().mx_prior_set_ranges(self._h, _ptr(r) if r.size else None, _ptr(v) if v.size else None, r.shape[0]))

    def set_ids(self, ids, values) -> None:
        """``ids[i]`` gets ``values[i]`` (one value per id, or one for all).  Ids may repeat and come in any order, but not with two
        different values in one call."""
        a = _id_array(ids)
        v = _per_item(values, a.size, np.float32, "values")
        check(lib().mx_prior_set_ids(self._h, _ptr(a) if a.size else None, _ptr(v) if v.size else None, a.size))

    def values_of(self, ids) -> np.ndarray:
        """-> float32 [n]: the value of the row each id names, 0 for an id that names no row."""
        a = _id_array(ids)
        out = np.zeros(a.size, dtype=np.float32)
        check(lib().mx_prior_get(self._h, _ptr(a) if a.size else None, a.size, _ptr(out) if out.size else None))
        return out

    def bound(self, refresh: bool = False) -> float:
        """The upper bound of the values that ``search_boosted``'s ``complete`` is decided with: never below a value of the array,
        raised by every edit, lowered only by ``refresh=True``, which recomputes the maximum of 0 and the live rows' values."""
        hi = ctypes.c_float(0.0)
        check(lib().mx_prior_bound(self._h, 1 if refresh else 0, ctypes.byref(hi)))
        return float(hi.value)


def _filter_ranges(ranges, ids) -> np.ndarray:
    if (ranges is None) == (ids is None):
        raise ValueError("give exactly one of ranges= and ids=")
    if ids is not None:
        return ids_to_ranges(ids)
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint64).reshape(-1, 2))
    return r


def merge_topk_device(device: int, ids, dists, out_ids, out_dists, out_scores) -> None:
    """ids/dists: device tensors [G,B,k] (gathered shard results) -> [B,k] global top-k."""
    G, B, k = (int(x) for x in ids.shape)
    check(lib().mx_topk_merge_device(int(device), ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(dists.data_ptr()),
                                     G, B, k, ctypes.c_void_p(out_ids.data_ptr()),
                                     ctypes.c_void_p(out_dists.data_ptr()),
                                     ctypes.c_void_p(out_scores.data_ptr()) if out_scores is not None else None))


def packed_result_block(B: int, k: int, device):
    """One contiguous device block [ids: B*k i64][dists: B*k f32] plus its two views: search results
    written through the views travel in ONE all-gather."""
    import torch
    block = torch.zeros((B * k * 12,), dtype=torch.uint8, device=device)
    ids = block[: B * k * 8].view(torch.int64).view(B, k)
    dists = block[B * k * 8:].view(torch.float32).view(B, k)
    return block, ids, dists


def merge_topk_packed_device(device: int, packed, G: int, B: int, k: int, out_ids, out_dists, out_scores,
                             stream: int | None = None) -> None:
    """packed: uint8 device tensor [G, B*k*12], shard blocks as laid out by packed_result_block.
    ``stream`` (raw hipStream_t): enqueue the merge there and return at once -- e.g. torch's current
    stream, right behind the all-gather; without it the call blocks until the merge is done."""
    args = (ctypes.c_void_p(packed.data_ptr()), int(G), int(B), int(k), ctypes.c_void_p(out_ids.data_ptr()),
            ctypes.c_void_p(out_dists.data_ptr()), ctypes.c_void_p(out_scores.data_ptr()) if out_scores is not None else None)
    if stream is None:
        check(lib().mx_topk_merge_packed_device(int(device), *args))
    else:
        check(lib().mx_topk_merge_packed_async(int(device), ctypes.c_void_p(stream), *args))
