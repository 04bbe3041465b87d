"""Host-side mirror of memex's vector-store surface, served by the HIP flat index.

Same names, argument meaning and error behaviour as the reference
(lib/libmemex/src/storage/mod.rs:17-139, lib/libmemex/src/storage/local.rs:21-166) so the parity
tests read like the reference's own tests (local.rs:168-243):

=====================  =======================================================================
reference              here
=====================  =======================================================================
``VectorData``         :class:`VectorData`                               (mod.rs:17-28)
``VectorStoreError``   :class:`VectorStoreError` + one subclass per variant (mod.rs:31-48)
``VectorStore`` trait  :class:`VectorStore` ABC                          (mod.rs:55-66)
``HnswStore``          :class:`HipFlatStore` (exact search on the GPU)   (local.rs:21-166)
``VectorStorage``      :class:`VectorStorage` (mutex wrapper)            (mod.rs:69-93)
``get_vector_storage`` :func:`get_vector_storage` (``hnsw://`` and ``hip://`` URIs) (mod.rs:95-139)
=====================  =======================================================================

The reference's methods are ``async`` (tokio); here they are plain blocking calls -- the C ABI
underneath is synchronous and the Rust shim of INTEGRATION.md wraps it in ``async fn`` again.
"""
from __future__ import annotations

import abc
import json
import os
import threading
from dataclasses import dataclass, field
from typing import Dict, List, Mapping, Sequence, Tuple
from urllib.parse import urlparse

import numpy as np

from . import _lib
from .index import FlatIndex

META_FILE = "vectors.meta.json"  # local.rs:19 -- same file name and JSON shape as the reference


@dataclass
class VectorData:
    """mod.rs:17-28."""
    _id: str
    document_id: str
    text: str
    vector: Sequence[float]
    segment_id: int = 0

    def to_json(self) -> dict:
        """The serialisation boundary (the reference writes the vector as JSON into the `embeddings` table:
        `vector.into()`, worker/tasks.rs:42-48): `vector` may be a numpy float32 row, which `json.dumps` refuses."""
        return {"_id": self._id, "document_id": self.document_id, "text": self.text,
                "vector": [float(x) for x in self.vector], "segment_id": int(self.segment_id)}


class VectorStoreError(Exception):
    """mod.rs:31-48; subclasses below are the enum variants."""


class ConnectionError_(VectorStoreError):
    pass


class DeleteError(VectorStoreError):
    pass


class FileIOError(VectorStoreError):
    pass


class InsertionError(VectorStoreError):
    pass


class SearchError(VectorStoreError):
    pass


class SerdeError(VectorStoreError):
    pass


class SaveError(VectorStoreError):
    pass


class Unsupported(VectorStoreError):
    pass


_STATUS_TO_ERROR = {
    _lib.MX_EINVAL: InsertionError,
    _lib.MX_EDEVICE: ConnectionError_,
    _lib.MX_EINSERT: InsertionError,
    _lib.MX_ESEARCH: SearchError,
    _lib.MX_EIO: FileIOError,
    _lib.MX_EUNSUPPORTED: Unsupported,
    _lib.MX_ENOMEM: InsertionError,
}


def _raise_from(e: _lib.MemexHipError, default=None):
    cls = _STATUS_TO_ERROR.get(e.code, default or VectorStoreError)
    if default is not None and e.code == _lib.MX_EINVAL:
        cls = default
    raise cls(e.msg) from e


VectorSearchResult = Tuple[str, float]  # (doc_id, score), mod.rs:51


class VectorStore(abc.ABC):
    """mod.rs:55-66."""

    @abc.abstractmethod
    def delete(self, id: str) -> None: ...

    @abc.abstractmethod
    def delete_all(self) -> None: ...

    @abc.abstractmethod
    def bulk_insert(self, data: Sequence[VectorData]) -> None: ...

    @abc.abstractmethod
    def insert(self, data: VectorData) -> None: ...

    @abc.abstractmethod
    def search(self, vec: Sequence[float], limit: int) -> List[VectorSearchResult]: ...


# Process-wide registry of resident stores, keyed by (real storage path, device).  The reference builds
# a store per request / per task (handlers.rs:61-63, worker/lib.rs:190) and pays a full reload each
# time (storage/mod.rs:115-116); here a collection that is already in HBM is attached in O(1): the
# SAME store object (GPU index + id map) is handed out as long as the files it last wrote / read are
# unchanged on disk.  (The Rust shim keeps the equivalent `HashMap<PathBuf, Arc<Mutex<HipFlatStore>>>`,
# INTEGRATION.md.)
_RESIDENT: Dict[tuple, "HipFlatStore"] = {}
_RESIDENT_MU = threading.Lock()


def _file_sig(path: str):
    try:
        st = os.stat(path)
        return (st.st_mtime_ns, st.st_size)
    except OSError:
        return None


def evict_resident(storage_path: str | None = None) -> None:
    """Drop resident stores (all, or the one for ``storage_path``): frees their HBM once unused."""
    with _RESIDENT_MU:
        for key in [k for k in _RESIDENT if storage_path is None or k[0] == os.path.realpath(str(storage_path))]:
            st = _RESIDENT.pop(key)
            with st._lock:      # a search in flight holds its own reference: the handle closes when that one goes
                st._index = None


def _rocchio_weights(beta: float, gamma: float, n_pos: int, n_neg: int) -> np.ndarray:
    """``search_like``'s example weights, f32 [n_pos + n_neg]: ``beta / n_pos`` then ``-gamma / n_neg``, each ONE f32 division of f32
    values -- what ``memex::HipFlatStore::search_like`` computes from its ``float`` parameters (a double division rounded afterwards
    differs from it by an ulp, e.g. for 0.15 / 5)."""
    pos = np.float32(beta) / np.float32(n_pos) if n_pos else np.float32(0)
    neg = -np.float32(gamma) / np.float32(n_neg) if n_neg else np.float32(0)
    return np.array([pos] * n_pos + [neg] * n_neg, dtype=np.float32)


class StoreFilter:
    """A resident filter of a ``HipFlatStore``, edited by ``_id`` string (``HipFlatStore.make_filter``)."""

    def __init__(self, store: "HipFlatStore", flt):
        self._store = store
        self._flt = flt

    def _edit(self, ids, allow: bool) -> None:
        with self._store._lock:
            rows = np.asarray(self._store._ids_named(ids), dtype=np.uint64)
            try:
                (self._flt.allow if allow else self._flt.deny)(ids=rows)
            except _lib.MemexHipError as e:
                _raise_from(e, SearchError)

    def allow(self, ids) -> None:
        """Add every row inserted under the given ``_id`` strings; unknown ones add nothing."""
        self._edit(ids, True)

    def deny(self, ids) -> None:
        """Take every row inserted under the given ``_id`` strings out of the set."""
        self._edit(ids, False)

    def _where(self, prior: "StorePrior", lo, hi, allow: bool) -> int:
        try:
            return (self._flt.allow_where if allow else self._flt.deny_where)(prior._pri, lo, hi)
        except _lib.MemexHipError as e:
            _raise_from(e, SearchError)

    def allow_where(self, prior: "StorePrior", lo: float = -np.inf, hi: float = np.inf) -> int:
        """Add every row whose value in ``prior`` lies in ``[lo, hi]`` (``IndexFilter.allow_where``): the device decides, the host
        needs no copy of the values.  Rows nobody set read 0.  -> rows selected."""
        return self._where(prior, lo, hi, True)

    def deny_where(self, prior: "StorePrior", lo: float = -np.inf, hi: float = np.inf) -> int:
        """Take every row whose value in ``prior`` lies in ``[lo, hi]`` out of the set.  -> rows selected."""
        return self._where(prior, lo, hi, False)

    def _documents(self, grouping: "StoreGrouping", documents, allow: bool) -> int:
        names = [documents] if isinstance(documents, str) else [str(d) for d in documents]
        with self._store._lock:  # a lookup only: an unknown name selects nothing and no key is handed out for it
            keys = [grouping._key_of[n] for n in dict.fromkeys(names) if n in grouping._key_of]
        try:
            return (self._flt.allow_keys if allow else self._flt.deny_keys)(grouping._grp, np.asarray(keys, dtype=np.uint32))
        except _lib.MemexHipError as e:
            _raise_from(e, SearchError)

    def allow_documents(self, grouping: "StoreGrouping", documents) -> int:
        """Add every segment ``grouping`` holds under one of the document names (``IndexFilter.allow_keys``): the host names
        documents, not their segments.  Unknown names add nothing.  -> rows selected."""
        return self._documents(grouping, documents, True)

    def deny_documents(self, grouping: "StoreGrouping", documents) -> int:
        """Take every segment ``grouping`` holds under one of the document names out of the set.  -> rows selected."""
        return self._documents(grouping, documents, False)

    def invert(self) -> None:
        """Replace the set by its complement within the rows the store holds at this moment (``IndexFilter.invert``)."""
        try:
            self._flt.invert()
        except _lib.MemexHipError as e:
            _raise_from(e, SearchError)

    def count(self):
        """-> (rows in the set, those of them that are not removed)."""
        try:
            return self._flt.count()
        except _lib.MemexHipError as e:
            _raise_from(e, SearchError)

    def close(self) -> None:
        self._flt.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class StoreGrouping:
    """Which segments of a ``HipFlatStore`` belong to which document (``HipFlatStore.make_grouping``): a resident grouping of the
    index, edited by document name and segment ``_id``.  Every document name gets a key 1, 2, ... the first time it is seen.  The
    grouping is not saved with the store: the host that owns the segment -> document mapping builds it again after a restart, and
    after ``compact()``, ``delete_all()`` or a reload, when every method but ``close`` raises."""

    def __init__(self, store: "HipFlatStore", grouping):
        self._store = store
        self._grp = grouping
        self._key_of: Dict[str, int] = {}
        self._name_of: Dict[int, str] = {}

    def key_of(self, document: str) -> int:
        """The key of a document name, handed out on first use."""
        name = str(document)
        key = self._key_of.get(name)
        if key is None:
            key = len(self._key_of) + 1
            if key > 0xFFFFFFFF:
                raise SearchError("a grouping holds at most 2^32 - 1 documents")
            self._key_of[name] = key
            self._name_of[key] = name
        return key

    def document_of(self, key: int) -> str | None:
        """The document name of a key; ``None`` for key 0 (ungrouped) or a key never handed out."""
        return self._name_of.get(int(key))

    def _set(self, pairs) -> None:
        """pairs: (key, segment _ids) -- one ``set_ids`` call for all of them (under the store's lock)."""
        rows: List[int] = []
        keys: List[int] = []
        for key, ids in pairs:
            named = self._store._ids_named(ids)
            rows.extend(named)
            keys.extend([key] * len(named))
        try:
            self._grp.set_ids(np.asarray(rows, dtype=np.uint64), np.asarray(keys, dtype=np.uint32))
        except _lib.MemexHipError as e:
            _raise_from(e, SearchError)

    def assign_all(self, documents) -> None:
        """``assign`` for a mapping document name -> segment ``_id``s, in one edit."""
        with self._store._lock:
            self._set([(self.key_of(doc), ids) for doc, ids in documents.items()])

    def assign(self, document: str, ids) -> None:
        """Put every row inserted under the given segment ``_id`` strings under ``document`` (ingest); unknown ones add nothing."""
        self.assign_all({document: ids})

    def release(self, ids) -> None:
        """Un-group every row inserted under the given segment ``_id`` strings (delete): each is a group of its own again."""
        with self._store._lock:
            self._set([(0, ids)])

    def count(self):
        """-> (rows under a document, those of them that are not removed)."""
        try:
            return self._grp.count()
        except _lib.MemexHipError as e:
            _raise_from(e, SearchError)

    def close(self) -> None:
        self._grp.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class StorePrior:
    """What a ``HipFlatStore``'s vectors do not say about its segments (``HipFlatStore.make_prior``): a resident prior of the index,
    edited by segment ``_id``, added to the score by ``search_boosted``.  Segments nobody set read 0.  The prior is not saved with
    the store: the host that owns the values builds it again after a restart, and after ``compact()``, ``delete_all()`` or a
    reload, when every method but ``close`` raises."""

    def __init__(self, store: "HipFlatStore", prior):
        self._store = store
        self._pri = prior

    def set(self, ids, values) -> None:
        """Every row inserted under segment ``ids[i]`` gets ``values[i]`` (one value per ``_id``, or one for all); unknown ``_id``s
        add nothing.  One ``set_ids`` call for all of them."""
        names = [ids] if isinstance(ids, str) else [str(i) for i in ids]
        vals = np.asarray(values, dtype=np.float32)
        vals = np.full(len(names), vals, dtype=np.float32) if vals.ndim == 0 else vals.reshape(-1)
        if vals.size != len(names):
            raise SearchError(f"expected {len(names)} values, got {vals.size}")
        rows: List[int] = []
        out: List[float] = []
        with self._store._lock:
            for name, v in zip(names, vals):
                named = self._store._ids_named([name])
                rows.extend(named)
                out.extend([v] * len(named))
            try:
                self._pri.set_ids(np.asarray(rows, dtype=np.uint64), np.asarray(out, dtype=np.float32))
            except _lib.MemexHipError as e:
                _raise_from(e, SearchError)

    def set_document(self, document_ids, value) -> None:
        """One value for all the segments of a document: ``set(document_ids, value)``."""
        self.set(list(document_ids), float(value))

    def bound(self, refresh: bool = False) -> float:
        """The upper bound of the values that ``complete`` is decided with (``IndexPrior.bound``)."""
        try:
            return self._pri.bound(refresh)
        except _lib.MemexHipError as e:
            _raise_from(e, SearchError)

    def close(self) -> None:
        self._pri.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


@dataclass
class HipFlatStore(VectorStore):
    """Drop-in for ``HnswStore``: same id map, same score formula, exact search on the GPU."""
    storage_path: str
    device: int = 0
    devices: Sequence[int] | None = None   # several GPUs: the in-library sharded index (mx_index_open_sharded)
    _id_map: Dict[int, str] = field(default_factory=dict)
    _index: FlatIndex | None = None
    _dim: int | None = None
    _lock: threading.RLock = field(default_factory=threading.RLock, repr=False, compare=False)
    _meta_sig: tuple | None = None          # (mtime_ns, size) of vectors.meta.json as last written / read
    _meta_ids: int = 0                      # ids that file holds
    _rows_of: Dict[str, List[int]] | None = field(default=None, repr=False, compare=False)  # _id -> ids (remove): built once, kept on insert

    # -- construction (local.rs:95-141) ----------------------------------------------------
    @classmethod
    def new(cls, storage_path: str, device: int = 0, devices: Sequence[int] | None = None) -> "HipFlatStore":
        store = cls(storage_path=str(storage_path), device=device, devices=devices)
        with _RESIDENT_MU:
            # a store this one replaces is NOT closed under its holders: earlier requests may still be inside
            # search() on it; its handle on the keyed GPU index goes away with its last reference
            _RESIDENT[store._rkey()] = store
        return store

    def _rkey(self) -> tuple:
        return (os.path.realpath(self.storage_path), int(self.device), tuple(int(d) for d in self.devices) if self.devices else None)

    @staticmethod
    def has_store(store_path: str) -> bool:
        return os.path.exists(os.path.join(str(store_path), META_FILE))  # local.rs:110-113

    @classmethod
    def load(cls, store_path: str, device: int = 0, devices: Sequence[int] | None = None) -> "HipFlatStore":
        store_path = str(store_path)
        meta = os.path.join(store_path, META_FILE)
        probe = cls(storage_path=store_path, device=device, devices=devices)
        with _RESIDENT_MU:
            res = _RESIDENT.get(probe._rkey())
        if res is not None:
            with res._lock:
                if res._meta_sig is not None and res._meta_sig == _file_sig(meta) and len(res._id_map) == res._meta_ids:
                    if not res._id_map:
                        return res
                    try:
                        res._index.load(store_path)      # O(1) when vectors.mxflat is what this index last wrote / read
                    except _lib.MemexHipError as e:
                        _raise_from(e)
                    if len(res._index) == len(res._id_map):
                        return res
        try:
            with open(meta, "r", encoding="utf-8") as f:
                raw = json.load(f)
        except OSError as e:
            raise FileIOError(str(e)) from e
        except ValueError as e:
            raise SerdeError(str(e)) from e
        store = probe
        try:
            store._id_map = {int(k): str(v) for k, v in raw.items()}
        except (AttributeError, ValueError) as e:
            raise SerdeError(str(e)) from e
        store._meta_sig = _file_sig(meta)
        store._meta_ids = len(store._id_map)
        store._rows_of = None
        if store._id_map:
            try:
                if not FlatIndex.has_store(store_path):
                    raise FileIOError(f"{store_path}: vector file missing")
                dim, _ = FlatIndex.store_info(store_path)
                store._open(dim)
                store._index.load(store_path)
            except _lib.MemexHipError as e:
                _raise_from(e)
            if len(store._index) != len(store._id_map):
                raise FileIOError(f"{store_path}: {len(store._index)} vectors vs {len(store._id_map)} ids")
        with _RESIDENT_MU:
            _RESIDENT[store._rkey()] = store     # (a replaced store keeps its handle for whoever still uses it)
        return store

    def save(self, store_path: str | None = None) -> None:
        """local.rs:143-165: vectors + ``vectors.meta.json`` (``{"<usize>": "<_id>"}``).  The reference
        calls this after EVERY insert (local.rs:67) and rewrites both files; here a save into the
        store's own directory appends: the index adds the new rows to ``vectors.mxflat``
        (``mx_index_save``) and the JSON object gets the new ``"id": "_id"`` pairs spliced in before
        its closing brace -- same file format, O(new rows) per insert."""
        store_path = str(store_path or self.storage_path)
        with self._lock:
            try:
                os.makedirs(store_path, exist_ok=True)
                if self._index is not None:
                    self._index.save(store_path)
                meta = os.path.join(store_path, META_FILE)
                own = os.path.realpath(store_path) == os.path.realpath(self.storage_path)
                n = len(self._id_map)
                appended = False
                if own and self._meta_sig is not None and self._meta_sig == _file_sig(meta) and 0 < self._meta_ids <= n:
                    appended = self._meta_ids == n or self._append_meta(meta, n)
                if not appended:
                    # full rewrite through a temporary file: the vectors are already on disk, so the id map must
                    # never be left shorter than them (also the way out of a file the splice does not recognise,
                    # e.g. one that a hand edit ended with a newline)
                    tmp = meta + ".tmp"
                    with open(tmp, "w", encoding="utf-8") as f:
                        json.dump({str(k): v for k, v in self._id_map.items()}, f)
                    os.replace(tmp, meta)
                if own:
                    self._meta_sig = _file_sig(meta)
                    self._meta_ids = n
            except _lib.MemexHipError as e:
                self._meta_sig = None
                raise SaveError(e.msg) from e
            except OSError as e:
                self._meta_sig = None
                raise FileIOError(str(e)) from e

    def _append_meta(self, meta: str, n: int) -> bool:
        """Splice ids _meta_ids+1 .. n in front of the closing brace of vectors.meta.json.  False = the file does
        not end the way this store left it (nothing written): the caller rewrites it."""
        tail = ",".join(f"{json.dumps(str(i))}: {json.dumps(self._id_map[i])}" for i in range(self._meta_ids + 1, n + 1))
        try:
            with open(meta, "r+b") as f:
                f.seek(-1, os.SEEK_END)
                if f.read(1) != b"}":
                    return False
                f.seek(-1, os.SEEK_END)
                f.write((", " + tail + "}").encode("utf-8"))
            return True
        except OSError:
            return False

    def _open(self, dim: int) -> None:
        # keyed by the collection's path: every handle on this collection shares ONE resident GPU index
        key = f"{os.path.realpath(self.storage_path)}@{'+'.join(map(str, self.devices)) if self.devices else self.device}"
        try:
            self._index = FlatIndex(dim, key=key, device=self.device, devices=self.devices)
        except _lib.MemexHipError as e:
            _raise_from(e)
        self._dim = dim

    # -- VectorStore (local.rs:27-92) -------------------------------------------------------
    def delete(self, id: str) -> None:
        # local.rs:29-32 is `unimplemented!()` (a panic); same contract, as an exception
        raise NotImplementedError("single-point delete is not supported (reference: unimplemented!())")

    def delete_all(self) -> None:
        with self._lock:
            for name in (META_FILE,):
                p = os.path.join(self.storage_path, name)
                if os.path.exists(p):
                    os.remove(p)
            try:
                FlatIndex.remove_files(self.storage_path)
                if self._index is not None:
                    self._index.clear()
            except _lib.MemexHipError as e:
                raise DeleteError(e.msg) from e
            self._id_map.clear()
            self._rows_of = None
            self._meta_sig = None
            self._meta_ids = 0

    def remove(self, ids: str | Sequence[str]) -> int:
        """Remove every row whose ``_id`` is in ``ids`` (rows inserted twice under one ``_id`` all go): the capability
        ``delete`` (local.rs:29-32, ``unimplemented!()``) lacks.  Tombstones: ids stay stable and ``vectors.meta.json``
        is unchanged; the removals are saved beside the store (``vectors.mxdead``) before this returns.  An unknown
        ``_id`` removes nothing (OpenSearch's delete of a missing document).  -> rows newly removed."""
        wanted = [ids] if isinstance(ids, str) else [str(i) for i in ids]
        with self._lock:
            if self._index is None or not self._id_map:
                return 0
            if self._rows_of is None:  # once per store: every later call looks its _ids up
                rows_of: Dict[str, List[int]] = {}
                for i, d_id in self._id_map.items():
                    rows_of.setdefault(d_id, []).append(i)
                self._rows_of = rows_of
            rows = [i for w in dict.fromkeys(wanted) for i in self._rows_of.get(w, ())]
            if not rows:
                return 0
            try:
                n = self._index.remove(rows)
            except _lib.MemexHipError as e:
                raise DeleteError(e.msg) from e
            try:
                self.save()
            except VectorStoreError as e:
                raise DeleteError(str(e)) from e
            return n

    def compact(self) -> np.ndarray:
        """Drop the rows ``remove`` took out for good (``FlatIndex.compact``): the live rows get dense ids again and
        ``_id_map`` is renumbered to match (new id -> the ``_id`` of the id it replaces).  Saved before this returns, like
        ``remove``: the index rewrites ``vectors.mxflat`` whole, then ``vectors.meta.json`` is rewritten through a
        temporary file.  A crash between the two leaves an id map longer than the vectors (a compaction that removed
        anything always shortens the store), which ``load`` rejects with ``FileIOError``: never a wrong id -> ``_id``
        mapping.  Nothing removed: a no-op.  -> uint64 array, the id every new id had before."""
        with self._lock:
            if self._index is None or not self._id_map:
                return np.zeros(0, dtype=np.uint64)
            if self._index.removed == 0:
                return np.arange(1, len(self._id_map) + 1, dtype=np.uint64)
            try:
                kept = self._index.compact()
            except _lib.MemexHipError as e:
                raise DeleteError(e.msg) from e
            self._id_map = {i + 1: self._id_map[int(old)] for i, old in enumerate(kept)}
            self._rows_of = None
            self._meta_sig = None   # the id map is rewritten whole, never appended to
            self._meta_ids = 0
            try:
                self.save()
            except VectorStoreError as e:
                raise DeleteError(str(e)) from e
            return kept

    def bulk_insert(self, data: Sequence[VectorData]) -> None:
        """local.rs:55-69 semantics (ids in order, store persisted before returning), one device
        transfer and one incremental save instead of a save per vector."""
        if not data:
            return
        rows = np.asarray([np.asarray(d.vector, dtype=np.float32) for d in data], dtype=np.float32)
        if rows.ndim != 2:
            raise InsertionError("vectors of one bulk_insert must share a dimension")
        with self._lock:
            if self._index is None:
                self._open(rows.shape[1])
                if len(self._index) != len(self._id_map):   # a stale resident index under this key
                    self._index.clear()
            if rows.shape[1] != self._dim:
                raise InsertionError(f"vector dimension {rows.shape[1]} != store dimension {self._dim}")
            try:
                first = self._index.add(rows)
            except _lib.MemexHipError as e:
                _raise_from(e, InsertionError)
            next_id = len(self._id_map) + 1  # local.rs:63
            assert first == next_id, (first, next_id)
            for i, d in enumerate(data):
                self._id_map[next_id + i] = str(d._id)
                if self._rows_of is not None:
                    self._rows_of.setdefault(str(d._id), []).append(next_id + i)
            try:
                self.save()  # local.rs:67 `let _ = self.save(..)`: errors are ignored there too
            except VectorStoreError:
                pass

    def insert(self, data: VectorData) -> None:
        self.bulk_insert([data])

    def search_within(self, vec: Sequence[float], limit: int, ids: Sequence[str]) -> List[VectorSearchResult]:
        """``search`` restricted to the rows inserted under the given ``_id`` strings (one document's segments, one tenant's
        rows): the exact top-``limit`` among them (``FlatIndex.search_filtered``), as ``(_id, score)`` pairs like ``search``.
        A document's segments are inserted in one call, so a handful of documents is a handful of id ranges.  An unknown
        ``_id`` selects nothing."""
        wanted = [ids] if isinstance(ids, str) else [str(i) for i in ids]
        with self._lock:
            idx = self._index
            if idx is None or limit <= 0 or not self._id_map:
                return []
            if self._rows_of is None:  # the map remove() builds: once per store, kept on insert
                rows_of: Dict[str, List[int]] = {}
                for i, d_id in self._id_map.items():
                    rows_of.setdefault(d_id, []).append(i)
                self._rows_of = rows_of
            allow = [i for w in dict.fromkeys(wanted) for i in self._rows_of.get(w, ())]
        q = np.asarray(vec, dtype=np.float32)
        if q.shape != (self._dim,):
            raise SearchError(f"query dimension {q.shape} != store dimension {self._dim}")
        try:
            ids_, scores, _, nf = idx.search_filtered(q, int(limit), ids=allow)  # not under the lock: combined like search
        except _lib.MemexHipError as e:
            _raise_from(e, SearchError)
        out: List[VectorSearchResult] = []
        with self._lock:
            for j in range(int(nf[0])):
                d_id = int(ids_[0, j])
                if d_id not in self._id_map:
                    raise SearchError("Internal inconsistency. Id from vector store not mapped.")
                out.append((self._id_map[d_id], float(scores[0, j])))
        return out

    def _ids_named(self, ids) -> List[int]:
        """The index ids inserted under the given ``_id`` strings (under the lock)."""
        wanted = [ids] if isinstance(ids, str) else [str(i) for i in ids]
        rows_of = self._rows_by_name()
        return [i for w in dict.fromkeys(wanted) for i in rows_of.get(w, ())]

    def make_filter(self, ids: Sequence[str] = ()) -> "StoreFilter":
        """A resident filter over the rows inserted under the given ``_id`` strings (``FlatIndex.make_filter``): one tenant's,
        one ACL group's or one tag's documents, registered once and named in every ``search_in``.  Bulk-inserting a document
        and then ``flt.allow([its _ids])`` is the tenant-ingest flow; ``flt.deny`` takes documents out.  After ``compact()``,
        ``delete_all()`` or a reload the filter raises: make a new one.  The store must hold at least one row."""
        with self._lock:
            if self._index is None:
                raise SearchError("a filter needs a store with rows: insert first")
            try:
                flt = StoreFilter(self, self._index.make_filter())
                flt.allow(ids)
            except _lib.MemexHipError as e:
                _raise_from(e, SearchError)
        return flt

    def combine_filters(self, a: "StoreFilter", b: "StoreFilter", op, out: "StoreFilter | None" = None) -> "StoreFilter":
        """``out = a op b`` over the rows (``FlatIndex.combine_filters``): ``op`` is "and", "or", "andnot" (``a`` and not ``b``) or
        "xor".  ``out`` may be ``a`` or ``b``; None makes a new filter.  -> ``out``."""
        with self._lock:
            idx = self._index
        if idx is None:
            raise SearchError("a filter needs a store with rows: insert first")
        try:
            res = idx.combine_filters(a._flt, b._flt, op, out._flt if out is not None else None)
        except _lib.MemexHipError as e:
            _raise_from(e, SearchError)
        return out if out is not None else StoreFilter(self, res)

    def search_in(self, vec: Sequence[float], limit: int, flt: "StoreFilter") -> List[VectorSearchResult]:
        """``search`` restricted to the rows of a resident filter (``FlatIndex.search_with``), as ``(_id, score)`` pairs."""
        with self._lock:
            idx = self._index
        if idx is None or limit <= 0:
            return []
        q = np.asarray(vec, dtype=np.float32)
        if q.shape != (self._dim,):
            raise SearchError(f"query dimension {q.shape} != store dimension {self._dim}")
        try:
            ids_, scores, _, nf = idx.search_with(flt._flt, q, int(limit))  # not under the lock: combined like search
        except _lib.MemexHipError as e:
            _raise_from(e, SearchError)
        out: List[VectorSearchResult] = []
        with self._lock:
            for j in range(int(nf[0])):
                d_id = int(ids_[0, j])
                if d_id not in self._id_map:
                    raise SearchError("Internal inconsistency. Id from vector store not mapped.")
                out.append((self._id_map[d_id], float(scores[0, j])))
        return out

    def search_above(self, vec: Sequence[float], min_score: float, limit: int) -> List[VectorSearchResult]:
        """Every row whose score against ``vec`` is at least ``min_score``, best first, at most ``limit`` (1 .. 4096) of them
        (``FlatIndex.search_range``), as ``(_id, score)`` pairs like ``search``: a near-duplicate check before ingest, or context
        chosen by relevance rather than by count.  Removed rows never appear."""
        with self._lock:
            idx = self._index
        if idx is None or limit <= 0:
            return []
        q = np.asarray(vec, dtype=np.float32)
        if q.shape != (self._dim,):
            raise SearchError(f"query dimension {q.shape} != store dimension {self._dim}")
        try:
            ids, scores, _, nf, _ = idx.search_range(q, float(min_score), int(limit))  # not under the lock: combined like search
        except _lib.MemexHipError as e:
            _raise_from(e, SearchError)
        out: List[VectorSearchResult] = []
        with self._lock:
            for j in range(int(nf[0])):
                d_id = int(ids[0, j])
                if d_id not in self._id_map:
                    raise SearchError("Internal inconsistency. Id from vector store not mapped.")
                out.append((self._id_map[d_id], float(scores[0, j])))
        return out

    def search_diverse(self, vec: Sequence[float], limit: int, fetch: int | None = None, lam: float = 0.5) -> List[VectorSearchResult]:
        """The ``limit`` most relevant rows that do not repeat each other (``FlatIndex.search_mmr``: exact MMR re-ranking of the
        top-``fetch`` rows), as ``(_id, score)`` pairs in selection order: context for a prompt without the same passage from
        several overlapping windows.  ``lam = 1`` is ``search``.  Removed rows never appear."""
        with self._lock:
            idx = self._index
        if idx is None or limit <= 0:
            return []
        q = np.asarray(vec, dtype=np.float32)
        if q.shape != (self._dim,):
            raise SearchError(f"query dimension {q.shape} != store dimension {self._dim}")
        try:
            ids, scores, _, nf = idx.search_mmr(q, int(limit), fetch, float(lam))  # not under the lock, like search
        except _lib.MemexHipError as e:
            _raise_from(e, SearchError)
        out: List[VectorSearchResult] = []
        with self._lock:
            for j in range(int(nf[0])):
                d_id = int(ids[0, j])
                if d_id not in self._id_map:
                    raise SearchError("Internal inconsistency. Id from vector store not mapped.")
                out.append((self._id_map[d_id], float(scores[0, j])))
        return out

    def search_fused(self, vecs: Sequence[Sequence[float]], limit: int, mode: str = "max", fetch: int | None = None,
                     weights: Sequence[float] | None = None) -> List[VectorSearchResult]:
        """One ranked list for SEVERAL query vectors -- the phrasings of a question, a question and a hypothetical answer, the last
        turns of a conversation (``FlatIndex.search_fused``) -- as ``(_id, score)`` pairs, each row once with the score of its best
        vector.  ``mode="max"``: the exact top-``limit`` by the best score over the vectors; ``"rrf"``: reciprocal-rank fusion of
        their top-``fetch`` lists.  ``weights``: one per vector, 0 leaves the vector out.  Removed rows never appear."""
        with self._lock:
            idx = self._index
        if idx is None or limit <= 0 or len(vecs) == 0:
            return []
        try:
            q = np.asarray(vecs, dtype=np.float32)
        except ValueError as e:                               # vectors of different lengths: a dimension mismatch like any other
            raise SearchError(f"query vectors of different dimensions: {e}") from e
        if q.ndim != 2 or q.shape[1] != self._dim:
            raise SearchError(f"query dimension {q.shape} != [m, store dimension {self._dim}]")
        try:
            ids, scores, _, nf, _, _ = idx.search_fused(q, int(limit), mode, fetch, weights)  # not under the lock, like search
        except _lib.MemexHipError as e:
            _raise_from(e, SearchError)
        out: List[VectorSearchResult] = []
        with self._lock:
            for j in range(int(nf[0])):
                d_id = int(ids[0, j])
                if d_id not in self._id_map:
                    raise SearchError("Internal inconsistency. Id from vector store not mapped.")
                out.append((self._id_map[d_id], float(scores[0, j])))
        return out

    def make_grouping(self, documents: Mapping[str, Sequence[str]] = {}) -> "StoreGrouping":  # noqa: B006 (read only)
        """A resident grouping (``FlatIndex.make_grouping``) with the segments of ``documents`` -- document name -> the segment
        ``_id``s under it -- grouped, every other row a group of its own.  Bulk-inserting a document and then
        ``grouping.assign(document, [its _ids])`` is the ingest flow; ``grouping.release`` takes segments out.  After ``compact()``,
        ``delete_all()`` or a reload the grouping raises: make a new one.  The store must hold at least one row."""
        with self._lock:
            if self._index is None:
                raise SearchError("a grouping needs a store with rows: insert first")
            try:
                grp = StoreGrouping(self, self._index.make_grouping())
            except _lib.MemexHipError as e:
                _raise_from(e, SearchError)
            try:
                if documents:
                    grp.assign_all(documents)
            except Exception:
                grp.close()
                raise
        return grp

    def search_documents(self, vec: Sequence[float], limit: int, grouping: "StoreGrouping", fetch: int | None = None,
                         flt: "StoreFilter | None" = None) -> Tuple[List[Tuple[str | None, str, float, int]], bool]:
        """The ``limit`` best DOCUMENTS for ``vec``, each by its best segment (``FlatIndex.search_grouped``) -> ``(hits, complete)``.
        Each hit is ``(document name or None for an ungrouped segment, best segment _id, score, group_rows)``, best first;
        ``group_rows`` counts the document's segments among the candidates looked at.  ``complete``: the hits are the exact top
        documents over the whole store (over ``flt``'s rows when given).  The candidates are the top-``fetch`` rows; when that
        answer is not complete the call asks ONCE more with 4096 candidates, so ``complete`` is false only for a store where even
        those hold fewer than ``limit`` documents.  Removed rows never appear."""
        with self._lock:
            idx = self._index
        if idx is None or limit <= 0:
            return [], True
        q = np.asarray(vec, dtype=np.float32)
        if q.shape != (self._dim,):
            raise SearchError(f"query dimension {q.shape} != store dimension {self._dim}")
        f = flt._flt if flt is not None else None
        first = FlatIndex._grouped_fetch(int(limit), fetch)
        try:
            ids, scores, _, keys, rows, nf, done = idx.search_grouped(grouping._grp, q, int(limit), first, f)  # not under the lock
            if not done[0] and first < 4096:
                ids, scores, _, keys, rows, nf, done = idx.search_grouped(grouping._grp, q, int(limit), 4096, f)
        except _lib.MemexHipError as e:
            _raise_from(e, SearchError)
        out: List[Tuple[str | None, str, float, int]] = []
        with self._lock:
            for j in range(int(nf[0])):
                d_id = int(ids[0, j])
                if d_id not in self._id_map:
                    raise SearchError("Internal inconsistency. Id from vector store not mapped.")
                out.append((grouping.document_of(int(keys[0, j])), self._id_map[d_id], float(scores[0, j]), int(rows[0, j])))
        return out, bool(done[0])

    def _one_query(self, vec: Sequence[float]) -> np.ndarray:
        q = np.asarray(vec, dtype=np.float32)
        if q.shape != (self._dim,):
            raise SearchError(f"query dimension {q.shape} != store dimension {self._dim}")
        return q

    def search_document_passages(self, vec: Sequence[float], limit: int, grouping: "StoreGrouping", passages: int = 3,
                                 fetch: int | None = None, flt: "StoreFilter | None" = None
                                 ) -> Tuple[List[Tuple[str | None, List[VectorSearchResult], bool]], bool]:
        """The ``limit`` best DOCUMENTS for ``vec``, each with its ``passages`` best segments (``FlatIndex.search_group_rows``) ->
        ``(hits, complete)``.  Each hit is ``(document name or None for an ungrouped segment, [(segment _id, score), ...] best first,
        members_complete)``; the first passage is the segment ``search_documents`` reports.  The passages of a hit are always the
        exact best ones of their document; ``members_complete`` says the document has no further segment that belongs among its
        first ``passages``.  ``complete``: the documents are the exact top documents over the whole store (over ``flt``'s rows when
        given).  When that is false the call asks ONCE more with 4096 candidates, as ``search_documents`` does."""
        with self._lock:
            idx = self._index
        if idx is None or limit <= 0 or passages <= 0:
            return [], True
        q = self._one_query(vec)
        f = flt._flt if flt is not None else None
        k, n = int(limit), int(passages)
        first = FlatIndex._group_rows_fetch(k, n, fetch)
        try:
            ids, scores, _, keys, _, mem, mdone, nf, done = idx.search_group_rows(grouping._grp, q, k, n, first, f)  # not under the lock
            if not done[0] and first < 4096:
                ids, scores, _, keys, _, mem, mdone, nf, done = idx.search_group_rows(grouping._grp, q, k, n, 4096, f)
        except _lib.MemexHipError as e:
            _raise_from(e, SearchError)
        out: List[Tuple[str | None, List[VectorSearchResult], bool]] = []
        with self._lock:
            for j in range(int(nf[0])):
                rows: List[VectorSearchResult] = []
                for r in range(int(mem[0, j])):
                    d_id = int(ids[0, j, r])
                    if d_id not in self._id_map:
                        raise SearchError("Internal inconsistency. Id from vector store not mapped.")
                    rows.append((self._id_map[d_id], float(scores[0, j, r])))
                out.append((grouping.document_of(int(keys[0, j])), rows, bool(mdone[0, j])))
        return out, bool(done[0])

    def search_spread(self, vec: Sequence[float], limit: int, grouping: "StoreGrouping", per_document: int = 2,
                      fetch: int | None = None, flt: "StoreFilter | None" = None) -> Tuple[List[Tuple[str | None, str, float]], bool]:
        """The ``limit`` best segments for ``vec`` with at most ``per_document`` segments of any one document
        (``FlatIndex.search_capped``) -> ``(hits, complete)``.  Each hit is ``(document name or None, segment _id, score)``, best
        first: a flat list.  ``complete``: the hits are the exact capped top segments over the whole store (over ``flt``'s rows when
        given); when that is false the call asks ONCE more with 4096 candidates, as ``search_documents`` does."""
        with self._lock:
            idx = self._index
        if idx is None or limit <= 0 or per_document <= 0:
            return [], True
        q = self._one_query(vec)
        f = flt._flt if flt is not None else None
        first = FlatIndex._grouped_fetch(int(limit), fetch)
        try:
            ids, scores, _, keys, nf, done = idx.search_capped(grouping._grp, q, int(limit), int(per_document), first, f)  # not under the lock
            if not done[0] and first < 4096:
                ids, scores, _, keys, nf, done = idx.search_capped(grouping._grp, q, int(limit), int(per_document), 4096, f)
        except _lib.MemexHipError as e:
            _raise_from(e, SearchError)
        out: List[Tuple[str | None, str, float]] = []
        with self._lock:
            for j in range(int(nf[0])):
                d_id = int(ids[0, j])
                if d_id not in self._id_map:
                    raise SearchError("Internal inconsistency. Id from vector store not mapped.")
                out.append((grouping.document_of(int(keys[0, j])), self._id_map[d_id], float(scores[0, j])))
        return out, bool(done[0])

    def make_prior(self) -> "StorePrior":
        """A resident prior (``FlatIndex.make_prior``), 0 for every segment.  Bulk-inserting a document and then
        ``prior.set_document([its _ids], value)`` is the ingest flow.  After ``compact()``, ``delete_all()`` or a reload the prior
        raises: make a new one.  The store must hold at least one row."""
        with self._lock:
            if self._index is None:
                raise SearchError("a prior needs a store with rows: insert first")
            try:
                return StorePrior(self, self._index.make_prior())
            except _lib.MemexHipError as e:
                _raise_from(e, SearchError)

    def search_boosted(self, vec: Sequence[float], limit: int, prior: "StorePrior", weight: float = 1.0, fetch: int | None = None,
                       flt: "StoreFilter | None" = None) -> Tuple[List[Tuple[str, float, float, float]], bool]:
        """The ``limit`` best segments for ``vec`` by ``score + weight * prior`` (``FlatIndex.search_boosted``) -> ``(hits,
        complete)``.  Each hit is ``(segment _id, score, prior, combined)``, best first.  ``complete``: the hits are the exact top
        segments over the whole store (over ``flt``'s rows when given).  The candidates are the top-``fetch`` rows; when that answer
        is not complete the call asks ONCE more with 4096 candidates.  Removed rows never appear."""
        with self._lock:
            idx = self._index
        if idx is None or limit <= 0:
            return [], True
        q = np.asarray(vec, dtype=np.float32)
        if q.shape != (self._dim,):
            raise SearchError(f"query dimension {q.shape} != store dimension {self._dim}")
        f = flt._flt if flt is not None else None
        first = FlatIndex._grouped_fetch(int(limit), fetch)
        try:
            ids, scores, _, priors, comb, nf, done = idx.search_boosted(prior._pri, q, int(limit), weight, first, f)  # not under the lock
            if not done[0] and first < 4096:
                ids, scores, _, priors, comb, nf, done = idx.search_boosted(prior._pri, q, int(limit), weight, 4096, f)
        except _lib.MemexHipError as e:
            _raise_from(e, SearchError)
        out: List[Tuple[str, float, float, float]] = []
        with self._lock:
            for j in range(int(nf[0])):
                d_id = int(ids[0, j])
                if d_id not in self._id_map:
                    raise SearchError("Internal inconsistency. Id from vector store not mapped.")
                out.append((self._id_map[d_id], float(scores[0, j]), float(priors[0, j]), float(comb[0, j])))
        return out, bool(done[0])

    def _rows_by_name(self) -> Dict[str, List[int]]:
        """(under the lock) ``_id`` -> the ids stored under it: built once per store, kept on insert."""
        if self._rows_of is None:
            rows_of: Dict[str, List[int]] = {}
            for i, d_id in self._id_map.items():
                rows_of.setdefault(d_id, []).append(i)
            self._rows_of = rows_of
        return self._rows_of

    def more_like(self, _id: str, limit: int) -> List[VectorSearchResult]:
        """More like this: the ``limit`` entries closest to what is stored under ``_id``, as ``(_id, score)`` pairs like ``search``,
        the asked ``_id`` itself left out.  Every row stored under ``_id`` is a query (``FlatIndex.search_by_id``: the rows never
        leave the device); the union of their answers is ranked by best score, each row once.  An unknown ``_id``, or one whose
        rows were all removed, returns ``[]``.  ``limit`` + the rows under ``_id`` may not exceed 4095 (the lists the device
        returns hold that many entries and the rows under ``_id`` take up places in them): ``Unsupported`` beyond."""
        with self._lock:
            idx = self._index
            if idx is None or limit <= 0 or not self._id_map:
                return []
            mine = list(self._rows_by_name().get(str(_id), ()))
        if not mine:
            return []
        if int(limit) + len(mine) > 4095:
            raise Unsupported(f"more_like: limit {int(limit)} + {len(mine)} rows under the _id exceeds 4095")
        try:
            # limit + the rows under _id: they are the only entries dropped below, so `limit` others are among them
            ids, scores, dists, nf = idx.search_by_id(mine, int(limit) + len(mine), exclude_self=True)
        except _lib.MemexHipError as e:
            _raise_from(e, SearchError)
        own = set(mine)
        best: Dict[int, Tuple[float, float]] = {}
        for b in range(len(mine)):
            for j in range(int(nf[b])):
                r = int(ids[b, j])
                if r in own:
                    continue
                key = (float(dists[b, j]), float(scores[b, j]))
                if r not in best or key < best[r]:
                    best[r] = key
        ranked = sorted(best.items(), key=lambda kv: (kv[1][0], kv[0]))[: int(limit)]     # (dist, id): the order search reports
        out: List[VectorSearchResult] = []
        with self._lock:
            for r, (_, score) in ranked:
                if r not in self._id_map:
                    raise SearchError("Internal inconsistency. Id from vector store not mapped.")
                out.append((self._id_map[r], score))
        return out

    def search_like(self, positive: Sequence[str], negative: Sequence[str] = (), limit: int = 10, vec: Sequence[float] | None = None,
                    alpha: float = 1.0, beta: float = 0.75, gamma: float = 0.15) -> List[VectorSearchResult]:
        """Relevance feedback (Rocchio) over segment ``_id``s: more like ``positive``, less like ``negative``, as ``(_id, score)``
        pairs like ``search``, the named segments themselves left out.  Every row stored under a named ``_id`` is an example
        (``FlatIndex.search_like``: the rows never leave the device), scaled to unit length and weighted ``beta / n_pos_rows``
        (positive) or ``-gamma / n_neg_rows`` (negative); ``vec``, the query the feedback is about, weighs ``alpha``.  Unknown
        ``_id``s are ignored; more than 16 rows in all raise ``ValueError``.  No example row and no ``vec`` returns ``[]``.  A row that
        was removed but not compacted away yet still counts in ``n_pos_rows`` / ``n_neg_rows``; it takes no part in the blend.
        The weights are f32 divisions of the f32 values of ``beta`` and ``gamma`` (``np.float32(beta) / np.float32(n_pos_rows)``): the
        C ABI takes ``float`` weights and the C++ and Rust callers hold ``f32`` parameters, so every host sends the same bits."""
        with self._lock:
            idx = self._index
            if idx is None or limit <= 0 or not self._id_map:
                return []
            by_name = self._rows_by_name()
            pos = [r for n in positive for r in by_name.get(str(n), ())]
            neg = [r for n in negative for r in by_name.get(str(n), ())]
        if len(pos) + len(neg) > 16:
            raise ValueError(f"{len(pos) + len(neg)} example rows: at most 16 per request")
        q = None
        if vec is not None:
            q = np.asarray(vec, dtype=np.float32)
            if q.shape != (self._dim,):
                raise SearchError(f"query dimension {q.shape} != store dimension {self._dim}")
        if not pos and not neg and q is None:
            return []
        ex = np.array(pos + neg if pos or neg else [0], dtype=np.uint64)
        w = _rocchio_weights(beta, gamma, len(pos), len(neg)) if pos or neg else np.zeros(1, dtype=np.float32)
        try:
            ids, scores, _, nf, _, _ = idx.search_like(ex, int(limit), w, q, None if q is None else float(alpha))  # not under the lock, like search
        except _lib.MemexHipError as e:
            _raise_from(e, SearchError)
        out: List[VectorSearchResult] = []
        with self._lock:
            for j in range(int(nf[0])):
                d_id = int(ids[0, j])
                if d_id not in self._id_map:
                    raise SearchError("Internal inconsistency. Id from vector store not mapped.")
                out.append((self._id_map[d_id], float(scores[0, j])))
        return out

    def rerank(self, vec: Sequence[float], ids: Sequence[str], limit: int | None = None) -> List[VectorSearchResult]:
        """Score the named segments against ``vec`` and rank them: the hits of a keyword backend, a cached result page, a caller's
        own working set, as ``(_id, score)`` pairs like ``search``, best first, cut to ``limit`` (None: all of them).  Every row
        stored under a named ``_id`` is a candidate (``FlatIndex.score_ids``: exact scores, the rows never leave the device); a
        segment is ranked by its best row, in the (dist, id) order ``search`` reports, and listed once.  Names the store does not
        know, and segments whose rows were all removed, are skipped."""
        with self._lock:
            idx = self._index
            if idx is None or not self._id_map or (limit is not None and limit <= 0):
                return []
            by_name = self._rows_by_name()
            rows = list(dict.fromkeys(r for n in ids for r in by_name.get(str(n), ())))
        if not rows:
            return []
        q = np.asarray(vec, dtype=np.float32)
        if q.shape != (self._dim,):
            raise SearchError(f"query dimension {q.shape} != store dimension {self._dim}")
        cap = 4096                                                    # ids per list: longer candidate sets go as several lists
        lists = [rows[i:i + cap] for i in range(0, len(rows), cap)]
        try:
            scores, dists, order, nf = idx.score_ids(np.broadcast_to(q, (len(lists), self._dim)), lists)  # not under the lock, like search
        except _lib.MemexHipError as e:
            _raise_from(e, SearchError)
        found = [(float(dists[b, j]), lists[b][j], float(scores[b, j])) for b in range(len(lists)) for j in order[b, :int(nf[b])]]
        if len(lists) > 1:
            found.sort(key=lambda e: (e[0], e[1]))
        out: List[VectorSearchResult] = []
        seen = set()
        with self._lock:
            for _, r, score in found:
                if r not in self._id_map:
                    raise SearchError("Internal inconsistency. Id from vector store not mapped.")
                name = self._id_map[r]
                if name in seen:
                    continue
                seen.add(name)
                out.append((name, score))
                if limit is not None and len(out) >= int(limit):
                    break
        return out

    def find_duplicates(self, min_score: float, per_row: int = 64) -> Tuple[List[Tuple[str, str, float]], List[str]]:
        """The rows of the collection that repeat each other: every pair of live rows whose score reaches ``min_score``
        (``FlatIndex.near_duplicates``, an exact self-join on the device) -> (``(_id_a, _id_b, score)`` per pair, in id order;
        the ``_id`` of every row with more than ``per_row`` rows in range).  A pair is missing only if both of its rows are
        in the second list; raise ``per_row`` (at most 4095) for those.  Hand one end of each pair to ``remove``."""
        with self._lock:
            idx = self._index
            if idx is None or not self._id_map:
                return [], []
        try:
            pairs, scores, truncated = idx.near_duplicates(float(min_score), int(per_row))
        except _lib.MemexHipError as e:
            _raise_from(e, SearchError)
        with self._lock:
            for r in list(pairs.reshape(-1)) + list(truncated):
                if int(r) not in self._id_map:
                    raise SearchError("Internal inconsistency. Id from vector store not mapped.")
            return ([(self._id_map[int(a)], self._id_map[int(b)], float(s)) for (a, b), s in zip(pairs, scores)],
                    [self._id_map[int(r)] for r in truncated])

    def search(self, vec: Sequence[float], limit: int) -> List[VectorSearchResult]:
        with self._lock:
            idx = self._index        # own reference: the store may be evicted / replaced while the GPU works
        if idx is None or limit <= 0:
            return []
        q = np.asarray(vec, dtype=np.float32)
        if q.shape != (self._dim,):
            raise SearchError(f"query dimension {q.shape} != store dimension {self._dim}")
        try:
            ids, scores, _, nf = idx.search(q, int(limit))      # not under the lock: concurrent callers are combined
        except _lib.MemexHipError as e:
            _raise_from(e, SearchError)
        out: List[VectorSearchResult] = []
        with self._lock:
            for j in range(int(nf[0])):
                d_id = int(ids[0, j])
                if d_id not in self._id_map:  # local.rs:80-83 panics here; we raise
                    raise SearchError("Internal inconsistency. Id from vector store not mapped.")
                out.append((self._id_map[d_id], float(scores[0, j])))
        return out


class VectorStorage:
    """mod.rs:69-93: a mutex around a ``VectorStore``."""

    def __init__(self, client: VectorStore):
        self.client = client
        self._mu = threading.Lock()

    def add_vectors(self, points: Sequence[VectorData]) -> None:
        with self._mu:
            self.client.bulk_insert(points)

    def delete_collection(self) -> None:
        with self._mu:
            self.client.delete_all()

    def search(self, query: Sequence[float], limit: int) -> List[VectorSearchResult]:
        with self._mu:
            return self.client.search(query, limit)

    def search_fused(self, queries: Sequence[Sequence[float]], limit: int, mode: str = "max", fetch: int | None = None,
                     weights: Sequence[float] | None = None) -> List[VectorSearchResult]:
        with self._mu:
            return self.client.search_fused(queries, limit, mode, fetch, weights)

    def search_documents(self, query: Sequence[float], limit: int, grouping: "StoreGrouping", fetch: int | None = None,
                         flt: "StoreFilter | None" = None):
        with self._mu:
            return self.client.search_documents(query, limit, grouping, fetch, flt)

    def search_document_passages(self, query: Sequence[float], limit: int, grouping: "StoreGrouping", passages: int = 3,
                                 fetch: int | None = None, flt: "StoreFilter | None" = None):
        with self._mu:
            return self.client.search_document_passages(query, limit, grouping, passages, fetch, flt)

    def search_spread(self, query: Sequence[float], limit: int, grouping: "StoreGrouping", per_document: int = 2,
                      fetch: int | None = None, flt: "StoreFilter | None" = None):
        with self._mu:
            return self.client.search_spread(query, limit, grouping, per_document, fetch, flt)

    def search_boosted(self, query: Sequence[float], limit: int, prior: "StorePrior", weight: float = 1.0, fetch: int | None = None,
                       flt: "StoreFilter | None" = None):
        with self._mu:
            return self.client.search_boosted(query, limit, prior, weight, fetch, flt)

    def search_like(self, positive: Sequence[str], negative: Sequence[str] = (), limit: int = 10, vec: Sequence[float] | None = None,
                    alpha: float = 1.0, beta: float = 0.75, gamma: float = 0.15) -> List[VectorSearchResult]:
        with self._mu:
            return self.client.search_like(positive, negative, limit, vec, alpha, beta, gamma)

    def rerank(self, vec: Sequence[float], ids: Sequence[str], limit: int | None = None) -> List[VectorSearchResult]:
        with self._mu:
            return self.client.rerank(vec, ids, limit)


def get_vector_storage(uri: str, collection: str, device: int = 0, devices: Sequence[int] | None = None) -> VectorStorage:
    """mod.rs:95-139.  ``hnsw://<dir>`` (the reference's file backend, now served from HBM) and
    ``hip://<dir>`` select the GPU store; collections are folders under ``<dir>``.  Called per
    request like the reference's; a collection that is already resident is attached, not reloaded."""
    try:
        scheme = urlparse(uri).scheme
    except ValueError:
        raise Unsupported(uri)
    if not scheme:
        raise Unsupported(uri)
    if scheme in ("hnsw", "hip"):
        storage = os.path.join(uri[len(scheme) + 3:], collection)
        try:
            os.makedirs(storage, exist_ok=True)
        except OSError as e:
            raise FileIOError(str(e)) from e
        if HipFlatStore.has_store(storage):
            store = HipFlatStore.load(storage, device, devices)
        else:
            probe = HipFlatStore(storage_path=storage, device=device, devices=devices)
            with _RESIDENT_MU:
                res = _RESIDENT.get(probe._rkey())
            # an empty resident store (created by an earlier request, nothing inserted yet) is reused
            store = res if res is not None and not res._id_map else HipFlatStore.new(storage, device, devices)
        return VectorStorage(store)
    # opensearch+https:// is a remote-service client in the reference (mod.rs:122-133): out of scope
    raise Unsupported(uri)
