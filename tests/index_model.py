"""A host model of the whole index (memex_amd.index.FlatIndex with its resident filters and groupings) -- TEST INFRASTRUCTURE, not
product code.  It makes no library call: every answer comes from the oracle and the per-feature models beside this file.

State: the rows as stored, which of them are alive, id_offset, the row epoch (how often the rows were renumbered or replaced), and the
filters and groupings made from it, each with the epoch it was made in.  ``IndexModel`` answers every method the random walk
(tests/random_walk.py) calls with the return shapes of ``FlatIndex``; ``ModelFilter`` and ``ModelGrouping`` stand in for
``IndexFilter`` and ``IndexGrouping``.  A call on a stale or foreign handle raises ``MemexHipError(MX_EINVAL)`` as the library does.

For a compressed corpus the caller appends what ``get_rows`` returned for the block, so the model never rounds to bf16 itself.

``tape``: the walk runs one seed many times (against the model itself, against each defective model, against the GPU).  The search
answers of the clean model are the same in every one of those runs, so a model may record them in call order (``tape_mode =
"record"``) and a later model of the same seed may read them back (``"replay"``) instead of computing them again.  The mutations are
always applied for real.
"""
import functools

import numpy as np

import by_id_model
import filtered_model
import fused_model
import grouped_model
import like_model
import mmr_model
import range_model
from memex_amd._lib import MX_EINVAL, MX_EUNSUPPORTED, MemexHipError
from oracle.search_oracle import score_from_dist

SEARCH_AUTO, SEARCH_EXACT = 0, 1


def _stale(kind):
    return MemexHipError(MX_EINVAL, f"the {kind} is stale: the rows of its index were renumbered or replaced; make a new one")


def _foreign(kind):
    return MemexHipError(MX_EINVAL, f"the {kind} belongs to another index")


def shard_rows(total, block_rows, shards, g):
    """the rows shard g holds when the handle holds `total` (shard_rows in memex_amd/csrc/index.hip): global row r lies in block
    r // block_rows, which belongs to shard block % shards; a plain index is its own only shard"""
    if shards == 1:
        return total
    full, tail = divmod(total, block_rows)
    return (full // shards) * block_rows + (block_rows if g < full % shards else 0) + (tail if full % shards == g else 0)


class Capacities:
    """The row capacity of every shard's storage, as memex_amd/csrc/index.hip keeps it: ensure_capacity grows a shard that must hold
    more rows than it can to max(rows, cap + cap / 2, 1024) rounded up to 64; clear and load keep the storage; a compaction that
    dropped rows gives a plain index back what is above round_up(max(n, 1024), 64) (release_capacity) and deals a sharded handle's
    rows to fresh shards in one append (compact_composite).  The resident filter's bitmap is sized by this number
    (ensure_filter_bits), so a shard's bits move exactly when its rows do."""

    def __init__(self, shards=1, block_rows=0):
        self.shards, self.block_rows = int(shards), int(block_rows)
        self.caps = [0] * self.shards

    def share(self, total):
        return [shard_rows(total, self.block_rows, self.shards, g) for g in range(self.shards)]

    def moves(self, total):
        """[(shard, its capacity now, its capacity then)] for every shard that a growth to `total` rows moves to new storage"""
        out = []
        for g, r in enumerate(self.share(total)):
            if r > self.caps[g]:
                out.append((g, self.caps[g], (max(r, self.caps[g] + self.caps[g] // 2, 1024) + 63) // 64 * 64))
        return out

    def grow(self, total):
        moved = self.moves(total)
        for g, _, cap in moved:
            self.caps[g] = cap
        return moved

    def compacted(self, total):
        fresh = [(max(r, 1024) + 63) // 64 * 64 if r or self.shards == 1 else 0 for r in self.share(total)]
        self.caps = fresh if self.shards > 1 else [min(self.caps[0], fresh[0])]

    def global_rows(self, g, lo, hi):
        """the global rows behind shard g's local rows lo .. hi - 1"""
        l = np.arange(lo, hi, dtype=np.int64)
        if self.shards == 1:
            return l
        return (l // self.block_rows * self.shards + g) * self.block_rows + l % self.block_rows


def taped(fn):
    """a search method whose answer goes to, or comes from, the model's tape"""
    @functools.wraps(fn)
    def call(self, *a, **kw):
        at = self.tape_at
        self.tape_at += 1
        if self.tape_mode == "replay" and fn.__name__ not in self.untaped:
            name, out = self.tape[at]
            assert name == fn.__name__, f"tape entry {at} is {name}, the call is {fn.__name__}: the walk left its recorded path"
            if isinstance(out, Exception):
                raise out
            return out
        try:
            out = fn(self, *a, **kw)
        except MemexHipError as e:
            out = e
        if self.tape_mode == "record":
            assert at == len(self.tape)
            self.tape.append((fn.__name__, out))
        if isinstance(out, Exception):
            raise out
        return out
    return call


class ModelFilter:
    """IndexFilter's surface over a boolean per global row"""

    def __init__(self, index):
        self.index = index
        self.epoch = index.epoch
        self.bits = np.zeros(0, bool)
        self.closed = False

    def _check(self):
        if self.epoch != self.index.epoch:
            raise _stale("filter")

    def mask(self):
        """bool over the rows of the index at this moment"""
        n = len(self.index)
        out = np.zeros(n, bool)
        m = min(n, self.bits.size)
        out[:m] = self.bits[:m]
        return out

    def _edit(self, ranges, ids, allow):
        if ranges is None and ids is None:
            raise ValueError("give ranges and / or ids")
        self._check()
        n, off = len(self.index), self.index.id_offset
        bits = self.mask()
        if ranges is not None:
            r = np.asarray(ranges, dtype=np.uint64).reshape(-1, 2)
            if (r[:, 0] > r[:, 1]).any():
                raise MemexHipError(MX_EINVAL, "lo > hi")
            bits[filtered_model.allowed_mask(n, r.astype(object), off)] = allow
        if ids is not None:
            for i in np.asarray(ids if isinstance(ids, np.ndarray) else list(ids), dtype=np.uint64).reshape(-1).tolist():
                if off < i <= off + n:
                    bits[i - off - 1] = allow
        self.bits = bits

    def allow(self, ranges=None, ids=None):
        self._edit(ranges, ids, True)

    def deny(self, ranges=None, ids=None):
        self._edit(ranges, ids, False)

    def count(self):
        self._check()
        m = self.mask()
        return int(m.sum()), int((m & self.index.alive).sum())

    def ranges(self):
        self._check()
        return filtered_model.model_ranges(self.mask(), self.index.id_offset)

    def close(self):
        self.closed = True


class ModelGrouping:
    """IndexGrouping's surface over grouped_model.GroupingModel"""

    def __init__(self, index):
        self.index = index
        self.epoch = index.epoch
        self.model = grouped_model.GroupingModel()
        self.closed = False

    def _check(self):
        if self.epoch != self.index.epoch:
            raise _stale("grouping")

    def row_keys(self):
        return grouped_model.row_keys(self.model, len(self.index))

    def set_ranges(self, ranges, keys):
        self._check()
        r = np.asarray(ranges, dtype=np.uint64).reshape(-1, 2)
        k = np.asarray(keys, dtype=np.uint32)
        k = np.full(len(r), k, np.uint32) if k.ndim == 0 else k.reshape(-1)
        try:
            self.model.set_ranges(r, k, self.index.id_offset, len(self.index))
        except ValueError as e:
            raise MemexHipError(MX_EINVAL, str(e))

    def set_ids(self, ids, keys):
        self._check()
        i = np.asarray(ids if isinstance(ids, np.ndarray) else list(ids), dtype=np.uint64).reshape(-1)
        k = np.asarray(keys, dtype=np.uint32)
        k = np.full(len(i), k, np.uint32) if k.ndim == 0 else k.reshape(-1)
        try:
            self.model.set_ids(i, k, self.index.id_offset, len(self.index))
        except ValueError as e:
            raise MemexHipError(MX_EINVAL, str(e))

    def keys_of(self, ids):
        self._check()
        i = np.asarray(ids if isinstance(ids, np.ndarray) else list(ids), dtype=np.uint64).reshape(-1)
        return self.model.keys_of(i, self.index.id_offset, len(self.index))

    def count(self):
        self._check()
        return self.model.count(len(self.index), self.index.alive)

    def close(self):
        self.closed = True


class IndexModel:
    def __init__(self, dim, oracle, compressed=False, tape=None, tape_mode=None):
        self.dim = int(dim)
        self.oracle = oracle
        self.compressed = bool(compressed)
        self.rows = np.zeros((0, self.dim), np.float32)
        self.alive = np.zeros(0, bool)
        self.id_offset = 0
        self.epoch = 0
        self.mode = SEARCH_AUTO
        self.copy_kind = "auto"
        self.stores = {}
        self.tape = tape if tape is not None else []
        self.tape_mode = tape_mode
        self.tape_at = 0
        self.untaped = ()

    # -- lifetime and configuration ------------------------------------------------------------
    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __len__(self):
        return self.rows.shape[0]

    @property
    def removed(self):
        return int((~self.alive).sum())

    def reserve(self, n_rows):
        pass

    def set_id_offset(self, off):
        self.id_offset = int(off)

    def set_search_mode(self, mode):
        if mode not in (SEARCH_AUTO, SEARCH_EXACT):
            raise MemexHipError(MX_EINVAL, f"unknown search mode {mode}")
        self.mode = mode

    def set_filter_copy(self, on):
        kind = on if isinstance(on, str) else ("auto" if on else "none")
        if kind not in ("none", "auto", "i8", "int8", "bf16"):
            raise KeyError(kind)
        if self.compressed and kind == "none":
            raise MemexHipError(MX_EINVAL, "a compressed corpus has no f32 rows to fall back to")
        self.copy_kind = kind

    def get_rows(self, first_row, n):
        if first_row < 0 or n < 0 or first_row + n > len(self):
            raise MemexHipError(MX_EINVAL, "rows out of range")
        return self.rows[first_row:first_row + n].copy()

    # -- mutation ---------------------------------------------------------------------------------
    def add(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim == 1:
            rows = rows[None, :]
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            raise MemexHipError(MX_EINVAL, f"expected [n, {self.dim}] rows, got {rows.shape}")
        if not np.isfinite(rows).all():
            raise MemexHipError(MX_EINVAL, "a row contains a non-finite value; nothing inserted")
        first = self.id_offset + len(self) + 1
        self.rows = np.concatenate([self.rows, rows])
        self.alive = np.concatenate([self.alive, np.ones(rows.shape[0], bool)])
        return first

    def replace_tail(self, rows):
        """the last len(rows) rows as the target stored them (a compressed corpus keeps their bf16 values)"""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.shape[0]:
            self.rows[len(self) - rows.shape[0]:] = rows

    def clear(self):
        self.rows = np.zeros((0, self.dim), np.float32)
        self.alive = np.zeros(0, bool)
        self.epoch += 1

    def remove(self, ids):
        a = np.asarray(ids, dtype=np.uint64).reshape(-1)
        off, n = self.id_offset, len(self)
        r = []
        for i in a.tolist():
            if not off < i <= off + n:
                raise MemexHipError(MX_EINVAL, f"id {i} is outside [{off + 1}, {off + n}]; nothing removed")
            r.append(i - off - 1)
        r = np.asarray(r, dtype=np.int64)
        before = self.removed
        self.alive[r] = False
        return self.removed - before

    def compact(self):
        kept = np.flatnonzero(self.alive).astype(np.uint64) + np.uint64(self.id_offset + 1)
        if self.removed:
            self.rows = np.ascontiguousarray(self.rows[self.alive])
            self.alive = np.ones(self.rows.shape[0], bool)
            self.epoch += 1
        return kept

    def save(self, directory):
        self.stores[str(directory)] = (self.rows.copy(), self.alive.copy())

    def load(self, directory):
        if str(directory) not in self.stores:
            raise MemexHipError(-5, f"cannot open {directory}")
        rows, alive = self.stores[str(directory)]
        self.rows, self.alive = rows.copy(), alive.copy()
        self.epoch += 1

    # -- handles ----------------------------------------------------------------------------------
    def make_filter(self, ranges=None, ids=None):
        f = ModelFilter(self)
        if ranges is not None or ids is not None:
            f.allow(ranges=ranges, ids=ids)
        return f

    def make_grouping(self):
        return ModelGrouping(self)

    def _use(self, handle, kind):
        if handle.index is not self:
            raise _foreign(kind)
        handle._check()

    # -- the candidate stage every form rests on ---------------------------------------------------
    def _queries(self, queries):
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise MemexHipError(MX_EINVAL, f"expected [B, {self.dim}] queries, got {q.shape}")
        if not np.isfinite(q).all():
            raise MemexHipError(MX_EINVAL, "a query contains a non-finite value")
        return q

    def _topk(self, Q, k, allowed=None):
        """(ids, scores, dists, n_found) of the exact top-k over the live (and allowed) rows"""
        if k < 1:
            raise MemexHipError(MX_EINVAL, "k < 1")
        if k > 4096:
            raise MemexHipError(MX_EUNSUPPORTED, "k > 4096")
        keep = self.alive if allowed is None else self.alive & allowed
        return filtered_model.subset_oracle(self.oracle, self.rows, keep, Q, k, self.id_offset)

    def _candidates(self, Q, fetch, allowed=None):
        """the lists the shared candidate block holds for MMR, fused and grouped search"""
        return self._topk(Q, fetch, allowed)

    # -- search -----------------------------------------------------------------------------------
    @taped
    def search(self, queries, k):
        return self._topk(self._queries(queries), k)

    @taped
    def search_filtered(self, queries, k, *, ranges=None, ids=None):
        if (ranges is None) == (ids is None):
            raise ValueError("give exactly one of ranges= and ids=")
        Q = self._queries(queries)
        if ids is not None:
            allowed = np.zeros(len(self), bool)
            for i in np.asarray(list(ids), dtype=np.uint64).reshape(-1).tolist():
                if self.id_offset < i <= self.id_offset + len(self):
                    allowed[i - self.id_offset - 1] = True
        else:
            r = np.asarray(ranges, dtype=np.uint64).reshape(-1, 2)
            if (r[:, 0] > r[:, 1]).any():
                raise MemexHipError(MX_EINVAL, "lo > hi")
            allowed = filtered_model.allowed_mask(len(self), r.astype(object), self.id_offset)
        return self._topk(Q, k, allowed)

    @taped
    def search_with(self, flt, queries, k):
        Q = self._queries(queries)
        self._use(flt, "filter")
        return self._topk(Q, k, flt.mask())

    @taped
    def search_range(self, queries, min_score, cap):
        Q = self._queries(queries)
        t = np.broadcast_to(np.asarray(min_score, dtype=np.float32), (Q.shape[0],))
        if cap < 1 or np.isnan(t).any():
            raise MemexHipError(MX_EINVAL, "cap < 1 or a NaN threshold")
        if cap > 4096:
            raise MemexHipError(MX_EUNSUPPORTED, "cap > 4096")
        return self._range(Q, t, cap)

    def _range(self, Q, t, cap):
        if len(self) == 0:
            return tuple(by_id_model.blank(Q.shape[0], cap, True))
        D = range_model.oracle_dists(self.oracle, self.rows, Q)
        return range_model.range_oracle(D, self.alive, t, cap, self.id_offset)

    @taped
    def search_mmr(self, queries, k, fetch=None, lam=0.5):
        Q = self._queries(queries)
        fetch = mmr_model.default_fetch(k) if fetch is None else int(fetch)
        if k < 1 or fetch < k or not 0.0 <= lam <= 1.0:
            raise MemexHipError(MX_EINVAL, "k < 1, fetch < k or lambda outside [0, 1]")
        if fetch > 1024:
            raise MemexHipError(MX_EUNSUPPORTED, "fetch > 1024")
        ci, cs, cd, cnf = self._candidates(Q, fetch)
        return self._select(ci, cs, cd, cnf, k, lam)

    def _select(self, ci, cs, cd, cnf, k, lam):
        return mmr_model.select_from_lists(self.oracle, self.rows, ci, cs, cd, cnf, k, lam, self.id_offset)

    @taped
    def search_fused(self, queries, k, mode="max", fetch=None, weights=None, rrf_c=60.0):
        Q = np.ascontiguousarray(queries, dtype=np.float32)
        if Q.ndim == 2:
            Q = Q[None]
        if mode not in ("max", "rrf") or Q.ndim != 3 or Q.shape[2] != self.dim:
            raise MemexHipError(MX_EINVAL, "bad mode or queries")
        R, m, d = Q.shape
        fetch = fused_model.default_fetch(k, mode) if fetch is None else int(fetch)
        W = np.ones((R, m), np.float32) if weights is None else np.broadcast_to(np.asarray(weights, np.float32), (R, m))
        if k < 1 or m < 1 or fetch < k or not np.isfinite(W).all() or (W < 0).any():
            raise MemexHipError(MX_EINVAL, "k < 1, m < 1, fetch < k or a bad weight")
        if m > 16 or fetch > 256:
            raise MemexHipError(MX_EUNSUPPORTED, "m > 16 or fetch > 256")
        ci, cs, cd, cnf = self._candidates(self._queries(Q.reshape(R * m, d)), fetch)
        out = [self._fuse(ci[r * m:(r + 1) * m], cd[r * m:(r + 1) * m], cs[r * m:(r + 1) * m], cnf[r * m:(r + 1) * m], W[r], k, mode, rrf_c)
               for r in range(R)]
        return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]),
                np.asarray([o[3] for o in out], np.int32), np.stack([o[4] for o in out]), np.stack([o[5] for o in out]))

    def _fuse(self, ids, dists, scores, nf, w, k, mode, rrf_c):
        return fused_model.fuse_lists(ids, dists, scores, nf, w, k, mode, rrf_c)

    @taped
    def search_grouped(self, grouping, queries, k, fetch=None, flt=None):
        Q = self._queries(queries)
        fetch = grouped_model.default_fetch(k) if fetch is None else int(fetch)
        if k < 1 or fetch < k:
            raise MemexHipError(MX_EINVAL, "k < 1 or fetch < k")
        if fetch > 4096:
            raise MemexHipError(MX_EUNSUPPORTED, "fetch > 4096")
        self._use(grouping, "grouping")
        if flt is not None:
            self._use(flt, "filter")
        ci, cs, cd, cnf = self._candidates(Q, fetch, None if flt is None else flt.mask())
        return self._group(ci, cs, cd, cnf, grouping.row_keys(), k, fetch)

    def _group(self, ci, cs, cd, cnf, keys, k, fetch):
        return grouped_model.group_lists(ci, cs, cd, cnf, keys, k, fetch, self.id_offset)

    # -- by stored row ----------------------------------------------------------------------------
    def _live_row(self, i):
        """the 0-based row a caller id names if it is alive, else None"""
        if self.id_offset < i <= self.id_offset + len(self) and self.alive[i - self.id_offset - 1]:
            return i - self.id_offset - 1
        return None

    def _query_rows(self, qids):
        """(the stored rows of the ids that name a live row [B, dim] (zeros elsewhere), mask of those ids)"""
        Q = np.zeros((len(qids), self.dim), np.float32)
        ok = np.zeros(len(qids), bool)
        for b, i in enumerate(qids.tolist()):
            r = self._live_row(i)
            if r is not None:
                Q[b], ok[b] = self.rows[r], True
        return Q, ok

    @taped
    def search_by_id(self, ids, k, exclude_self=True):
        qids = np.asarray(ids, dtype=np.uint64).reshape(-1)
        e = int(bool(exclude_self))
        if k < 1:
            raise MemexHipError(MX_EINVAL, "k < 1")
        if k + e > 4096:
            raise MemexHipError(MX_EUNSUPPORTED, "k + e > 4096")
        Q, ok = self._query_rows(qids)
        if not ok.any():
            return tuple(by_id_model.blank(len(qids), k))
        return tuple(by_id_model.drop_own(self._topk(Q, k + e), qids, ok, k, e))

    @taped
    def search_range_by_id(self, ids, min_score, cap, exclude_self=True):
        qids = np.asarray(ids, dtype=np.uint64).reshape(-1)
        e = int(bool(exclude_self))
        t = np.broadcast_to(np.asarray(min_score, dtype=np.float32), (len(qids),))
        if cap < 1 or np.isnan(t).any():
            raise MemexHipError(MX_EINVAL, "cap < 1 or a NaN threshold")
        if cap + e > 4096:
            raise MemexHipError(MX_EUNSUPPORTED, "cap + e > 4096")
        Q, ok = self._query_rows(qids)
        if not ok.any():
            return tuple(by_id_model.blank(len(qids), cap, True))
        full = self._range(Q, t, max(len(self), 1))                          # a cap that lists everything in range
        return tuple(self._drop_own_range(full, qids, ok, cap, e))

    def _drop_own_range(self, full, qids, ok, cap, e):
        return by_id_model.drop_own(full[:4], qids, ok, cap, e, counts=full[4])

    # -- by examples ------------------------------------------------------------------------------
    def _example_row(self, i):
        r = self._live_row(i)
        return None if r is None else self.rows[r]

    @taped
    def search_like(self, example_ids, k, weights=None, queries=None, query_weights=None, exclude_examples=True):
        ex = np.asarray(example_ids, dtype=np.uint64)
        ex = ex[None, :] if ex.ndim == 1 else ex
        R, m = ex.shape
        E = m if exclude_examples else 0
        if k < 1 or m < 1:
            raise MemexHipError(MX_EINVAL, "k < 1 or m < 1")
        if m > 16 or k + E > 4096:
            raise MemexHipError(MX_EUNSUPPORTED, "m > 16 or k + E > 4096")
        q = None if queries is None else self._queries(queries)
        comb, used, n_used = like_model.like_combined(self._example_row, ex, weights, q, query_weights, dim=self.dim)
        n_used = self._n_used(ex, weights, used, n_used)
        lists = self._topk(comb, k + E)
        return tuple(like_model.drop_examples(lists, ex, used, comb, k, bool(exclude_examples))) + (n_used, comb)

    def _n_used(self, ex, weights, used, n_used):
        return n_used

    # -- scoring of named rows --------------------------------------------------------------------
    @taped
    def score_ids(self, queries, ids):
        Q = self._queries(queries)
        a = np.asarray(ids, dtype=np.uint64)
        a = a[None, :] if a.ndim == 1 else a
        if a.ndim != 2 or a.shape[0] != Q.shape[0] or a.shape[1] < 1:
            raise MemexHipError(MX_EINVAL, f"expected [{Q.shape[0]}, m] candidate ids, got {a.shape}")
        if a.shape[1] > 4096:
            raise MemexHipError(MX_EUNSUPPORTED, "m > 4096")
        return self._score(Q, a, self.id_offset)

    def _score(self, Q, a, off):
        """straight from the header: found = a live row with a defined dist; order by (dist, id, position)"""
        B, m = a.shape
        n = len(self)
        sc = np.zeros((B, m), np.float32)
        di = np.full((B, m), np.inf, np.float32)
        order = np.full((B, m), -1, np.int32)
        nf = np.zeros(B, np.int32)
        for b in range(B):
            D = self.oracle.all_dists(self.rows, Q[b]) if n else np.zeros(0, np.float32)
            c = a[b]
            ok = (c > np.uint64(off)) & (c <= np.uint64(off + n))
            r = np.where(ok, c - np.uint64(off + 1), 0).astype(np.int64)
            found = ok.copy()
            if n:
                found &= self.alive[r] & ~np.isnan(D[r])
                di[b, found] = D[r[found]]
                sc[b, found] = score_from_dist(D[r[found]])
            js = np.flatnonzero(found)
            js = js[np.lexsort((js, c[js], di[b, js]))]
            order[b, :len(js)] = js
            nf[b] = len(js)
        return sc, di, order, nf


# -- defective models: what the random walk must notice ---------------------------------------------------------------------------

DEFECTS = {
    # name: (what goes wrong, the taped methods whose answers it changes)
    "filter_bits_lost_on_growth": ("filter bits are not carried across a growth of the row storage: rows past the old capacity read as "
                                   "allowed or denied at random", ("search_with", "search_grouped")),
    "grouping_keys_lost_on_growth": ("grouping keys are lost across a growth of the row storage", ("search_grouped",)),
    "candidates_previous_stride": ("the shared candidate list is read with the previous call's stride",
                                   ("search_mmr", "search_fused", "search_grouped")),
    "by_id_ignores_tombstones": ("search by id ignores the tombstone of the query row", ("search_by_id", "search_range_by_id")),
    "like_counts_removed_example": ("search by examples counts a removed example as used", ("search_like",)),
    "score_ids_ignores_id_offset": ("score_ids translates its ids without id_offset", ("score_ids",)),
    "grouped_ignores_filter": ("a grouped search with a filter ignores the filter", ("search_grouped",)),
    "compact_keeps_filters": ("a compaction that dropped rows leaves the filters usable", ("search_with", "search_grouped")),
    "range_by_id_counts_self": ("range search by id does not take the query's own row out of n_in_range", ("search_range_by_id",)),
    "mmr_candidate_order": ("MMR returns candidate order instead of selection order", ("search_mmr",)),
    "fused_max_honours_zero_weight": ("fused max consults the list of a sub-query whose weight is zero", ("search_fused",)),
    "complete_against_k": ("complete is computed against k instead of fetch", ("search_grouped",)),
}


class DefectiveModel(IndexModel):
    """the model with ONE named defect switched on; everything else answers as the clean model does"""

    def __init__(self, defect, *a, shards=1, block_rows=0, **kw):
        super().__init__(*a, **kw)
        assert defect in DEFECTS
        self.defect = defect
        self.untaped = DEFECTS[defect][1]
        self.capacity = Capacities(shards, block_rows)   # per shard, as ensure_capacity (memex_amd/csrc/index.hip) would hold it
        self.prev_fetch = None
        self.noise = np.random.default_rng(20261)
        self.handles = []

    def make_filter(self, ranges=None, ids=None):
        f = super().make_filter(ranges, ids)
        self.handles.append(f)
        return f

    def make_grouping(self):
        g = super().make_grouping()
        self.handles.append(g)
        return g

    def _grow(self, rows):
        """every shard whose share of `rows` is past its capacity moves to new storage: its filter bits past the old capacity, and
        the grouping keys, are lost there"""
        moved = self.capacity.grow(rows)
        for h in self.handles if moved else ():
            if h.closed or h.epoch != self.epoch:
                continue
            if self.defect == "filter_bits_lost_on_growth" and isinstance(h, ModelFilter):
                bits = np.zeros(max(rows, h.bits.size), bool)
                bits[:h.bits.size] = h.bits
                for g, old, _ in moved:
                    lost = self.capacity.global_rows(g, old, self.capacity.share(rows)[g])
                    bits[lost] = self.noise.random(lost.size) < 0.5
                h.bits = bits
            if self.defect == "grouping_keys_lost_on_growth" and isinstance(h, ModelGrouping):
                h.model.keys[:] = 0

    def reserve(self, n_rows):
        self._grow(int(n_rows))

    def add(self, rows):
        n = np.asarray(rows).reshape(-1, self.dim).shape[0]
        first = super().add(rows)
        self._grow(len(self))
        if self.defect == "filter_bits_lost_on_growth":  # (bits past the rows are not part of the set)
            for h in self.handles:
                if isinstance(h, ModelFilter) and not h.closed and h.epoch == self.epoch:
                    h.bits = h.bits[:len(self)]
        return first

    def compact(self):
        dropped = self.removed > 0
        keep = self.alive.copy()
        kept = super().compact()
        if dropped:
            self.capacity.compacted(len(self))
        if dropped and self.defect == "compact_keeps_filters":
            for h in self.handles:
                if isinstance(h, ModelFilter) and not h.closed and h.epoch == self.epoch - 1:
                    h.epoch = self.epoch
                    h.bits = h.bits[:keep.size][keep[:h.bits.size]]
        return kept

    def _candidates(self, Q, fetch, allowed=None):
        ci, cs, cd, cnf = super()._candidates(Q, fetch, allowed)
        prev, self.prev_fetch = self.prev_fetch, fetch
        if self.defect == "candidates_previous_stride" and prev is not None and prev != fetch:
            B = ci.shape[0]
            pad = max(0, (B - 1) * prev + fetch - B * fetch)
            flat = [np.r_[ci.reshape(-1), np.zeros(pad, np.uint64)], np.r_[cs.reshape(-1), np.zeros(pad, np.float32)],
                    np.r_[cd.reshape(-1), np.full(pad, np.inf, np.float32)]]
            ci, cs, cd = (np.stack([f[b * prev:b * prev + fetch] for b in range(B)]) for f in flat)
        return ci, cs, cd, cnf

    def _query_rows(self, qids):
        if self.defect != "by_id_ignores_tombstones":
            return super()._query_rows(qids)
        alive, self.alive = self.alive, np.ones(len(self), bool)
        try:
            return super()._query_rows(qids)
        finally:
            self.alive = alive

    def _n_used(self, ex, weights, used, n_used):
        if self.defect != "like_counts_removed_example":
            return n_used
        w = np.ones(ex.shape, np.float32) if weights is None else np.broadcast_to(np.asarray(weights, np.float32), ex.shape)
        out = n_used.copy()
        for r in range(ex.shape[0]):
            for s, i in enumerate(ex[r].tolist()):
                if w[r, s] != 0 and self.id_offset < i <= self.id_offset + len(self) and not self.alive[i - self.id_offset - 1]:
                    out[r] += 1
        return out

    def _score(self, Q, a, off):
        return super()._score(Q, a, 0 if self.defect == "score_ids_ignores_id_offset" else off)

    def search_grouped(self, grouping, queries, k, fetch=None, flt=None):
        if self.defect == "grouped_ignores_filter" and flt is not None:
            self._use(flt, "filter")
            flt = None
        return super().search_grouped(grouping, queries, k, fetch, flt)

    def _drop_own_range(self, full, qids, ok, cap, e):
        out = super()._drop_own_range(full, qids, ok, cap, e)
        if self.defect == "range_by_id_counts_self":
            out[4][ok] = full[4][ok]
        return out

    def _select(self, ci, cs, cd, cnf, k, lam):
        if self.defect != "mmr_candidate_order":
            return super()._select(ci, cs, cd, cnf, k, lam)
        out = by_id_model.blank(ci.shape[0], k)
        for b in range(ci.shape[0]):
            n = min(k, int(cnf[b]))
            out[0][b, :n], out[1][b, :n], out[2][b, :n], out[3][b] = ci[b, :n], cs[b, :n], cd[b, :n], n
        return tuple(out)

    def _fuse(self, ids, dists, scores, nf, w, k, mode, rrf_c):
        if self.defect == "fused_max_honours_zero_weight" and mode == "max":
            w = np.where(np.asarray(w) == 0, np.float32(1), w)
        return super()._fuse(ids, dists, scores, nf, w, k, mode, rrf_c)

    def _group(self, ci, cs, cd, cnf, keys, k, fetch):
        out = super()._group(ci, cs, cd, cnf, keys, k, fetch)
        if self.defect == "complete_against_k":
            out = out[:6] + ((out[5] == k) | (cnf < k),)
        return out
