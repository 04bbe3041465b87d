"""The contract of grouped search (mx_grouping, mx_index_search_grouped) restated in NumPy -- TEST
INFRASTRUCTURE, not product code.

A grouping is one u32 key per global row (id - id_offset - 1), 0 = ungrouped; ``GroupingModel`` keeps it as a NumPy array and applies
the edit rules of the header.  The candidate list of a query comes from ``COracle.search`` (the exact top-``fetch`` in (dist, id)
order, over the live -- and, with a filter, allowed -- rows); the grouping of the list is the header's:

    head        an entry whose key is 0, or whose key no earlier entry of the list has
    output      the first k heads in list order: the entry's id, score and dist unchanged, its key, and group_rows = the entries of the
                list with that key (1 for key 0); n_found = min(k, heads); blanks id 0 / score 0 / dist +inf / key 0 / group_rows 0
    complete    n_found == k, or the list holds fewer than fetch entries
"""
import numpy as np


def default_fetch(k):
    return min(4096, max(k, min(256, max(32, 4 * k))))


class GroupingModel:
    """the keys of a grouping as an array over the global rows; rows past the array have key 0"""

    def __init__(self):
        self.keys = np.zeros(0, np.uint32)

    def _cover(self, size):
        if size > self.keys.size:
            self.keys = np.concatenate([self.keys, np.zeros(size - self.keys.size, np.uint32)])

    def set_ranges(self, ranges, keys, id_offset, size):
        """ranges [m, 2] half-open id ranges under id_offset, keys [m]; size: the rows of the index at this moment.  ValueError where
        the call is MX_EINVAL (lo > hi; two non-empty ranges that overlap), the keys unchanged."""
        r = np.asarray(ranges, np.uint64).reshape(-1, 2).astype(object)
        k = np.asarray(keys, np.uint32).reshape(-1)
        assert len(r) == len(k)
        if any(lo > hi for lo, hi in r):
            raise ValueError("lo > hi")
        spans = sorted((int(lo), int(hi), int(key)) for (lo, hi), key in zip(r, k) if lo < hi)
        if any(a[1] > b[0] for a, b in zip(spans, spans[1:])):
            raise ValueError("overlap")
        self._cover(size)
        for lo, hi, key in spans:
            a = max(lo - id_offset - 1, 0)
            b = min(max(hi - id_offset - 1, 0), size)
            if a < b:
                self.keys[a:b] = key

    def set_ids(self, ids, keys, id_offset, size):
        """ids [m] under id_offset, keys [m].  ValueError where the call is MX_EINVAL: an id with two different keys."""
        i = np.asarray(ids, np.uint64).reshape(-1)
        k = np.asarray(keys, np.uint32).reshape(-1)
        assert len(i) == len(k)
        seen = {}
        for a, b in zip(i.tolist(), k.tolist()):
            if seen.setdefault(a, b) != b:
                raise ValueError("an id with two keys")
        self._cover(size)
        for a, b in seen.items():
            if id_offset < a <= id_offset + size:
                self.keys[a - id_offset - 1] = b

    def keys_of(self, ids, id_offset, size):
        out = np.zeros(len(ids), np.uint32)
        for j, a in enumerate(np.asarray(ids, np.uint64).tolist()):
            if id_offset < a <= id_offset + size and a - id_offset - 1 < self.keys.size:
                out[j] = self.keys[a - id_offset - 1]
        return out

    def count(self, size, alive=None):
        k = self.keys[:size]
        live = np.ones(k.size, bool) if alive is None else np.asarray(alive, bool)[:k.size]
        return int((k != 0).sum()), int(((k != 0) & live).sum())


def row_keys(keys, n):
    """the key array of a grouping (a GroupingModel, an array that may be shorter than the rows, or None) over n rows"""
    if isinstance(keys, GroupingModel):
        keys = keys.keys
    out = np.zeros(n, np.uint32)
    if keys is not None:
        m = min(n, len(keys))
        out[:m] = np.asarray(keys, np.uint32)[:m]
    return out


def group_list(ids, scores, dists, n, ekeys, k, fetch):
    """one query's list (ids / scores / dists [fetch], n entries) and the keys of its entries [n] -> the seven outputs, [k] each"""
    oi = np.zeros(k, np.uint64)
    osc = np.zeros(k, np.float32)
    od = np.full(k, np.inf, np.float32)
    ok = np.zeros(k, np.uint32)
    orows = np.zeros(k, np.int32)
    total = {}
    for key in ekeys[:n].tolist():
        total[key] = total.get(key, 0) + 1
    seen = set()
    heads = 0
    for j in range(n):
        key = int(ekeys[j])
        if key != 0 and key in seen:
            continue
        seen.add(key)
        if heads < k:
            oi[heads], osc[heads], od[heads], ok[heads] = ids[j], scores[j], dists[j], key
            orows[heads] = 1 if key == 0 else total[key]
        heads += 1
    nf = min(k, heads)
    return oi, osc, od, ok, orows, nf, bool(nf == k or n < fetch)


def group_lists(ci, cs, cd, cnf, keys, k, fetch, id_offset=0):
    """lists [B, fetch] as a search returns them (ids under id_offset) and the keys per global row -> what FlatIndex.search_grouped
    returns: (ids, scores, dists, keys, group_rows, n_found, complete)"""
    keys = np.asarray(keys, np.uint32)
    out = []
    for b in range(ci.shape[0]):
        n = int(cnf[b])
        r = ci[b, :n].astype(np.int64) - 1 - id_offset
        ek = np.zeros(n, np.uint32)
        inside = (r >= 0) & (r < keys.size)
        ek[inside] = keys[r[inside]]
        out.append(group_list(ci[b], cs[b], cd[b], n, ek, k, fetch))
    B = ci.shape[0]
    return (np.stack([o[0] for o in out]) if B else np.zeros((0, k), np.uint64),
            np.stack([o[1] for o in out]) if B else np.zeros((0, k), np.float32),
            np.stack([o[2] for o in out]) if B else np.zeros((0, k), np.float32),
            np.stack([o[3] for o in out]) if B else np.zeros((0, k), np.uint32),
            np.stack([o[4] for o in out]) if B else np.zeros((0, k), np.int32),
            np.asarray([o[5] for o in out], np.int32), np.asarray([o[6] for o in out], bool))


def candidate_lists(oracle, rows, Q, fetch, alive=None, allowed=None, id_offset=0):
    """the lists of the candidate stage: the oracle's top-fetch over the live (and allowed) rows, positions mapped back to ids ->
    (ids, scores, dists, n_found)"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    if Q.ndim == 1:
        Q = Q[None]
    mask = np.ones(rows.shape[0], bool)
    if alive is not None:
        mask &= np.asarray(alive, bool)
    if allowed is not None:
        mask &= np.asarray(allowed, bool)
    live = np.flatnonzero(mask)
    if live.size == 0 or Q.shape[0] == 0:
        B = Q.shape[0]
        return (np.zeros((B, fetch), np.uint64), np.zeros((B, fetch), np.float32), np.full((B, fetch), np.inf, np.float32),
                np.zeros(B, np.int32))
    ci, cd, cs, cnf = oracle.search(rows[live], Q, fetch)
    for b in range(Q.shape[0]):                                           # positions among the live rows -> ids
        n = int(cnf[b])
        ci[b, :n] = live[ci[b, :n].astype(np.int64) - 1].astype(np.uint64) + np.uint64(1 + id_offset)
    return ci, cs, cd, cnf


def grouped_model(oracle, rows, Q, k, keys, fetch=None, alive=None, allowed=None, id_offset=0):
    """rows: the rows as stored [n, d]; Q [B, d]; keys: per global row (GroupingModel, array or None); alive: mask of the rows not
    removed; allowed: mask of a filter's rows -> what FlatIndex.search_grouped returns"""
    fetch = default_fetch(k) if fetch is None else fetch
    ci, cs, cd, cnf = candidate_lists(oracle, rows, Q, fetch, alive, allowed, id_offset)
    return group_lists(ci, cs, cd, cnf, row_keys(keys, np.asarray(rows).shape[0]), k, fetch, id_offset)


def brute_force_groups(oracle, rows, q, k, keys, alive=None):
    """the definition `complete` is held to: all live rows with a non-NaN dist in (dist, id) order, groups ordered by their best row;
    the first k groups -> (ids [n], dists [n], keys [n]) of their best rows, n = min(k, groups)"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    keys = row_keys(keys, rows.shape[0])
    d = oracle.all_dists(rows, np.ascontiguousarray(q, dtype=np.float32))
    live = np.ones(rows.shape[0], bool) if alive is None else np.asarray(alive, bool)
    order = sorted((r for r in range(rows.shape[0]) if live[r] and d[r] == d[r]), key=lambda r: (float(d[r]), r))
    seen = set()
    heads = []
    for r in order:
        key = int(keys[r])
        if key != 0 and key in seen:
            continue
        seen.add(key)
        heads.append(r)
        if len(heads) == k:
            break
    h = np.asarray(heads, np.int64)
    return h.astype(np.uint64) + np.uint64(1), d[h].astype(np.float32), keys[h]


def random_keys(rng, n, ungrouped=0.2, biggest=4, order=None):
    """keys over n rows: a random partition into groups of 1 .. biggest rows (keys 1, 2, ...), a share of the rows left at key 0.
    order: the rows in the order they are cut into groups (default: a random one) -- neighbours in it tend to share a group"""
    keys = np.zeros(n, np.uint32)
    perm = rng.permutation(n) if order is None else np.asarray(order)
    at, key = 0, 0
    while at < n:
        size = int(rng.integers(1, biggest + 1))
        key += 1
        keys[perm[at:at + size]] = key
        at += size
    keys[rng.random(n) < ungrouped] = 0
    return keys
