"""The contract of boosted search (mx_prior, mx_index_search_boosted) restated in NumPy -- TEST INFRASTRUCTURE,
not product code.

A prior is one f32 per global row (id - id_offset - 1), 0 where nothing was set; ``PriorModel`` keeps it as a NumPy array with the
bound ``hi`` and applies the edit rules of the header.  The candidate list of a query comes from ``grouped_model.candidate_lists``
(the exact top-``fetch`` in (dist, id) order); its re-ranking is the header's:

    combined    c_j = float64(score_j) + float64(w) * float64(prior_j): the product of two f32 values is exact in f64, one rounding
    order       c descending, then position in the list ascending; the first min(k, m) entries, id / score / dist unchanged
    complete    m < fetch, or the k-th reported c > U = float64(score_last) + float64(w) * float64(hi)
"""
import functools

import numpy as np

from grouped_model import candidate_lists, default_fetch  # noqa: F401 (default_fetch: the same rule as grouped search)
from oracle.search_oracle import score_from_dist


def combine(score, w, prior):
    return np.float64(np.float32(score)) + np.float64(np.float32(w)) * np.float64(np.float32(prior))


class PriorModel:
    """the values of a prior as an array over the global rows; rows past the array read 0.  hi: the bound the certificate uses"""

    def __init__(self):
        self.vals = np.zeros(0, np.float32)
        self.hi = np.float32(0.0)

    def _cover(self, size):
        if size > self.vals.size:
            self.vals = np.concatenate([self.vals, np.zeros(size - self.vals.size, np.float32)])

    @staticmethod
    def _finite(v):
        if not np.isfinite(v).all():
            raise ValueError("a value that is not finite")

    def _raise_hi(self, v):
        if v.size:
            self.hi = max(self.hi, np.float32(v.max()))

    def set_ranges(self, ranges, values, id_offset, size):
        """ranges [m, 2] half-open id ranges under id_offset, values [m]; size: the rows of the index at this moment.  ValueError
        where the call is MX_EINVAL (a value not finite; lo > hi; two non-empty ranges that overlap), nothing changed."""
        r = np.asarray(ranges, np.uint64).reshape(-1, 2).astype(object)
        v = np.asarray(values, np.float32).reshape(-1)
        assert len(r) == len(v)
        self._finite(v)
        if any(lo > hi for lo, hi in r):
            raise ValueError("lo > hi")
        spans = sorted((int(lo), int(hi), j) for j, (lo, hi) in enumerate(r) if lo < hi)
        if any(a[1] > b[0] for a, b in zip(spans, spans[1:])):
            raise ValueError("overlap")
        self._cover(size)
        self._raise_hi(v)
        for lo, hi, j in spans:
            a = max(lo - id_offset - 1, 0)
            b = min(max(hi - id_offset - 1, 0), size)
            if a < b:
                self.vals[a:b] = v[j]

    def set_ids(self, ids, values, id_offset, size):
        """ids [m] under id_offset, values [m].  ValueError where the call is MX_EINVAL: a value not finite, an id with two values of
        different bits."""
        i = np.asarray(ids, np.uint64).reshape(-1)
        v = np.asarray(values, np.float32).reshape(-1)
        assert len(i) == len(v)
        self._finite(v)
        seen = {}
        for a, b in zip(i.tolist(), v.view(np.uint32).tolist()):
            if seen.setdefault(a, b) != b:
                raise ValueError("an id with two values")
        self._cover(size)
        self._raise_hi(v)
        for a, b in seen.items():
            if id_offset < a <= id_offset + size:
                self.vals[a - id_offset - 1] = np.asarray([b], np.uint32).view(np.float32)[0]

    def values_of(self, ids, id_offset, size):
        out = np.zeros(len(ids), np.float32)
        for j, a in enumerate(np.asarray(ids, np.uint64).tolist()):
            if id_offset < a <= id_offset + size and a - id_offset - 1 < self.vals.size:
                out[j] = self.vals[a - id_offset - 1]
        return out

    def bound(self, refresh=False, size=None, alive=None):
        """refresh: hi becomes the maximum of 0 and the values of the live rows among the first `size`"""
        if refresh:
            v = self.vals[:size]
            if alive is not None:
                v = v[np.asarray(alive, bool)[:v.size]]
            self.hi = np.float32(max(0.0, float(v.max()))) if v.size else np.float32(0.0)
        return self.hi


def row_priors(priors, n):
    """the value array of a prior (a PriorModel, an array that may be shorter than the rows, or None) over n rows"""
    if isinstance(priors, PriorModel):
        priors = priors.vals
    out = np.zeros(n, np.float32)
    if priors is not None:
        m = min(n, len(priors))
        out[:m] = np.asarray(priors, np.float32)[:m]
    return out


def precedes(ca, ia, cb, ib):
    """entry a (combined ca, position ia) comes before entry b"""
    if ca > cb:
        return True
    if ca < cb:
        return False
    return ia < ib


def boost_list(ids, scores, dists, n, epri, w, hi, k, fetch):
    """one query's list (ids / scores / dists [fetch], n entries) and the priors of its entries [n] -> the seven outputs"""
    oi = np.zeros(k, np.uint64)
    osc = np.zeros(k, np.float32)
    od = np.full(k, np.inf, np.float32)
    op = np.zeros(k, np.float32)
    oc = np.zeros(k, np.float64)
    c = [combine(scores[j], w, epri[j]) for j in range(n)]
    # ordered by explicit comparisons of (c, position), not by a float sort key
    order = sorted(range(n), key=functools.cmp_to_key(lambda a, b: -1 if precedes(c[a], a, c[b], b) else 1))
    nf = min(k, n)
    for s, j in enumerate(order[:nf]):
        oi[s], osc[s], od[s], op[s], oc[s] = ids[j], scores[j], dists[j], epri[j], c[j]
    if n < fetch:
        done = True
    else:                                                                   # n == fetch >= k: the k-th reported entry exists
        done = bool(oc[k - 1] > combine(scores[n - 1], w, hi))
    return oi, osc, od, op, oc, nf, done


def boost_lists(ci, cs, cd, cnf, priors, w, hi, k, fetch, id_offset=0):
    """lists [B, fetch] as a search returns them (ids under id_offset), the values per global row, w a scalar or [B], hi the bound ->
    what FlatIndex.search_boosted returns: (ids, scores, dists, priors, combined, n_found, complete)"""
    priors = np.asarray(priors, np.float32)
    B = ci.shape[0]
    w = np.broadcast_to(np.asarray(w, np.float32), (B,))
    out = []
    for b in range(B):
        n = int(cnf[b])
        r = ci[b, :n].astype(np.int64) - 1 - id_offset
        ep = np.zeros(n, np.float32)
        inside = (r >= 0) & (r < priors.size)
        ep[inside] = priors[r[inside]]
        out.append(boost_list(ci[b], cs[b], cd[b], n, ep, w[b], hi, k, fetch))
    kinds = (np.uint64, np.float32, np.float32, np.float32, np.float64)
    cols = [np.stack([o[i] for o in out]) if B else np.zeros((0, k), t) for i, t in enumerate(kinds)]
    return (*cols, np.asarray([o[5] for o in out], np.int32), np.asarray([o[6] for o in out], bool))


def boosted_model(oracle, rows, Q, k, priors, w=1.0, hi=None, fetch=None, alive=None, allowed=None, id_offset=0):
    """rows: the rows as stored [n, d]; priors: per global row (PriorModel, array or None); hi: the bound (default: the PriorModel's, or
    the maximum of 0 and the array) -> what FlatIndex.search_boosted returns"""
    fetch = default_fetch(k) if fetch is None else fetch
    n = np.asarray(rows).shape[0]
    pv = row_priors(priors, n)
    if hi is None:
        hi = priors.hi if isinstance(priors, PriorModel) else np.float32(max(0.0, float(pv.max()))) if n else np.float32(0.0)
    ci, cs, cd, cnf = candidate_lists(oracle, rows, Q, fetch, alive, allowed, id_offset)
    return boost_lists(ci, cs, cd, cnf, pv, w, hi, k, fetch, id_offset)


def brute_force_boosted(oracle, X, q, priors, w, k, alive=None):
    """the definition `complete` is held to: all live rows with a non-NaN dist ordered by (c descending, dist, id); the first k ->
    (ids [n], dists [n], combined [n]), n = min(k, rows)"""
    X = np.ascontiguousarray(X, dtype=np.float32)
    pv = row_priors(priors, X.shape[0])
    d = oracle.all_dists(X, np.ascontiguousarray(q, dtype=np.float32))
    sc = score_from_dist(d)
    live = np.ones(X.shape[0], bool) if alive is None else np.asarray(alive, bool)
    c = sc.astype(np.float64) + np.float64(np.float32(w)) * pv.astype(np.float64)
    rows = [r for r in range(X.shape[0]) if live[r] and d[r] == d[r]]
    rows.sort(key=lambda r: (-float(c[r]), float(d[r]), r))                 # (exact: f64 and f32 values are Python floats unchanged)
    h = np.asarray(rows[:k], np.int64)
    return h.astype(np.uint64) + np.uint64(1), d[h].astype(np.float32), c[h]


def case_a():
    """Case A: the near-copy corpus at 2000 x 64 (100 documents of 20 windows), 6 queries near cluster centres, priors uniform in
    [0, 1); meant for w = 0.05, k = 5, fetch = 32 -> (X, Q, priors).  A query's own cluster fills the first 20 entries with scores near
    1 and the 32nd entry belongs to an unrelated cluster, so the margin dwarfs w * hi <= 0.05: every query must come out complete."""
    from mmr_model import near_copy_corpus, queries_near_centres
    rng = np.random.default_rng(3170)
    X, centres = near_copy_corpus(rng, clusters=100, per=20, d=64)
    Q = queries_near_centres(rng, centres, 6)
    return X, Q, rng.random(X.shape[0]).astype(np.float32)


def case_b(oracle):
    """Case B: Case A's rows and queries, all priors 0 except the row farthest from query 0, which gets 100; meant for w = 1, k = 5,
    fetch = 32: that row is not in query 0's list, and wins over all rows -> (X, Q, priors, far row)"""
    X, Q, _ = case_a()
    far = int(np.argmax(oracle.all_dists(X, Q[0])))
    pv = np.zeros(X.shape[0], np.float32)
    pv[far] = 100.0
    return X, Q, pv, far
