"""The contract of search by examples (mx_index_search_like) restated in NumPy -- TEST INFRASTRUCTURE, not
product code.

    na       = the f64 sum, in element order, of fl32(v_j * v_j)                     (np.float32 products, np.float64 scalar adds)
    used     = weight != 0, the id names a live row, na > 0                           (the caller vector: weight != 0, na != 0)
    c_j      = +0.0, then c_j += (double)w * ((double)v_j / sqrt(na)) over the used terms: the caller vector first, then the examples
               in ascending slot order; every operation one np.float64 scalar operation, nothing fused
    combined = np.float32(c_j)                                                        (round to nearest even)

``drop_examples`` is the last step on a plain search's lists: with ``exclude`` the entries whose id is a used example's are dropped,
the rest keeps its order and is cut to k; a request whose combined vector is all zeros is blank.
"""
import numpy as np


def norm2(v):
    """na: f32 products summed sequentially in f64, in element order"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    prod = (v * v).astype(np.float32)                       # fl32(v_j * v_j), one rounding each
    if prod.size == 0:
        return np.float64(0.0)
    return np.cumsum(prod.astype(np.float64))[-1]           # (a running sum: strictly sequential, one f64 add per element)


def combine_one(dim, terms):
    """terms: (weight, vector or None) in contract order (the caller term first) -> (combined f32 [dim], used flags per term)"""
    c = np.zeros(dim, dtype=np.float64)
    used = []
    for w, v in terms:
        w = np.float32(w)
        ok = v is not None and w != 0
        if ok:
            na = norm2(v)
            ok = not bool(na == 0)                          # (NaN, from a non-finite caller vector: used)
        used.append(ok)
        if not ok:
            continue
        length = np.sqrt(na)                                # f64, correctly rounded
        v64 = np.ascontiguousarray(v, dtype=np.float32).astype(np.float64)
        c = c + np.float64(w) * (v64 / length)              # elementwise: one division, one product, one sum per column
    with np.errstate(over="ignore"):
        return c.astype(np.float32), used


def like_combined(rows_of, example_ids, weights=None, queries=None, query_weights=None, dim=None):
    """rows_of(id) -> the stored row the id names as f32 [dim], or None when it names no live row.  example_ids [R, m].  dim: needed
    only when no request has a vector at all.
    -> (combined f32 [R, dim], used bool [R, m], n_used i32 [R])"""
    ids = np.asarray(example_ids, dtype=np.uint64)
    R, m = ids.shape
    w = np.ones((R, m), np.float32) if weights is None else np.broadcast_to(np.asarray(weights, np.float32), (R, m))
    qw = None
    if queries is not None:
        queries = np.ascontiguousarray(queries, dtype=np.float32)
        qw = np.ones(R, np.float32) if query_weights is None else np.broadcast_to(np.asarray(query_weights, np.float32), (R,))
    out, used = [], np.zeros((R, m), bool)
    for r in range(R):
        terms = [] if queries is None else [(qw[r], queries[r])]
        vecs = [rows_of(int(i)) if w[r, s] != 0 else None for s, i in enumerate(ids[r])]
        terms += [(w[r, s], vecs[s]) for s in range(m)]
        if dim is None:
            dim = next((len(v) for _, v in terms if v is not None), None)
        out.append(terms)
    if dim is None:
        raise ValueError("no vector anywhere: pass dim")
    comb = np.zeros((R, dim), np.float32)
    for r, terms in enumerate(out):
        comb[r], u = combine_one(dim, terms)
        used[r] = u[len(u) - m:]
    return comb, used, used.sum(axis=1).astype(np.int32)


def blank(R, k):
    return [np.zeros((R, k), np.uint64), np.zeros((R, k), np.float32), np.full((R, k), np.inf, np.float32), np.zeros(R, np.int32)]


def drop_examples(lists, example_ids, used, combined, k, exclude):
    """lists: (ids, scores, dists, n_found) of a plain search at k + (m if exclude else 0) -> the caller's lists [R, k]"""
    ids, sc, di, nf = lists
    ex = np.asarray(example_ids, dtype=np.uint64)
    R = ex.shape[0]
    out = blank(R, k)
    for r in range(R):
        if not (combined[r] != 0).any():                    # a blank request
            continue
        gone = set(int(i) for i in ex[r][used[r]]) if exclude else set()
        keep = [j for j in range(int(nf[r])) if int(ids[r, j]) not in gone][:k]
        out[0][r, :len(keep)], out[1][r, :len(keep)], out[2][r, :len(keep)], out[3][r] = ids[r, keep], sc[r, keep], di[r, keep], len(keep)
    return out
