"""The contract of fused search (mx_index_search_fused) restated in NumPy and Python floats -- TEST
INFRASTRUCTURE, not product code.

The lists come from ``COracle.search`` (the exact top-``fetch`` of every sub-query in (dist, id) order); the fusion runs in Python
floats (IEEE f64) exactly as the header states it:

    best(row)  = the consulted list that holds the row with the smallest (dist, sub-query index)
    MAX        rows by (best dist, id); fused = float(score)
    RRF        fused(row) = sum, over the consulted lists that hold the row in ascending i, of  float(w_i) / (float(c) + rank_i),
               rank_i 1-based; rows by (-fused, id)

with w_i and c the f32 arguments widened and a list consulted iff its weight is > 0.
"""
import numpy as np

MAX, RRF = "max", "rrf"


def default_fetch(k, mode):
    return k if mode == MAX else min(max(4 * k, 32), 256)


def fuse_lists(ids, dists, scores, nf, weights, k, mode, rrf_c=60.0):
    """ids / dists / scores [m, fetch] and nf [m]: one request's lists -> (ids, scores, dists, n_found, best_sub, fused), [k] each"""
    m = ids.shape[0]
    c = float(np.float32(rrf_c))
    seen = {}                                                             # id -> [fused, (dist, sub), rank0 in the best list]
    for i in range(m):
        w = float(np.float32(weights[i]))
        if not w > 0.0:
            continue
        for r in range(int(nf[i])):
            row = int(ids[i, r])
            key = (float(dists[i, r]), i)
            term = w / (c + float(r + 1)) if mode == RRF else 0.0
            if row not in seen:
                seen[row] = [0.0 + term, key, r]
            else:
                e = seen[row]
                e[0] = e[0] + term                                        # ascending i: the order of the sum
                if key < e[1]:
                    e[1], e[2] = key, r
    if mode == RRF:
        order = sorted(seen, key=lambda row: (-seen[row][0], row))[:k]
    else:
        order = sorted(seen, key=lambda row: (seen[row][1][0], row))[:k]
    oi = np.zeros(k, np.uint64)
    osc = np.zeros(k, np.float32)
    od = np.full(k, np.inf, np.float32)
    ob = np.full(k, -1, np.int32)
    of = np.zeros(k, np.float64)
    for t, row in enumerate(order):
        f, (_, sub), r = seen[row]
        oi[t], osc[t], od[t], ob[t] = row, scores[sub, r], dists[sub, r], sub
        of[t] = f if mode == RRF else float(scores[sub, r])
    return oi, osc, od, len(order), ob, of


def fused_model(oracle, rows, Q, k, mode=MAX, fetch=None, weights=None, rrf_c=60.0, alive=None, id_offset=0):
    """rows: the rows as stored [n, d]; Q [R, m, d]; weights [R, m] or None; alive: mask of the rows not removed ->
    (ids, scores, dists, n_found, best_sub, fused) as FlatIndex.search_fused returns them"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    if Q.ndim == 2:
        Q = Q[None]
    R, m, d = Q.shape
    fetch = default_fetch(k, mode) if fetch is None else fetch
    W = np.ones((R, m), np.float32) if weights is None else np.broadcast_to(np.asarray(weights, np.float32), (R, m))
    live = np.arange(rows.shape[0]) if alive is None else np.flatnonzero(alive)
    ci, cd, cs, cnf = oracle.search(rows[live], Q.reshape(R * m, d), fetch)
    for b in range(R * m):                                                # positions among the live rows -> ids
        n = int(cnf[b])
        ci[b, :n] = live[ci[b, :n].astype(np.int64) - 1].astype(np.uint64) + np.uint64(1 + id_offset)
    out = [fuse_lists(ci[r * m:(r + 1) * m], cd[r * m:(r + 1) * m], cs[r * m:(r + 1) * m], cnf[r * m:(r + 1) * m], W[r], k, mode, rrf_c)
           for r in range(R)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]),
            np.asarray([o[3] for o in out], np.int32), np.stack([o[4] for o in out]), np.stack([o[5] for o in out]))


def brute_force_max(oracle, rows, Q, k, id_offset=0):
    """the definition MX_FUSE_MAX is held to: the top-k of min_i dist_i(row) over ALL rows, ordered (dist, id); Q [m, d] ->
    (ids [k], dists [k], best_sub [k])"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    D = np.stack([oracle.all_dists(rows, q) for q in np.ascontiguousarray(Q, dtype=np.float32)])   # [m, n]
    best = D.min(axis=0)
    sub = D.argmin(axis=0)                                                # the first minimum: the smallest sub-query index
    order = sorted(range(rows.shape[0]), key=lambda r: (float(best[r]), r))[:k]
    return (np.asarray(order, np.uint64) + np.uint64(1 + id_offset), best[order].astype(np.float32), sub[order].astype(np.int32))


def tripled_corpus(rng, clusters=40, per=10, d=64):
    """near_copy_corpus with every row stored three times (exact ties in every list) -> (rows [3 * clusters * per, d], centres)"""
    from mmr_model import near_copy_corpus
    X, centres = near_copy_corpus(rng, clusters=clusters, per=per, d=d)
    return np.ascontiguousarray(np.concatenate([X, X, X])), centres
