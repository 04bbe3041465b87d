"""The contract of diversified search (mx_index_search_mmr) restated in NumPy and Python floats --
TEST INFRASTRUCTURE, not product code.

Candidates come from ``COracle.search`` (the exact top-``fetch`` in (dist, id) order), pair distances from the oracle's DistCosine
(``COracle.dist`` arithmetic; ``all_dists`` runs the same C function over a block of rows), scores from ``score_from_dist``, and the
greedy loop runs in Python floats (IEEE f64) exactly as the header states it:

    v_i = lam * rel_i - (1.0 - lam) * pen_i,  pen_i = max over the picked j of sim(i, j),  sim = score(DistCosine(row_j, row_i))

with lam the f32 argument widened, a NaN sim counted as 1.0, a NaN v as -inf and ties given to the earlier candidate.
"""
import numpy as np

from oracle.search_oracle import score_from_dist


def default_fetch(k):
    return min(max(4 * k, 32), 1024)


def greedy(oracle, cand_rows, rel, n_pick, lam):
    """cand_rows: [m, d] stored rows of the candidates in (dist, id) order; rel: their f32 scores -> the picked positions in order"""
    m = cand_rows.shape[0]
    lam = float(np.float32(lam))
    order = [0] if n_pick > 0 else []
    picked = np.zeros(m, dtype=bool)
    pen = np.full(m, -np.inf, dtype=np.float32)
    while len(order) < n_pick:
        j = order[-1]
        picked[j] = True
        sim = score_from_dist(oracle.all_dists(cand_rows, cand_rows[j]))   # DistCosine(row_j, row_i) for every i
        sim[np.isnan(sim)] = np.float32(1.0)
        best, best_v = -1, 0.0
        for i in range(m):
            if picked[i]:
                continue
            if sim[i] > pen[i]:
                pen[i] = sim[i]
            with np.errstate(all="ignore"):
                v = lam * float(rel[i]) - (1.0 - lam) * float(pen[i])
            if v != v:
                v = -np.inf
            if best < 0 or v > best_v:
                best, best_v = i, v
        order.append(best)
    return order


def mmr_model(oracle, rows, Q, k, fetch=None, lam=0.5, alive=None, id_offset=0):
    """rows: the rows as stored [n, d]; alive: mask of the rows not removed -> (ids, scores, dists, n_found) as
    FlatIndex.search_mmr returns them"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    if Q.ndim == 1:
        Q = Q[None, :]
    fetch = default_fetch(k) if fetch is None else fetch
    live = np.arange(rows.shape[0]) if alive is None else np.flatnonzero(alive)
    ci, cd, cs, cnf = oracle.search(rows[live], Q, fetch)
    for b in range(Q.shape[0]):                                           # positions among the live rows -> ids
        m = int(cnf[b])
        ci[b, :m] = live[ci[b, :m].astype(np.int64) - 1].astype(np.uint64) + np.uint64(1 + id_offset)
    return select_from_lists(oracle, rows, ci, cs, cd, cnf, k, lam, id_offset)


def select_from_lists(oracle, rows, ci, cs, cd, cnf, k, lam=0.5, id_offset=0):
    """the selection stage on candidate lists [B, fetch] as a search returns them (ids under id_offset, (dist, id) order) ->
    (ids, scores, dists, n_found) in selection order"""
    B = ci.shape[0]
    ids = np.zeros((B, k), np.uint64)
    sc = np.zeros((B, k), np.float32)
    di = np.full((B, k), np.inf, np.float32)
    nf = np.zeros(B, np.int32)
    for b in range(B):
        m = int(cnf[b])
        cand = ci[b, :m].astype(np.int64) - 1 - id_offset                 # 0-based stored rows, (dist, id) order
        n_pick = min(k, m)
        order = greedy(oracle, rows[cand], cs[b, :m], n_pick, lam)
        nf[b] = n_pick
        ids[b, :n_pick] = ci[b, order]
        sc[b, :n_pick] = cs[b, order]
        di[b, :n_pick] = cd[b, order]
    return ids, sc, di, nf


def near_copy_corpus(rng, clusters=150, per=20, d=384, noise=0.05):
    """clusters x per rows: every row is its cluster's centre plus noise of about `noise` of the centre's length -- cluster
    members stand in for the overlapping windows of one document.  -> (rows f32 [clusters * per, d], centres f64 [clusters, d])"""
    centres = rng.standard_normal((clusters, d))
    length = np.linalg.norm(centres, axis=1, keepdims=True)
    X = np.repeat(centres, per, axis=0) + rng.standard_normal((clusters * per, d)) * np.repeat(length, per, axis=0) * (noise / np.sqrt(d))
    return X.astype(np.float32), centres


def queries_near_centres(rng, centres, B, noise=0.05):
    d = centres.shape[1]
    c = centres[rng.integers(0, centres.shape[0], B)]
    return (c + rng.standard_normal((B, d)) * np.linalg.norm(c, axis=1, keepdims=True) * (noise / np.sqrt(d))).astype(np.float32)
