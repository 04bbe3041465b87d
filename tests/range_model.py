"""The contract of range search (mx_index_search_range) restated in NumPy -- TEST INFRASTRUCTURE, not product
code.  The expected answer comes from the oracle's distances: score_from_dist, mask score >= t, order by (dist, id).
"""
import numpy as np

from oracle.search_oracle import score_from_dist


def oracle_dists(oracle, rows, Q):
    return np.stack([oracle.all_dists(rows, q) for q in np.asarray(Q, dtype=np.float32)])


def range_oracle(D, alive, t, cap, off=0):
    """D: [B, n] oracle dists -> (ids, scores, dists, n_found, n_in_range) as FlatIndex.search_range returns them"""
    B = D.shape[0]
    ids = np.zeros((B, cap), np.uint64)
    sc = np.zeros((B, cap), np.float32)
    di = np.full((B, cap), np.inf, np.float32)
    nf = np.zeros(B, np.int32)
    nr = np.zeros(B, np.uint64)
    for b in range(B):
        s = score_from_dist(D[b])
        r = np.flatnonzero((s >= np.float32(t[b])) & alive)
        r = r[np.lexsort((r, D[b][r]))]
        nr[b] = r.size
        m = min(cap, r.size)
        nf[b] = m
        ids[b, :m] = r[:m].astype(np.uint64) + 1 + off
        sc[b, :m] = s[r[:m]]
        di[b, :m] = D[b][r[:m]]
    return ids, sc, di, nf, nr
