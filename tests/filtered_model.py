"""The contract of filtered search and of resident filters (mx_index_search_filtered, mx_filter, DESIGN.md sections 3.8 and 3.12)
restated in NumPy -- TEST INFRASTRUCTURE, not product code.

A filter is a boolean per global row (id - id_offset - 1).  The answer of a filtered search is the oracle's on the allowed rows that
are not removed, with the oracle's row numbers mapped back to ids (the oracle orders ties by row, and that order is monotone in id, so
the tie order carries over).
"""
import numpy as np


def allowed_mask(n, ranges, off=0):
    a = np.zeros(n, dtype=bool)
    for lo, hi in np.asarray(ranges, dtype=np.int64).reshape(-1, 2):
        lo, hi = max(lo - off - 1, 0), min(hi - off - 1, n)
        if lo < hi:
            a[lo:hi] = True
    return a


def subset_oracle(oracle, rows, keep, Q, k, off=0):
    """-> (ids, scores, dists, n_found), the order FlatIndex.search returns them in"""
    ids = np.flatnonzero(keep).astype(np.uint64) + 1 + off
    if ids.size == 0:  # nothing allowed: every slot empty
        B = Q.shape[0]
        return (np.zeros((B, k), np.uint64), np.zeros((B, k), np.float32), np.full((B, k), np.inf, np.float32), np.zeros(B, np.int32))
    oi, od, os_, onf = oracle.search(rows[keep], Q, k)
    mapped = np.where(oi > 0, ids[np.maximum(oi.astype(np.int64) - 1, 0)], 0).astype(np.uint64)
    return mapped, os_, od, onf


def model_ranges(a, off=0):
    """bool [n] -> the normalised id ranges mx_filter_get_ranges must report"""
    e = np.flatnonzero(np.diff(np.r_[0, a.astype(np.int8), 0]))
    return (e.reshape(-1, 2) + 1 + off).astype(np.uint64)


def ids_of(ranges):
    r = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    return np.concatenate([np.arange(lo, hi) for lo, hi in r] + [np.zeros(0, np.int64)]).astype(np.uint64)
