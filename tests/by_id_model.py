"""The contract of search by stored row (mx_index_search_by_id / mx_index_search_range_by_id) restated in
NumPy -- TEST INFRASTRUCTURE, not product code.

The answer is stated through the plain calls: the stored row as the query at k + e (or a range search that lists everything in
range), the own id dropped, the rest cut to k.  ``drop_own`` is those last steps on whatever produced the plain lists: the library's
own plain calls in tests/test_by_id_gpu.py, the oracle in tests/index_model.py.
"""
import numpy as np


def blank(B, k, counts=False):
    out = [np.zeros((B, k), np.uint64), np.zeros((B, k), np.float32), np.full((B, k), np.inf, np.float32), np.zeros(B, np.int32)]
    return out + [np.zeros(B, np.uint64)] if counts else out


def drop_own(lists, qids, ok, k, e, counts=None):
    """the contract's last three steps on the plain call's lists: drop the own id, cut to k, count"""
    ids, sc, di, nf = lists
    out = blank(len(qids), k, counts is not None)
    for b in np.flatnonzero(ok):
        keep = [j for j in range(int(nf[b])) if not (e and int(ids[b, j]) == int(qids[b]))]
        if counts is not None:                                  # (everything in range is listed: membership is "it is in the list")
            assert counts[b] == nf[b], "the model's cap does not list everything in range"
            out[4][b] = len(keep)
        keep = keep[:k]
        out[0][b, :len(keep)], out[1][b, :len(keep)], out[2][b, :len(keep)], out[3][b] = ids[b, keep], sc[b, keep], di[b, keep], len(keep)
    return out
