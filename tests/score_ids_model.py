"""The contract of the scoring of named rows (mx_index_score_ids) restated in NumPy -- TEST INFRASTRUCTURE,
not product code.

An entry is found iff the plain search over every live row would list its id, and then holds that list's score and dist; ``order`` is
the found positions sorted by (place in the plain list, position in the candidate list).  ``from_plain_lists`` takes the plain lists
from whoever computed them; tests/test_score_ids_gpu.py gives it the library's own plain call.  (tests/index_model.py does not use
this module: its ``IndexModel._score`` is written straight from the header, from the oracle's dist of every row, so that the random
walk's expectation shares no step with this one.)
"""
import numpy as np


def from_plain_lists(plain, n, ids, off=0):
    """plain: (ids, scores, dists, n_found) of a plain search that lists every live row; n: the rows of the index; ids [B, m] ->
    (scores, dists, order, n_found) as FlatIndex.score_ids returns them"""
    pi, ps, pd, pnf = plain
    B, m = ids.shape
    sc = np.zeros((B, m), np.float32)
    di = np.full((B, m), np.inf, np.float32)
    order = np.full((B, m), -1, np.int32)
    nf = np.zeros(B, np.int32)
    for b in range(B):
        place = np.full(n + 1, -1, np.int64)                               # row (1-based, offset taken off) -> place in the plain list
        place[(pi[b, :pnf[b]] - np.uint64(off)).astype(np.int64)] = np.arange(pnf[b])
        c = ids[b]
        ok = (c > np.uint64(off)) & (c <= np.uint64(off + n))
        p = np.where(ok, place[np.where(ok, c - np.uint64(off), 0).astype(np.int64)], -1)
        found = p >= 0
        sc[b, found] = ps[b, p[found]]
        di[b, found] = pd[b, p[found]]
        js = np.flatnonzero(found)
        js = js[np.lexsort((js, p[js]))]
        order[b, :len(js)] = js
        nf[b] = len(js)
    return sc, di, order, nf
