"""tests/like_model.py, the NumPy statement of mx_index_search_like's contract, against things that do not share its code: a second
evaluation of the chain in Python floats, the direction the blend must point in, and a brute-force ranking of the rows that are not
examples.  No GPU."""
import itertools
import math

import numpy as np

from like_model import blank, combine_one, drop_examples, like_combined, norm2


def small_corpus(seed=5, n=60, d=8):
    """n rows of d values; rows 10 .. 15 are exact copies of row 9 and row 40 is zero"""
    X = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    X[10:16] = X[9]
    X[40] = 0
    return X


def rows_of(X, dead=()):
    return lambda i: X[i - 1] if 1 <= i <= len(X) and i not in dead else None


def chain_in_python_floats(terms, dim):
    """the contract once more, on Python floats (IEEE f64) and math.sqrt"""
    c = [0.0] * dim
    for w, v in terms:
        if v is None or float(np.float32(w)) == 0.0:
            continue
        na = 0.0
        for x in v:
            na += float(np.float32(np.float32(x) * np.float32(x)))
        if not na > 0.0:
            continue
        length = math.sqrt(na)
        for j in range(dim):
            c[j] = c[j] + float(np.float32(w)) * (float(v[j]) / length)
    return np.array(c, dtype=np.float64).astype(np.float32)


def test_norm_and_chain_match_a_second_evaluation():
    X = small_corpus()
    rng = np.random.default_rng(6)
    for trial in range(20):
        m = int(rng.integers(1, 6))
        terms = [(np.float32(rng.uniform(-2, 2)), X[int(rng.integers(0, 40))]) for _ in range(m)]   # (row 40 is zero)
        if trial % 3 == 0:
            terms.insert(0, (np.float32(0.7), rng.standard_normal(8).astype(np.float32)))
        got, used = combine_one(8, terms)
        np.testing.assert_array_equal(got.view(np.uint32), chain_in_python_floats(terms, 8).view(np.uint32))
        assert all(used)
        # and it is the blend it claims to be, to rounding
        ref = sum(float(w) * v.astype(np.float64) / np.linalg.norm(v.astype(np.float64)) for w, v in terms)
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-6)
    assert norm2(X[40]) == 0.0 and norm2(np.array([3, 4], np.float32)) == 25.0


def test_positive_and_negative_weights_padding_and_cancelling():
    X = small_corpus()
    ids = np.array([[3, 7, 41, 99, 5, 8],          # a zero row, an id past the end
                    [3, 3, 0, 0, 0, 0],            # the same row twice: it counts twice
                    [3, 3, 0, 0, 0, 0],            # ... once as +w and once as -w: nothing is left
                    [21, 22, 23, 24, 25, 26]], dtype=np.uint64)
    w = np.array([[1, -0.5, 1, 1, 0, 2],
                  [1, 1, 0, 0, 0, 0],
                  [0.25, -0.25, 0, 0, 0, 0],
                  [0, 0, 0, 0, 0, 0]], dtype=np.float32)
    comb, used, n_used = like_combined(rows_of(X), ids, w)
    np.testing.assert_array_equal(used[0], [True, True, False, False, False, True])
    np.testing.assert_array_equal(n_used, [3, 2, 2, 0])
    unit = lambda v: v.astype(np.float64) / np.linalg.norm(v.astype(np.float64))  # noqa: E731
    np.testing.assert_allclose(comb[0], unit(X[2]) - 0.5 * unit(X[6]) + 2 * unit(X[7]), atol=1e-6)
    np.testing.assert_allclose(comb[1], 2 * unit(X[2]), atol=1e-6)
    assert not comb[2].any() and not comb[3].any()
    # weight-0 slots are not even looked up: the same request without them
    short, _, _ = like_combined(rows_of(X), ids[:1, [0, 1, 5]], w[:1, [0, 1, 5]])
    np.testing.assert_array_equal(short.view(np.uint32), comb[:1].view(np.uint32))
    # a caller vector comes first in the chain, and alone it is itself at unit length
    q = np.random.default_rng(8).standard_normal((1, 8)).astype(np.float32)
    alone, used, n_used = like_combined(rows_of(X), ids[3:], w[3:], q, [2.0])
    np.testing.assert_allclose(alone[0], 2 * unit(q[0]), atol=1e-6)
    assert n_used[0] == 0
    zero, _, _ = like_combined(rows_of(X), ids[3:], w[3:], np.zeros((1, 8), np.float32))
    assert not zero.any()
    # removed rows are skipped like ids that name nothing
    comb2, used2, _ = like_combined(rows_of(X, dead={7}), ids[:1], w[:1])
    np.testing.assert_array_equal(used2[0], [True, False, False, False, False, True])
    np.testing.assert_allclose(comb2[0], unit(X[2]) + 2 * unit(X[7]), atol=1e-6)


def brute_force(oracle, X, alive, combined, gone, k):
    """the exact top-k of the live rows other than `gone` (ids), ranked by the oracle on those rows alone"""
    keep = np.array([i for i in np.flatnonzero(alive) if i + 1 not in gone], dtype=np.int64)
    ids, di, sc, nf = oracle.search(X[keep], combined[None, :], k)
    n = int(nf[0])
    return keep[ids[0, :n].astype(np.int64) - 1] + 1, di[0, :n]


def test_drop_from_a_sorted_prefix_is_the_top_k_of_the_rest(oracle):
    """for EVERY subset of the examples being listed or not: search at k + m, drop the used examples, cut to k == brute force over
    the rows that are not used examples.  Exact copies of an example (rows 10 .. 15 of row 9) stay and tie with it."""
    X = small_corpus()
    alive = np.ones(len(X), bool)
    alive[[4, 30]] = False                                    # ids 5 and 31 are removed
    live_rows = np.flatnonzero(alive)
    k = 5
    pool = [10, 12, 33, 50, 5]                                # an example with copies, a copy of it, two others, a removed row
    for size in range(1, len(pool) + 1):
        for ex in itertools.combinations(pool, size):
            for sign in (1.0, -1.0):
                m = len(ex)
                w = np.ones((1, m), np.float32)
                w[0, 1:] = sign * 0.5                         # the later examples pull away when sign < 0: they leave the list
                ids = np.array([ex], dtype=np.uint64)
                comb, used, n_used = like_combined(rows_of(X, dead={5, 31}), ids, w, dim=8)
                assert n_used[0] == m - (5 in ex)
                if n_used[0] == 0:                            # the removed row alone: a blank request
                    assert not comb.any()
                    continue
                oi, od, osc, onf = oracle.search(X[live_rows], comb, k + m)
                oi = np.where(oi != 0, live_rows[np.maximum(oi.astype(np.int64), 1) - 1] + 1, 0).astype(np.uint64)
                got = drop_examples((oi, osc, od, onf), ids, used, comb, k, True)
                gone = set(int(i) for i in ids[0][used[0]])
                want_ids, want_d = brute_force(oracle, X, alive, comb[0], gone, k)
                assert got[3][0] == k
                np.testing.assert_array_equal(got[0][0], want_ids.astype(np.uint64))
                np.testing.assert_array_equal(got[2][0].view(np.uint32), want_d.view(np.uint32))
                assert not gone & set(int(i) for i in got[0][0])
                kept = drop_examples((oi, osc, od, onf), ids, used, comb, k, False)      # exclude = 0: the plain list, cut
                np.testing.assert_array_equal(kept[0][0], oi[0, :k])
    # the example with the largest id among seven exact copies, positives only: six copies fill the k + 1 listed, nothing is dropped
    ids = np.array([[16]], dtype=np.uint64)
    comb, used, _ = like_combined(rows_of(X), ids)
    oi, od, osc, onf = oracle.search(X, comb, k + 1)
    got = drop_examples((oi, osc, od, onf), ids, used, comb, k, True)
    np.testing.assert_array_equal(got[0][0], [10, 11, 12, 13, 14])


def test_blank_requests_find_nothing(oracle):
    X = small_corpus()
    ids = np.array([[3, 3], [41, 99], [3, 4]], dtype=np.uint64)
    w = np.array([[1, -1], [1, 1], [1, 1]], dtype=np.float32)
    comb, used, n_used = like_combined(rows_of(X), ids, w)
    np.testing.assert_array_equal(n_used, [2, 0, 2])
    oi, od, osc, onf = oracle.search(X, comb, 6)              # a zero query lists the first rows by id at dist 0: not an answer
    assert onf[0] == 6
    got = drop_examples((oi, osc, od, onf), ids, used, comb, 4, True)
    want = blank(3, 4)
    for g, wnt in zip(got, want):
        np.testing.assert_array_equal(g[:2], wnt[:2])
    assert got[3][2] == 4 and not np.isin(got[0][2], [3, 4]).any()
