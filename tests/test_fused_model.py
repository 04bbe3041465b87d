"""The statement of fused search (tests/fused_model.py) checked against what it claims, without a GPU: MX_FUSE_MAX computed from the
per-sub-query top-`fetch` lists IS the global top-k by the best dist over the sub-queries, and the f64 sum of MX_FUSE_RRF does not
depend on which of two mirrored rows is which."""
import numpy as np

from conftest import bits
from fused_model import MAX, RRF, brute_force_max, default_fetch, fuse_lists, fused_model, tripled_corpus
from mmr_model import queries_near_centres


def test_max_from_the_lists_is_the_global_top_k(oracle):
    """every row stored three times: exact ties inside every list and across the cut at k and at fetch"""
    rng = np.random.default_rng(7)
    X, centres = tripled_corpus(rng, clusters=40, per=10, d=64)
    m, k = 4, 10
    for trial in range(6):
        # two sub-queries near one centre, two near others: the lists overlap partly
        c = rng.integers(0, len(centres), 3)
        Q = queries_near_centres(rng, centres[[c[0], c[0], c[1], c[2]]], m) if trial else queries_near_centres(rng, centres[[c[0]] * m], m)
        want_ids, want_d, want_sub = brute_force_max(oracle, X, Q, k)
        for fetch in (k, 3 * k):
            ids, sc, di, nf, best, fused = fused_model(oracle, X, Q, k, mode=MAX, fetch=fetch)
            assert nf[0] == k
            np.testing.assert_array_equal(ids[0], want_ids, err_msg=f"trial {trial}, fetch {fetch}")
            np.testing.assert_array_equal(bits(di[0]), bits(want_d))
            np.testing.assert_array_equal(best[0], want_sub)
            np.testing.assert_array_equal(fused[0], sc[0].astype(np.float64))
        # (condition on the input: the ties are there -- the three copies of a row sit side by side)
        assert (np.diff(bits(want_d).astype(np.int64)) == 0).sum() >= k // 2


def test_max_finds_min_k_live_rows_and_ignores_absent_lists(oracle):
    rng = np.random.default_rng(8)
    X, centres = tripled_corpus(rng, clusters=3, per=2, d=16)            # 18 rows
    Q = queries_near_centres(rng, centres, 3)
    ids, sc, di, nf, best, fused = fused_model(oracle, X, Q, 25, mode=MAX, fetch=30)
    assert nf[0] == 18 and (ids[0, 18:] == 0).all() and (best[0, 18:] == -1).all() and np.isposinf(di[0, 18:]).all()
    assert (sc[0, 18:] == 0).all() and (fused[0, 18:] == 0).all()
    assert sorted(ids[0, :18]) == list(range(1, 19))                     # each row once
    # weight 0 = the call without that sub-query, best_sub mapped
    a = fused_model(oracle, X, Q, 10, mode=MAX, weights=[[1.0, 0.0, 2.0]])
    b = fused_model(oracle, X, Q[[0, 2]], 10, mode=MAX)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[4], np.asarray([0, 2])[b[4]])
    assert fused_model(oracle, X, Q, 10, mode=RRF, weights=[[0.0, 0.0, 0.0]])[3][0] == 0


def test_rrf_mirrored_pair_is_bit_equal_and_falls_in_id_order():
    # list 0: rows 9, 4, 7; list 1: rows 4, 9, 8 -- rows 9 and 4 sit at ranks (1, 2) and (2, 1)
    ids = np.asarray([[9, 4, 7], [4, 9, 8]], np.uint64)
    d = np.asarray([[0.1, 0.2, 0.3], [0.05, 0.25, 0.3]], np.float32)
    s = (1 - d).astype(np.float32)
    for w, c in ((1.0, 60.0), (0.3, 0.0), (7.5, 1e-3)):
        oi, osc, od, n, ob, of = fuse_lists(ids, d, s, [3, 3], [w, w], 4, RRF, rrf_c=c)
        assert n == 4 and list(oi) == [4, 9, 7, 8]                        # the pair in id order, then 7 and 8 (equal fused) in id order
        assert of[0].tobytes() == of[1].tobytes() and of[2].tobytes() == of[3].tobytes()
        w32, c32 = float(np.float32(w)), float(np.float32(c))
        assert of[1] == w32 / (c32 + 1.0) + w32 / (c32 + 2.0) and of[2] == w32 / (c32 + 3.0)
        assert list(ob) == [1, 0, 0, 1]                                   # row 4 is nearer in list 1, row 9 in list 0
        np.testing.assert_array_equal(bits(od), bits(np.asarray([0.05, 0.1, 0.3, 0.3], np.float32)))
    # unequal weights break the tie
    oi = fuse_lists(ids, d, s, [3, 3], [1.0, 2.0], 2, RRF)[0]
    assert list(oi) == [4, 9]
    oi = fuse_lists(ids, d, s, [3, 3], [2.0, 1.0], 2, RRF)[0]
    assert list(oi) == [9, 4]


def test_default_fetch():
    assert default_fetch(10, MAX) == 10 and default_fetch(10, RRF) == 40 and default_fetch(2, RRF) == 32 and default_fetch(100, RRF) == 256
