"""The NumPy statement of diversified search (tests/mmr_model.py) against cases worked out by hand and against the properties the
contract promises.  No GPU: this pins the model the GPU tests compare with, bit for bit."""
import numpy as np

from conftest import bits
from mmr_model import default_fetch, greedy, mmr_model, near_copy_corpus, queries_near_centres
from oracle.search_oracle import score_from_dist


def test_hand_case_skips_the_near_copy(oracle):
    """q = (1, 0).  a = (1, .05) and b = (1, .06) are near-copies (cosine 0.99995), c = (.8, -.6), d = (0, 1).
    Plain order: a (0.99875), b (0.99820), c (0.8), d (0).  After a, at lam = 0.5:
      v_b = .5 * .99820 - .5 * .99995 = -0.0009,  v_c = .5 * .8 - .5 * .7690 = +0.0155,  v_d = 0 - .5 * .0499 = -0.0250  -> c
    then pen_b stays .99995 (sim(b, c) = .7626), pen_d stays .0499 (sim(d, c) = -.6): v_b = -0.0009 > v_d = -0.0250 -> b, then d."""
    X = np.array([[1, .05], [1, .06], [.8, -.6], [0, 1]], np.float32)
    q = np.array([[1, 0]], np.float32)
    ids, sc, di, nf = mmr_model(oracle, X, q, 4, fetch=4, lam=0.5)
    assert ids.tolist() == [[1, 3, 2, 4]] and nf.tolist() == [4]
    pi, pd, ps, _ = oracle.search(X, q, 4)
    assert pi.tolist() == [[1, 2, 3, 4]]
    # every entry keeps its candidate's score and dist
    np.testing.assert_array_equal(bits(sc[0]), bits(ps[0][[0, 2, 1, 3]]))
    np.testing.assert_array_equal(bits(di[0]), bits(pd[0][[0, 2, 1, 3]]))
    assert abs(float(sc[0, 1]) - 0.8) < 1e-6
    # k = 2: the second pick is c, not the near-copy
    assert mmr_model(oracle, X, q, 2, fetch=4, lam=0.5)[0].tolist() == [[1, 3]]
    # lam = 1: relevance only
    assert mmr_model(oracle, X, q, 2, fetch=4, lam=1.0)[0].tolist() == [[1, 2]]
    assert mmr_model(oracle, X, q, 4, fetch=4, lam=1.0)[0].tolist() == [[1, 2, 3, 4]]


def test_block_distances_are_the_pair_distances(oracle):
    """the model takes a picked row's distances to all candidates from all_dists: the same values as COracle.dist pair by pair"""
    rng = np.random.default_rng(3)
    R = rng.standard_normal((40, 100)).astype(np.float32)
    R[5] = 0
    R[6] = R[2]
    for j in (0, 2, 5, 17):
        blk = oracle.all_dists(R, R[j])
        one = np.array([oracle.dist(R[j], R[i]) for i in range(40)], np.float32)
        np.testing.assert_array_equal(bits(blk), bits(one))


def test_lam_one_is_the_plain_prefix(oracle):
    rng = np.random.default_rng(4)
    X, centres = near_copy_corpus(rng, clusters=20, per=10, d=64)
    Q = queries_near_centres(rng, centres, 9)
    for k, fetch in ((1, 1), (5, 5), (5, 40), (10, None)):
        ids, sc, di, nf = mmr_model(oracle, X, Q, k, fetch=fetch, lam=1.0)
        pi, pd, ps, pnf = oracle.search(X, Q, k)
        np.testing.assert_array_equal(ids, pi)
        np.testing.assert_array_equal(bits(sc), bits(ps))
        np.testing.assert_array_equal(bits(di), bits(pd))
        np.testing.assert_array_equal(nf, pnf)
    assert default_fetch(10) == 40 and default_fetch(3) == 32 and default_fetch(500) == 1024


def test_fetch_equal_k_is_a_permutation_starting_with_the_best(oracle):
    rng = np.random.default_rng(5)
    X, centres = near_copy_corpus(rng, clusters=20, per=10, d=64)
    Q = queries_near_centres(rng, centres, 9)
    for lam in (0.0, 0.3, 0.7):
        ids, sc, di, nf = mmr_model(oracle, X, Q, 12, fetch=12, lam=lam)
        pi, pd, ps, _ = oracle.search(X, Q, 12)
        np.testing.assert_array_equal(ids[:, 0], pi[:, 0])
        np.testing.assert_array_equal(np.sort(ids, axis=1), np.sort(pi, axis=1))
        for b in range(9):                                              # scores and dists travel with their ids
            back = {int(i): (s, d) for i, s, d in zip(pi[b], bits(ps[b]), bits(pd[b]))}
            assert all(back[int(i)] == (s, d) for i, s, d in zip(ids[b], bits(sc[b]), bits(di[b])))
    assert (mmr_model(oracle, X, Q, 12, fetch=12, lam=0.3)[0] != oracle.search(X, Q, 12)[0]).any()
    # more wanted than the corpus holds: n_found = rows, the unused slots blank
    ids, sc, di, nf = mmr_model(oracle, X[:7], Q, 10, fetch=16, lam=0.5)
    assert (nf == 7).all() and (ids[:, 7:] == 0).all() and (sc[:, 7:] == 0).all() and np.isinf(di[:, 7:]).all()


def test_exact_duplicates_of_the_first_pick_come_last_among_equals(oracle):
    """Rows 4 and 9 repeat row 1 (the query): their similarity to the first pick is exactly 1, the largest penalty there is.  At lam = 0
    they are therefore picked after every other row, and between the two of them -- equal values -- the smaller id goes first."""
    rng = np.random.default_rng(6)
    X = rng.standard_normal((12, 16)).astype(np.float32)
    X[4] = X[1]
    X[9] = X[1]
    q = X[1:2]
    sim = score_from_dist(oracle.all_dists(X, X[1]))
    assert sim[4] == 1.0 and sim[9] == 1.0 and (np.delete(sim, [1, 4, 9]) < 1.0).all()
    ids = mmr_model(oracle, X, q, 12, fetch=12, lam=0.0)[0]
    assert ids[0, 0] == 2 and ids[0, -2:].tolist() == [5, 10]
    # with relevance in play the duplicates still tie with each other: the earlier candidate first
    ids = mmr_model(oracle, X, q, 12, fetch=12, lam=0.5)[0][0].tolist()
    assert ids[0] == 2 and ids.index(5) < ids.index(10)
    # the tie rule on its own: equal values go to the smaller position
    R = np.array([[1, 0], [0, 1], [0, 1], [0, 1]], np.float32)
    assert greedy(oracle, R, np.array([1, 0, 0, 0], np.float32), 4, 0.5) == [0, 1, 2, 3]


def test_near_copy_corpus_is_diversified(oracle):
    """150 clusters of 20 near-copies at 384 dims (overlapping windows of 150 documents): at lam = 0.5 the selection differs from the
    plain top-10 for at least half of 32 queries drawn near cluster centres.  A condition on the inputs the GPU tests reuse."""
    rng = np.random.default_rng(7)
    X, centres = near_copy_corpus(rng)
    assert X.shape == (3000, 384)
    Q = queries_near_centres(rng, centres, 32)
    ids, sc, di, nf = mmr_model(oracle, X, Q, 10, fetch=64, lam=0.5)
    pi = oracle.search(X, Q, 10)[0]
    differs = (ids != pi).any(axis=1)
    assert differs.sum() >= 16, int(differs.sum())
    assert (ids[:, 0] == pi[:, 0]).all() and (nf == 10).all()
    # the plain top-10 sits in one cluster; the selection reaches into others
    spread = lambda rows: np.mean([len({(int(i) - 1) // 20 for i in row}) for row in rows])  # noqa: E731  clusters per answer
    assert spread(pi) < 1.5 and spread(ids) > spread(pi)
