"""The statement of boosted search (tests/boosted_model.py) against brute force over all rows, without a GPU: whenever the model says
`complete`, its answer is the true top-k of all rows by (combined descending, dist, id) -- the certificate of DESIGN.md section 3.17."""
import numpy as np
import pytest

from boosted_model import PriorModel, boost_lists, boosted_model, brute_force_boosted, case_a, case_b, combine, default_fetch
from conftest import bits
from grouped_model import candidate_lists

_CACHE = {}


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def tied():
    """200 vectors at d = 16, each stored three times (exact ties in score): 600 rows.  By draw the three copies of a vector share one
    prior (ties in the combined value, broken by id) or get three different ones (the copies are re-ordered)"""
    if "tied" not in _CACHE:
        rng = np.random.default_rng(317)
        V = rng.standard_normal((200, 16)).astype(np.float32)
        X = np.ascontiguousarray(np.concatenate([V, V, V]))
        Q = (V[rng.integers(0, 200, 6)] + 0.2 * rng.standard_normal((6, 16))).astype(np.float32)
        shared = rng.random(200).astype(np.float32)
        pv = np.where(np.tile(rng.random(200) < 0.5, 3), np.tile(shared, 3), rng.random(600).astype(np.float32)).astype(np.float32)
        _CACHE["tied"] = (X, Q, pv)
    return _CACHE["tied"]


def same_as_brute_force(oracle, X, q, pv, w, k, got, b, alive=None):
    ids, sc, di, pr, cb, nf, done = got
    wi, wd, wc = brute_force_boosted(oracle, X, q, pv, w, k, alive)
    n = int(nf[b])
    assert n == len(wi)
    np.testing.assert_array_equal(ids[b, :n], wi)
    np.testing.assert_array_equal(bits(di[b, :n]), bits(wd))
    np.testing.assert_array_equal(bits64(cb[b, :n]), bits64(wc))


@pytest.mark.parametrize("k", [1, 5, 10])
@pytest.mark.parametrize("w", [0.0, 0.05, 1.0])
def test_complete_means_the_true_top_k(k, w, oracle):
    X, Q, pv = tied()
    seen = {True: 0, False: 0}
    for fetch in (k, 4 * k, 64, 300, 601):
        got = boosted_model(oracle, X, Q, k, pv, w=w, fetch=fetch)
        if fetch > 600:
            assert got[6].all(), "a list shorter than fetch holds every row"
        for b in range(len(Q)):
            seen[bool(got[6][b])] += 1
            if got[6][b]:
                same_as_brute_force(oracle, X, Q[b], pv, w, k, got, b)
    assert seen[True] and seen[False], "(condition on the input) both outcomes of the certificate must occur"


def test_equal_priors_order_ties_by_position(oracle):
    """the three copies of a vector have bit-equal scores: under one prior they stay in id order, and a larger prior on the last copy
    moves it to the front"""
    X, Q, _ = tied()
    pv = np.full(600, 0.25, np.float32)
    ids, _, _, _, cb, nf, done = boosted_model(oracle, X, Q, 3, pv, w=0.5, fetch=601)
    for b in range(len(Q)):
        assert list(ids[b]) == [ids[b, 0], ids[b, 0] + 200, ids[b, 0] + 400] and len(set(bits64(cb[b]).tolist())) == 1
    first = ids[:, 0].astype(np.int64) - 1
    pv2 = pv.copy()
    pv2[first + 400] = 0.5
    ids2 = boosted_model(oracle, X, Q, 3, pv2, w=0.5, fetch=601)[0]
    for b in range(len(Q)):
        assert list(ids2[b]) == [ids[b, 0] + 400, ids[b, 0], ids[b, 0] + 200]


def test_case_a_every_query_is_complete(oracle):
    X, Q, pv = case_a()
    got = boosted_model(oracle, X, Q, 5, pv, w=0.05, fetch=32)
    assert got[6].all() and (got[5] == 5).all(), "(condition on the input) Case A must be complete for every query"
    plain = candidate_lists(oracle, X, Q, 5)[0]
    assert (got[0] != plain).any(), "(condition on the input) the priors must re-order some answer"
    for b in range(len(Q)):
        same_as_brute_force(oracle, X, Q[b], pv, 0.05, 5, got, b)


def test_case_b_a_far_row_with_a_large_prior_is_not_claimed(oracle):
    X, Q, pv, far = case_b(oracle)
    ci, cs, cd, cnf = candidate_lists(oracle, X, Q, 32)
    assert far + 1 not in ci[0].tolist(), "(condition on the input) the far row must be outside query 0's list"
    ids, _, _, pr, _, nf, done = boost_lists(ci, cs, cd, cnf, pv, 1.0, np.float32(100.0), 5, 32)
    assert not done[0] and nf[0] == 5 and (pr[0] == 0).all()
    assert brute_force_boosted(oracle, X, Q[0], pv, 1.0, 5)[0][0] == far + 1
    # with every candidate in the list (fetch past the rows) the row is found, first, and the answer is complete
    got = boosted_model(oracle, X, Q[:1], 5, pv, w=1.0, hi=np.float32(100.0), fetch=2001)
    assert got[6][0] and got[0][0, 0] == far + 1 and got[3][0, 0] == 100.0
    same_as_brute_force(oracle, X, Q[0], pv, 1.0, 5, got, 0)


def test_weight_zero_is_the_plain_list(oracle):
    X, Q, pv = case_a()
    ci, cs, cd, cnf = candidate_lists(oracle, X, Q, 32)
    ids, sc, di, pr, cb, nf, _ = boost_lists(ci, cs, cd, cnf, pv, 0.0, np.float32(1.0), 10, 32)
    np.testing.assert_array_equal(ids, ci[:, :10])
    np.testing.assert_array_equal(bits(sc), bits(cs[:, :10]))
    np.testing.assert_array_equal(bits(di), bits(cd[:, :10]))
    np.testing.assert_array_equal(bits64(cb), bits64(cs[:, :10].astype(np.float64)))
    assert (pr == pv[ci[:, :10].astype(np.int64) - 1]).all() and (nf == 10).all()


def test_negative_priors_are_a_penalty(oracle):
    X, Q, _ = case_a()
    best = candidate_lists(oracle, X, Q, 32)[0][:, 0].astype(np.int64) - 1
    pv = np.zeros(X.shape[0], np.float32)
    pv[best] = -3.0
    got = boosted_model(oracle, X, Q, 5, pv, w=1.0, fetch=32)               # hi = 0: the rest of the corpus has prior 0
    assert got[6].all()
    for b in range(len(Q)):
        assert best[b] + 1 not in got[0][b].tolist()
        same_as_brute_force(oracle, X, Q[b], pv, 1.0, 5, got, b)
    # with k = fetch the penalised row is reported last, and nothing outside is ruled out: the k-th c is below U
    got = boosted_model(oracle, X, Q, 32, pv, w=1.0, fetch=32)
    assert (got[0][:, -1] == best + 1).all() and not got[6].any()


def test_short_lists_blanks_and_alive(oracle):
    X, Q, pv = tied()
    alive = np.ones(600, bool)
    alive[::3] = False
    got = boosted_model(oracle, X[:7], Q, 10, pv[:7], w=0.3, fetch=16, alive=alive[:7])
    ids, sc, di, pr, cb, nf, done = got
    assert (nf == 4).all() and done.all()
    assert (ids[:, 4:] == 0).all() and (sc[:, 4:] == 0).all() and np.isinf(di[:, 4:]).all() and (pr[:, 4:] == 0).all() and (cb[:, 4:] == 0).all()
    for b in range(len(Q)):
        same_as_brute_force(oracle, X[:7], Q[b], pv[:7], 0.3, 10, got, b, alive=alive[:7])
    got = boosted_model(oracle, X, Q, 5, pv, w=0.05, fetch=601, alive=alive)
    for b in range(len(Q)):
        same_as_brute_force(oracle, X, Q[b], pv, 0.05, 5, got, b, alive=alive)


def test_an_exact_tie_with_the_bound_is_not_complete():
    """one list of two entries, k = 1, fetch = 2: the reported c equals U bit for bit -> 0; one ulp more -> 1"""
    ci = np.asarray([[1, 2]], np.uint64)
    cs = np.asarray([[0.75, 0.5]], np.float32)
    cd = np.asarray([[0.25, 0.5]], np.float32)
    cnf = np.asarray([2], np.int32)
    pv = np.asarray([0.25, 0.5], np.float32)                                # c = 1.0 and 1.0; U = 0.5 + 1 * 0.5 = 1.0
    out = boost_lists(ci, cs, cd, cnf, pv, 1.0, np.float32(0.5), 1, 2)
    assert out[0][0, 0] == 1 and out[4][0, 0] == 1.0 and not out[6][0]
    pv[0] = np.nextafter(np.float32(0.25), np.float32(1))
    out = boost_lists(ci, cs, cd, cnf, pv, 1.0, np.float32(0.5), 1, 2)
    assert out[6][0]


def test_the_edit_rules_and_the_bound():
    p = PriorModel()
    assert p.bound() == 0
    p.set_ranges([[1, 5], [9, 11]], [0.5, -2.0], 0, 10)
    assert p.vals.tolist() == [0.5, 0.5, 0.5, 0.5, 0, 0, 0, 0, -2.0, -2.0] and p.bound() == 0.5
    p.set_ids([5, 5, 12, 0], [3.0, 3.0, 9.0, 4.0], 0, 10)                  # the same bits twice are fine; ids outside are ignored
    assert p.vals[4] == 3.0 and p.bound() == 9.0, "hi follows what the call was handed"
    before, hi = p.vals.copy(), p.hi
    for bad in (lambda: p.set_ranges([[1, 5], [4, 6]], [1, 2], 0, 10), lambda: p.set_ranges([[5, 4]], [1], 0, 10),
                lambda: p.set_ids([2, 3, 2], [1.0, 1.0, 2.0], 0, 10), lambda: p.set_ids([2], [np.nan], 0, 10),
                lambda: p.set_ids([2, 3], [50.0, np.inf], 0, 10), lambda: p.set_ranges([[1, 3]], [-np.inf], 0, 10),
                lambda: p.set_ids([2, 2], [0.0, -0.0], 0, 10)):
        with pytest.raises(ValueError):
            bad()
        assert (p.vals == before).all() and p.hi == hi
    # overwriting large values with small ones leaves hi where it was; refresh recomputes it over the live rows and 0
    p.set_ids([5], [0.25], 0, 10)
    assert p.bound() == 9.0 and p.bound(refresh=True, size=10) == 0.5
    alive = np.ones(10, bool)
    alive[:4] = False
    assert p.bound(refresh=True, size=10, alive=alive) == 0.25
    p.set_ranges([[1, 11]], [-1.0], 0, 10)
    assert p.bound() == 0.25 and p.bound(refresh=True, size=10) == 0.0, "0 is always a member: rows nobody set read 0"
    p.set_ids([105], [6.0], 100, 12)                                        # under an id offset, after two rows were appended
    assert p.values_of([105, 109, 113, 100, 5], 100, 12).tolist() == [6.0, -1.0, 0, 0, 0] and p.vals.size == 12


def test_combined_is_rounded_once():
    rng = np.random.default_rng(5)
    s, w, v = (rng.standard_normal(1000).astype(np.float32) for _ in range(3))
    exact = [float(a) + float(b) * float(c) for a, b, c in zip(s, w, v)]     # f32 x f32 is exact in f64: one rounding, in the sum
    assert all(bits64(combine(a, b, c)) == bits64(e) for a, b, c, e in zip(s, w, v, exact))
    import math
    assert all(math.fma(float(b), float(c), float(a)) == e for a, b, c, e in zip(s, w, v, exact)) if hasattr(math, "fma") else True


def test_default_fetch():
    assert [default_fetch(k) for k in (1, 8, 10, 64, 100, 256, 300, 4096)] == [32, 32, 40, 256, 256, 256, 300, 4096]
