"""The statement of grouped search (tests/grouped_model.py) against brute force over all rows, without a GPU: whenever the model says
`complete`, its heads are the true top-k groups with their true best rows -- the certificate of DESIGN.md section 3.16."""
import numpy as np
import pytest

from conftest import bits
from grouped_model import GroupingModel, brute_force_groups, default_fetch, grouped_model, random_keys

_CACHE = {}


def tied():
    """200 vectors at d = 16, each stored three times (exact ties): 600 rows; keys in groups of 1 - 4 rows, a fifth ungrouped.  The
    groups are cut from the rows ordered by vector, so the copies of a vector tend to share one and meet in the lists"""
    if "tied" not in _CACHE:
        rng = np.random.default_rng(316)
        V = rng.standard_normal((200, 16)).astype(np.float32)
        X = np.ascontiguousarray(np.concatenate([V, V, V]))
        Q = (V[rng.integers(0, 200, 6)] + 0.2 * rng.standard_normal((6, 16))).astype(np.float32)
        order = (rng.permutation(200)[:, None] + 200 * np.arange(3)[None, :]).reshape(-1)
        _CACHE["tied"] = (X, Q, random_keys(rng, 600, order=order))
    return _CACHE["tied"]


@pytest.mark.parametrize("k", [1, 5, 10])
def test_complete_means_the_true_top_k_groups(k, oracle):
    X, Q, keys = tied()
    seen_incomplete = False
    for fetch in (k, 2 * k, 4 * k, 64):
        ids, sc, di, gk, rows, nf, done = grouped_model(oracle, X, Q, k, keys, fetch=fetch)
        if fetch >= 4 * k:
            assert done.all(), "groups hold at most 4 rows: 4 k entries hold k heads"
        seen_incomplete |= bool((~done).any())
        for b in range(len(Q)):
            if not done[b]:
                assert nf[b] < k
                continue
            wi, wd, wk = brute_force_groups(oracle, X, Q[b], k, keys)
            n = int(nf[b])
            assert n == len(wi) == k
            np.testing.assert_array_equal(ids[b, :n], wi, err_msg=f"k {k} fetch {fetch} query {b}: heads")
            np.testing.assert_array_equal(bits(di[b, :n]), bits(wd))
            np.testing.assert_array_equal(gk[b, :n], wk)
            assert (rows[b, :n] >= 1).all() and (rows[b, :n][gk[b, :n] == 0] == 1).all()
    if k > 1:
        assert seen_incomplete, "(condition on the input) fetch = k must fall short for some query: tied rows share lists"


def test_ties_are_listed_in_id_order(oracle):
    """the three copies of a vector have bit-equal dists: under three different keys they head three groups, smallest id first"""
    X, Q, _ = tied()
    keys = np.repeat(np.asarray([1, 2, 3], np.uint32), 200)
    ids, _, di, gk, rows, nf, done = grouped_model(oracle, X, Q, 3, keys, fetch=9)
    assert done.all() and (nf == 3).all()
    for b in range(len(Q)):
        assert list(gk[b]) == [1, 2, 3] and list(ids[b]) == [ids[b, 0], ids[b, 0] + 200, ids[b, 0] + 400]
        assert len(set(bits(di[b]).tolist())) == 1 and list(rows[b]) == [3, 3, 3]


def test_one_large_group_is_reported_incomplete(oracle):
    """40 near-copies of the query under one key fill the 32 candidates: one head, and the model does not claim more"""
    rng = np.random.default_rng(317)
    X = rng.standard_normal((600, 16)).astype(np.float32)
    q = rng.standard_normal(16).astype(np.float32)
    X[100:140] = q + 1e-3 * rng.standard_normal((40, 16)).astype(np.float32)
    keys = np.zeros(600, np.uint32)
    keys[100:140] = 9
    ids, _, _, gk, rows, nf, done = grouped_model(oracle, X, q, 3, keys, fetch=32)
    assert not done[0] and nf[0] == 1 and gk[0, 0] == 9 and rows[0, 0] == 32 and 101 <= ids[0, 0] <= 140
    assert (ids[0, 1:] == 0).all() and (gk[0, 1:] == 0).all() and (rows[0, 1:] == 0).all()
    ids, _, _, gk, rows, nf, done = grouped_model(oracle, X, q, 3, keys, fetch=64)       # 40 + 24: three heads
    assert done[0] and nf[0] == 3 and list(gk[0]) == [9, 0, 0] and list(rows[0]) == [40, 1, 1]
    wi, _, wk = brute_force_groups(oracle, X, q, 3, keys)
    np.testing.assert_array_equal(ids[0], wi)
    np.testing.assert_array_equal(gk[0], wk)
    # a list shorter than fetch holds every row: complete although fewer than k groups exist
    ids, _, _, gk, _, nf, done = grouped_model(oracle, X[100:140], q, 3, keys[100:140], fetch=64)
    assert done[0] and nf[0] == 1


def test_removed_and_filtered_rows(oracle):
    X, Q, keys = tied()
    alive = np.ones(600, bool)
    alive[::7] = False
    allowed = np.zeros(600, bool)
    allowed[50:500] = True
    ids, _, di, gk, _, nf, done = grouped_model(oracle, X, Q, 5, keys, fetch=20, alive=alive, allowed=allowed)
    assert done.all()
    for b in range(len(Q)):
        wi, wd, wk = brute_force_groups(oracle, X, Q[b], 5, keys, alive=alive & allowed)
        np.testing.assert_array_equal(ids[b], wi)
        np.testing.assert_array_equal(bits(di[b]), bits(wd))
        np.testing.assert_array_equal(gk[b], wk)


def test_the_edit_rules():
    g = GroupingModel()
    g.set_ranges([[1, 5], [9, 11]], [7, 8], 0, 10)
    assert g.keys.tolist() == [7, 7, 7, 7, 0, 0, 0, 0, 8, 8]               # clipped to the 10 rows
    g.set_ids([5, 5, 12, 0], [3, 3, 4, 4], 0, 10)                          # the same key twice is fine; ids outside are ignored
    assert g.keys.tolist() == [7, 7, 7, 7, 3, 0, 0, 0, 8, 8]
    before = g.keys.copy()
    for bad in (lambda: g.set_ranges([[1, 5], [4, 6]], [1, 2], 0, 10), lambda: g.set_ranges([[5, 4]], [1], 0, 10),
                lambda: g.set_ids([2, 3, 2], [1, 1, 2], 0, 10)):
        with pytest.raises(ValueError):
            bad()
        assert (g.keys == before).all()
    g.set_ranges([[3, 3], [1, 5]], [9, 0], 0, 10)                          # an empty range overlaps nothing; key 0 un-groups
    assert g.keys.tolist() == [0, 0, 0, 0, 3, 0, 0, 0, 8, 8]
    g.set_ids([105], [6], 100, 12)                                         # under an id offset, after two rows were appended
    assert g.keys.tolist() == [0, 0, 0, 0, 6, 0, 0, 0, 8, 8, 0, 0]
    assert g.keys_of([105, 109, 113, 100, 5], 100, 12).tolist() == [6, 8, 0, 0, 0]
    alive = np.ones(12, bool)
    alive[8] = False
    assert g.count(12) == (3, 3) and g.count(12, alive) == (3, 2)


def test_default_fetch():
    assert [default_fetch(k) for k in (1, 8, 10, 64, 100, 256, 300, 4096)] == [32, 32, 40, 256, 256, 256, 300, 4096]
