"""The statement of grouped search with members (tests/group_rows_model.py) against brute force over all rows, without a GPU: what
`complete` and `members_complete` promise holds on data with exact ties and removed rows, and both outcomes
of both flags occur often enough for that to mean something."""
import numpy as np
import pytest

from conftest import bits
from group_rows_model import (brute_capped, brute_group_members, capped_model, default_fetch_rows, full_order, group_rows_model,
                              key_counts_model, settle_model)
from grouped_model import grouped_model, random_keys, row_keys

_CACHE = {}
FETCHES = (0, 1, 2, 3)


def tied():
    """100 vectors at d = 16, each stored six times (exact ties): 600 rows; keys in groups of 1 - 8 rows cut from the rows ordered
    by vector, so the copies of a vector tend to share a group and meet in the lists; a fifth ungrouped; every ninth row removed"""
    if "tied" not in _CACHE:
        rng = np.random.default_rng(319)
        V = rng.standard_normal((100, 16)).astype(np.float32)
        X = np.ascontiguousarray(np.concatenate([V] * 6))
        Q = (V[rng.integers(0, 100, 6)] + 0.2 * rng.standard_normal((6, 16))).astype(np.float32)
        order = (rng.permutation(100)[:, None] + 100 * np.arange(6)[None, :]).reshape(-1)
        alive = np.ones(600, bool)
        alive[::9] = False
        _CACHE["tied"] = (X, Q, random_keys(rng, 600, biggest=8, order=order), alive)
    return _CACHE["tied"]


def orders(oracle):
    if "orders" not in _CACHE:
        X, Q, _, alive = tied()
        _CACHE["orders"] = [full_order(oracle, X, Q[b], alive)[0] for b in range(len(Q))]
    return _CACHE["orders"]


def test_flags_against_brute_force(oracle):
    X, Q, keys, alive = tied()
    rk = row_keys(keys, 600)
    n_live = int(alive.sum())
    tally = {("c", 0): 0, ("c", 1): 0, ("m", 0): 0, ("m", 1): 0}
    for k in (3, 5):
        for n in (2, 4, 8):
            for fetch in [k + a for a in FETCHES] + [3 * k, 6 * k, 700]:
                ids, sc, di, gk, rows, mem, mc, nf, done = group_rows_model(oracle, X, Q, k, n, keys, fetch=fetch, alive=alive)
                for b in range(len(Q)):
                    want = brute_group_members(orders(oracle)[b], rk, k)
                    tally["c", int(done[b])] += 1
                    if done[b]:
                        assert nf[b] == min(k, len(want))
                    assert nf[b] <= len(want)
                    for j in range(int(nf[b])):                            # a reported head is a head of the full walk, in its place
                        key, members = want[j]
                        tally["m", int(mc[b, j])] += 1
                        assert gk[b, j] == key
                        m = int(mem[b, j])
                        assert m == min(n, int(rows[b, j])) and 1 <= m
                        if mc[b, j]:
                            assert m == min(n, len(members)), f"k {k} n {n} fetch {fetch} query {b} head {j}"
                        else:
                            assert m < n and fetch <= n_live and key != 0
                        np.testing.assert_array_equal(ids[b, j, :m], np.asarray(members[:m], np.uint64) + np.uint64(1))
                        assert (ids[b, j, m:] == 0).all() and (sc[b, j, m:] == 0).all() and np.isinf(di[b, j, m:]).all()
                        assert rows[b, j] <= len(members)
                    assert (ids[b, nf[b]:] == 0).all() and (rows[b, nf[b]:] == 0).all() and not mc[b, nf[b]:].any()
    cases_c = tally["c", 0] + tally["c", 1]
    cases_m = tally["m", 0] + tally["m", 1]
    for v in (0, 1):                                                       # (conditions on the input)
        assert 4 * tally["c", v] >= cases_c, tally
        assert 4 * tally["m", v] >= cases_m, tally


def test_capped_against_brute_force(oracle):
    X, Q, keys, alive = tied()
    rk = row_keys(keys, 600)
    tally = [0, 0]
    for k in (3, 5, 10):
        for per_key in (1, 2, 3):
            for fetch in [k + a for a in FETCHES] + [3 * k, 6 * k, 700]:
                ids, sc, di, gk, nf, done = capped_model(oracle, X, Q, k, per_key, keys, fetch, alive=alive)
                for b in range(len(Q)):
                    want = brute_capped(orders(oracle)[b], rk, k, per_key)
                    tally[int(done[b])] += 1
                    m = int(nf[b])
                    if done[b]:
                        assert m == len(want)
                    np.testing.assert_array_equal(ids[b, :m], np.asarray(want[:m], np.uint64) + np.uint64(1))
                    np.testing.assert_array_equal(gk[b, :m], rk[np.asarray(want[:m], np.int64)])
                    assert (ids[b, m:] == 0).all() and (gk[b, m:] == 0).all() and np.isinf(di[b, m:]).all()
    assert 4 * tally[0] >= sum(tally) and 4 * tally[1] >= sum(tally), tally


@pytest.mark.parametrize("k,fetch", [(1, 1), (3, 12), (5, 48), (10, 700)])
def test_identities_with_grouped_search(k, fetch, oracle):
    X, Q, keys, alive = tied()
    g = grouped_model(oracle, X, Q, k, keys, fetch=fetch, alive=alive)
    ids, sc, di, gk, rows, mem, mc, nf, done = group_rows_model(oracle, X, Q, k, 1, keys, fetch=fetch, alive=alive)
    for a, b in zip((ids[:, :, 0], sc[:, :, 0], di[:, :, 0], gk, rows, nf, done), g):
        np.testing.assert_array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b)
    assert mc[mem > 0].all(), "n = 1: the head is the member"
    c = capped_model(oracle, X, Q, k, 1, keys, fetch, alive=alive)
    for a, b in zip(c, (g[0], g[1], g[2], g[3], g[5], g[6])):
        np.testing.assert_array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b)
    plain = oracle.search(X[alive], Q, k)
    c = capped_model(oracle, X, Q, k, fetch, keys, fetch, alive=alive)
    live = np.flatnonzero(alive)
    np.testing.assert_array_equal(c[0], live[plain[0].astype(np.int64) - 1].astype(np.uint64) + np.uint64(1))


def test_settle_and_key_counts(oracle):
    X, Q, keys, alive = tied()
    rk = row_keys(keys, 600)
    ids, _, _, gk, rows, mem, mc, nf, _ = group_rows_model(oracle, X, Q, 5, 5, keys, fetch=24, alive=alive)
    settled = settle_model(gk, mem, mc, nf, keys, 600, alive)
    assert (settled >= mc).all() and (settled != mc).any() and not settled[mem > 0].all(), "(condition on the input)"
    for b in range(len(Q)):
        want = brute_group_members(orders(oracle)[b], rk, 5)
        for j in range(int(nf[b])):
            assert settled[b, j] == (int(mem[b, j]) == min(5, len(want[j][1])))
    a, l = key_counts_model(keys[:500], 600, [0, 1, 1, 4000000000], alive)
    assert a[0] == int((rk[:500] == 0).sum()) + 100 and a[1] == a[2] == int((rk[:500] == 1).sum()) and a[3] == 0 and (l <= a).all()
    assert l[0] == int(((row_keys(keys[:500], 600) == 0) & alive).sum())


def test_default_fetch_rows():
    got = [default_fetch_rows(k, n) for k, n in ((1, 1), (1, 16), (3, 2), (10, 3), (10, 16), (300, 2), (256, 16))]
    assert got == [32, 64, 32, 120, 256, 300, 256]
