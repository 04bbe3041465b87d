"""Boosted search (mx_prior, mx_index_search_boosted) on the GPU against its statement in NumPy
(tests/boosted_model.py).  Every case compares ids, n_found and complete with integer equality and scores, dists, priors and combined
by their bits -- against the model over the lists the index itself returns in that run, against the model over the oracle's lists, and
against brute force over all rows wherever complete = 1.  The shapes are small: the re-ranking never looks past the top-`fetch` list."""
import threading

import numpy as np
import pytest

from boosted_model import PriorModel, boost_lists, boosted_model, brute_force_boosted, case_a, case_b
from conftest import bits
from grouped_model import candidate_lists

pytestmark = pytest.mark.gpu

N, D = 2000, 64
NAMES = ("ids", "scores", "dists", "priors", "combined", "n_found", "complete")
_CACHE = {}


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def small():
    """Case A's corpus (the near-copy corpus, 100 clusters x 20 rows x 64 dims), its 6 queries near cluster centres and its priors"""
    if "small" not in _CACHE:
        _CACHE["small"] = case_a()
    return _CACHE["small"]


def model(oracle, key, *a, **kw):
    """boosted_model, computed once per named case"""
    if key not in _CACHE:
        _CACHE[key] = boosted_model(oracle, *a, **kw)
    return _CACHE[key]


def same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        if name in ("scores", "dists", "priors"):
            g, w = bits(g), bits(w)
        elif name == "combined":
            g, w = bits64(g), bits64(w)
        np.testing.assert_array_equal(np.asarray(g), np.asarray(w), err_msg=f"{what}: {name}")


def blanks_ok(got, k):
    ids, sc, di, pr, cb, nf, _ = got
    for b in range(len(nf)):
        n = int(nf[b])
        assert 0 <= n <= k
        assert (ids[b, n:] == 0).all() and (bits(sc[b, n:]) == 0).all() and np.isposinf(di[b, n:]).all()
        assert (bits(pr[b, n:]) == 0).all() and (bits64(cb[b, n:]) == 0).all()


def from_lists(idx, pv, w, hi, Q, k, fetch, flt=None, id_offset=0):
    """the model over the lists the index itself returns for k = fetch in this run"""
    ci, cs, cd, cnf = idx.search(Q, fetch) if flt is None else idx.search_with(flt, Q, fetch)
    return boost_lists(ci, cs, cd, cnf, pv, w, hi, k, fetch, id_offset)


def brute_where_complete(oracle, X, Q, pv, w, k, got, alive=None):
    """-> how many queries were complete; each of them equals brute force over all rows"""
    w = np.broadcast_to(np.asarray(w, np.float32), (len(Q),))
    for b in np.flatnonzero(got[6]):
        wi, wd, wc = brute_force_boosted(oracle, X, Q[b], pv, w[b], k, alive)
        n = int(got[5][b])
        assert n == len(wi)
        np.testing.assert_array_equal(got[0][b, :n], wi, err_msg=f"query {b}: complete, but not the top-k of all rows")
        np.testing.assert_array_equal(bits(got[2][b, :n]), bits(wd))
        np.testing.assert_array_equal(bits64(got[4][b, :n]), bits64(wc))
    return int(np.count_nonzero(got[6]))


def set_priors(pri, pv, id_offset=0):
    pri.set_ids(np.arange(1, len(pv) + 1, dtype=np.uint64) + np.uint64(id_offset), pv)


def hi_of(pv):
    return np.float32(max(0.0, float(np.max(pv))))


# ---- the prior object -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sharded", [False, True], ids=["plain", "3-shards"])
def test_edits_gets_and_bounds_match_the_numpy_array(sharded, lib_built):
    from memex_amd import _lib
    from memex_amd.index import FlatIndex
    X = small()[0]
    rng = np.random.default_rng(3171)
    kw = dict(devices=[0, 0, 0], block_rows=96) if sharded else {}
    with FlatIndex(D, **kw) as idx:
        idx.add(X[:1200])
        off, size = 0, 1200
        m = PriorModel()
        alive = np.ones(N, bool)

        def check(pri, what):
            probe = np.concatenate([np.arange(0, size + 40, dtype=np.uint64) + np.uint64(max(off - 20, 0)),
                                    np.asarray([0, 1, off, off + size + 1, 2 ** 40, 2 ** 64 - 1], dtype=np.uint64)])
            np.testing.assert_array_equal(bits(pri.values_of(probe)), bits(m.values_of(probe, off, size)), err_msg=what)
            assert bits(pri.bound()) == bits(m.bound()), what

        with idx.make_prior() as pri:
            check(pri, "a new prior: 0 everywhere")
            assert pri.bound() == 0.0 and pri.bound(refresh=True) == 0.0
            for step in range(12):
                if step == 4:                                           # rows appended after an edit: 0 until named; the next edit
                    idx.add(X[1200:1700])                               # that names one regrows the array
                    size = 1700
                    check(pri, "after an append")
                    assert (pri.values_of(np.arange(1201, 1701, dtype=np.uint64)) == 0).all()
                if step == 6:
                    off = 5000
                    idx.set_id_offset(off)                              # the ids move along with the rows
                    check(pri, "after set_id_offset")
                if step == 8:
                    idx.add(X[1700:])
                    size = N
                    top = 10                                            # one row gets the largest value and is then removed
                    pri.set_ids([off + top + 1], [50.0])
                    m.set_ids([off + top + 1], [50.0], off, size)
                    gone = np.unique(np.concatenate([rng.choice(size, 150, replace=False), [top]]))
                    idx.remove(gone.astype(np.uint64) + np.uint64(off + 1))
                    alive[gone] = False                                 # removed rows keep their value
                    check(pri, "after removals")
                    before = m.bound()
                    want = m.bound(refresh=True, size=size, alive=alive)
                    assert want < before, "(condition on the input) the refresh must lower the bound"
                    assert bits(pri.bound(refresh=True)) == bits(want), "refresh ignores removed rows"
                if step % 2 == 0:
                    cuts = np.sort(rng.choice(np.arange(1, size + 60), 24, replace=False)) + off
                    r = np.stack([cuts[0::2], cuts[1::2]], axis=1).astype(np.uint64)        # 12 disjoint ranges, some past the rows
                    r = r[rng.permutation(len(r))]                                          # in any order
                    v = rng.uniform(-1.0, 2.0, len(r)).astype(np.float32)                   # negative values are a penalty
                    pri.set_ranges(r, v)
                    m.set_ranges(r, v, off, size)
                else:
                    i = rng.integers(max(off - 5, 0), off + size + 30, 300).astype(np.uint64)
                    i = np.concatenate([i, i[:40]])                                         # repeats, with the same value
                    v = (i % np.uint64(7)).astype(np.float32) * np.float32(0.125 * step) - np.float32(1)   # a function of the id
                    pri.set_ids(i, v)
                    m.set_ids(i, v, off, size)
                check(pri, f"step {step}")
                if step in (3, 9, 11):                                  # overwritten large values: the bound stays until refreshed
                    assert bits(pri.bound(refresh=True)) == bits(m.bound(refresh=True, size=size, alive=alive)), f"refresh at step {step}"
                    check(pri, f"step {step}, refreshed")
            assert (m.vals != 0).sum() > 100 and (m.vals < 0).any() and m.vals.size == N            # (conditions on the input)
            # refused edits change nothing, the bound included
            everyone = np.arange(off + 1, off + size + 1, dtype=np.uint64)
            before, hi = pri.values_of(everyone), pri.bound()
            for bad in (lambda: pri.set_ranges([[off + 10, off + 20], [off + 19, off + 30]], [1.0, 2.0]),
                        lambda: pri.set_ranges([[off + 30, off + 20]], [1.0]),
                        lambda: pri.set_ids([off + 5, off + 9, off + 5], [3.0, 3.0, 4.0]),
                        lambda: pri.set_ids([off + 5, off + 5], [0.0, -0.0]),               # different bits
                        lambda: pri.set_ids([off + 5, off + 6], [99.0, np.nan]),
                        lambda: pri.set_ids([off + 5], [np.inf]),
                        lambda: pri.set_ranges([[off + 10, off + 20], [off + 40, off + 50]], [99.0, -np.inf]),
                        lambda: pri.set_ranges([[off + 10, off + 10]], [np.nan])):          # also on an empty range
                with pytest.raises(_lib.MemexHipError) as e:
                    bad()
                assert e.value.code == _lib.MX_EINVAL
                np.testing.assert_array_equal(bits(pri.values_of(everyone)), bits(before))
                assert pri.bound() == hi
            pri.set_ranges([[off + 10, off + 20], [off + 20, off + 30], [off + 15, off + 15]], [1.5, 2.5, 9.0])   # touching and empty: fine
            pri.set_ids([off + 5, off + 5], [3.0, 3.0])
            m.set_ranges([[off + 10, off + 20], [off + 20, off + 30], [off + 15, off + 15]], [1.5, 2.5, 9.0], off, size)
            m.set_ids([off + 5, off + 5], [3.0, 3.0], off, size)
            check(pri, "touching ranges, an empty range, an id twice with one value")
            assert pri.bound() == 9.0, "the bound follows what the call was handed, an empty range's value included"


# ---- search against the model -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,fetches", [(1, (1, 32)), (10, (32, 255, 256))], ids=["k1", "k10"])
def test_search_equals_the_model(k, fetches, oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, Q, pv = small()
    hi = hi_of(pv)
    complete = 0
    with FlatIndex(D) as idx, idx.make_prior() as pri:
        idx.add(X)
        set_priors(pri, pv)
        assert bits(pri.bound()) == bits(hi)
        for fetch in fetches:
            for w in (0.05, 1.0):
                got = idx.search_boosted(pri, Q, k, weight=w, fetch=fetch)
                what = f"k {k} fetch {fetch} w {w}"
                same(got, from_lists(idx, pv, w, hi, Q, k, fetch), what + ": the lists of this run")
                same(got, model(oracle, ("small", k, fetch, w), X, Q, k, pv, w=w, hi=hi, fetch=fetch), what)
                blanks_ok(got, k)
                complete += brute_where_complete(oracle, X, Q, pv, w, k, got)
                ci, cs, cd, _ = idx.search(Q, fetch)                    # every reported entry is literally an entry of the list
                for b in range(len(Q)):
                    at = [list(ci[b]).index(i) for i in got[0][b]]
                    np.testing.assert_array_equal(bits(got[1][b]), bits(cs[b, at]))
                    np.testing.assert_array_equal(bits(got[2][b]), bits(cd[b, at]))
                    np.testing.assert_array_equal(bits(got[3][b]), bits(pv[ci[b, at].astype(np.int64) - 1]))
        assert complete > 0, "(condition on the input) some answer must carry the certificate"
        one = idx.search_boosted(pri, Q[0], k)                          # [dim]: one query, the default fetch and weight
        same(one, tuple(a[:1] for a in model(oracle, ("small", k, "default"), X, Q, k, pv, hi=hi)), "one query, defaults")


def test_case_a_and_case_b(oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, Q, pv = small()
    with FlatIndex(D) as idx, idx.make_prior() as pri:
        idx.add(X)
        set_priors(pri, pv)
        got = idx.search_boosted(pri, Q, 5, weight=0.05, fetch=32)      # Case A: every query complete, and the true top-5
        same(got, model(oracle, "case-a", X, Q, 5, pv, w=0.05, hi=hi_of(pv), fetch=32), "Case A")
        assert got[6].all() and brute_where_complete(oracle, X, Q, pv, 0.05, 5, got) == len(Q)
        assert (got[0] != idx.search(Q, 5)[0]).any(), "(condition on the input) the priors re-order some answer"
    X, Q, pb, far = case_b(oracle)
    with FlatIndex(D) as idx, idx.make_prior() as pri:
        idx.add(X)
        pri.set_ids([far + 1], [100.0])
        assert pri.bound() == 100.0
        got = idx.search_boosted(pri, Q, 5, weight=1.0, fetch=32)       # Case B: the far row is outside the list
        same(got, model(oracle, "case-b", X, Q, 5, pb, w=1.0, hi=np.float32(100.0), fetch=32), "Case B")
        assert not got[6][0] and far + 1 not in got[0][0].tolist()
        assert brute_force_boosted(oracle, X, Q[0], pb, 1.0, 5)[0][0] == far + 1
        full = idx.search_boosted(pri, Q[:1], 5, weight=1.0, fetch=4096)               # 2000 rows < fetch: complete, the row first
        assert full[6][0] and full[0][0, 0] == far + 1 and full[3][0, 0] == 100.0
        assert brute_where_complete(oracle, X, Q[:1], pb, 1.0, 5, full) == 1


def big():
    """5000 random rows at d = 64, three queries, priors uniform in [0, 1)"""
    if "big" not in _CACHE:
        rng = np.random.default_rng(3173)
        X = rng.standard_normal((5000, D)).astype(np.float32)
        Q = np.stack([rng.standard_normal(D), X[17] + 0.1, -X[99]]).astype(np.float32)
        _CACHE["big"] = (X, Q, rng.random(5000).astype(np.float32))
    return _CACHE["big"]


@pytest.mark.parametrize("fetch", [1025, 4096])
def test_long_lists(fetch, oracle, lib_built):
    """the EXACT path's lists; 1025: one entry in the second ownership round; 4096: every thread owns four, the LDS array is full"""
    from memex_amd.index import FlatIndex
    X, Q, pv = big()
    hi = hi_of(pv)
    w = np.asarray([0.01, 0.3, 2.0], np.float32)
    with FlatIndex(D) as idx, idx.make_prior() as pri:
        idx.add(X)
        set_priors(pri, pv)
        for k in (10, fetch):
            got = idx.search_boosted(pri, Q, k, weight=w, fetch=fetch)
            same(got, from_lists(idx, pv, w, hi, Q, k, fetch), f"fetch {fetch} k {k}: the lists of this run")
            if k == 10:
                same(got, boosted_model(oracle, X, Q, k, pv, w=w, hi=hi, fetch=fetch), f"fetch {fetch} k {k}")
                brute_where_complete(oracle, X, Q, pv, w, k, got)
            else:
                assert (got[5] == fetch).all() and not got[6].any()     # k = fetch: the last entry cannot beat its own bound
                assert all(sorted(got[0][b].tolist()) == sorted(idx.search(Q[b], fetch)[0][0].tolist()) for b in range(3))
                assert (np.diff(got[4], axis=1) <= 0).all()


def test_short_lists_an_empty_index_and_two_batches(oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, Q, pv = small()
    with FlatIndex(D) as idx, idx.make_prior() as pri:                  # fetch larger than the index: m < fetch, complete
        idx.add(X[:300])
        set_priors(pri, pv[:300])
        for k, fetch in ((10, 301), (10, 1024), (300, 300), (400, 4096)):
            got = idx.search_boosted(pri, Q, k, weight=0.5, fetch=fetch)
            same(got, boosted_model(oracle, X[:300], Q, k, pv[:300], w=0.5, fetch=fetch), f"300 rows, k {k} fetch {fetch}")
            blanks_ok(got, k)
            assert (got[5] == min(k, 300)).all() and got[6].all() == (fetch > 300)
            assert brute_where_complete(oracle, X[:300], Q, pv[:300], 0.5, k, got) == (len(Q) if fetch > 300 else 0)
        rng = np.random.default_rng(3174)                               # B = 513: batches of 512 and 1; per-query weights
        Qb = rng.standard_normal((513, D)).astype(np.float32)
        wb = rng.uniform(0.0, 2.0, 513).astype(np.float32)
        wb[::50] = 0.0
        got = idx.search_boosted(pri, Qb, 5, weight=wb, fetch=16)
        same(got, from_lists(idx, pv[:300], wb, hi_of(pv[:300]), Qb, 5, 16), "513 queries")
        assert got[6].any() and (~got[6]).any()                         # (condition on the input)
        for b in (0, 50, 511, 512):
            same(idx.search_boosted(pri, Qb[b], 5, weight=wb[b], fetch=16), tuple(a[b:b + 1] for a in got), f"query {b} alone")
        got = idx.search_boosted(pri, np.zeros((0, D), np.float32), 5)  # B = 0
        assert got[0].shape == (0, 5) and got[4].shape == (0, 5) and got[5].shape == (0,)
    with FlatIndex(D) as idx, idx.make_prior() as pri:                  # an index without rows finds nothing, completely
        got = idx.search_boosted(pri, Q, 5, weight=2.0)
        assert (got[5] == 0).all() and got[6].all()
        blanks_ok(got, 5)
        assert pri.bound(refresh=True) == 0.0 and (pri.values_of([1, 2]) == 0).all()


def test_ties(oracle, lib_built):
    """every row stored three times: bit-equal scores.  Equal priors keep the copies in id order; an exact tie with U is not complete"""
    from memex_amd.index import FlatIndex
    X, Q, _ = small()
    V = X[:600]
    T = np.ascontiguousarray(np.concatenate([V, V, V]))
    pv = np.tile(np.random.default_rng(3175).random(600).astype(np.float32), 3)
    with FlatIndex(D) as idx, idx.make_prior() as pri:
        idx.add(T)
        set_priors(pri, pv)
        for k, fetch in ((3, 3), (6, 12), (10, 40)):
            got = idx.search_boosted(pri, Q, k, weight=0.05, fetch=fetch)
            same(got, boosted_model(oracle, T, Q, k, pv, w=0.05, fetch=fetch), f"tripled rows, k {k} fetch {fetch}")
        for b in range(len(Q)):                                         # the copies of one row: ids i, i + 600, i + 1200, in that order
            trip = [int(i) for i in got[0][b] if (int(i) - 1) % 600 == (int(got[0][b, 0]) - 1) % 600]
            assert trip == sorted(trip) and len(trip) == 3
        assert (np.diff(bits64(got[4]).astype(np.int64), axis=1) == 0).any()               # (condition: equal combined values are reported)
        # k = 1, fetch = 2 with w = 1: both entries are copies of one row (score s) with the prior 0.5 = hi: c = s + 0.5 = U exactly
        best = int(idx.search(Q[0], 1)[0][0, 0]) - 1
        pri.set_ranges([[1, 1801]], [0.0])
        pri.set_ids(np.asarray([best % 600 + 1 + 600 * c for c in range(3)], np.uint64), [0.5, 0.5, 0.5])
        assert pri.bound(refresh=True) == 0.5
        pt = np.zeros(1800, np.float32)
        pt[best % 600::600] = 0.5
        got = idx.search_boosted(pri, Q[:1], 1, weight=1.0, fetch=2)
        same(got, boosted_model(oracle, T, Q[:1], 1, pt, w=1.0, fetch=2), "a tie with U")
        s = np.float64(got[1][0, 0])
        assert not got[6][0] and bits64(got[4][0, 0]) == bits64(s + 0.5) and got[0][0, 0] == best % 600 + 1
        got = idx.search_boosted(pri, Q[:1], 1, weight=1.0, fetch=4)    # the fourth entry scores lower: U drops below c
        same(got, boosted_model(oracle, T, Q[:1], 1, pt, w=1.0, fetch=4), "past the copies")
        assert got[6][0] and got[0][0, 0] == best % 600 + 1
        assert brute_where_complete(oracle, T, Q[:1], pt, 1.0, 1, got) == 1


def test_weights(oracle, lib_built):
    from memex_amd import _lib
    from memex_amd.index import FlatIndex
    X, Q, pv = small()
    pn = (pv - np.float32(0.5)).astype(np.float32)                      # negative priors: a penalty
    with FlatIndex(D) as idx, idx.make_prior() as pri:
        idx.add(X)
        set_priors(pri, pn)
        w = np.asarray([0.0, 0.05, 0.5, 1.0, 0.0, 3.0], np.float32)    # per query, two of them 0
        got = idx.search_boosted(pri, Q, 10, weight=w, fetch=40)
        same(got, model(oracle, "weights", X, Q, 10, pn, w=w, hi=hi_of(pn), fetch=40), "per-query weights")
        brute_where_complete(oracle, X, Q, pn, w, 10, got)
        zero = idx.search_boosted(pri, Q, 10, weight=0.0, fetch=40)     # w = 0: search(k), bit for bit
        ids, sc, di, nf = idx.search(Q, 10)
        np.testing.assert_array_equal(zero[0], ids)
        np.testing.assert_array_equal(bits(zero[1]), bits(sc))
        np.testing.assert_array_equal(bits(zero[2]), bits(di))
        np.testing.assert_array_equal(bits64(zero[4]), bits64(sc.astype(np.float64)))
        np.testing.assert_array_equal(bits(zero[3]), bits(pn[ids.astype(np.int64) - 1]))
        np.testing.assert_array_equal(zero[5], nf)
        for b in (0, 4):
            for a, z in zip(got, zero):
                np.testing.assert_array_equal(np.asarray(a[b]), np.asarray(z[b]))
        for bad in (-1.0, np.nan, np.inf, [1.0, 1.0, 1.0, 1.0, 1.0, -0.0001]):
            with pytest.raises(_lib.MemexHipError) as e:
                idx.search_boosted(pri, Q, 10, weight=bad)
            assert e.value.code == _lib.MX_EINVAL


def test_filter_removed_rows_and_id_offset(oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, Q, pv = small()
    allowed = np.zeros(N, bool)
    allowed[300:1500] = True
    off = 7000
    with FlatIndex(D) as idx, idx.make_prior() as pri:
        idx.add(X)
        set_priors(pri, pv)
        idx.set_id_offset(off)                                          # the values stay with the rows
        flt = idx.make_filter(ranges=[[off + 301, off + 1501]])
        first = idx.search_boosted(pri, Q, 5, weight=0.05, fetch=32)
        gone = np.unique(first[0][:, :2].astype(np.int64) - 1 - off)    # the two best of every query
        idx.remove(gone.astype(np.uint64) + np.uint64(off + 1))
        alive = np.ones(N, bool)
        alive[gone] = False
        hi = hi_of(pv)
        for k, fetch, f, mask in ((5, 32, None, None), (10, 40, flt, allowed), (5, 300, flt, allowed)):
            got = idx.search_boosted(pri, Q, k, weight=0.05, fetch=fetch, flt=f)
            what = f"k {k} fetch {fetch} filter {f is not None}"
            same(got, boosted_model(oracle, X, Q, k, pv, w=0.05, hi=hi, fetch=fetch, alive=alive, allowed=mask, id_offset=off), what)
            same(got, from_lists(idx, pv, 0.05, hi, Q, k, fetch, flt=f, id_offset=off), what + ": the lists of this run")
            rows = got[0][got[0] != 0].astype(np.int64) - 1 - off
            assert alive[rows].all() and (mask is None or mask[rows].all())
            live = alive if mask is None else alive & mask
            for b in np.flatnonzero(got[6]):                            # complete: the top-k of the live (allowed) rows
                wi, _, wc = brute_force_boosted(oracle, X, Q[b], pv, 0.05, k, live)
                np.testing.assert_array_equal(got[0][b], wi + np.uint64(off))
                np.testing.assert_array_equal(bits64(got[4][b]), bits64(wc))
        flt.close()
        with idx.make_filter() as empty:                                # the empty filter finds nothing: a short list, complete
            got = idx.search_boosted(pri, Q, 3, flt=empty)
            assert (got[5] == 0).all() and got[6].all()


@pytest.mark.parametrize("shards,block", [(3, 96)], ids=["3-shards"])
def test_sharded_equals_plain(shards, block, oracle, lib_built):
    from memex_amd.index import FlatIndex
    X, Q, pv = small()
    gone = np.concatenate([np.arange(block, block + 30), np.arange(2 * block + 5, 2 * block + 25)])   # rows of the second and third block
    alive = np.ones(N, bool)
    alive[gone] = False
    w = np.asarray([0.0, 0.05, 0.05, 0.5, 1.0, 2.0], np.float32)
    with FlatIndex(D) as plain, FlatIndex(D, devices=[0] * shards, block_rows=block) as sh:
        pris = []
        for idx in (plain, sh):
            idx.add(X)
            idx.remove(gone.astype(np.uint64) + np.uint64(1))
            pris.append(idx.make_prior())
            set_priors(pris[-1], pv)
        try:
            for k, fetch in ((10, 40), (10, 10), (5, 300)):
                a = sh.search_boosted(pris[1], Q, k, weight=w, fetch=fetch)
                same(a, plain.search_boosted(pris[0], Q, k, weight=w, fetch=fetch), f"{shards} shards vs plain, k {k} fetch {fetch}")
                same(a, boosted_model(oracle, X, Q, k, pv, w=w, hi=hi_of(pv), fetch=fetch, alive=alive), f"{shards} shards vs model, k {k}")
            assert bits(pris[1].bound(refresh=True)) == bits(pris[0].bound(refresh=True)) == bits(hi_of(pv[alive]))
            with sh.make_filter(ranges=[[301, 1501]]) as fs, plain.make_filter(ranges=[[301, 1501]]) as fp:
                same(sh.search_boosted(pris[1], Q, 10, weight=w, fetch=40, flt=fs),
                     plain.search_boosted(pris[0], Q, 10, weight=w, fetch=40, flt=fp), f"{shards} shards vs plain, filtered")
        finally:
            for p in pris:
                p.close()


def test_device_pointer_variant_equals_the_host_variant(lib_built):
    import torch
    from memex_amd.index import FlatIndex
    X, Q, pv = small()
    w = np.asarray([0.0, 0.05, 0.05, 0.5, 1.0, 2.0], np.float32)
    with FlatIndex(D) as plain, FlatIndex(D, devices=[0, 0], block_rows=64) as sh:
        for idx in (plain, sh):
            idx.add(X)
            with idx.make_prior() as pri, idx.make_filter(ranges=[[301, 1501]]) as flt:
                set_priors(pri, pv)
                for k, fetch, extras, f, wt in ((10, None, True, None, w), (7, 300, True, flt, 0.3), (7, 12, False, None, 1.0)):
                    B = len(Q)
                    q = torch.from_numpy(Q).cuda()
                    ids = torch.full((B, k), -1, dtype=torch.int64, device="cuda")
                    sc = torch.full((B, k), -1.0, dtype=torch.float32, device="cuda")
                    nf = torch.full((B,), -1, dtype=torch.int32, device="cuda")
                    di = torch.full((B, k), -1.0, dtype=torch.float32, device="cuda") if extras else None
                    pr = torch.full((B, k), -7.0, dtype=torch.float32, device="cuda") if extras else None
                    cb = torch.full((B, k), -7.0, dtype=torch.float64, device="cuda") if extras else None
                    done = torch.full((B,), 9, dtype=torch.uint8, device="cuda") if extras else None
                    idx.search_boosted_device(pri, q, k, ids, sc, di, pr, cb, nf, done, weight=wt, fetch=fetch, flt=f)
                    h = idx.search_boosted(pri, Q, k, weight=wt, fetch=fetch, flt=f)
                    np.testing.assert_array_equal(ids.cpu().numpy().astype(np.uint64), h[0])
                    np.testing.assert_array_equal(bits(sc.cpu().numpy()), bits(h[1]))
                    np.testing.assert_array_equal(nf.cpu().numpy(), h[5])
                    if extras:
                        np.testing.assert_array_equal(bits(di.cpu().numpy()), bits(h[2]))
                        np.testing.assert_array_equal(bits(pr.cpu().numpy()), bits(h[3]))
                        np.testing.assert_array_equal(bits64(cb.cpu().numpy()), bits64(h[4]))
                        np.testing.assert_array_equal(done.cpu().numpy().astype(bool), h[6])


def test_staleness_and_foreign_handles(oracle, lib_built, tmp_path):
    from memex_amd import _lib
    from memex_amd.index import FlatIndex
    X, Q, pv = small()

    def stale(idx, pri):
        for call in (lambda: idx.search_boosted(pri, Q, 5), lambda: pri.set_ranges([[1, 5]], [1.0]), lambda: pri.set_ids([3], [1.0]),
                     lambda: pri.values_of([1, 2]), pri.bound, lambda: pri.bound(refresh=True)):
            with pytest.raises(_lib.MemexHipError, match="stale") as e:
                call()
            assert e.value.code == _lib.MX_EINVAL
        pri.close()                                                     # still works

    with FlatIndex(D) as idx, FlatIndex(D) as other:
        idx.add(X)
        other.add(X[:100])
        pri = idx.make_prior()
        set_priors(pri, pv)
        assert idx.compact().size == N                                  # nothing removed: a no-op, the prior stays valid
        same(idx.search_boosted(pri, Q, 5, weight=0.05, fetch=32), model(oracle, "case-a", X, Q, 5, pv, w=0.05, hi=hi_of(pv), fetch=32),
             "after a no-op compact")
        with pytest.raises(_lib.MemexHipError, match="another index") as e:
            other.search_boosted(pri, Q, 5)
        assert e.value.code == _lib.MX_EINVAL
        with other.make_filter(ranges=[[1, 50]]) as foreign, pytest.raises(_lib.MemexHipError, match="another index") as e:
            idx.search_boosted(pri, Q, 5, flt=foreign)
        assert e.value.code == _lib.MX_EINVAL
        idx.remove([5, 150])
        idx.compact()
        stale(idx, pri)
        pri = idx.make_prior()
        idx.save(str(tmp_path))
        idx.load(str(tmp_path))
        stale(idx, pri)
        pri = idx.make_prior()
        idx.clear()
        stale(idx, pri)


def test_boosted_callers_beside_plain_callers(oracle, lib_built):
    """two threads issue boosted searches (two weights) while two issue plain ones on the same index: every answer equals its model"""
    from memex_amd.index import FlatIndex
    X, Q, pv = small()
    hi = hi_of(pv)
    want_b = {w: model(oracle, ("small", 10, 32, w), X, Q, 10, pv, w=w, hi=hi, fetch=32) for w in (0.05, 1.0)}
    want_p = candidate_lists(oracle, X, Q, 10)
    assert any((a != b).any() for a, b in zip(want_b[0.05][:1], want_b[1.0][:1]))          # (condition: the two weights differ)
    with FlatIndex(D) as idx, idx.make_prior() as pri:
        idx.add(X)
        set_priors(pri, pv)
        got, errs = [], []

        def boosted(w):
            try:
                for _ in range(6):
                    got.append(("b", w, idx.search_boosted(pri, Q, 10, weight=w, fetch=32)))
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        def plain():
            try:
                for _ in range(6):
                    got.append(("p", None, idx.search(Q, 10)))
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        ths = [threading.Thread(target=boosted, args=(0.05,)), threading.Thread(target=boosted, args=(1.0,)),
               threading.Thread(target=plain), threading.Thread(target=plain)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errs, errs
        assert len(got) == 24
        for kind, w, g in got:
            if kind == "b":
                same(g, want_b[w], f"a boosted caller at w {w}")
            else:
                np.testing.assert_array_equal(g[0], want_p[0])
                np.testing.assert_array_equal(bits(g[1]), bits(want_p[1]))
                np.testing.assert_array_equal(bits(g[2]), bits(want_p[2]))
                np.testing.assert_array_equal(g[3], want_p[3])
